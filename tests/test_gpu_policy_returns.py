"""rc_policy_returns / policy_returns against its binary32 specification (tests/policy_returns_spec.c), bit for bit: the two
checkpoints with a reward head and a synthetic critic (racing_dreamer_amd.critic.init_critic: no checkpoint ships one), both modes,
starts x horizons x lambdas that reach every row mapping, with and without the pcont head, from live latents and from a given
state; against the device's own policy_imagine; policy_value; purity after a real run; shards, slot masks, mixed tracks; output
subsets; the refusals; world_model.behaviour_terms and the planners' bootstrap."""
import ctypes as C
import math

import numpy as np
import pytest

from policy_observe_spec import PolicyObserveSpec
from policy_returns_spec import PolicyReturnsSpec
from policy_sample_spec import EpisodeClock
from test_golden_policy import weights
from test_gpu_policy_device import _recorded_inputs
from test_gpu_policy_imagine import _cpu, _drive

pytestmark = pytest.mark.gpu
MODES = ("mean", "sample")
WITH_HEAD = ("austria", "treitlstrasse")
SERIES = ("reward", "value", "pcont", "returns", "weight", "actions", "features")
STARTS = ("reward_start", "value_start", "pcont_start")
NAMES = {"actions": "action", "features": "feature"}          # the device's output names -> the spec's
_cache = {}


def _critic(pcont=True):
    from racing_dreamer_amd.critic import init_critic
    return init_critic(5, pcont=pcont)


def _spec(name, pcont=True):
    if (name, pcont) not in _cache:
        _cache[name, pcont] = PolicyReturnsSpec(weights(name), _critic(pcont))
    return _cache[name, pcont]


def _latents(n):
    """[n, 232] recorded latents (97 distinct ones)."""
    if "latents" not in _cache:
        _cache["latents"] = _recorded_inputs(97, seed=3)[1]
    return _cache["latents"][:n].copy()


def _env(name, n, cars=1, pcont=True, state=None, **kw):
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", n, cars, auto_reset=True, remap_actions=True, **kw)
    env.reset(mode="random", seed=1)
    env.load_policy(weights(name))
    env.load_critic(_critic(pcont))
    assert env.policy_has_value_head and env.policy_has_pcont_head == pcont
    if state is not None:
        env.policy_state.copy_(torch.from_numpy(state))
    return env


def _same(got, want, what, rows=slice(None)):
    for k, g in got.items():
        w = want[NAMES.get(k, k)]
        assert g.shape == w.shape and g[rows].tobytes() == w[rows].tobytes(), (what, k, float(np.abs(g[rows] - w[rows]).max()))


# (starts, horizon, lambda_, pcont head): one row; one row past a workgroup; three workgroups and a partial one; H = 2 is one step
# of the recursion, 64 the longest; lambda 0 and 1 are the recursion's two ends
CASES = ((1, 64, 0.95, True), (33, 2, 0.0, True), (33, 3, 1.0, False), (97, 15, 0.95, True), (97, 3, 0.95, False))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", WITH_HEAD)
def test_one_call_is_the_spec_bit_for_bit(name, mode):
    """Recorded latents written into policy_state, and the same latents given as `state` under a row_offset: every output of one
    policy_returns equals the spec in every row."""
    import torch
    for s, h, lam, pcont in CASES:
        state = _latents(s)
        env = _env(name, s, pcont=pcont, state=state)
        outputs = SERIES + STARTS[:3 if pcont else 2]
        clock = EpisodeClock(s)
        clock.reset()
        got = _cpu(env.policy_returns(h, mode, seed=77, lambda_=lam, discount=0.97, outputs=outputs))
        want = _spec(name, pcont).returns(state, keys=clock.keys(), horizon=h, mode=mode, seed=77, lambda_=lam, discount=0.97)
        assert set(got) == set(outputs)
        _same(got, want, (name, mode, s, h, "live"))
        assert np.abs(got["returns"]).max() > 1e-3 and got["weight"][:, 0].min() == 1.0
        if not pcont:
            assert np.all(got["pcont"] == np.float32(0.97))
        offset = (1 << 33) + 5
        got = _cpu(env.policy_returns(h, mode, seed=77, lambda_=lam, discount=0.97, state=torch.from_numpy(state), row_offset=offset, outputs=outputs))
        want = _spec(name, pcont).returns(state, ids=offset + np.arange(s, dtype=np.uint64), horizon=h, mode=mode, seed=77, lambda_=lam, discount=0.97)
        _same(got, want, (name, mode, s, h, "given"))
        env.close()


@pytest.mark.parametrize("mode", MODES)
def test_live_starts_dream_the_devices_own_imagination(mode):
    """On live latents reward, actions and features are byte for byte policy_imagine's for the same seed, closed loop and open
    loop (a third of the given actions beyond +-1)."""
    import torch
    n, h = 35, 15
    env = _env("austria", n, state=_latents(n))
    acts = torch.from_numpy(np.random.default_rng(2).uniform(-1.5, 1.5, (n, h, 2)).astype(np.float32))
    for a in (None, acts):
        got = _cpu(env.policy_returns(h, mode, seed=9, actions=a, outputs=("reward", "actions", "features", "reward_start")))
        own = _cpu(env.policy_imagine(h, mode, seed=9, actions=a, features=True, start_reward=True))
        for k, o in (("reward", "reward"), ("actions", "action"), ("features", "feature"), ("reward_start", "reward_start")):
            assert got[k].tobytes() == own[o].tobytes(), (mode, a is None, k)
    env.close()


def test_policy_value_is_the_value_of_the_returned_features():
    """policy_value(features)[..., t] equals policy_returns' value[:, t] (and reward, pcont), byte for byte; on the live latents it
    is value_start; the leading shape is kept."""
    n, h = 33, 3
    env = _env("austria", n, state=_latents(n))
    got = env.policy_returns(h, "sample", seed=4, outputs=("features", "value", "reward", "pcont", "value_start"))
    val = env.policy_value(got["features"], outputs=("value", "reward", "pcont"))
    assert val["value"].shape == (n, h)
    got, val = _cpu(got), _cpu(val)
    for k in ("value", "reward", "pcont"):
        assert val[k].tobytes() == got[k].tobytes(), k
    live = _cpu(env.policy_value())
    assert set(live) == {"value"} and live["value"].tobytes() == got["value_start"].tobytes()
    env.close()


def test_after_a_real_run_nothing_else_changes():
    """30 closed-loop agent steps with resets, then policy_returns from the live latents in both modes: the spec's, keyed by the
    counters the last step left.  policy_state, action_in and the whole arena (observation views, episode counters) are byte for
    byte what they were, and the next policy_act equals that of a twin env that never made the call."""
    import torch
    n = 48
    kw = dict(terminate_on_collision=True, time_limit_steps=7)
    env, twin = _env("austria", n, **kw), _env("austria", n, **kw)
    for e in (env, twin):
        e.reset(mode="random", seed=5)
    clock = EpisodeClock(n)
    clock.reset()
    clock.reset()                        # (_env's reset, and the one above)
    _drive(env, 30, clock)
    _drive(twin, 30)
    torch.cuda.synchronize()
    state = env.policy_state.cpu().numpy()
    assert clock.episode.min() >= 5 and np.abs(state[:, 30:230]).max() > 0.1
    before = [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes()]
    for mode in MODES:
        got = _cpu(env.policy_returns(15, mode, seed=11, outputs=SERIES + STARTS))
        _same(got, _spec("austria").returns(state, keys=clock.keys(), horizon=15, mode=mode, seed=11), mode)
    torch.cuda.synchronize()
    assert before == [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes()]
    a, b = env.policy_act().cpu().numpy(), twin.policy_act().cpu().numpy()
    assert a.tobytes() == b.tobytes() and env.policy_state.cpu().numpy().tobytes() == twin.policy_state.cpu().numpy().tobytes()
    env.close()
    twin.close()


def test_shards_slot_mask_and_mixed_tracks():
    """Two shards of a given state with their row_offset reproduce the full batch in `sample`; a slot mask on a 2-car env leaves
    the other cars' rows as the caller filled them; a MixedTrackEnv writes its blocks' rows; envs [0, 9) and [9, 20) on two
    handles with first_env offsets give the rows of one handle over [0, 20)."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    outputs, h = ("returns", "weight", "value", "actions"), 4
    state = _latents(40)
    env = _env("austria", 20, cars=2)
    dev = torch.from_numpy(state).to(env.device)
    full = _cpu(env.policy_returns(h, "sample", seed=8, state=dev, outputs=outputs))
    for lo, hi in ((0, 7), (7, 40)):
        part = _cpu(env.policy_returns(h, "sample", seed=8, state=dev[lo:hi], row_offset=lo, outputs=outputs))
        assert all(part[k].tobytes() == full[k][lo:hi].tobytes() for k in full)
    wrong = _cpu(env.policy_returns(h, "sample", seed=8, state=dev[7:], row_offset=0, outputs=("returns",)))
    assert not np.array_equal(wrong["returns"], full["returns"][7:])
    # the mask: slot 1 only, the rows of slot 0 keep the sentinel
    env.policy_state.copy_(dev)
    clock = EpisodeClock(20, 2)
    clock.reset()
    want = _spec("austria").returns(state, keys=clock.keys(), horizon=h, mode="sample", seed=14)
    out = {k: torch.full(v.shape, 7.0, device=env.device) for k, v in full.items()}
    got = env.policy_returns(h, "sample", seed=14, slots=(1,), outputs=outputs, out=out)
    assert all(got[k] is out[k] for k in out)
    got = _cpu(got)
    _same(got, want, "mask", np.arange(1, 40, 2))
    assert all(np.all(g[::2] == 7.0) for g in got.values())
    env.close()

    mixed = MixedTrackEnv(["columbia", "austria", "barcelona"], [13, 20, 7], auto_reset=True, remap_actions=True)
    mixed.reset(mode="random", seed=4)
    mixed.load_policy(weights("austria"))
    mixed.load_critic(_critic())
    assert mixed.policy_has_value_head and mixed.policy_has_pcont_head
    clock = EpisodeClock(40)
    clock.reset()
    _drive(mixed, 3, clock)
    torch.cuda.synchronize()
    st = mixed.policy_state.cpu().numpy()
    got = _cpu(mixed.policy_returns(h, "sample", seed=21, outputs=outputs))
    _same(got, _spec("austria").returns(st, keys=clock.keys(), horizon=h, mode="sample", seed=21), "mixed")
    given = _cpu(mixed.policy_returns(h, "sample", seed=21, state=torch.from_numpy(st), outputs=outputs))
    _same(given, _spec("austria").returns(st, horizon=h, mode="sample", seed=21), "mixed, given state")
    val = _cpu(mixed.policy_value(outputs=("value", "pcont")))
    assert val["value"].shape == (40,) and 0.0 < val["pcont"].min() and val["pcont"].max() < 1.0
    mixed.close()

    def run(n, first):
        e = BatchedRaceEnv("austria", n, 2, auto_reset=True, remap_actions=True, terminate_on_collision=True, time_limit_steps=4, first_env=first)
        e.reset(mode="random", seed=5)
        e.load_policy(weights("austria"))
        e.load_critic(_critic())
        _drive(e, 6)
        res = _cpu(e.policy_returns(h, "sample", seed=31, outputs=outputs))
        e.close()
        return res
    whole = run(20, 0)
    for lo, hi in ((0, 9), (9, 20)):
        part = run(hi - lo, lo)
        assert all(np.array_equal(part[k], whole[k][2 * lo:2 * hi]) for k in whole)


def test_a_subset_of_the_outputs_gives_the_same_bytes():
    """`returns` alone (the kernel then skips the reward and pcont heads at the last step and writes nothing else), `weight`
    alone, `value` alone: the bytes of the call that asks for everything.  H = 2 and 15, with and without the pcont head."""
    for pcont in (True, False):
        n = 33
        env = _env("austria", n, pcont=pcont, state=_latents(n))
        for h in (2, 15):
            full = _cpu(env.policy_returns(h, "sample", seed=6, outputs=SERIES + STARTS[:2]))
            for names in (("returns",), ("weight",), ("value",), ("pcont", "weight"), ("returns", "weight")):
                part = _cpu(env.policy_returns(h, "sample", seed=6, outputs=names))
                assert set(part) == set(names) and all(part[k].tobytes() == full[k].tobytes() for k in names), (pcont, h, names)
        env.close()


def test_refusals():
    """Every RC_ERR_INVALID of rc_policy_returns and rc_policy_load_critic names its cause; nothing is launched."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 4, 2, auto_reset=True)
    env.reset(mode="grid", seed=1)
    lib, n, h = env._lib, env.n_cars, 15
    buf = {k: torch.zeros((n, 64 * 230), device=env.device) for k in ("a", "b", "state")}
    ptr = {k: v.data_ptr() for k, v in buf.items()}

    def call(**kw):
        a = L.RcPolicyReturnsArgs(C.sizeof(L.RcPolicyReturnsArgs), h, 0, 3, 0.95, 0.99, 0, 0, 0)
        a.returns = ptr["a"]
        for key, v in kw.items():
            setattr(a, key, v)
        rc = lib.rc_policy_returns(env._h, C.byref(a))
        return rc, lib.rc_last_error()

    critic, keep = L.policy_critic(_critic())
    assert lib.rc_policy_load_critic(env._h, C.byref(critic)) == -1 and b"no policy loaded" in lib.rc_last_error()
    rc, msg = call()
    assert rc == -1 and b"no policy loaded" in msg
    w = {key: weights("austria")[key] for key in weights("austria").files if not key.startswith(("img2", "img3"))}
    env.load_policy(w)
    rc, msg = call()
    assert rc == -1 and b"img2 / img3" in msg
    env.load_policy(weights("austria"))
    for field in ("returns", "value", "value_start"):
        rc, msg = call(**{"returns": None, field: ptr["a"]})
        assert rc == -1 and b"no value head" in msg, field
    assert call(returns=None, reward=ptr["a"], weight=ptr["b"])[0] == 0                    # (no critic: the reward head and the constant pcont)
    env.load_critic(_critic(pcont=False))
    assert not env.policy_has_pcont_head
    rc, msg = call(returns=None, pcont_start=ptr["a"])
    assert rc == -1 and b"no pcont head" in msg
    env.load_critic(_critic())
    assert call()[0] == 0
    for kw, text in ((dict(struct_size=8), b"struct_size"), (dict(horizon=1), b"horizon"), (dict(horizon=0), b"horizon"), (dict(horizon=65), b"horizon"),
                     (dict(horizon=-1, returns=None, value_start=ptr["a"]), b"horizon"), (dict(horizon=0, returns=None, value=ptr["a"]), b"horizon"),
                     (dict(horizon=1, returns=None, weight=ptr["a"]), b"horizon"), (dict(mode=2), b"unknown mode"), (dict(mode=-1), b"unknown mode"),
                     (dict(lambda_=1.5), b"lambda_"), (dict(lambda_=-0.1), b"lambda_"), (dict(lambda_=float("nan")), b"lambda_"),
                     (dict(discount=1.5), b"discount"), (dict(discount=float("nan")), b"discount"), (dict(discount=float("inf")), b"discount"),
                     (dict(returns=None), b"no output"),
                     (dict(state_in=ptr["state"], starts=n), b"slot mask"), (dict(state_in=ptr["state"], slot_mask=0, starts=0), b"starts"),
                     (dict(state_in=ptr["state"], slot_mask=0, starts=1 << 40), b"starts"),
                     (dict(slot_mask=0), b"mask is empty"), (dict(slot_mask=4), b"beyond cars_per_env")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    assert call(horizon=0, returns=None, value_start=ptr["a"], pcont_start=ptr["b"])[0] == 0
    assert call(horizon=64, lambda_=0.0, discount=0.0, slot_mask=2)[0] == 0
    assert call(state_in=ptr["state"], slot_mask=0, starts=n, horizon=2)[0] == 0
    for bad in (dict(mode="deploy"), dict(lambda_=1.01), dict(discount=-0.5), dict(outputs=("return",)), dict(horizon=65), dict(state=buf["state"][:, :230])):
        with pytest.raises(ValueError):
            env.policy_returns(**bad)
    with pytest.raises(ValueError):
        env.policy_value(buf["state"][:, :229])
    with pytest.raises(L.RacecarHipError, match="slot mask"):
        env.policy_returns(state=buf["state"][:, :232], slots=(0,))
    # a critic with a wrong shape or half a pcont head; dropping the critic; the reward-less checkpoint
    bad = _critic()
    bad["value_h2_w"] = np.zeros((400, 399), np.float32)
    critic, keep = L.policy_critic(bad)
    assert lib.rc_policy_load_critic(env._h, C.byref(critic)) == -1 and b"value_h2_w has shape [400, 399]" in lib.rc_last_error()
    half = _critic()
    del half["pcont_h1_b"]
    critic = L.RcPolicyCritic(C.sizeof(L.RcPolicyCritic))
    keep = L._fill_arrays(critic, half, [k for k in L.CRITIC_KEYS if k in half])
    assert lib.rc_policy_load_critic(env._h, C.byref(critic)) == -1 and b"7 of the eight pcont_*" in lib.rc_last_error()
    assert call()[0] == 0                                                                  # (a refused load leaves the loaded critic alone)
    env.load_critic(None)
    assert not env.policy_has_value_head and b"no value head" in call()[1]
    env.load_critic(_critic())
    env.load_policy(weights("treitlstrasse_20210220"))                                     # (drops the critic; has no reward head)
    assert not env.policy_has_value_head and b"no value head" in call()[1]
    env.load_critic(_critic())
    rc, msg = call()
    assert rc == -1 and b"no reward head" in msg
    assert call(returns=None, value=ptr["a"], weight=ptr["b"])[0] == 0
    both = dict(weights("austria"))
    both.update(_critic())
    env.load_policy(both)                                                                  # (value_* in the mapping: loaded with the policy)
    assert env.policy_has_value_head and env.policy_has_pcont_head and call()[0] == 0
    env.unload_policy()
    assert not env.policy_has_value_head and b"no policy loaded" in call()[1]
    torch.cuda.synchronize()
    env.close()


def test_behaviour_terms_are_the_specs():
    """world_model.behaviour_terms on a batch of 4 windows x 6 steps: the posterior features of PolicyObserveSpec in `sample`,
    without each window's last step (a pcont head is loaded), as the starts of PolicyReturnsSpec; returns, weight and value bit
    for bit, the two losses assembled in NumPy at float64 within rtol 1e-6."""
    import torch
    from racing_dreamer_amd.world_model import behaviour_terms
    b, t, h = 4, 6, 15
    scan = _recorded_inputs(b * t, seed=3)[0].reshape(b, t, 1080)
    rec = np.random.default_rng(4).uniform(-1, 1, (b, t, 2)).astype(np.float32)
    env = _env("austria", 2)
    got = behaviour_terms(env, dict(lidar=torch.from_numpy(scan), action=torch.from_numpy(rec)), horizon=h, lambda_=0.95, seed=13)
    feat = PolicyObserveSpec(weights("austria")).observe(scan, rec, mode="sample", seed=13)["feature"][:, :-1].reshape(-1, 230)
    want = _spec("austria").returns(feat, horizon=h, mode="sample", seed=13, lambda_=0.95, discount=0.99)
    host = _cpu({k: got[k] for k in ("returns", "weight", "value")})
    assert host["returns"].shape == (b * (t - 1), h - 1)
    _same(host, want, "behaviour")
    w, r, v = (want[k].astype(np.float64) for k in ("weight", "returns", "value"))
    actor = -(w * r).mean()
    value = -(w * (-0.5 * (v[:, :-1] - r) ** 2 - 0.5 * math.log(2.0 * math.pi))).mean()
    assert math.isclose(float(got["actor_loss"]), actor, rel_tol=1e-6) and math.isclose(float(got["value_loss"]), value, rel_tol=1e-6)
    env.close()


def test_dream_shooting_act_with_a_bootstrap():
    """On a live env: the candidate with the highest return + discount^H value(final feature) - assembled here in NumPy from
    dream_ahead's and policy_value's outputs - is the one whose first action action_in holds afterwards; without the flag the
    choice is the plain return's."""
    import torch
    from racing_dreamer_amd.planning import dream_shooting_act, shooting_candidates
    n, k, h, disc = 40, 16, 6, 0.9
    env = _env("austria", n)
    env.reset(mode="random", seed=3)
    _drive(env, 4)
    env.policy_act()
    cand = shooting_candidates(env, k, h, hold=2, seed=9)
    got = env.dream_ahead(cand.reshape(n, k, h, 2), discount=disc, outputs=("return", "final_feature"))
    value = _cpu(env.policy_value(got["final_feature"]))["value"]
    got = _cpu(got)
    score = got["return"] + np.float32(disc ** h) * value
    best = score.argmax(axis=1)
    plain = _cpu(env.dream_ahead(cand.reshape(n, k, h, 2)))["return"].argmax(axis=1)
    assert np.any(best != plain)
    out = dream_shooting_act(env, candidates=k, horizon=h, hold=2, seed=9, bootstrap=True, discount=disc)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), cand.cpu().numpy()[np.arange(n), best, 0].reshape(n, 1, 2))
    env.close()
