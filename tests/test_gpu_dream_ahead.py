"""rc_policy_dream_ahead / dream_ahead against its binary32 specification (tests/policy_dream_spec.c), bit for bit: the two
checkpoints with a reward head, both modes, starts x candidates x horizons that reach every row mapping (one start alone, a start's
rows straddling two workgroups, several starts in one workgroup, hundreds of workgroups), both discounts; against the device's own
open-loop policy_imagine; from policy_observe's state and in shards; purity after a real run; slot masks, mixed tracks, shards by
first_env; the refusals; dream_shooting_act on a live env."""
import ctypes as C

import numpy as np
import pytest

from policy_dream_spec import PolicyDreamSpec
from test_golden_policy import weights
from test_gpu_policy_device import _recorded_inputs
from test_gpu_policy_imagine import _cpu, _drive

pytestmark = pytest.mark.gpu
MODES = ("mean", "sample")
WITH_HEAD = ("austria", "treitlstrasse")
ALL = ("return", "reward", "final_feature")
_cache = {}


def _spec(name):
    if name not in _cache:
        _cache[name] = PolicyDreamSpec(weights(name))
    return _cache[name]


def _latents(n):
    """[n, 232] recorded latents (97 distinct ones, scaled a little from one repeat to the next)."""
    if "latents" not in _cache:
        _cache["latents"] = _recorded_inputs(97, seed=3)[1]
    state = np.concatenate([_cache["latents"]] * -(-n // 97))[:n]
    return state * (1.0 + 0.001 * (np.arange(n) // 97))[:, None].astype(np.float32)


def _actions(s, k, h, seed=2):
    """[s, k, h, 2], a third of the entries beyond +-1."""
    return np.random.default_rng(seed).uniform(-1.5, 1.5, (s, k, h, 2)).astype(np.float32)


def _same(got, want, what, rows=slice(None)):
    for k, g in got.items():
        assert g[rows].tobytes() == want[k][rows].tobytes(), (what, k, float(np.abs(g[rows] - want[k][rows]).max()))


# (starts, candidates, horizon, discount): S in {1, 3, 33}, K in {1, 5, 32, 33}, H in {1, 2, 15} each reached; 1 x 33 and 33 x 1
# are one row above a multiple of 32 (33 candidates of one start straddle two workgroups), 3 x 5 puts three starts into one
# workgroup, 33 x 256 = 8 448 rows are 264 workgroups
CASES = ((1, 33, 15, 0.99), (3, 5, 2, 1.0), (33, 1, 1, 0.99), (3, 32, 2, 0.99), (33, 5, 1, 1.0), (33, 256, 2, 0.99))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", WITH_HEAD)
def test_one_call_is_the_spec_bit_for_bit(name, mode):
    """Recorded latents written into policy_state, one dream_ahead from them: return, reward and final_feature equal the spec in
    every row, a third of the actions beyond +-1."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    envs = {}
    for s, k, h, discount in CASES:
        state = _latents(s)
        if s not in envs:
            envs[s] = BatchedRaceEnv("austria", s, 1, auto_reset=True, remap_actions=True)
            envs[s].reset(mode="random", seed=1)
            envs[s].load_policy(weights(name))
            envs[s].policy_state.copy_(torch.from_numpy(state))
        acts = _actions(s, k, h, seed=s + k + h)
        got = _cpu(envs[s].dream_ahead(torch.from_numpy(acts), mode, seed=77, discount=discount, outputs=ALL))
        want = _spec(name).dream(state, acts, None, mode, seed=77, discount=discount)
        assert set(got) == set(ALL)
        _same(got, want, (name, mode, s, k, h))
        assert np.abs(got["return"]).max() > 1e-3 and np.abs(acts).max() > 1.0
        if h > 1 and discount < 1.0:
            assert not np.array_equal(got["return"], got["reward"].sum(-1, dtype=np.float32))
    for env in envs.values():
        env.close()


@pytest.mark.parametrize("name", WITH_HEAD)
def test_every_candidate_is_the_devices_own_open_loop_imagination(name):
    """For each k, reward[:, k] and final_feature[:, k] are byte for byte what policy_imagine(actions=actions[:, k]) returns from
    the same latents (`mean`), and with discount 1 the return is the sum of that reward in step order."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n, k, h = 35, 3, 15
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=1)
    env.load_policy(weights(name))
    env.policy_state.copy_(torch.from_numpy(_latents(n)))
    acts = torch.from_numpy(_actions(n, k, h, seed=9)).to(env.device)
    got = _cpu(env.dream_ahead(acts, outputs=ALL))
    for j in range(k):
        own = _cpu(env.policy_imagine(h, "mean", actions=acts[:, j], features=True))
        assert got["reward"][:, j].tobytes() == own["reward"].tobytes(), j
        assert got["final_feature"][:, j].tobytes() == np.ascontiguousarray(own["feature"][:, -1]).tobytes(), j
        acc = np.zeros(n, np.float32)
        for t in range(h):
            acc = acc + own["reward"][:, t]
        assert np.array_equal(got["return"][:, j], acc)
    env.close()


def test_from_an_observed_window_and_in_shards():
    """policy_observe over recorded windows gives `state`; dream_ahead(state=...) plans from its rows: the spec's answer from those
    rows, keyed by row_offset + row (also beyond 2^32).  Two shards with their row_offset reproduce the whole batch in `sample`.
    The env's own cars do not enter: it has two."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    rows, t_len, k, h = 7, 3, 5, 3
    scan = _recorded_inputs(rows * t_len, seed=3)[0].reshape(rows, t_len, 1080)
    rec = np.random.default_rng(4).uniform(-1, 1, (rows, t_len, 2)).astype(np.float32)
    env = BatchedRaceEnv("austria", 2, 1, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=1)
    env.load_policy(weights("austria"))
    state = env.policy_observe(torch.from_numpy(scan), torch.from_numpy(rec), outputs=("state",))["state"]
    assert state.shape == (rows, 232)
    host = _cpu({"s": state})["s"]
    assert np.abs(host[:, 30:230]).max() > 0.1
    acts = _actions(rows, k, h, seed=6)
    dev_acts = torch.from_numpy(acts).to(env.device)
    for mode in MODES:
        for offset in (0, (1 << 33) + 11):
            got = _cpu(env.dream_ahead(dev_acts, mode, seed=8, state=state, row_offset=offset, discount=0.99, outputs=ALL))
            want = _spec("austria").dream(host, acts, offset + np.arange(rows, dtype=np.uint64), mode, seed=8, discount=0.99)
            _same(got, want, (mode, offset))
    full = _cpu(env.dream_ahead(dev_acts, "sample", seed=8, state=state, outputs=ALL))
    for lo, hi in ((0, 2), (2, rows)):
        part = _cpu(env.dream_ahead(dev_acts[lo:hi], "sample", seed=8, state=state[lo:hi], row_offset=lo, outputs=ALL))
        assert all(part[key].tobytes() == full[key][lo:hi].tobytes() for key in full)
    wrong = _cpu(env.dream_ahead(dev_acts[2:], "sample", seed=8, state=state[2:], row_offset=0, outputs=("return",)))
    assert not np.array_equal(wrong["return"], full["return"][2:])
    env.close()


def test_after_a_real_run_with_resets_and_nothing_else_changes():
    """30 closed-loop agent steps on austria with resets (as the imagination's test drives them), then planning from the live
    latents in both modes: the spec's.  policy_state, action_in and the whole arena are byte for byte what they were, and a second
    call returns the same bytes."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n, k, h = 48, 3, 4
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True, terminate_on_collision=True, time_limit_steps=7)
    env.reset(mode="random", seed=5)
    env.load_policy(weights("austria"))
    _drive(env, 30)
    torch.cuda.synchronize()
    state = env.policy_state.cpu().numpy()
    assert np.abs(state[:, 30:230]).max() > 0.1
    acts = _actions(n, k, h, seed=3)
    dev_acts = torch.from_numpy(acts).to(env.device)
    before = [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes()]
    for mode in MODES:
        got = _cpu(env.dream_ahead(dev_acts, mode, seed=11, discount=0.99, outputs=ALL))
        _same(got, _spec("austria").dream(state, acts, None, mode, seed=11, discount=0.99), mode)
        again = _cpu(env.dream_ahead(dev_acts, mode, seed=11, discount=0.99, outputs=ALL))
        assert all(got[key].tobytes() == again[key].tobytes() for key in got)
    torch.cuda.synchronize()
    assert before == [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes()]
    env.close()


def test_slot_mask_leaves_the_other_rows_alone():
    """slots=(1, 2, 3) of four cars per env: slot A's rows keep the caller's sentinel (zero without `out`), the others equal the
    spec, whose draws carry the global car id."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n_envs, cars, k, h = 19, 4, 3, 2
    env = BatchedRaceEnv("austria", n_envs, cars, auto_reset=True, remap_actions=True)
    env.reset(mode="grid", seed=2)
    env.load_policy(weights("austria"))
    n = env.n_cars
    _drive(env, 3)
    torch.cuda.synchronize()
    state = env.policy_state.cpu().numpy()
    acts = _actions(n, k, h, seed=5)
    dev_acts = torch.from_numpy(acts).to(env.device)
    want = _spec("austria").dream(state, acts, None, "sample", seed=14)
    others = np.flatnonzero(np.arange(n) % cars != 0)
    out = {key: torch.full(shape, 7.0, device=env.device) for key, shape in (("return", (n, k)), ("reward", (n, k, h)), ("final_feature", (n, k, 230)))}
    got = env.dream_ahead(dev_acts, "sample", seed=14, slots=(1, 2, 3), outputs=ALL, out=out)
    assert all(got[key] is out[key] for key in out)
    got = _cpu(got)
    _same(got, want, "mask", others)
    assert all(np.all(g[::cars] == 7.0) for g in got.values())
    got = _cpu(env.dream_ahead(dev_acts, "sample", seed=14, slots=(1, 2, 3), outputs=ALL))
    _same(got, want, "mask, own tensors", others)
    assert all(np.all(g[::cars] == 0.0) for g in got.values())
    env.close()


def test_mixed_tracks_and_two_shards():
    """A MixedTrackEnv of three tracks writes its blocks' slices of one tensor per output: the spec's, keyed by global car ids; a
    given state goes through its first block.  Envs [0, 20) of two cars on one handle, and [0, 9) and [9, 20) on two handles with
    first_env offsets, give the same rows in `sample`."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    k, h = 5, 3
    env = MixedTrackEnv(["columbia", "austria", "barcelona"], [13, 20, 7], auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=4)
    env.load_policy(weights("austria"))
    _drive(env, 3)
    torch.cuda.synchronize()
    state = env.policy_state.cpu().numpy()
    acts = _actions(40, k, h, seed=7)
    got = _cpu(env.dream_ahead(torch.from_numpy(acts), "sample", seed=21, discount=0.99, outputs=ALL))
    want = _spec("austria").dream(state, acts, None, "sample", seed=21, discount=0.99)
    _same(got, want, "mixed")
    given = _cpu(env.dream_ahead(torch.from_numpy(acts), "sample", seed=21, state=torch.from_numpy(state), discount=0.99, outputs=ALL))
    _same(given, want, "mixed, given state")
    env.close()

    def run(n, first):
        env = BatchedRaceEnv("austria", n, 2, auto_reset=True, remap_actions=True, terminate_on_collision=True, time_limit_steps=4, first_env=first)
        env.reset(mode="random", seed=5)
        env.load_policy(weights("austria"))
        _drive(env, 6)
        a = torch.from_numpy(_actions(40, k, h, seed=8)[2 * first:2 * (first + n)])
        out = _cpu(env.dream_ahead(a, "sample", seed=31, outputs=ALL))
        env.close()
        return out
    full = run(20, 0)
    for lo, hi in ((0, 9), (9, 20)):
        part = run(hi - lo, lo)
        assert all(np.array_equal(part[key], full[key][2 * lo:2 * hi]) for key in full)


def test_refusals():
    """Every RC_ERR_INVALID of rc_policy_dream_ahead; `return` and `reward` need a head, final_feature alone works without one."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 4, 2, auto_reset=True)
    env.reset(mode="grid", seed=1)
    lib, n, k, h = env._lib, env.n_cars, 3, 15
    buf = {key: torch.zeros(shape, device=env.device) for key, shape in (("actions_in", (n, k, 64, 2)), ("ret", (n, k)), ("reward", (n, k, h)),
                                                                          ("final_feature", (n, k, 230)), ("state_in", (n, 232)))}

    def call(**kw):
        a = L.RcPolicyDreamAheadArgs(C.sizeof(L.RcPolicyDreamAheadArgs), h, 0, k, 3, 1.0, 0, 0, 0)
        a.actions_in, a.ret = buf["actions_in"].data_ptr(), buf["ret"].data_ptr()
        for key, v in kw.items():
            setattr(a, key, v)
        rc = lib.rc_policy_dream_ahead(env._h, C.byref(a))
        return rc, lib.rc_last_error()

    rc, msg = call()
    assert rc == -1 and b"no policy loaded" in msg
    w = {key: weights("austria")[key] for key in weights("austria").files if not key.startswith(("img2", "img3"))}
    env.load_policy(w)
    rc, msg = call()
    assert rc == -1 and b"img2 / img3" in msg
    env.load_policy(weights("austria"))
    assert call()[0] == 0
    state = buf["state_in"].data_ptr()
    for kw, text in ((dict(struct_size=8), b"struct_size"), (dict(horizon=0), b"horizon"), (dict(horizon=65), b"horizon"), (dict(candidates=0), b"candidates"),
                     (dict(candidates=1 << 30), b"not below 2^31"), (dict(mode=2), b"unknown mode"), (dict(mode=-1), b"unknown mode"),
                     (dict(discount=1.5), b"discount"), (dict(discount=-0.1), b"discount"), (dict(discount=float("nan")), b"discount"),
                     (dict(discount=float("inf")), b"discount"), (dict(actions_in=None), b"actions_in is NULL"), (dict(ret=None), b"no output"),
                     (dict(state_in=state, starts=n), b"slot mask"), (dict(state_in=state, slot_mask=0, starts=0), b"starts"),
                     (dict(state_in=state, slot_mask=0, starts=1 << 40), b"not below 2^31"),
                     (dict(slot_mask=0), b"mask is empty"), (dict(slot_mask=4), b"beyond cars_per_env")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    assert call(horizon=64, discount=0.0, slot_mask=2)[0] == 0
    assert call(state_in=state, slot_mask=0, starts=n, reward=buf["reward"].data_ptr(), final_feature=buf["final_feature"].data_ptr())[0] == 0
    acts = torch.zeros((n, k, h, 2), device=env.device)
    for bad in (dict(mode="deploy"), dict(discount=1.01), dict(outputs=("value",)), dict(state=buf["state_in"][:2]), dict(state=buf["state_in"][:, :230])):
        with pytest.raises(ValueError):
            env.dream_ahead(acts, **bad)
    with pytest.raises(ValueError):
        env.dream_ahead(torch.zeros(n, k, 65, 2))
    with pytest.raises(ValueError):
        env.dream_ahead(acts[:, :0])
    with pytest.raises(L.RacecarHipError, match="slot mask"):
        env.dream_ahead(acts, state=buf["state_in"], slots=(0,))
    # the checkpoint without a reward head: no return, no reward; the final feature alone works
    env.load_policy(weights("treitlstrasse_20210220"))
    assert not env.policy_has_reward_head
    for field in ("ret", "reward"):
        rc, msg = call(**{"ret": None, field: buf[field].data_ptr()})
        assert rc == -1 and b"no reward head" in msg
    with pytest.raises(L.RacecarHipError, match="no reward head"):
        env.dream_ahead(acts)
    feat = env.dream_ahead(acts, outputs=("final_feature",))
    assert set(feat) == {"final_feature"} and feat["final_feature"].shape == (n, k, 230)
    env.unload_policy()
    assert b"no policy loaded" in call()[1]
    torch.cuda.synchronize()
    env.close()


def test_the_head_less_checkpoints_final_feature_is_the_spec():
    """treitlstrasse_20210220 has no reward head: final_feature alone runs the prior's layers only and equals the spec."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    s, k, h = 3, 5, 2
    state, acts = _latents(s), _actions(s, k, h, seed=12)
    env = BatchedRaceEnv("austria", s, 1, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=1)
    env.load_policy(weights("treitlstrasse_20210220"))
    env.policy_state.copy_(torch.from_numpy(state))
    for mode in MODES:
        got = _cpu(env.dream_ahead(torch.from_numpy(acts), mode, seed=3, outputs=("final_feature",)))
        want = _spec("treitlstrasse_20210220").dream(state, acts, None, mode, seed=3)
        assert got["final_feature"].tobytes() == want["final_feature"].tobytes(), mode
    env.close()


def test_dream_shooting_act_writes_the_best_candidates_first_action():
    """On a live env: the first action of the candidate with the highest imagined return - computed here from dream_ahead's
    returns of the same candidates - is what action_in holds afterwards, for every car."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.planning import dream_shooting_act, shooting_candidates
    n, k, h = 40, 16, 6
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=3)
    env.load_policy(weights("austria"))
    _drive(env, 4)
    env.policy_act()
    cand = shooting_candidates(env, k, h, hold=2, seed=9)                               # [n, k, h, 1, 2]; candidate 0 = action_in
    ret = _cpu(env.dream_ahead(cand.reshape(n, k, h, 2)))["return"]
    best = ret.argmax(axis=1)                                                           # (numpy: the first among equals)
    assert len(set(best.tolist())) > 1
    out = dream_shooting_act(env, candidates=k, horizon=h, hold=2, seed=9)
    assert out is env.views["action_in"]
    torch.cuda.synchronize()
    want = cand.cpu().numpy()[np.arange(n), best, 0].reshape(n, 1, 2)
    assert np.array_equal(out.cpu().numpy(), want)
    env.close()
