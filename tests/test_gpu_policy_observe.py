"""rc_policy_observe / policy_observe against its binary32 specification (tests/policy_observe_spec.c), bit for bit on every output:
partial and several workgroups, lengths and contexts, both modes, three kinds of checkpoint; against the device's own policy_act
and policy_imagine; the longest sequence; that nothing but the outputs changes; shards; replay windows and mixed tracks; the
world_model helpers; the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

from policy_observe_spec import PolicyObserveSpec
from test_golden_policy import weights

pytestmark = pytest.mark.gpu
OUTPUTS = ("feature", "post_mean", "post_std", "prior_mean", "prior_std", "kl", "state")
OBSERVED_ONLY = ("post_mean", "post_std", "kl")          # written for t < context
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def _spec(name):
    return PolicyObserveSpec(weights(name))


@functools.lru_cache(maxsize=None)
def _recorded(steps=28):
    """An 8-env x 2-car run on austria under policy_act (the austria checkpoint, random starts, a time limit of 9 agent steps: a
    reset inside): per car and step the scan and the raw previous action as the reference's episodes store it - the action that
    led to the scan, 0 on the first row after a reset.  Returns (scan [16, steps, 1080], action [16, steps, 2], fresh [16, steps])."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 8, 2, auto_reset=True, remap_actions=True, terminate_on_collision=True, time_limit_steps=9)
    env.reset(mode="random", seed=5)
    env.load_policy(weights("austria"))
    n = env.n_cars
    scans, acts, fresh = [], [], []
    for _ in range(steps):
        torch.cuda.synchronize()
        fr = env.views["fresh"].view(n).cpu().numpy() != 0
        scans.append(env.views["lidar"].view(n, 1080).cpu().numpy().copy())
        acts.append(np.where(fr[:, None], 0.0, env.policy_state[:, 230:].cpu().numpy()).astype(np.float32))
        fresh.append(fr)
        env.policy_act()
        env.step(None, repeat=4)
    env.close()
    scan, act, fresh = np.stack(scans, 1), np.stack(acts, 1), np.stack(fresh, 1)
    assert fresh[:, 1:].any() and np.abs(act).max() > 0.01
    return scan, act, fresh


def _windows(rows, length):
    """`rows` windows of `length` steps of the recorded run: window q is car q % 16 from step q // 16 on."""
    scan, act, _ = _recorded()
    q = np.arange(rows)
    car, s0 = q % 16, q // 16
    assert s0.max() + length <= scan.shape[1]
    idx = s0[:, None] + np.arange(length)
    return np.ascontiguousarray(scan[car[:, None], idx]), np.ascontiguousarray(act[car[:, None], idx])


@functools.lru_cache(maxsize=None)
def _env(name, track="austria", n=4, cars=1):
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv(track, n, cars, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=1)
    env.load_policy(weights(name))
    return env


def _cpu(d):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(got, want, context, what):
    for k, g in got.items():
        w = want[k]
        if k in OBSERVED_ONLY:
            g, w = g[:, :context], w[:, :context]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)), (what, k, float(np.nanmax(np.abs(g - w))))


CASES = [("austria", 1, 1, 1, "mean"), ("austria", 33, 7, 7, "mean"), ("austria", 67, 7, 3, "mean"), ("austria", 67, 7, 3, "sample"),
         ("treitlstrasse", 33, 7, 1, "sample"), ("treitlstrasse", 67, 7, 7, "sample"), ("treitlstrasse", 1, 7, 3, "mean"),
         ("treitlstrasse_occupancy", 33, 7, 3, "mean"), ("treitlstrasse_occupancy", 1, 1, 1, "sample"), ("treitlstrasse_occupancy", 67, 7, 1, "mean")]


@pytest.mark.parametrize("name, rows, length, context, mode", CASES)
def test_the_device_is_the_spec_bit_for_bit(name, rows, length, context, mode):
    """Recorded windows (1 row: a partial workgroup; 33: a full one and one row; 67: three, the last partial), a start state
    taken from the recording, every output at once - with `reward` where the checkpoint has a head: each equals the spec as bit
    patterns, `post_*` and `kl` for t < context."""
    import torch
    spec_pol, env = _spec(name), _env(name)
    assert spec_pol.has_head == (name != "treitlstrasse_occupancy") == env.policy_has_reward_head
    scan, act = _windows(rows, length)
    state = np.random.default_rng(rows).normal(0.0, 0.3, (rows, 232)).astype(np.float32)
    outputs = OUTPUTS + (("reward",) if spec_pol.has_head else ())
    got = _cpu(env.policy_observe(torch.from_numpy(scan), torch.from_numpy(act), context=context, mode=mode, seed=77, state=torch.from_numpy(state),
                                  row_offset=5, outputs=outputs))
    want = spec_pol.observe(scan, act, context=context, mode=mode, seed=77, state=state, row_offset=5)
    assert set(got) == set(outputs)
    _same(got, want, context, (name, rows, length, context, mode))
    assert np.all(np.isfinite(want["kl"][:, :context])) and want["kl"][:, :context].min() > -1e-4 and want["feature"].std() > 0.01


def test_observe_is_the_devices_own_agent_and_hands_over_to_imagination():
    """33 cars, 7 closed-loop policy_act steps from a reset in `mean` mode, recording the scan, the raw previous action and the
    policy_state after each step: policy_observe from zeros gives feature[:, t] = that snapshot's stoch | deter.  With context 4,
    steps 4 .. 6 equal policy_imagine(actions=action[:, 4:]) from `state` of a 4-step observe written into policy_state."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n, T, K = 33, 7, 4
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True, terminate_on_collision=False)      # (no reset inside the 7 steps)
    env.reset(mode="random", seed=9)
    env.load_policy(weights("austria"))
    scans, acts, snaps = [], [], []
    for k in range(T):
        scans.append(env.views["lidar"].view(n, 1080).clone())
        fresh = env.views["fresh"].view(n, 1) != 0
        assert bool(fresh.all()) == (k == 0) and bool(fresh.any()) == (k == 0)
        acts.append(torch.where(fresh, torch.zeros_like(env.policy_state[:, 230:]), env.policy_state[:, 230:]))
        env.policy_act()
        snaps.append(env.policy_state.clone())
        env.step(None, repeat=4)
    scan, act = torch.stack(scans, 1), torch.stack(acts, 1)
    got = env.policy_observe(scan, act, outputs=("feature", "state"))
    for t in range(T):
        assert torch.equal(got["feature"][:, t], snaps[t][:, :230]), t
    assert torch.equal(got["state"][:, :230], snaps[-1][:, :230]) and torch.equal(got["state"][:, 230:], act[:, -1])
    mixed = env.policy_observe(scan, act, context=K, outputs=("feature", "reward"))
    head = env.policy_observe(scan[:, :K], act[:, :K], outputs=("feature", "state"))
    assert torch.equal(mixed["feature"][:, :K], head["feature"]) and torch.equal(head["feature"], got["feature"][:, :K])
    env.policy_state.copy_(head["state"])
    dream = env.policy_imagine(T - K, "mean", actions=act[:, K:].contiguous(), features=True)
    assert torch.equal(dream["feature"], mixed["feature"][:, K:]) and torch.equal(dream["reward"], mixed["reward"][:, K:])
    assert float(mixed["feature"][:, K:].std()) > 0.01
    env.close()


def test_the_longest_sequence():
    """T = 64 (the recording repeated), 33 rows, context 40, `sample`: every output equals the spec."""
    import torch
    scan, act = _windows(33, 16)
    scan, act = np.tile(scan, (1, 4, 1)), np.tile(act, (1, 4, 1))
    env = _env("austria")
    got = _cpu(env.policy_observe(torch.from_numpy(scan), torch.from_numpy(act), context=40, mode="sample", seed=3, outputs=OUTPUTS + ("reward",)))
    _same(got, _spec("austria").observe(scan, act, context=40, mode="sample", seed=3), 40, "T = 64")


def test_nothing_else_changes_and_only_what_was_asked_for_is_written():
    """policy_state, action_in and the arena are byte for byte what they were; the result holds the requested names only; into
    `out` tensors filled with a sentinel, post_* and kl keep it at t >= context and every other entry is written."""
    import torch
    env = _env("austria")
    scan, act = (torch.from_numpy(x).to(env.device) for x in _windows(33, 7))
    before = [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes()]
    assert set(env.policy_observe(scan, act)) == {"feature"}
    assert set(env.policy_observe(scan, act, outputs=("kl",))) == {"kl"}
    shapes = dict(feature=(33, 7, 230), post_mean=(33, 7, 30), post_std=(33, 7, 30), prior_mean=(33, 7, 30), prior_std=(33, 7, 30), kl=(33, 7),
                  reward=(33, 7), state=(33, 232))
    out = {k: torch.full(s, SENTINEL, device=env.device) for k, s in shapes.items()}
    got = env.policy_observe(scan, act, context=3, mode="sample", seed=1, outputs=tuple(shapes), out=out)
    assert all(got[k] is out[k] for k in shapes)
    got = _cpu(got)
    for k, g in got.items():
        if k in OBSERVED_ONLY:
            assert np.all(g[:, 3:] == SENTINEL) and not np.any(g[:, :3] == SENTINEL), k
        else:
            assert not np.any(g == SENTINEL), k
    torch.cuda.synchronize()
    assert before == [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes()]


def test_two_shards_with_their_row_offset_are_the_whole_batch():
    import torch
    env = _env("austria")
    scan, act = (torch.from_numpy(x).to(env.device) for x in _windows(67, 7))
    outputs = OUTPUTS + ("reward",)
    kw = dict(context=3, mode="sample", outputs=outputs)
    full = _cpu(env.policy_observe(scan, act, seed=11, row_offset=2 ** 32 - 20, **kw))
    again = _cpu(env.policy_observe(scan, act, seed=11, row_offset=2 ** 32 - 20, **kw))
    other = _cpu(env.policy_observe(scan, act, seed=12, row_offset=2 ** 32 - 20, **kw))
    for lo, hi in ((0, 30), (30, 67)):
        part = _cpu(env.policy_observe(scan[lo:hi], act[lo:hi], seed=11, row_offset=2 ** 32 - 20 + lo, **kw))
        for k in outputs:
            sl = (slice(lo, hi), slice(0, 3)) if k in OBSERVED_ONLY else (slice(lo, hi),)
            psl = (slice(None), slice(0, 3)) if k in OBSERVED_ONLY else (slice(None),)
            assert part[k][psl].tobytes() == full[k][sl].tobytes(), k
    for k in outputs:
        sl = (slice(None), slice(0, 3)) if k in OBSERVED_ONLY else (slice(None),)
        assert again[k][sl].tobytes() == full[k][sl].tobytes(), k
    assert not np.array_equal(other["feature"][:, :, :30], full["feature"][:, :, :30])
    assert np.array_equal(other["prior_mean"][:, 0], full["prior_mean"][:, 0])          # (the first prior sees no draw)
    want = _spec("austria").observe(scan.cpu().numpy(), act.cpu().numpy(), context=3, mode="sample", seed=11, row_offset=2 ** 32 - 20)
    _same(full, want, 3, "rows across 2^32")


def test_replay_windows_keep_their_leading_dimensions_and_mixed_tracks_forward():
    """TrajectoryRing.sample(6, 10) of a device ring filled under policy_act, as [2, 3, 10, ...]: the outputs keep [2, 3] and equal
    the spec on the same windows; a MixedTrackEnv returns the same bits."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    from racing_dreamer_amd.replay import TrajectoryRing
    env = BatchedRaceEnv("austria", 8, 2, auto_reset=True, remap_actions=True, action_repeat=4)
    env.load_policy(weights("austria"))
    ring = TrajectoryRing(env, capacity=16)
    ring.reset(mode="random", seed=3)
    for _ in range(14):
        env.policy_act()
        ring.step(None)
    batch = ring.sample(6, 10, generator=torch.Generator(device="cuda").manual_seed(1))
    lidar, action = batch["lidar"], batch["action"]
    assert lidar.shape == (6, 10, 1080) and action.shape == (6, 10, 2) and float(action.abs().max()) <= 1.0
    got = env.policy_observe(lidar.view(2, 3, 10, 1080), action.view(2, 3, 10, 2), context=5, outputs=("feature", "kl", "reward", "state"))
    assert got["feature"].shape == (2, 3, 10, 230) and got["kl"].shape == (2, 3, 10) and got["reward"].shape == (2, 3, 10) and got["state"].shape == (2, 3, 232)
    want = _spec("austria").observe(lidar.cpu().numpy(), action.cpu().numpy(), context=5)
    flat = {k: v.reshape((6,) + v.shape[2:]) for k, v in _cpu(got).items()}
    _same(flat, want, 5, "ring")
    mixed = MixedTrackEnv(["columbia", "austria"], [3, 2], auto_reset=True, remap_actions=True)
    mixed.reset(mode="random", seed=4)
    mixed.load_policy(weights("austria"))
    fwd = mixed.policy_observe(lidar.view(2, 3, 10, 1080), action.view(2, 3, 10, 2), context=5, outputs=("feature", "kl", "reward", "state"))
    for k in got:
        a, b = got[k], fwd[k]
        if k == "kl":
            a, b = a[..., :5], b[..., :5]
        assert a.shape == b.shape and torch.equal(a, b), k
    mixed.close(); env.close()


def test_the_open_loop_summary_and_the_model_terms():
    """open_loop_summary on the occupancy checkpoint: `model` is policy_decode's image of policy_observe's features, `error` takes
    values in {0, 1/2, 1}, the mismatch count is the number of differing pixels.  model_terms: div and the reward log-likelihood
    equal the same formulas in float64 on the spec's outputs to within the float32 reduction error derived below."""
    import torch
    from racing_dreamer_amd import world_model
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("treitlstrasse_v2", 6, 1, obs_type="lidar_occupancy", auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=3)
    env.load_policy(weights("treitlstrasse_occupancy"))
    rec = {k: [] for k in ("lidar", "action", "lidar_occupancy")}
    for _ in range(8):
        fresh = env.views["fresh"].view(6, 1) != 0
        rec["lidar"].append(env.views["lidar"].view(6, 1080).clone())
        rec["lidar_occupancy"].append(env.views["lidar_occupancy"].view(6, 64, 64, 1).clone())
        rec["action"].append(torch.where(fresh, torch.zeros_like(env.policy_state[:, 230:]), env.policy_state[:, 230:]))
        env.policy_act()
        env.step(None, repeat=4)
    batch = {k: torch.stack(v, 1) for k, v in rec.items()}
    s = world_model.open_loop_summary(env, batch, context=5)
    feat = env.policy_observe(batch["lidar"], batch["action"], context=5)["feature"]
    image = env.policy_decode(features=feat)["image"]
    assert s["model"].shape == (6, 8, 64, 64) and torch.equal(s["model"], image.to(s["model"].dtype))
    assert torch.equal(s["truth"], batch["lidar_occupancy"].view(6, 8, 64, 64).to(s["truth"].dtype))
    assert set(np.unique(s["error"].cpu().numpy())) <= {0.0, 0.5, 1.0} and torch.equal(s["error"], (s["model"] - s["truth"] + 1) / 2)
    assert torch.equal(s["mismatch"], (s["model"] != s["truth"]).flatten(2).sum(2)) and 0 < int(s["mismatch"].max()) < 4096
    terms = world_model.model_terms(env, batch)
    assert set(terms) == {"div"}                                      # (this checkpoint ships no reward head)
    env.close()
    # a checkpoint with a head: B T = 33 x 7 values per mean.  A float32 mean of m values of magnitude <= v, summed in any order,
    # is off by at most (m - 1) 2^-24 v (+ one rounding of the division); the log-likelihood's terms -(r - p)^2 / 2 - log(2 pi) / 2
    # add three roundings each.  With m = 231: (m + 3) 2^-24 max|term| bounds both.
    env = _env("austria")
    scan, act = _windows(33, 7)
    reward = np.random.default_rng(0).normal(0.0, 0.05, (33, 7)).astype(np.float32)
    batch = dict(lidar=torch.from_numpy(scan).to(env.device), action=torch.from_numpy(act).to(env.device), reward=torch.from_numpy(reward).to(env.device))
    terms = {k: float(v) for k, v in world_model.model_terms(env, batch).items()}
    want = _spec("austria").observe(scan, act)
    kl64 = want["kl"].astype(np.float64)
    ll64 = -0.5 * (reward.astype(np.float64) - want["reward"].astype(np.float64)) ** 2 - 0.5 * np.log(2 * np.pi)
    m = kl64.size
    assert set(terms) == {"div", "reward_loglik"}
    for got, ref in ((terms["div"], kl64), (terms["reward_loglik"], ll64)):
        bound = (m + 3) * 2.0 ** -24 * np.abs(ref).max()
        print(f"model term {got:.8g} against {ref.mean():.8g}, bound {bound:.3g}")
        assert abs(got - ref.mean()) <= bound


def test_refusals():
    """Every RC_ERR_INVALID of rc_policy_observe names its cause, and the handle still works afterwards."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 4, 1, auto_reset=True, remap_actions=True)
    env.reset(mode="grid", seed=1)
    lib, rows, T = env._lib, 5, 4
    scan, act = (torch.from_numpy(x).to(env.device) for x in _windows(rows, T))
    buf = {k: torch.zeros(s, device=env.device) for k, s in (("features", (rows, T, 230)), ("reward", (rows, T)), ("kl", (rows, T)))}

    def call(**kw):
        a = L.RcPolicyObserveArgs(C.sizeof(L.RcPolicyObserveArgs), T, T, 0, rows, 0, 0, scan.data_ptr(), act.data_ptr())
        a.features = buf["features"].data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.rc_policy_observe(env._h, C.byref(a))
        return rc, lib.rc_last_error()

    rc, msg = call()
    assert rc == -1 and b"no policy loaded" in msg
    w = weights("austria")
    env.load_policy({k: w[k] for k in w.files if not k.startswith(("img2", "img3"))})
    rc, msg = call()
    assert rc == -1 and b"img2 / img3" in msg
    env.load_policy(w)
    assert call()[0] == 0
    for kw, text in ((dict(struct_size=8), b"struct_size"), (dict(rows=0), b"rows"), (dict(length=0), b"length"), (dict(length=65, context=65), b"length"),
                     (dict(context=0), b"context"), (dict(context=T + 1), b"context"), (dict(mode=2), b"unknown mode"), (dict(mode=-1), b"unknown mode"),
                     (dict(scan=None), b"scan is NULL"), (dict(actions=None), b"actions is NULL"), (dict(features=None), b"no output")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, kw
    assert call(features=None, kl=buf["kl"].data_ptr())[0] == 0 and call(reward=buf["reward"].data_ptr())[0] == 0
    env.load_policy({k: w[k] for k in w.files if not k.startswith("reward_")})
    rc, msg = call(reward=buf["reward"].data_ptr())
    assert rc == -1 and b"no reward head" in msg
    with pytest.raises(L.RacecarHipError):
        env.policy_observe(scan, act, outputs=("reward",))
    for bad in (dict(mode="deploy"), dict(context=0), dict(context=T + 1), dict(outputs=("stoch",))):
        with pytest.raises(ValueError):
            env.policy_observe(scan, act, **bad)
    with pytest.raises(ValueError):
        env.policy_observe(scan, act[:, :3])
    got = env.policy_observe(scan, act)["feature"]
    torch.cuda.synchronize()
    assert got.shape == (rows, T, 230) and bool(torch.isfinite(got).all())
    env.policy_act()
    env.step(None, repeat=4)
    torch.cuda.synchronize()
    env.close()
