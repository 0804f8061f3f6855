"""The track set on the MI355X (include/racecar_hip.h, rc_set_track_set / rc_set_next_track / rc_track_ids): every output and the
per-env track against the test-side restatement (tests/track_set_oracle.py) bit for bit, the equivalences with what exists
(a plain handle, MixedTrackEnv, sharding) and the refusals."""
import ctypes as C

import numpy as np
import pytest

from dr_oracle import DROracleEnv
from helpers import compare_outputs
from oracle import racecar_oracle as ro
from track_set_oracle import make_track_set_oracle

pytestmark = pytest.mark.gpu

TRACKS = ("columbia", "austria", "barcelona")          # barcelona: the render's unpadded, clamped bitmap
WIDE_LO = (0.168, 2.0, 0.4, 3.0, 0.02)
WIDE_HI = (0.294, 8.0, 1.6, 8.0, 0.05)
RC_ERR_INVALID = -1                               # include/racecar_hip.h


def _load(names):
    from racing_dreamer_amd.track_assets import load_track
    return [load_track(n) for n in names]


def _arena(env):
    import torch
    torch.cuda.synchronize()
    return env._arena_view.clone()


def _restatement_rollout(order, obs, dr, n):
    """Three tracks, random_ball with 2 cars, auto-reset with a 25-step time limit (every env switches about a dozen times in
    300 steps): every output and track_id after every step; vehicle randomization and LiDAR noise on where `dr`."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    tracks, A, steps = _load(TRACKS), 2, 300
    kw = dict(auto_reset=True, time_limit_steps=25)
    env = BatchedRaceEnv.with_track_set(tracks, n, A, order=order, seed=(5 << 32) | 3, obs_type=obs, **kw)
    ora = make_track_set_oracle(tracks, order=order, seed=(5 << 32) | 3, base=DROracleEnv, num_envs=n, cars_per_env=A,
                                render_occupancy=obs == "lidar_occupancy", **kw)
    assert env.track_names == list(TRACKS) and env.track_id.dtype == torch.int32 and env.track_id.shape == (n,)
    if dr:
        env.set_vehicle_randomization(WIDE_LO, WIDE_HI, seed=21)
        ora.set_vehicle_randomization(WIDE_LO, WIDE_HI, seed=21)
        env.set_lidar_noise(0.2, 0.03, 8)
        ora.set_lidar_noise(0.2, 0.03, 8)
    dv, ov = env.reset(mode="random_ball", seed=13), ora.reset(mode=2, seed=13)
    switches = 0
    last = ora.track.copy()
    for k in range(steps + 1):
        if k:
            act = ro.random_actions(31, k, n * A)
            act[:, 0] = np.abs(act[:, 0])
            dv = env.step(torch.from_numpy(act).cuda())
            ov = ora.step(act)
            switches += int((ora.track != last).sum())
            last = ora.track.copy()
        compare_outputs(dv, ov, n, A, f"{order} {obs} step {k}")
        assert np.array_equal(env.track_id.cpu().numpy(), ov["track_id"]), k
        if dr:
            assert np.array_equal(env.vehicle_params.cpu().numpy(), ora.vp), k
    assert switches >= 5 * n
    assert env.scan_kernel_name().startswith("rc_raycast_ts_kernel<2,")
    env.close()


@pytest.mark.parametrize("order,obs,dr", [("sequential", "lidar_occupancy", False), ("random", "lidar", True),
                                          ("random", "lidar_occupancy", True)])
def test_track_set_equals_the_restatement(order, obs, dr):
    """(24 envs: the NumPy oracle beside them keeps the file inside `-m gpu`'s budget)"""
    _restatement_rollout(order, obs, dr, 24)


@pytest.mark.gpu_slow
@pytest.mark.parametrize("order", ["sequential", "random"])
def test_track_set_equals_the_restatement_at_a_few_hundred_envs(order):
    _restatement_rollout(order, "lidar_occupancy", True, 256)


def test_one_track_set_equals_a_plain_handle():
    """A set of one track against a plain handle on that track: the whole arena after every step."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    (t,) = _load(["barcelona"])
    n, kw = 512, dict(obs_type="lidar_occupancy", auto_reset=True, time_limit_steps=20)
    plain = BatchedRaceEnv(t, n, 1, **kw)
    ts = BatchedRaceEnv.with_track_set([t], n, 1, **kw)
    plain.reset(mode="random", seed=2)
    ts.reset(mode="random", seed=2)
    import torch
    assert torch.equal(_arena(plain), _arena(ts))
    for k in range(120):
        plain.step_random(seed=4, step=k)
        ts.step_random(seed=4, step=k)
        assert torch.equal(_arena(plain), _arena(ts)), k
    assert (ts.track_id == 0).all()
    plain.close(); ts.close()


def test_manual_set_at_the_initial_split_equals_mixed_track_env():
    """order manual with next_track = the contiguous initial assignment: every env stays on its block's track, as MixedTrackEnv's
    blocks do; both key resets by first_env + e."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    tracks, counts = _load(TRACKS), [342, 341, 341]
    n, kw = sum(counts), dict(obs_type="lidar_occupancy", auto_reset=True, time_limit_steps=15)
    mixed = MixedTrackEnv(tracks, counts, **kw)
    ts = BatchedRaceEnv.with_track_set(tracks, n, 1, order="manual", **kw)
    init = ts.track_id.clone()
    assert init.tolist() == sum(([k] * c for k, c in enumerate(counts)), [])
    ts.set_next_track(init)
    mixed.reset(mode="random", seed=6)
    ts.reset(mode="random", seed=6)
    for k in range(80):
        if k:
            mixed.step_random(seed=1, step=k)
            ts.step_random(seed=1, step=k)
        torch.cuda.synchronize()
        for name, view in mixed.views.items():
            if name != "action_in":
                assert torch.equal(view, ts.views[name]), (k, name)
    assert torch.equal(ts.track_id, init) and torch.equal(mixed.track_id, init)
    mixed.close(); ts.close()


def test_two_shards_reproduce_the_full_job():
    """Random order: shards first_env 0 and B/2 with the full job's initial tracks see its tracks and outputs."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    tracks, B = _load(TRACKS), 256
    kw = dict(obs_type="lidar_occupancy", auto_reset=True, time_limit_steps=12, order="random", seed=77)
    full = BatchedRaceEnv.with_track_set(tracks, B, 1, **kw)
    init = full.track_id.clone()
    shards = [BatchedRaceEnv.with_track_set(tracks, B // 2, 1, first_env=h * B // 2, initial=init[h * B // 2:(h + 1) * B // 2], **kw)
              for h in range(2)]
    for e in [full, *shards]:
        e.reset(mode="random", seed=3)
    for k in range(60):
        full.step_random(seed=9, step=k)
        for s in shards:
            s.step_random(seed=9, step=k)                  # (random actions by global car id)
        torch.cuda.synchronize()
        for h, s in enumerate(shards):
            sl = slice(h * B // 2, (h + 1) * B // 2)
            assert torch.equal(full.track_id[sl], s.track_id), k
            for name in ("lidar", "pose", "reward", "done", "lidar_occupancy"):
                assert torch.equal(full.views[name][sl], s.views[name]), (k, name)
    assert not torch.equal(full.track_id, init)
    for e in [full, *shards]:
        e.close()


def test_refusals_and_off():
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    tracks = _load(TRACKS[:2])
    with pytest.raises(L.RacecarHipError):               # the exact render holds per-handle scratch of one source frame
        BatchedRaceEnv.with_track_set(tracks, 8, 1, obs_type="lidar_occupancy_reference")
    env = BatchedRaceEnv.with_track_set(tracks, 64, 1, obs_type="lidar_occupancy", auto_reset=True)
    env.reset(mode="random", seed=1)
    lib = env._lib
    handles = (C.c_void_p * 1)(env._h)
    assert lib.rc_step_group(handles, 1, None, 1) == RC_ERR_INVALID           # no track-set handle in a group
    assert lib.rc_set_pose(env._h, np.zeros((64, 3), np.float32).ctypes.data) == RC_ERR_INVALID
    env.debug_set("scan_bounded", 1)                                             # the bounded validation build
    assert lib.rc_step(env._h, None, 1) == RC_ERR_INVALID
    env.debug_set("scan_bounded", 0)
    env.step_random(seed=0, step=0)
    # bad arguments
    h = (C.c_void_p * 9)(*([env._h] * 9))
    assert lib.rc_set_track_set(env._h, h, 9, 0, None, None, C.c_uint64(0)) == RC_ERR_INVALID
    assert lib.rc_set_track_set(env._h, h, 2, 3, None, None, C.c_uint64(0)) == RC_ERR_INVALID
    w = np.float32([1.0, 0.0])
    assert lib.rc_set_track_set(env._h, h, 2, 1, w.ctypes.data, None, C.c_uint64(0)) == RC_ERR_INVALID
    bad = torch.full((64,), 2, dtype=torch.int32, device="cuda")
    assert lib.rc_set_track_set(env._h, h, 2, 0, None, C.c_void_p(bad.data_ptr()), C.c_uint64(0)) == RC_ERR_INVALID
    assert env.scan_kernel_name().startswith("rc_raycast_ts_kernel")
    # n = 0: the production kernels again
    env.clear_track_set()
    assert env.scan_kernel_name() == "rc_raycast_car_kernel<1, true, false>" or env.scan_kernel_name().startswith("rc_raycast_car_kernel<1,")
    env.reset(mode="random", seed=1)
    env.step_random(seed=0, step=1)
    torch.cuda.synchronize()
    env.close()
