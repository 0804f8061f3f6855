"""The step's entry paths, bit for bit (EXPERIMENTS.md 0000.3).

The scan (racecar_scan.h: scan_args_at_entry, scan_one_wave_per_car): the one-wave-per-car build has `split` and `part` as
constants and every build fetches its arguments in one batch - scans from set poses at the batch sizes that pick each build, with
and without the track-order array, against the plain-C oracle.

The dynamics (racecar_kernels.hip: dynamics_env, prepare_reset / apply_reset): the cases that a reordering of its loads has to
keep - a reset in every wave, with given and with drawn actions; no reset at all, with envs that are already done; vehicle
randomization and a track set together.  (The reordering itself, tools/experiments/step_entry_dynamics.patch, passes them and
did not merge: it was not faster by the rule.  The cases with four cars take a quarter of a minute each, nearly all of it the
NumPy oracle beside 768 cars.)
"""
import numpy as np
import pytest

from helpers import EXACT_FLOAT, EXACT_INT, compare_outputs, make_oracle
from oracle import racecar_oracle as ro

pytestmark = pytest.mark.gpu

ACT_SEED = (7 << 32) | 19


def _rollout_both_ways(cars, repeat, auto_reset, mode, num_envs=192, steps=8, track_name="columbia"):
    """One oracle rollout, two device rollouts compared with it after every step: the actions given (rc_step) and the same
    actions drawn inside the dynamics kernel (rc_step_random).  Returns the number of finished (env, step)s."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    from racing_dreamer_amd import spec
    track = load_track(track_name)
    kw = dict(auto_reset=auto_reset, time_limit_steps=2)
    given = BatchedRaceEnv(track, num_envs, cars, **kw)
    drawn = BatchedRaceEnv(track, num_envs, cars, **kw)
    ora = make_oracle(track, num_envs=num_envs, cars_per_env=cars, **kw)
    ov = ora.reset(mode=spec.RESET_MODES[mode], seed=5)
    compare_outputs(given.reset(mode=mode, seed=5), ov, num_envs, cars, "reset, given")
    compare_outputs(drawn.reset(mode=mode, seed=5), ov, num_envs, cars, "reset, drawn")
    n_done = 0
    for k in range(steps):
        act = ro.random_actions(ACT_SEED, k, num_envs * cars)
        ov = ora.step(act, repeat=repeat)
        compare_outputs(given.step(torch.from_numpy(act).cuda(), repeat=repeat), ov, num_envs, cars, f"step {k}, given")
        compare_outputs(drawn.step_random(seed=ACT_SEED, step=k, repeat=repeat), ov, num_envs, cars, f"step {k}, drawn")
        n_done += int(np.asarray(ov["done"]).reshape(num_envs, cars).any(1).sum())
    given.close()
    drawn.close()
    return n_done


@pytest.mark.parametrize("repeat", [1, 4])
@pytest.mark.parametrize("cars", [1, 2, 4])
def test_a_reset_in_every_wave_at_every_other_step(cars, repeat):
    """192 envs = three waves, a time limit of two agent steps: every env of every wave resets at steps 1, 3, 5, 7 (random mode:
    the jittered pose and its progress value), and the steps between run the first sub-step on a fresh episode."""
    assert _rollout_both_ways(cars, repeat, auto_reset=True, mode="random") >= 4 * 192


@pytest.mark.parametrize("repeat", [1, 4])
@pytest.mark.parametrize("cars", [1, 2, 4])
def test_no_reset_is_prepared_and_done_envs_stand_still(cars, repeat):
    """auto_reset off, grid start: nothing is gathered, and from step 2 on every env is done and takes the arm without a
    sub-step."""
    assert _rollout_both_ways(cars, repeat, auto_reset=False, mode="grid") >= 6 * 192


@pytest.mark.parametrize("cars,mode", [(1, "random"), (2, "random_ball")])
def test_vehicle_randomization_and_a_track_set_together(cars, mode):
    """130 envs (two full waves and two lanes), three tracks, a reset every second step: the per-lane track loads, the draw of the
    next track and of the vehicle in front of the spawn gather."""
    import torch
    from dr_oracle import DROracleEnv
    from track_set_oracle import make_track_set_oracle
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    from racing_dreamer_amd import spec
    tracks = [load_track(n) for n in ("columbia", "austria", "barcelona")]
    n, lo, hi = 130, (0.168, 2.0, 0.4, 3.0, 0.02), (0.294, 8.0, 1.6, 8.0, 0.05)
    kw = dict(auto_reset=True, time_limit_steps=2)
    env = BatchedRaceEnv.with_track_set(tracks, n, cars, order="random", seed=(5 << 32) | 3, **kw)
    ora = make_track_set_oracle(tracks, order="random", seed=(5 << 32) | 3, base=DROracleEnv, num_envs=n, cars_per_env=cars, **kw)
    env.set_vehicle_randomization(lo, hi, seed=21)
    ora.set_vehicle_randomization(lo, hi, seed=21)
    dv, ov = env.reset(mode=mode, seed=13), ora.reset(mode=spec.RESET_MODES[mode], seed=13)
    compare_outputs(dv, ov, n, cars, "reset")
    for k in range(6):
        act = ro.random_actions(31, k, n * cars)
        dv, ov = env.step(torch.from_numpy(act).cuda(), repeat=2), ora.step(act, repeat=2)
        compare_outputs(dv, ov, n, cars, f"step {k}")
        assert np.array_equal(env.track_id.cpu().numpy(), ov["track_id"]), k
        assert np.array_equal(env.vehicle_params.cpu().numpy(), ora.vp), k
    env.close()


# ---- the scan alone, from set poses, against the plain-C oracle

_SCAN = {}


def _scan_case(n):
    """Poses of n cars on austria and the C oracle's ranges for them, computed once per batch size: scattered over the drivable
    area, and in every batch cars off the grid (near and far), cars standing in a wall cell and a car whose heading is not finite
    (the scan takes heading 0 for it: racecar_scan.h, scan_car)."""
    if n not in _SCAN:
        from oracle import c_oracle
        from racing_dreamer_amd.track_assets import load_track
        t = load_track("austria")
        rng = np.random.default_rng(n)
        free, wall = np.argwhere(t.drivable), np.argwhere(t.occ)
        pick = free[rng.integers(0, len(free), n)]
        poses = np.stack([t.origin[0] + (pick[:, 1] + rng.uniform(0, 1, n)) * t.resolution,
                          t.origin[1] + (pick[:, 0] + rng.uniform(0, 1, n)) * t.resolution,
                          rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)
        h, w = t.occ.shape
        poses[1, :2] = (t.origin[0] - 3.0, t.origin[1] + 2.0)                                   # off the grid, left of it
        poses[n // 2, :2] = (t.origin[0] + (w + 40) * t.resolution, t.origin[1] + (h + 7) * t.resolution)   # beyond the far corner
        poses[n - 2, :2] = (t.origin[0] + 5.0, t.origin[1] - 900.0)                             # far below
        for i, c in zip((3, n // 3, n - 1), wall[rng.integers(0, len(wall), 3)]):               # in a wall cell
            poses[i, :2] = (t.origin[0] + (c[1] + 0.5) * t.resolution, t.origin[1] + (c[0] + 0.5) * t.resolution)
        bad = 5
        cfg = ro.OracleConfig(num_envs=n, cars_per_env=1)
        ora = c_oracle.COracleEnv(t.occ, t.drivable, t.progress, t.centerline, t.origin, t.resolution, cfg, threads=8)
        ora.reset()
        ora.arr["x"][:], ora.arr["y"][:], ora.arr["theta"][:] = poses[:, 0], poses[:, 1], poses[:, 2]
        ora.arr["st"][:], ora.arr["ct"][:] = ro.sincos32(poses[:, 2])
        ora.arr["ct"][bad], ora.arr["st"][bad] = 1.0, 0.0
        ora._observe()
        poses[bad, 2] = np.nan
        _SCAN[n] = (t, poses, ora.lidar.copy())
    return _SCAN[n]


def _compare_lidar(got, want, n, context):
    """helpers.compare_outputs over the LiDAR rows alone (a set pose defines nothing else)."""
    import torch
    blank_d, blank_o = torch.zeros(n, device="cuda"), np.zeros(n, np.float32)
    dev = {k: blank_d for k in EXACT_INT + EXACT_FLOAT}
    ora = {k: blank_o for k in EXACT_INT + EXACT_FLOAT}
    dev["lidar"], ora["lidar"] = got, want
    compare_outputs(dev, ora, n, 1, context)


def _order_min_cars():
    """RC_ORDER_MIN_CARS as the library is compiled: from this batch size on the scan takes the cars through the track-order array
    at every observation (racecar_abi.hip, sort_cars_if_due)."""
    import os
    import re
    from racing_dreamer_amd import build
    with open(os.path.join(build.CSRC, "racecar_internal.h")) as f:
        return int(re.search(r"#define\s+RC_ORDER_MIN_CARS\s+(\d+)", f.read()).group(1))


@pytest.mark.parametrize("n,kernel", [(65, "rc_raycast_car_kernel<1, true, false>"), (4160, "rc_raycast_car_kernel<1, false, false>"),
                                      (16448, "rc_raycast_car_kernel<1, false, false>")])
def test_scan_from_set_poses_is_the_c_oracles(n, kernel):
    """65 cars: several waves per car (split > 1, the division stays); 4 160: the smallest batch above 16 cars per CU, one wave
    per car (split and part constants); 16 448: above RC_ORDER_MIN_CARS, where the library sorts the cars at every observation
    (order[slot] in the chain).  Each with the order array as the library decides and switched off (the scan_order knob: the
    slot is the car), and in the bounded build."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    t, poses, want = _scan_case(n)
    if n == 16448:
        assert n >= _order_min_cars()                   # (a changed threshold must not quietly end this case's coverage)
    env = BatchedRaceEnv(t, n, 1, auto_reset=True)
    env.reset()
    assert env.scan_kernel_name() == kernel
    _compare_lidar(env.set_pose(poses)["lidar"], want, n, f"{n} cars")
    _compare_lidar(env.set_pose(poses)["lidar"], want, n, f"{n} cars, again (an order by the last scan's rows)")
    env.debug_set("scan_order", 1)                      # no order array: car = slot
    _compare_lidar(env.set_pose(poses)["lidar"], want, n, f"{n} cars, no order")
    env.debug_set("scan_order", 0)
    env.debug_set("scan_bounded", 1)                    # the bounded build: any split, the same arguments
    assert env.scan_kernel_name() == "rc_raycast_car_kernel<1, false, true>"
    _compare_lidar(env.set_pose(poses)["lidar"], want, n, f"{n} cars, bounded")
    env.close()
