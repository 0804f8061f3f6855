"""Per-episode domain randomization on the MI355X: per-car vehicle parameters in the dynamics kernel and LiDAR noise / dropout
in the scan (include/racecar_hip.h, rc_set_vehicle_randomization / rc_set_vehicle_params / rc_vehicle_params /
rc_set_lidar_noise) against the test-side restatement (tests/dr_oracle.py), bit for bit."""
import numpy as np
import pytest

from dr_oracle import VP_NOMINAL, apply_noise, make_dr_oracle, noise_car_key, transform
from helpers import compare_outputs, make_oracle
from oracle import racecar_oracle as ro

pytestmark = pytest.mark.gpu

WIDE_LO = (0.168, 2.0, 0.4, 3.0, 0.02)          # the deployment lock + wide bands on accel_max, drag, max_vel, steer_step
WIDE_HI = (0.294, 8.0, 1.6, 8.0, 0.05)


def _arena_bytes(env):
    import torch
    torch.cuda.synchronize()
    return env._arena_view.clone()


@pytest.mark.parametrize("track_name", ["austria", "treitlstrasse_v2"])
@pytest.mark.parametrize("cars", [1, 2])
def test_degenerate_randomization_equals_off_bit_for_bit(track_name, cars):
    """Random mode with lo == hi == nominal against a plain env: every arena section and the vehicle parameters identical through
    200 steps with auto-reset, repeat 1 and 4."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n = 512
    for repeat in (1, 4):
        plain = BatchedRaceEnv(track_name, n, cars, auto_reset=True, time_limit_steps=60)
        dr = BatchedRaceEnv(track_name, n, cars, auto_reset=True, time_limit_steps=60,
                            vehicle_randomization=(VP_NOMINAL, VP_NOMINAL, 77))
        assert dr.vehicle_params.shape == (n * cars, 5)
        mode = "random_ball" if cars > 1 else "random"
        plain.reset(mode=mode, seed=5)
        dr.reset(mode=mode, seed=5)
        assert torch.equal(_arena_bytes(plain), _arena_bytes(dr))
        done = 0
        for k in range(200):
            plain.step_random(seed=3, step=k, repeat=repeat)
            dr.step_random(seed=3, step=k, repeat=repeat)
            a, b = _arena_bytes(plain), _arena_bytes(dr)
            assert torch.equal(a, b), (track_name, cars, repeat, k)
            done += int(plain.views["done"].sum())
        assert done > 0
        want = torch.from_numpy(np.tile(VP_NOMINAL, (n * cars, 1))).cuda()
        assert torch.equal(dr.vehicle_params, want) and torch.equal(plain.vehicle_params, want)
        plain.close(); dr.close()


def _dr_rollout(track_name, num_envs, cars, steps, repeat, fixed=None, noise=None, lidar_transform=0, first_env=0):
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    t = load_track(track_name)
    names = {0: "metres", 1: "dreamer", 2: "unit"}
    env = BatchedRaceEnv(t, num_envs, cars, auto_reset=True, lidar_transform=names[lidar_transform], first_env=first_env)
    ora = make_dr_oracle(t, num_envs=num_envs, cars_per_env=cars, auto_reset=True, first_env=first_env)
    if fixed is not None:
        env.set_vehicle_params(torch.from_numpy(fixed).cuda())
        ora.set_vehicle_params(fixed)
    else:
        env.set_vehicle_randomization(WIDE_LO, WIDE_HI, seed=(9 << 32) | 21)
        ora.set_vehicle_randomization(WIDE_LO, WIDE_HI, seed=(9 << 32) | 21)
    if noise is not None:
        env.set_lidar_noise(*noise)
        ora.set_lidar_noise(*noise)
    mode = "random_ball" if cars > 1 else "random"
    dv = env.reset(mode=mode, seed=13)
    ov = ora.reset(mode=2 if cars > 1 else 1, seed=13)
    n_done = 0
    for k in range(steps + 1):
        if k:
            act = ro.random_actions(31, k, num_envs * cars)
            act[:, 0] = np.abs(act[:, 0])
            dv = env.step(torch.from_numpy(act).cuda(), repeat=repeat)
            ov = ora.step(act, repeat=repeat)
            n_done += int(np.asarray(ov["done"]).sum())
        ov = dict(ov, lidar=transform(ov["lidar"], lidar_transform))
        compare_outputs(dv, ov, num_envs, cars, f"{track_name} A={cars} step {k}")
        torch.cuda.synchronize()
        assert np.array_equal(env.vehicle_params.cpu().numpy(), ora.vp), k
    env.close()
    return n_done, ora


@pytest.mark.parametrize("cars,num_envs,track_name", [(1, 96, "treitlstrasse_v2"), (2, 48, "treitlstrasse_v2"), (4, 16, "columbia")])
def test_randomized_dynamics_equal_the_restatement(cars, num_envs, track_name):
    """The deployment lock + wide bands on the longitudinal law, random resets with collisions and auto-reset: every output and
    the per-car parameters after every step; then the same in fixed mode."""
    n_done, ora = _dr_rollout(track_name, num_envs, cars, steps=40, repeat=3)
    assert n_done > 0
    assert (ora.vp[:, 0] != VP_NOMINAL[0]).all() and len(np.unique(ora.vp[:, 1])) > num_envs * cars // 2
    rng = np.random.default_rng(cars)
    fixed = (np.asarray(WIDE_LO, np.float32) + rng.uniform(0, 1, (num_envs * cars, 5)).astype(np.float32)
             * (np.asarray(WIDE_HI, np.float32) - np.asarray(WIDE_LO, np.float32))).astype(np.float32)
    n_done, ora = _dr_rollout(track_name, num_envs, cars, steps=40, repeat=3, fixed=fixed)
    assert n_done > 0 and np.array_equal(ora.vp, fixed)       # nothing drawn at the resets


@pytest.mark.parametrize("lidar_transform", [0, 1, 2])
def test_noisy_scan_equals_the_restatement_in_a_rollout(lidar_transform):
    """Noise + dropout + vehicle randomization, two cars per env (inter-car returns), every lidar_transform."""
    _dr_rollout("treitlstrasse_v2", 40, 2, steps=12, repeat=2, noise=(0.3, 0.05, (3 << 32) | 8), lidar_transform=lidar_transform)


def _oracle_scan(track, poses):
    from oracle import c_oracle
    cfg = ro.OracleConfig(num_envs=len(poses), cars_per_env=1)
    env = c_oracle.COracleEnv(track.occ, track.drivable, track.progress, track.centerline, track.origin, track.resolution, cfg, threads=8)
    env.reset()
    env.arr["x"][:], env.arr["y"][:], env.arr["theta"][:] = poses[:, 0], poses[:, 1], poses[:, 2]
    env.arr["st"][:], env.arr["ct"][:] = ro.sincos32(poses[:, 2])
    env._observe()
    return env.lidar.copy()


@pytest.mark.parametrize("n", [257, 4096, 4097])
def test_the_noise_is_the_same_however_a_cars_rounds_are_dealt_to_waves(n):
    """Every way of dealing a car's 17 rounds to waves gives the restatement's noisy ranges - fp32 rows and the uint16 copy
    (which quantises the noisy value) - for every lidar_transform."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    t = load_track("treitlstrasse_v2")
    rng = np.random.default_rng(n + 1)
    free = np.argwhere(t.drivable)
    pick = free[rng.integers(0, len(free), n)]
    poses = np.stack([t.origin[0] + (pick[:, 1] + rng.uniform(0, 1, n)) * t.resolution,
                      t.origin[1] + (pick[:, 0] + rng.uniform(0, 1, n)) * t.resolution,
                      rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)
    seed = (1 << 40) | 5
    # after the first reset every env stands at episode 1, sub-step 0
    want_m = apply_noise(_oracle_scan(t, poses), noise_car_key(seed, np.arange(n), np.ones(n), np.zeros(n)), 0.25, 0.1)
    for lt, name in enumerate(("metres", "dreamer", "unit")):
        env = BatchedRaceEnv(t, n, 1, lidar_transform=name, lidar_noise=(0.25, 0.1, seed))
        env.reset()
        env.enable_compact(buffers=1)
        assert env.scan_kernel_name().startswith("rc_raycast_car_noise_kernel<1, ")
        want = transform(want_m, lt)
        for split in ((0, 1, 2, 5, 16, 17) if lt == 0 else (0, 17)):
            env.debug_set("ray_split", split)
            got = env.set_pose(poses)["lidar"]
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy().reshape(n, 1080), want), (n, lt, split)
            q = env.compact[:env.compact_layout[0]].cpu().numpy().view(np.uint16).reshape(n, 1080)
            assert np.array_equal(q, ro.quantise_lidar_u16(want, lt)), (n, lt, split)
            env.compact.zero_()
        env.set_lidar_noise(0.0, 0.0)                                            # off: the production scan again
        assert env.scan_kernel_name().startswith("rc_raycast_car_kernel<")
        assert np.array_equal(env.set_pose(poses)["lidar"].cpu().numpy().reshape(n, 1080), transform(_oracle_scan(t, poses), lt))
        env.close()


def test_a_shard_sees_the_noise_and_the_vehicles_of_the_full_job():
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    kw = dict(auto_reset=True, vehicle_randomization=(WIDE_LO, WIDE_HI, 4), lidar_noise=(0.3, 0.02, 6))
    full = BatchedRaceEnv("austria", 64, 1, **kw)
    part = BatchedRaceEnv("austria", 32, 1, first_env=32, **kw)
    a, b = full.reset(mode="random", seed=3), part.reset(mode="random", seed=3)
    for k in range(30):
        act = ro.random_actions(1, k, 64)
        act[:, 0] = np.abs(act[:, 0])
        a = full.step(torch.from_numpy(act).cuda(), repeat=4)
        b = part.step(torch.from_numpy(act[32:]).cuda(), repeat=4)
        torch.cuda.synchronize()
        for name in ("lidar", "pose", "reward", "done", "progress"):
            assert torch.equal(a[name][32:], b[name]), (name, k)
        assert torch.equal(full.vehicle_params[32:], part.vehicle_params), k
    full.close(); part.close()


def test_mixed_track_group_with_both_features_equals_separate_envs():
    """MixedTrackEnv (three tracks, one dynamics and one scan launch per step: rc_step_group) with vehicle randomization and LiDAR
    noise on equals three separate envs with the same settings; a group in which only some blocks have them on runs the others
    unchanged; and step_random equals fill_random_actions + step."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    names, sizes = ["columbia", "austria", "treitlstrasse_v2"], [70, 50, 40]
    n = sum(sizes)
    kw = dict(cars_per_env=2, auto_reset=True)
    mixed = MixedTrackEnv(names, sizes, **kw)
    mixed.set_vehicle_randomization(WIDE_LO, WIDE_HI, seed=12)
    mixed.set_lidar_noise(0.2, 0.03, seed=17)
    seps = []
    for nm, (a, b) in zip(names, mixed.blocks):
        e = BatchedRaceEnv(nm, b - a, 2, auto_reset=True, first_env=a)
        e.set_vehicle_randomization(WIDE_LO, WIDE_HI, seed=12)
        e.set_lidar_noise(0.2, 0.03, seed=17)
        seps.append(e)
    dv = mixed.reset(mode="random_ball", seed=2)
    for e in seps:
        e.reset(mode="random_ball", seed=2)
    for k in range(25):
        act = ro.random_actions(8, k, n * 2)
        act[:, 0] = np.abs(act[:, 0])
        t = torch.from_numpy(act).cuda().view(n, 2, 2)
        dv = mixed.step(t, repeat=2)
        for e, (a, b) in zip(seps, mixed.blocks):
            e.step(t[a:b].contiguous(), repeat=2)
        torch.cuda.synchronize()
        for e, (a, b) in zip(seps, mixed.blocks):
            for name in dv:
                assert torch.equal(dv[name][a:b], e.views[name]), (k, name)
        assert torch.equal(mixed.vehicle_params, torch.cat([e.vehicle_params for e in seps]))
    # step_random == fill_random_actions + step, the features on in the first block only
    x = MixedTrackEnv(names, sizes, **kw)
    y = MixedTrackEnv(names, sizes, **kw)
    for m in (x, y):
        m.parts[0].set_vehicle_randomization(WIDE_LO, WIDE_HI, seed=1)
        m.parts[0].set_lidar_noise(0.3, 0.05, seed=2)
        m.reset(mode="random_ball", seed=9)
    plain = MixedTrackEnv(names, sizes, **kw)
    plain.reset(mode="random_ball", seed=9)
    for k in range(15):
        x.step_random(seed=4, step=k, repeat=3)
        for p in y.parts:
            p.fill_random_actions(seed=4, step=k)
        y.step(None, repeat=3)
        plain.step_random(seed=4, step=k, repeat=3)
        torch.cuda.synchronize()
        for name in x.views:
            assert torch.equal(x.views[name], y.views[name]), (k, name)
            a0 = mixed.blocks[0][1]
            assert torch.equal(x.views[name][a0:], plain.views[name][a0:]), (k, name)     # the blocks with both off: unchanged
    for m in (mixed, x, y, plain, *seps):
        m.close()


def test_agents_keep_the_nominal_gain_and_the_api_refuses_what_it_does_not_carry():
    """The follow-the-gap agents map an angle to a command with the nominal 0.19 rad whatever the car (an agent does not know its
    car); bad bands and noise settings are refused; the record layout does not change."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    a = BatchedRaceEnv("austria", 64, 1)
    b = BatchedRaceEnv("austria", 64, 1)
    b.set_vehicle_params(torch.tensor([[0.294, 6.0, 1.0, 6.0, 0.05]] * 64))
    a.reset(mode="random", seed=1); b.reset(mode="random", seed=1)
    assert torch.equal(a.follow_the_gap_reference(), b.follow_the_gap_reference())
    assert a.arena_nbytes == b.arena_nbytes
    with pytest.raises(L.RacecarHipError, match="lo <= hi"):
        a.set_vehicle_randomization((0.3, 4, 0.8, 5, 0.032), (0.2, 4, 0.8, 5, 0.032))
    with pytest.raises(L.RacecarHipError, match="p_drop"):
        a.set_lidar_noise(0.1, 1.5)
    a.set_lidar_noise(0.1, 0.0)
    a.debug_set("scan_bounded", 1)
    with pytest.raises(L.RacecarHipError, match="variant 7"):
        a.step_random(seed=1, step=0)
    a.close(); b.close()
