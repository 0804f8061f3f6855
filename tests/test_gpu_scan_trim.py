"""The scan after its per-trip and per-round instructions were trimmed (racecar_scan.h: the exit side kept as a lane mask, one
pinned LDS address, the zero-time test hoisted to a per-car predicate, the last round's lanes by a constant mask, the beam
table stepped on the scalar side, lidar_transform applied in the flush): every output bit as before, against the C oracle -
ranges compare as BIT PATTERNS, so -0.0 differs from +0.0."""
import numpy as np
import pytest

from dr_oracle import apply_noise, noise_car_key, transform
from oracle import racecar_oracle as ro

pytestmark = pytest.mark.gpu

f32 = np.float32


def _oracle_scan(track, poses):
    """LiDAR of the C oracle for arbitrary poses [n, 3] (one car per env)."""
    from oracle import c_oracle
    cfg = ro.OracleConfig(num_envs=len(poses), cars_per_env=1)
    env = c_oracle.COracleEnv(track.occ, track.drivable, track.progress, track.centerline, track.origin, track.resolution, cfg, threads=8)
    env.reset()
    env.arr["x"][:], env.arr["y"][:], env.arr["theta"][:] = poses[:, 0], poses[:, 1], poses[:, 2]
    env.arr["st"][:], env.arr["ct"][:] = ro.sincos32(poses[:, 2])
    env._observe()
    return env.lidar.copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scan(env, poses):
    import torch
    got = env.set_pose(poses)["lidar"]
    torch.cuda.synchronize()
    return got.cpu().numpy().reshape(len(poses), 1080)


def _free_poses(track, n, seed):
    rng = np.random.default_rng(seed)
    free = np.argwhere(track.drivable)
    pick = free[rng.integers(0, len(free), n)]
    return np.stack([track.origin[0] + (pick[:, 1] + rng.uniform(0, 1, n)) * track.resolution,
                     track.origin[1] + (pick[:, 0] + rng.uniform(0, 1, n)) * track.resolution,
                     rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)


def _sensor_grid(track, poses):
    """The sensor's grid coordinates as the scan computes them: one binary32 operation per operator (racecar_oracle.py, scan)."""
    st, ct = ro.sincos32(poses[:, 2])
    org_x, org_y, inv_res = f32(track.origin[0]), f32(track.origin[1]), f32(1.0 / track.resolution)
    lx = poses[:, 0] + f32(0.25) * ct
    ly = poses[:, 1] + f32(0.25) * st
    return (lx - org_x) * inv_res, (ly - org_y) * inv_res


def _snap(track, pose, want_gx, want_gy):
    """Move the car by a few ulps until the sensor's grid x (y) IS the integer asked for (None: leave that axis alone)."""
    pose = pose.copy()
    for axis, want in ((0, want_gx), (1, want_gy)):
        if want is None:
            continue
        cand = np.tile(pose, (129, 1))
        cand[:, axis] = (pose[axis:axis + 1].view(np.int32) + np.arange(-64, 65, dtype=np.int32)).view(np.float32)   # +- 64 ulps
        hit = np.nonzero(_sensor_grid(track, cand)[axis] == f32(want))[0]
        if hit.size == 0:
            return None
        pose = cand[hit[np.argmin(np.abs(hit - 64))]]
    return pose


def test_sensor_on_a_cell_boundary():
    """A ray's boundary time can be zero only if the sensor lies exactly on a cell boundary: the scan tests that once per car
    and skips the -0.0 fix-up's compare in every round of every other car.  256 cars on austria: 64 with an integral grid x, 64
    with an integral y, 64 with both - all on the faces of free cells NEXT TO A WALL, so rays stop at time zero -, headings
    axis-parallel and a few ulps off; and 64 ordinary cars among them."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    t = load_track("austria")
    rng = np.random.default_rng(5)
    free = ~t.occ
    near = free & (np.roll(t.occ, 1, 0) | np.roll(t.occ, -1, 0) | np.roll(t.occ, 1, 1) | np.roll(t.occ, -1, 1))
    near[:2, :] = near[-2:, :] = near[:, :2] = near[:, -2:] = False
    cy, cx = np.nonzero(near)
    base = [0.0, np.pi / 2, np.pi, -np.pi / 2]
    poses, kinds = [], []
    tries = 0
    while len(poses) < 192 and tries < 4000:
        tries += 1
        kind = len(poses) // 64                                       # 0: x integral, 1: y integral, 2: both
        i = rng.integers(0, len(cx))
        th = f32(base[rng.integers(0, 4)])
        for _ in range(int(rng.choice([0, 0, 1, 2, 5]))):             # (half of them a few ulps off the axis)
            th = np.nextafter(th, f32(rng.choice([-4.0, 4.0])))
        if th == 0 and rng.random() < 0.5:
            th = f32(rng.choice([-1.0, 1.0]) * 2.0 ** -23 * rng.integers(1, 4))
        s, c = ro.sincos32(np.array([th], np.float32))
        gx = cx[i] + int(rng.integers(0, 2)) if kind != 1 else cx[i] + rng.uniform(0.05, 0.95)
        gy = cy[i] + int(rng.integers(0, 2)) if kind != 0 else cy[i] + rng.uniform(0.05, 0.95)
        p = np.array([t.origin[0] + gx * t.resolution - 0.25 * float(c[0]), t.origin[1] + gy * t.resolution - 0.25 * float(s[0]), th], np.float32)
        p = _snap(t, p, gx if kind != 1 else None, gy if kind != 0 else None)
        if p is not None:
            poses.append(p)
            kinds.append(kind)
    assert len(poses) == 192, (len(poses), tries)
    poses = np.concatenate([np.stack(poses), _free_poses(t, 64, 6)])
    order = rng.permutation(256)                                       # boundary cars and ordinary ones side by side
    poses = poses[order]
    gx, gy = _sensor_grid(t, poses)
    on_x, on_y = gx == np.floor(gx), gy == np.floor(gy)
    assert on_x.sum() >= 128 and on_y.sum() >= 128 and (on_x & on_y).sum() >= 64 and (~on_x & ~on_y).sum() >= 60
    want = _oracle_scan(t, poses)
    zero = want == 0
    minus = zero & np.signbit(want)
    # what the hoisted test can get wrong is there to be got wrong: rays that stop at time zero, of either sign, on cars of
    # every kind - and none on a car off the boundaries
    assert minus.any(1).sum() >= 32 and (zero & ~np.signbit(want)).any(1).sum() >= 32, (minus.any(1).sum(), zero.any(1).sum())
    assert not minus[~on_x & ~on_y].any()
    env = BatchedRaceEnv(t, 256, 1)
    env.reset()
    for knob, value in ((None, 0), ("ray_split", 2), ("scan_bounded", 1)):       # plain, overlapped and bounded build
        if knob:
            env.debug_set(knob, value)
        got = _scan(env, poses)
        bad = np.nonzero(_bits(got) != _bits(want))
        assert bad[0].size == 0, (knob, bad[0][:5], bad[1][:5], got[bad][:5], want[bad][:5], poses[bad[0][:5]])
    env.close()


def test_the_last_round_writes_its_56_beams_and_nothing_else():
    """Round 16 of a car has 56 beams; its lanes are now chosen by a constant mask and the scalar round counter.  Two handles fill
    ONE arena (MixedTrackEnv): with the arena full of a canary, scanning one block alone leaves the other block's rows - the row
    of the NEXT car - and the bytes behind the last car's row as they were; beams 1024 - 1079 equal the oracle's."""
    import torch
    from racing_dreamer_amd.batched_env import MixedTrackEnv
    from racing_dreamer_amd.track_assets import load_track
    t = load_track("columbia")
    na, nb = 5, 3
    mixed = MixedTrackEnv([t, t], [na, nb])
    mixed.reset()
    torch.cuda.synchronize()
    poses = _free_poses(t, na + nb, 3)
    want = _oracle_scan(t, poses)
    lidar = mixed.views["lidar"].view(na + nb, 1080)
    end = lidar.data_ptr() + lidar.numel() * 4 - mixed._raw.data_ptr()        # first byte behind the last car's row
    behind = mixed._raw[end:end + 16]                                          # (the next section's block A part, or the arena's padding)
    assert behind.numel() == 16
    canary = 0xA5
    for part, rows, others in ((0, slice(0, na), slice(na, na + nb)), (1, slice(na, na + nb), slice(0, na))):
        mixed._raw.fill_(canary)
        torch.cuda.synchronize()
        mixed.parts[part].set_pose(poses[rows])
        torch.cuda.synchronize()
        got = lidar[rows].cpu().numpy()
        assert np.array_equal(_bits(got[:, 1024:]), _bits(want[rows][:, 1024:])), part
        assert np.array_equal(_bits(got), _bits(want[rows])), part
        assert bool((lidar[others].contiguous().view(torch.uint8) == canary).all()), part
        if part == 1:
            assert bool((behind == canary).all())
    mixed.close()


def _transformed(want, lt):
    if lt == 1:
        return (want / f32(15.0) - f32(0.5)).astype(np.float32)
    if lt == 2:
        return (want * f32(1.0 / 15.0)).astype(np.float32)
    return want


@pytest.fixture(scope="module")
def small_batch():
    from racing_dreamer_amd.track_assets import load_track
    t = load_track("treitlstrasse_v2")
    poses = _free_poses(t, 96, 17)
    poses[:8, 2] = np.array([0.0, np.pi / 2, np.pi, -np.pi / 2] * 2, np.float32)      # axis-parallel beams: the IEEE division path
    return t, poses, _oracle_scan(t, poses)


@pytest.mark.parametrize("lt,name", [(0, "metres"), (1, "dreamer"), (2, "unit")])
def test_every_build_of_the_scan_and_every_transform(small_batch, lt, name):
    """One batch of 96 cars through the plain build (one wave per car), the overlapped one (2, 3 and 17 waves per car: 17 is one
    round per wave, the last with 56 lanes) and the bounded one (one and three waves per car), for each lidar_transform - which
    the scan now applies in its flush -, with the uint16 copy of the rows enabled: the oracle's ranges and their quantised copy."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    t, poses, metres = small_batch
    want = _transformed(metres, lt)
    assert np.array_equal(_bits(want), _bits(transform(metres, lt)))
    n = len(poses)
    env = BatchedRaceEnv(t, n, 1, lidar_transform=name)
    env.reset()
    env.enable_compact(buffers=1)
    for bounded, split in ((0, 1), (0, 2), (0, 3), (0, 17), (1, 1), (1, 3)):
        env.debug_set("scan_bounded", bounded)
        env.debug_set("ray_split", split)
        kernel = env.scan_kernel_name()
        assert kernel == f"rc_raycast_car_kernel<1, {'true' if split > 1 and not bounded else 'false'}, {'true' if bounded else 'false'}>", kernel
        got = _scan(env, poses)
        assert np.array_equal(_bits(got), _bits(want)), (name, bounded, split)
        q = env.compact[:env.compact_layout[0]].cpu().numpy().view(np.uint16).reshape(n, 1080)
        assert np.array_equal(q, ro.quantise_lidar_u16(want, lt)), (name, bounded, split)
        env.compact.zero_()
    assert env.scan_overruns() == 0
    env.close()


@pytest.mark.parametrize("lt,name", [(0, "metres"), (1, "dreamer")])
def test_the_noisy_builds(small_batch, lt, name):
    """The same batch with LiDAR noise and dropout on (the noise kernels: plain and overlapped), against the restatement."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    t, poses, metres = small_batch
    n = len(poses)
    seed = (1 << 40) | 9
    noisy = apply_noise(metres, noise_car_key(seed, np.arange(n), np.ones(n), np.zeros(n)), 0.25, 0.1)   # (episode 1, sub-step 0)
    want = transform(noisy, lt)
    env = BatchedRaceEnv(t, n, 1, lidar_transform=name, lidar_noise=(0.25, 0.1, seed))
    env.reset()
    for split in (1, 2, 17):
        env.debug_set("ray_split", split)
        assert env.scan_kernel_name().startswith("rc_raycast_car_noise_kernel<1, ")
        assert np.array_equal(_bits(_scan(env, poses)), _bits(want)), (name, split)
    env.close()


def test_a_group_launch_and_a_track_set_equal_plain_handles():
    """The other two ways into the scan - one launch over two handles (rc_step_group) and a track set - against plain handles on
    the same envs, which the tests above equate with the oracle: every output after every step, bit for bit."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    from racing_dreamer_amd.track_assets import load_track
    names, sizes = ["columbia", "austria"], [40, 24]
    mixed = MixedTrackEnv(names, sizes, auto_reset=True)
    seps = [BatchedRaceEnv(nm, b - a, 1, auto_reset=True, first_env=a) for nm, (a, b) in zip(names, mixed.blocks)]
    t = load_track("columbia")
    ts = BatchedRaceEnv.with_track_set([t], 40, 1, auto_reset=True)
    assert ts.scan_kernel_name().startswith("rc_raycast_ts_kernel<1,")
    mixed.reset(mode="random", seed=4)
    ts.reset(mode="random", seed=4)
    for e in seps:
        e.reset(mode="random", seed=4)
    for k in range(6):
        dv = mixed.step_random(seed=2, step=k, repeat=2)
        ts.step_random(seed=2, step=k, repeat=2)
        for e in seps:
            e.step_random(seed=2, step=k, repeat=2)
        torch.cuda.synchronize()
        for e, (a, b) in zip(seps, mixed.blocks):
            for name in dv:
                assert torch.equal(dv[name][a:b].contiguous().view(torch.uint8), e.views[name].contiguous().view(torch.uint8)), (k, name)
        assert torch.equal(ts.views["lidar"].view(torch.int32), seps[0].views["lidar"].view(torch.int32)), k
    assert bool((seps[0].views["lidar"] < 15.0).any())
    mixed.close(); ts.close()
    for e in seps:
        e.close()
