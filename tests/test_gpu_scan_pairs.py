"""The scan with one 16-byte beam load per pair of rounds in the builds that run one wave per car (racecar_scan.h: scan_car; the
paired image of the beam table: racecar_beam_pairs.h) - and the cases a production trip loop with two trips per pass needs
(tools/experiments/scan_trim_two_trips_per_pass.patch: measured slower, EXPERIMENTS.md 0000.5, so the loop in the tree makes one
trip per pass; these cases passed on the patched build and are what any change to that loop has to pass).  No output bit may change.

References: the BOUNDED build of the same scan (`scan_bounded`: the per-round beam table and load, a trip budget in the loop) on
the device, the C oracle on the host.  Ranges compare as BIT PATTERNS (-0.0 differs from +0.0), the uint16 rows as integers.

The trip-parity cases first assert that their poses exercise the loop - rays that stop after 1, 2, 3, 4 and more trips, rounds that
hold rays of both parities, the exact path taken on odd and on even trips.  The counts come from the instrumented build's per-lane
counters (rc_debug_scan_stamps, slots 8 - 15: racecar_scan.h), which walks the same tables with the same trips."""
import numpy as np
import pytest

from dr_oracle import apply_noise, noise_car_key, transform
from oracle import racecar_oracle as ro
from test_gpu_scan_trim import _bits, _free_poses, _oracle_scan, _scan, _sensor_grid, _snap, _transformed

pytestmark = pytest.mark.gpu

f32 = np.float32
PLAIN = "rc_raycast_car_kernel<1, false, false>"          # one wave per car: the production loop, the paired beam load
BOUNDED = "rc_raycast_car_kernel<1, false, true>"         # the reference build: bounded loop, per-round beam load
OVERLAP = "rc_raycast_car_kernel<1, true, false>"         # split > 1: the first trip peeled, per-round beam load


def _same(got, want, what):
    bad = np.nonzero(_bits(got) != _bits(want))
    assert bad[0].size == 0, (what, bad[0].size, bad[0][:5], bad[1][:5], got[bad][:5], want[bad][:5])


def _build(env, bounded, split):
    env.debug_set("scan_bounded", bounded)
    env.debug_set("ray_split", split)
    return env.scan_kernel_name()


@pytest.mark.parametrize("track_name,seed", [("austria", 31), ("columbia", 32)])
def test_rays_that_stop_after_odd_and_even_trips(track_name, seed):
    """256 on-track cars (up to 276 480 rays).  The inputs must exercise a loop body of two trips in both halves and at both exits:
    at least 100 rays stop after each of 1, 2, 3 and 4 trips and some after 5 or more; at least 50 rounds hold rays that stop after
    an odd and rays that stop after an even number of trips; rays take the exact path on an odd and on an even trip.  Then
    plain == bounded == oracle.  (On the GPU: austria 176 877 / 55 255 / 12 530 / 4 330 / 5 888 rays after 1 / 2 / 3 / 4 / 5+ trips,
    3 224 of 4 352 rounds with both parities, the exact path on an odd trip of 137 rays and on an even trip of 49; columbia
    151 658 / 81 607 / 22 094 / 6 674 / 7 967, 3 998 rounds, 190 and 99.)"""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    t = load_track(track_name)
    n = 256
    poses = _free_poses(t, n, seed)
    want = _oracle_scan(t, poses)
    env = BatchedRaceEnv(t, n, 1)
    env.reset()
    env.debug_set("ray_split", 1)
    stamps = env.debug_scan_stamps(n)                     # one wave per car: a row of counters per car
    counted = _scan(env, poses)
    s = stamps.cpu().numpy()
    env.debug_scan_stamps(0)
    by_trips, both = s[:, 8:13].sum(0), int(s[:, 13].sum())
    exact_odd, exact_even = int(s[:, 14].sum()), int(s[:, 15].sum())
    print(f"{track_name}: rays that stop after 1, 2, 3, 4, 5+ trips {by_trips.tolist()}, rounds with both parities {both} of {17 * n}, "
          f"rays with the exact path on an odd trip {exact_odd}, on an even trip {exact_even}")
    # (an on-track car's sensor, 0.25 m ahead of it, may stand in a wall cell: all 1080 rays of such a car make no trip)
    gx, gy = _sensor_grid(t, poses)
    started = ~t.occ[np.floor(gy).astype(int), np.floor(gx).astype(int)]
    assert started.sum() >= 200 and by_trips.sum() == started.sum() * 1080, (by_trips, started.sum())
    assert (by_trips[:4] >= 100).all() and by_trips[4] > 0, by_trips
    assert both >= 50, both
    assert exact_odd > 0 and exact_even > 0, (exact_odd, exact_even)
    _same(counted, want, "instrumented")
    assert _build(env, 0, 1) == PLAIN
    plain = _scan(env, poses)
    assert _build(env, 1, 1) == BOUNDED
    bounded = _scan(env, poses)
    _same(plain, bounded, "plain against bounded")
    _same(plain, want, "plain against the oracle")
    assert env.scan_overruns() == 0
    env.close()


def test_the_production_path_at_16384_cars():
    """16 384 cars on austria: the batch size from which the scan takes the cars in track order, on the kernel and launch the
    benchmark runs (no knob set for the plain build).  plain == bounded == oracle."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    t = load_track("austria")
    n = 16384
    poses = _free_poses(t, n, 33)
    want = _oracle_scan(t, poses)
    env = BatchedRaceEnv(t, n, 1)
    env.reset()
    assert env.scan_kernel_name() == PLAIN
    plain = _scan(env, poses)
    env.debug_set("scan_bounded", 1)
    assert env.scan_kernel_name() == BOUNDED
    bounded = _scan(env, poses)
    _same(plain, bounded, "plain against bounded")
    _same(plain, want, "plain against the oracle")
    assert env.scan_overruns() == 0
    env.close()


def test_sensor_on_a_cell_boundary_and_in_a_stop_cell():
    """256 cars on austria through the plain build: 128 with the sensor exactly on a cell boundary next to a wall (rays that stop at
    time zero: the -0.0 fix-up behind the loop reads the entry the loop ended on), 64 with the sensor INSIDE a wall cell (range 0
    on every beam, the loop never entered), 64 ordinary ones among them."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    t = load_track("austria")
    rng = np.random.default_rng(34)
    near = ~t.occ & (np.roll(t.occ, 1, 0) | np.roll(t.occ, -1, 0) | np.roll(t.occ, 1, 1) | np.roll(t.occ, -1, 1))
    near[:2, :] = near[-2:, :] = near[:, :2] = near[:, -2:] = False
    cy, cx = np.nonzero(near)
    on_edge = []
    for tries in range(4000):
        if len(on_edge) == 128:
            break
        kind = len(on_edge) % 3                                        # 0: x integral, 1: y integral, 2: both
        i = rng.integers(0, len(cx))
        th = f32(rng.choice([0.0, np.pi / 2, np.pi, -np.pi / 2]))
        for _ in range(int(rng.choice([0, 0, 1, 2, 5]))):              # (half of them a few ulps off the axis)
            th = np.nextafter(th, f32(rng.choice([-4.0, 4.0])))
        s, c = ro.sincos32(np.array([th], np.float32))
        gx = cx[i] + int(rng.integers(0, 2)) if kind != 1 else cx[i] + rng.uniform(0.05, 0.95)
        gy = cy[i] + int(rng.integers(0, 2)) if kind != 0 else cy[i] + rng.uniform(0.05, 0.95)
        p = np.array([t.origin[0] + gx * t.resolution - 0.25 * float(c[0]), t.origin[1] + gy * t.resolution - 0.25 * float(s[0]), th], np.float32)
        p = _snap(t, p, gx if kind != 1 else None, gy if kind != 0 else None)
        if p is not None:
            on_edge.append(p)
    assert len(on_edge) == 128
    wall = t.occ.copy()
    wall[:2, :] = wall[-2:, :] = wall[:, :2] = wall[:, -2:] = False
    wy, wx = np.nonzero(wall)
    k = rng.integers(0, len(wx), 64)
    th = rng.uniform(-np.pi, np.pi, 64).astype(np.float32)
    s, c = ro.sincos32(th)
    in_wall = np.stack([t.origin[0] + (wx[k] + 0.5) * t.resolution - 0.25 * c, t.origin[1] + (wy[k] + 0.5) * t.resolution - 0.25 * s, th], 1).astype(np.float32)
    poses = np.concatenate([np.stack(on_edge), in_wall, _free_poses(t, 64, 35)])
    kind = np.repeat([0, 1, 2], [128, 64, 64])
    order = rng.permutation(256)                                       # the three kinds side by side
    poses, kind = poses[order], kind[order]
    gx, gy = _sensor_grid(t, poses)
    assert ((gx == np.floor(gx)) | (gy == np.floor(gy)))[kind == 0].all()
    assert t.occ[np.floor(gy).astype(int), np.floor(gx).astype(int)][kind == 1].all()
    want = _oracle_scan(t, poses)
    zero = want == 0
    assert (zero & np.signbit(want))[kind == 0].any(1).sum() >= 16 and (zero & ~np.signbit(want))[kind == 0].any(1).sum() >= 16
    assert zero[kind == 1].all() and not np.signbit(want[kind == 1]).any()
    env = BatchedRaceEnv(t, 256, 1)
    env.reset()
    for bounded, split, name in ((0, 1, PLAIN), (1, 1, BOUNDED)):
        assert _build(env, bounded, split) == name
        _same(_scan(env, poses), want, name)
    env.close()


@pytest.mark.parametrize("lt,name", [(0, "metres"), (1, "dreamer"), (2, "unit")])
def test_the_last_round_pair_and_nothing_behind_the_rows(lt, name):
    """The last record of the paired beam table serves round 16 alone (56 beams); its second half is padding that no round reads.
    For every lidar_transform, on the plain build, beams 960 - 1079 (rounds 15 and 16: the last pair and the lone last round)
    equal the oracle's in fp32 and in uint16, and nothing is written behind a row:
    * fp32: two handles fill ONE arena (MixedTrackEnv); with the arena full of a canary, scanning one block leaves the other
      block's rows - the row of the NEXT car - and the bytes behind the last car's row as they were;
    * uint16: a handle of its own with the compact record on (a slice of a shared arena has none), slab and slack full of the
      canary: the rows equal the quantised oracle, the slack around the slab keeps the canary, and what follows the rows in the
      slab (the summary: another kernel's) is byte for byte what the bounded build leaves there."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    from racing_dreamer_amd.track_assets import load_track
    t = load_track("columbia")
    na, nb = 5, 3
    n = na + nb
    poses = _free_poses(t, n, 36)
    want = _transformed(_oracle_scan(t, poses), lt)
    canary = 0xA5
    mixed = MixedTrackEnv([t, t], [na, nb], lidar_transform=name)
    mixed.reset()
    for part in mixed.parts:
        part.debug_set("ray_split", 1)
        assert part.scan_kernel_name() == PLAIN
    torch.cuda.synchronize()
    lidar = mixed.views["lidar"].view(n, 1080)
    end = lidar.data_ptr() + lidar.numel() * 4 - mixed._raw.data_ptr()        # first byte behind the last car's row
    behind = mixed._raw[end:end + 16]
    assert behind.numel() == 16
    for part, rows, others in ((0, slice(0, na), slice(na, n)), (1, slice(na, n), slice(0, na))):
        mixed._raw.fill_(canary)
        torch.cuda.synchronize()
        mixed.parts[part].set_pose(poses[rows])
        torch.cuda.synchronize()
        got = lidar[rows].cpu().numpy()
        assert np.array_equal(_bits(got[:, 960:]), _bits(want[rows][:, 960:])), part
        _same(got, want[rows], part)
        assert bool((lidar[others].contiguous().view(torch.uint8) == canary).all()), part
        if part == 1:
            assert bool((behind == canary).all())
    mixed.close()
    env = BatchedRaceEnv(t, n, 1, lidar_transform=name)
    env.reset()
    env.enable_compact(buffers=1)
    raw = env._compact[0][0]                                                   # the slab with its 64 bytes of slack
    head = env.compact.data_ptr() - raw.data_ptr()
    u16_bytes = env.compact_layout[0]
    assert u16_bytes == n * 2160
    left = {}
    for bounded, kernel in ((0, PLAIN), (1, BOUNDED)):
        assert _build(env, bounded, 1) == kernel
        raw.fill_(canary)
        torch.cuda.synchronize()
        _same(_scan(env, poses), want, kernel)
        q = env.compact[:u16_bytes].cpu().numpy().view(np.uint16).reshape(n, 1080)
        assert np.array_equal(q[:, 960:], ro.quantise_lidar_u16(want, lt)[:, 960:]), kernel
        assert np.array_equal(q, ro.quantise_lidar_u16(want, lt)), kernel
        assert bool((raw[:head] == canary).all()) and bool((raw[head + env.compact.numel():] == canary).all()), kernel
        left[kernel] = raw.clone()
    assert torch.equal(left[PLAIN], left[BOUNDED])
    env.close()


@pytest.fixture(scope="module")
def small_batch():
    from racing_dreamer_amd.track_assets import load_track
    t = load_track("treitlstrasse_v2")
    poses = _free_poses(t, 96, 37)
    poses[:8, 2] = np.array([0.0, np.pi / 2, np.pi, -np.pi / 2] * 2, np.float32)      # axis-parallel beams: the IEEE division path
    return t, poses, _oracle_scan(t, poses)


def test_a_split_launch_against_one_wave_per_car(small_batch):
    """The builds that run with any split keep the per-round beam table: 2, 3 and 17 waves per car (17: one round per wave) and
    the bounded build with 3 against the plain build with one wave per car, and against the oracle."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    t, poses, want = small_batch
    env = BatchedRaceEnv(t, len(poses), 1)
    env.reset()
    assert _build(env, 0, 1) == PLAIN
    plain = _scan(env, poses)
    _same(plain, want, "plain")
    for bounded, split, name in ((0, 2, OVERLAP), (0, 3, OVERLAP), (0, 17, OVERLAP), (1, 3, BOUNDED)):
        assert _build(env, bounded, split) == name
        _same(_scan(env, poses), plain, (bounded, split))
    assert env.scan_overruns() == 0
    env.close()


@pytest.mark.parametrize("lt,name", [(0, "metres"), (1, "dreamer")])
def test_the_noise_builds(small_batch, lt, name):
    """LiDAR noise and dropout on: the noise kernel with one wave per car takes the paired load, the one with a split does not;
    both against the restatement of the noise on the oracle's ranges."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    t, poses, metres = small_batch
    n = len(poses)
    seed = (1 << 40) | 11
    noisy = apply_noise(metres, noise_car_key(seed, np.arange(n), np.ones(n), np.zeros(n)), 0.25, 0.1)   # (episode 1, sub-step 0)
    want = transform(noisy, lt)
    env = BatchedRaceEnv(t, n, 1, lidar_transform=name, lidar_noise=(0.25, 0.1, seed))
    env.reset()
    for split in (1, 3):
        env.debug_set("ray_split", split)
        assert env.scan_kernel_name() == f"rc_raycast_car_noise_kernel<1, {'true' if split > 1 else 'false'}>"
        _same(_scan(env, poses), want, (name, split))
    env.close()


def test_a_group_launch_and_a_track_set_on_the_one_wave_builds():
    """One launch over two handles (rc_step_group) and a track set, every handle held to one wave per car so that the group and
    track-set kernels run their paired-load builds, against plain handles on the same envs (which the tests above equate with the
    oracle): every output after every step, bit for bit."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    from racing_dreamer_amd.track_assets import load_track
    names, sizes = ["columbia", "austria"], [40, 24]
    mixed = MixedTrackEnv(names, sizes, auto_reset=True)
    seps = [BatchedRaceEnv(nm, b - a, 1, auto_reset=True, first_env=a) for nm, (a, b) in zip(names, mixed.blocks)]
    ts = BatchedRaceEnv.with_track_set([load_track("columbia")], 40, 1, auto_reset=True)
    for e in mixed.parts + seps + [ts]:
        e.debug_set("ray_split", 1)
    assert ts.scan_kernel_name() == "rc_raycast_ts_kernel<1, false, false>"
    assert all(e.scan_kernel_name() == PLAIN for e in seps)
    mixed.reset(mode="random", seed=5)
    ts.reset(mode="random", seed=5)
    for e in seps:
        e.reset(mode="random", seed=5)
    for k in range(6):
        dv = mixed.step_random(seed=3, step=k, repeat=2)
        ts.step_random(seed=3, step=k, repeat=2)
        for e in seps:
            e.step_random(seed=3, step=k, repeat=2)
        torch.cuda.synchronize()
        for e, (a, b) in zip(seps, mixed.blocks):
            for name in dv:
                assert torch.equal(dv[name][a:b].contiguous().view(torch.uint8), e.views[name].contiguous().view(torch.uint8)), (k, name)
        assert torch.equal(ts.views["lidar"].view(torch.int32), seps[0].views["lidar"].view(torch.int32)), k
    assert bool((seps[0].views["lidar"] < 15.0).any())
    mixed.close(); ts.close()
    for e in seps:
        e.close()
