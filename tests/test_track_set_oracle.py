"""Track set, CPU side: the test-side restatement (tests/track_set_oracle.py) that the GPU tests compare against, and the C-ABI
surface (include/racecar_hip.h, rc_set_track_set / rc_set_next_track / rc_track_ids)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dr_oracle import DROracleEnv, VP_NOMINAL
from helpers import make_oracle
from oracle import racecar_oracle as ro
from track_set_oracle import contiguous_initial, draw_tracks, make_track_set_oracle, weight_thresholds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rc_set_track_set", "rc_set_next_track", "rc_track_ids")


def _tracks(*names):
    from racing_dreamer_amd.track_assets import load_track
    return [load_track(n) for n in names]


@pytest.mark.parametrize("cars", [1, 2])
def test_one_track_set_equals_the_base_oracle(cars):
    """A set of one track, sequential (every reset 'switches' to the same track): every output of the composite is the base
    oracle's, through 500 steps with auto-reset."""
    (t,) = _tracks("austria")
    n = 6
    base = make_oracle(t, num_envs=n, cars_per_env=cars, auto_reset=True, time_limit_steps=45)
    ts = make_track_set_oracle([t], num_envs=n, cars_per_env=cars, auto_reset=True, time_limit_steps=45)
    mode = 2 if cars > 1 else 1
    a, b = base.reset(mode=mode, seed=4), ts.reset(mode=mode, seed=4)
    resets = 0
    for k in range(500):
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (k, key)
        assert (b["track_id"] == 0).all()
        act = ro.random_actions(3, k, n * cars)
        act[:, 0] = np.abs(act[:, 0])
        a, b = base.step(act), ts.step(act)
        resets += int(np.asarray(a["done"]).reshape(n, cars).any(1).sum())
    assert resets >= 2 * n                              # every env went through the auto-reset path several times


def test_sequential_cycles_and_the_first_reset_keeps_the_initial_track():
    ts = make_track_set_oracle(_tracks("columbia", "austria", "barcelona"), num_envs=7, auto_reset=True, time_limit_steps=3)
    assert list(contiguous_initial(7, 3)) == [0, 0, 0, 1, 1, 2, 2]
    out = ts.reset(mode=1, seed=1)
    assert list(out["track_id"]) == [0, 0, 0, 1, 1, 2, 2]          # the first reset keeps the initial assignment
    seen = [out["track_id"].copy()]
    for k in range(9):
        out = ts.step(np.zeros((7, 2), np.float32))
        seen.append(out["track_id"].copy())
    seen = np.array(seen)
    # time limit 3 agent steps: an env switches after steps 3, 6, 9 (its episode ends with no collision at zero throttle)
    for j, s in enumerate((1, 2, 3)):
        assert (seen[3 * s] == (seen[0] + s) % 3).all(), seen
        assert (seen[3 * s - 1] == (seen[0] + s - 1) % 3).all(), seen
    # a masked reset switches only the envs it resets
    before = ts.track.copy()
    mask = np.array([1, 0, 0, 0, 0, 0, 1], np.uint8)
    out = ts.reset(mask=mask, mode=1, seed=1)
    assert list(out["track_id"]) == [(before[0] + 1) % 3, *before[1:6], (before[6] + 1) % 3]


def test_manual_order_follows_next_track():
    ts = make_track_set_oracle(_tracks("columbia", "austria", "barcelona"), order="manual", num_envs=5, initial=[2, 2, 1, 0, 0])
    out = ts.reset(mode=1, seed=1)
    assert list(out["track_id"]) == [2, 2, 1, 0, 0]
    ts.set_next_track([1, 0, 2, 2, 7])                              # 7: outside [0, T), keeps the current track
    out = ts.reset(mode=1, seed=1)
    assert list(out["track_id"]) == [1, 0, 2, 2, 0]
    out = ts.reset(mode=1, seed=1)                                   # the array persists
    assert list(out["track_id"]) == [1, 0, 2, 2, 0]
    # the spawn of a switched env is the base law on its new track: the same pose as a plain oracle of that track
    (t_col, t_aus, _), n = _tracks("columbia", "austria", "barcelona"), 5
    plain = make_oracle(t_aus, num_envs=n)
    for _ in range(3):
        p = plain.reset(mode=1, seed=1)
    assert np.array_equal(out["pose"][0], p["pose"][0])


def test_random_draws_are_the_philox_law_and_weights_thresholds():
    T, n = 3, 4096
    g, ep = np.arange(n, dtype=np.uint64) + 1000, np.full(n, 5, np.uint32)
    seed = (7 << 32) | 11
    k = draw_tracks(seed, g, ep, T)
    r = ro.philox4x32(g.astype(np.uint32), ep, np.uint32(0), np.uint32(3), seed & 0xFFFFFFFF, seed >> 32)[0]
    assert np.array_equal(k, [(int(x) * T) >> 32 for x in r])
    assert abs(np.bincount(k, minlength=T) / n - 1 / 3).max() < 0.03
    # weights: c_k = min(floor(2^32 S_k / S + 0.5), 2^32 - 1)
    c = weight_thresholds([1.0, 2.0, 1.0])
    assert list(c) == [1 << 30, 3 << 30]
    c = weight_thresholds(np.float32([0.1, 0.7, 0.2]))
    w = [float(np.float32(v)) for v in (0.1, 0.7, 0.2)]
    s = w[0] + w[1] + w[2]
    assert list(c) == [int(np.floor(2.0 ** 32 * w[0] / s + 0.5)), int(np.floor(2.0 ** 32 * (w[0] + w[1]) / s + 0.5))]
    kw = draw_tracks(seed, g, ep, T, c)
    assert np.array_equal(kw, [int(int(x) >= c[0]) + int(int(x) >= c[1]) for x in r])
    assert abs(np.bincount(kw, minlength=T) / n - np.array([0.1, 0.7, 0.2])).max() < 0.03
    assert weight_thresholds([1.0, 1e-30])[0] == 0xFFFFFFFF            # a sliver of a last weight: the clamp
    # the draw depends on the global env id and the episode only (sharding)
    assert np.array_equal(draw_tracks(seed, g[n // 2:], ep[n // 2:], T), k[n // 2:])


def test_random_order_composes_with_vehicle_randomization():
    """The track draw uses its own counter word (3): the spawn (0) and the vehicle draw (2) are those of a set without it."""
    tr = _tracks("columbia", "austria")
    ts = make_track_set_oracle(tr, order="random", seed=5, base=DROracleEnv, num_envs=8, auto_reset=True, time_limit_steps=2)
    ts.set_vehicle_randomization(VP_NOMINAL * np.float32(0.9), VP_NOMINAL * np.float32(1.1), seed=9)
    ts.reset(mode=1, seed=3)
    for k in range(6):
        ts.step(np.zeros((8, 2), np.float32))
    assert (ts.vp != VP_NOMINAL).any(1).all()
    ep = ts.episode.copy()
    assert (ep == 4).all()                                           # the first reset, then resets at steps 2, 4, 6
    want = draw_tracks(5, np.arange(8), ep - 1, 2)
    assert np.array_equal(ts.track, want)


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "racecar_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(", text)))


def test_new_entry_points_are_declared_exported_and_bound(hip_lib):
    from racing_dreamer_amd import _lib
    declared = _declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(hip_lib, name), name
        assert name in _lib.SYMBOLS, name
    assert hip_lib.rc_abi_version() == 3                              # the layout does not change
    # error paths that need no device
    assert hip_lib.rc_set_track_set(None, None, 0, 0, None, None, C.c_uint64(0)) == -1
    assert hip_lib.rc_set_next_track(None, None) == -1
    p = C.c_void_p()
    assert hip_lib.rc_track_ids(None, C.byref(p), None) == -1


def test_new_kernels_are_in_the_builds_refusals():
    from racing_dreamer_amd import build
    for k in ("rc_raycast_ts_kernel", "rc_patch_ts_kernel"):
        assert k in build.NO_SPILL_KERNELS and build.MIN_WAVES_PER_SIMD[k] == 8
    import inspect
    assert "rc_raycast_ts_kernel" in inspect.signature(build.check_async_load_registers).parameters["kernels"].default
