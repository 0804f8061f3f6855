"""Per-episode domain randomization, CPU side: the test-side restatement (tests/dr_oracle.py) that the GPU tests compare
against, and the C-ABI surface (include/racecar_hip.h, rc_set_vehicle_randomization / rc_set_vehicle_params /
rc_vehicle_params / rc_set_lidar_noise)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dr_oracle import (VP_NOMINAL, apply_noise, draw_vehicle, lowbias32, make_dr_oracle, noise_car_key, noise_params,
                       noise_words, noise_z_and_drop)
from helpers import make_oracle
from oracle import racecar_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rc_set_vehicle_randomization", "rc_set_vehicle_params", "rc_vehicle_params", "rc_set_lidar_noise")


def test_nominal_values_are_the_spec_constants_bit_for_bit():
    from racing_dreamer_amd import spec
    assert np.array_equal(VP_NOMINAL, np.array(spec.VEHICLE_NOMINAL, np.float32))
    assert np.array_equal(VP_NOMINAL, np.array([ro.WHEEL_MAX, ro.ACCEL_MAX, ro.DRAG, ro.MAX_VEL, ro.STEER_STEP], np.float32))
    assert np.float32(-VP_NOMINAL[0]) == ro.STEER_GAIN
    text = open(os.path.join(ROOT, "racing_dreamer_amd", "csrc", "racecar_spec.h")).read()
    for name, v in zip(("RCS_WHEEL_MAX", "RCS_ACCEL_MAX", "RCS_DRAG", "RCS_MAX_VEL", "RCS_STEER_STEP"), VP_NOMINAL):
        assert np.float32(re.search(name + r"\s+([-0-9.e]+)f", text).group(1)) == v, name
    lo, hi = (np.asarray(spec.DR_DEPLOYMENT_LOCK[k], np.float32) for k in ("lo", "hi"))
    assert (lo[0], hi[0]) == (np.float32(0.168), np.float32(0.294)) and np.array_equal(lo[1:], VP_NOMINAL[1:])
    assert np.array_equal(hi[1:], VP_NOMINAL[1:])


@pytest.mark.parametrize("track_name,cars", [("austria", 1), ("austria", 2), ("treitlstrasse_v2", 1), ("treitlstrasse_v2", 2)])
def test_degenerate_randomization_equals_the_base_oracle(track_name, cars):
    """lo == hi == nominal, noise off: every output of the subclass is the base oracle's, through 300 steps with auto-reset."""
    from racing_dreamer_amd.track_assets import load_track
    t = load_track(track_name)
    n = 6
    base = make_oracle(t, num_envs=n, cars_per_env=cars, auto_reset=True)
    dr = make_dr_oracle(t, num_envs=n, cars_per_env=cars, auto_reset=True)
    dr.set_vehicle_randomization(VP_NOMINAL, VP_NOMINAL, seed=99)
    a, b = base.reset(mode=2 if cars > 1 else 1, seed=4), dr.reset(mode=2 if cars > 1 else 1, seed=4)
    resets = 0
    for k in range(300):
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (k, key)
        act = ro.random_actions(3, k, n * cars)
        act[:, 0] = np.abs(act[:, 0])
        a, b = base.step(act, repeat=2), dr.step(act, repeat=2)
        resets += int(np.asarray(a["done"]).sum())
    assert np.array_equal(dr.vp, np.tile(VP_NOMINAL, (n * cars, 1)))
    assert resets > 0                                   # the auto-reset path (and its draw) was taken


def test_drawn_parameters_lie_in_the_band_hold_for_an_episode_and_change_at_resets():
    lo = np.array([0.168, 2.0, 0.4, 3.0, 0.02], np.float32)
    hi = np.array([0.294, 6.0, 1.2, 7.0, 0.05], np.float32)
    v = draw_vehicle(12345, np.arange(64), np.zeros(64, np.uint32), lo, hi, 2)
    assert v.shape == (64, 2, 5) and (v >= lo).all() and (v <= hi).all()
    assert len(np.unique(v[:, :, 0])) == 128                    # every car its own value
    # a shard starting at env 32 draws what envs 32.. of the 64-env job draw
    part = draw_vehicle(12345, 32 + np.arange(32), np.zeros(32, np.uint32), lo, hi, 2)
    assert np.array_equal(part, v[32:])
    # constant within an episode, new at every reset
    from racing_dreamer_amd.track_assets import load_track
    t = load_track("austria")
    env = make_dr_oracle(t, num_envs=8, cars_per_env=1, auto_reset=True, time_limit_steps=20)
    env.set_vehicle_randomization(lo, hi, seed=7)
    env.reset(mode=1, seed=1)
    assert np.array_equal(env.vp, draw_vehicle(7, np.arange(8), np.zeros(8, np.uint32), lo, hi, 1)[:, 0])
    changed = 0
    for k in range(60):
        before = env.vp.copy()
        act = ro.random_actions(2, k, 8)
        out = env.step(act, repeat=4)
        done = np.asarray(out["done"]).astype(bool)
        assert np.array_equal(env.vp[~done], before[~done]), k
        if done.any():
            changed += int((env.vp[done] != before[done]).any(axis=1).sum())
            assert (env.vp[done] >= lo).all() and (env.vp[done] <= hi).all()
    assert changed > 0
    # starts do not change: the spawn draw uses counter word 3 = 0, the vehicle draw 2
    plain = make_oracle(t, num_envs=8, cars_per_env=1, auto_reset=True)
    a = plain.reset(mode=1, seed=1)
    env2 = make_dr_oracle(t, num_envs=8, cars_per_env=1, auto_reset=True)
    env2.set_vehicle_randomization(lo, hi, seed=7)
    b = env2.reset(mode=1, seed=1)
    assert np.array_equal(a["pose"], b["pose"])


def test_lowbias32_known_values_and_integer_restatement():
    # lowbias32(0) = 0; values computed in pure Python integers
    def ref(x):
        x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF; x ^= x >> 16
        return x
    xs = np.array([0, 1, 2, 0xFFFFFFFF, 0x9E3779B9, 123456789], np.uint32)
    assert lowbias32(xs).tolist() == [ref(int(x)) for x in xs]
    scale, drop = noise_params(0.3, 0.05)
    assert scale == np.float32(np.float32(0.3) * np.float32(4.2286398820579052e-4)) and drop == 3277


def test_noise_statistics():
    """>= 10^6 samples: z has zero mean and unit variance, the dropout rate is p, and neighbouring beams, steps and cars are
    uncorrelated."""
    cars = 1024
    key = noise_car_key(0xC0FFEE, np.arange(cars), np.full(cars, 3), np.full(cars, 40))
    w0, w1 = noise_words(key)
    kz, d = noise_z_and_drop(w0, w1)
    z = kz * float(np.float32(4.2286398820579052e-4))          # [1024, 1080]: 1.1 M samples
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(0.8 / n)           # var of z^2 for Irwin-Hall(4) standardised: 1.8 - 1 = 0.8
    assert np.abs(z).max() <= 2 * np.sqrt(3) + 1e-6
    for p in (0.01, 0.1, 0.5):
        thr = int(np.floor(p * 65536 + 0.5))
        rate = (d < thr).mean()
        assert abs(rate - p) < 5 * np.sqrt(p * (1 - p) / n), p
    tol = 5 / np.sqrt(n)
    corr = lambda a, b: np.corrcoef(a.ravel(), b.ravel())[0, 1]
    assert abs(corr(z[:, :-1], z[:, 1:])) < tol                                          # neighbouring beams
    assert abs(corr(z[:-1], z[1:])) < tol                                                # neighbouring cars
    key2 = noise_car_key(0xC0FFEE, np.arange(cars), np.full(cars, 3), np.full(cars, 41))
    z2 = noise_z_and_drop(*noise_words(key2))[0] * 1.0
    assert abs(corr(z, z2)) < tol                                                        # neighbouring sub-steps
    key3 = noise_car_key(0xC0FFEE, np.arange(cars), np.full(cars, 4), np.full(cars, 40))
    assert abs(corr(z, noise_z_and_drop(*noise_words(key3))[0] * 1.0)) < tol            # next episode
    assert abs(corr(z, d.astype(np.float64))) < tol                                      # noise vs dropout
    # sigma = p = 0 is the clean scan; a clean range at 15 m stays 15 m; every range stays in [0, 15]
    r = np.random.default_rng(0).uniform(0, 15, (cars, 1080)).astype(np.float32)
    r[:, ::7] = 15.0
    assert np.array_equal(apply_noise(r, key, 0.0, 0.0), r)
    noisy = apply_noise(r, key, 0.3, 0.05)
    assert (noisy >= 0).all() and (noisy <= 15).all() and (noisy[:, ::7] == 15.0).all()
    moved = (r < 15) & (noisy < 15)
    err = (noisy - r)[moved & (r > 2) & (r < 13)]
    assert abs(err.std() - 0.3) < 0.01 and abs(err.mean()) < 0.01


def test_noisy_oracle_scan_is_the_clean_scan_plus_noise_and_sharding_does_not_change_it():
    from racing_dreamer_amd.track_assets import load_track
    t = load_track("austria")
    full = make_dr_oracle(t, num_envs=8, cars_per_env=2)
    part = make_dr_oracle(t, num_envs=4, cars_per_env=2, first_env=4)
    clean = make_oracle(t, num_envs=8, cars_per_env=2)
    for e in (full, part):
        e.set_lidar_noise(0.3, 0.05, seed=11)
    a, b, c = full.reset(mode=2, seed=5), part.reset(mode=2, seed=5), clean.reset(mode=2, seed=5)
    assert np.array_equal(a["lidar"][8:], b["lidar"])
    assert not np.array_equal(a["lidar"], c["lidar"])
    frac = (a["lidar"] == 15.0).mean() - (c["lidar"] == 15.0).mean()
    assert 0.02 < frac < 0.08                                 # ~5 % of the beams dropped


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
    assert hip_lib.rc_abi_version() == 3
    # error paths that need no device
    lo = (C.c_float * 5)(*VP_NOMINAL)
    assert hip_lib.rc_set_vehicle_randomization(None, lo, lo, C.c_uint64(0)) == -1
    assert hip_lib.rc_set_vehicle_params(None, None) == -1
    assert hip_lib.rc_set_lidar_noise(None, 0.3, 0.0, C.c_uint64(0)) == -1
    p = C.c_void_p()
    assert hip_lib.rc_vehicle_params(None, C.byref(p), None) == -1


def test_new_scan_instantiations_are_in_the_builds_refusals():
    from racing_dreamer_amd import build
    for k in ("rc_raycast_car_noise_kernel", "rc_raycast_group_noise_kernel"):
        assert k in build.NO_SPILL_KERNELS
    assert build.MIN_WAVES_PER_SIMD["rc_raycast_car_noise_kernel"] == 8
    def block(k, spill=0):
        return (f"k.h:1:1: remark: Function Name: _ZN12_GLOBAL__N_1{len(k)}{k}ILi1ELb0EEEv8RcParamsi\n"
                f"k.h:1:1: remark:     ScratchSize [bytes/lane]: 0\nk.h:1:1: remark:     VGPRs Spill: {spill}\n"
                f"k.h:1:1: remark:     Occupancy [waves/SIMD]: 8")
    required = ("rc_raycast_car_kernel", "rc_patch_car_kernel", "rc_raycast_car_noise_kernel", "rc_raycast_group_noise_kernel")
    three = "\n".join(block(k) for k in required[:3])
    with pytest.raises(RuntimeError, match="rc_raycast_group_noise_kernel"):     # a build without the group noise scan's remarks
        build.check_resource_usage(three, required=required)
    build.check_resource_usage(three + "\n" + block(required[3]), required=required)
    with pytest.raises(RuntimeError, match="VGPRs Spill"):
        build.check_resource_usage(three + "\n" + block(required[3], spill=4), required=required)
