"""The binary32 specification of the deterministic Dreamer agent (tests/policy_spec.c) against the NumPy port of
the reference's agent (oracle/dreamer_policy_port.py), against float64, and in closed loop on the C oracle; the C-ABI's new
symbols on a box without a GPU."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from oracle import racecar_oracle as ro
from oracle.dreamer_policy_port import DreamerPolicy
from policy_spec import PolicySpec, scalar_map
from test_golden_policy import GOLDEN, c_env, drive, weights

CHECKPOINTS = sorted(os.path.basename(p)[len("dreamer_policy_"):-4] for p in glob.glob(os.path.join(GOLDEN, "dreamer_policy_*.npz")))
# test_the_spec_is_the_port_to_rounding: the spec's largest error against float64 may exceed the port's by this factor.
# Measured (all four checkpoints, grid and random starts, 200 agent steps, every 8th step evaluated):
#   spec  action 1.20e-03, stoch 1.08e-04, deter 3.41e-06      port  action 5.08e-04, stoch 5.88e-05, deter 3.00e-06
#   ratios 2.35, 1.84, 1.14 -> 4 is the smallest power of two they all clear  (the action's figures are the two "normalized"
#   checkpoints': their batch normalisation divides the output layer's error by a standard deviation of a few hundredths)
MARGIN = 4.0


def _act64(w, scan, state):
    """One deterministic agent step in float64: the port's formulas, every array promoted."""
    w = {k: np.asarray(w[k], np.float64) for k in w.files if k != "source"}
    elu = lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    stoch, deter, prev = (np.asarray(state[k], np.float64) for k in ("stoch", "deter", "action"))
    embed = np.clip(np.asarray(scan, np.float64), 0.0, 15.0) / 15.0 - 0.5
    x = elu(np.concatenate([stoch, prev], 1) @ w["img1_w"] + w["img1_b"])
    mx, mh = x @ w["gru_kernel"] + w["gru_bias"][0], deter @ w["gru_recurrent"] + w["gru_bias"][1]
    z, r = sig(mx[:, :200] + mh[:, :200]), sig(mx[:, 200:400] + mh[:, 200:400])
    deter = z * deter + (1.0 - z) * np.tanh(mx[:, 400:] + r * mh[:, 400:])
    x = elu(np.concatenate([deter, embed], 1) @ w["obs1_w"] + w["obs1_b"])
    stoch = (x @ w["obs2_w"] + w["obs2_b"])[:, :30]
    h = np.concatenate([stoch, deter], 1)
    for i in range(4):
        h = elu(h @ w[f"h{i}_w"] + w[f"h{i}_b"])
    out = (h @ w["hout_w"] + w["hout_b"])[:, :2]
    if "hnorm_gamma" in w:
        mu = (out - w["hnorm_mean"][:2]) / np.sqrt(w["hnorm_var"][:2] + 1e-3) * w["hnorm_gamma"][:2] + w["hnorm_beta"][:2]
    else:
        mu = 5.0 * np.tanh(out / 5.0)
    return np.tanh(mu), stoch, deter


def test_the_spec_is_the_port_to_rounding():
    """(scan, state) pairs from runs of the port on the C oracle - 16 cars, grid and random starts, 200 agent steps, all four
    checkpoints - evaluated one step from identical inputs by the port, by PolicySpec and in float64.  The spec's largest error
    against float64 (action, stoch, deter separately) stays within MARGIN times the port's own: a sequential fmaf chain over
    k = 1 280 rounds somewhat worse than BLAS's blocked sums, a wrong formula would be orders of magnitude off.
    Measured: spec 1.20e-03 / 1.08e-04 / 3.41e-06, port 5.08e-04 / 5.88e-05 / 3.00e-06 (action / stoch / deter); ratios 2.35, 1.84, 1.14."""
    assert len(CHECKPOINTS) == 4
    n = 16
    err_spec, err_port = np.zeros(3), np.zeros(3)
    for name in CHECKPOINTS:
        w = weights(name)
        port, spec_pol = DreamerPolicy(w, sample=False), PolicySpec(w)
        track = "austria" if name == "austria" else "treitlstrasse_v2"
        for mode in (ro.RESET_GRID, ro.RESET_RANDOM):
            env = c_env(track, n)
            out = env.reset(mode=mode, seed=2)
            state = port.initial(n)
            for k in range(200):
                scan = np.asarray(out["lidar"]).reshape(n, 1080)
                fresh = np.asarray(out["fresh"]).reshape(n) != 0
                if k and fresh.any():
                    keep = (~fresh)[:, None].astype(np.float32)
                    state = {key: v * keep for key, v in state.items()}
                a_port, s_port = port.act(scan, state)
                if k % 8 == 0:
                    a_spec, s_spec = spec_pol.act(scan, state)
                    a64, st64, de64 = _act64(w, scan, state)
                    for j, (got_s, got_p, ref) in enumerate(((a_spec, a_port, a64), (s_spec["stoch"], s_port["stoch"], st64),
                                                              (s_spec["deter"], s_port["deter"], de64))):
                        err_spec[j] = max(err_spec[j], np.abs(got_s - ref).max())
                        err_port[j] = max(err_port[j], np.abs(got_p - ref).max())
                state = s_port
                out = env.step(a_port, repeat=4)
    print("largest error against float64 (action, stoch, deter): spec", err_spec, "port", err_port, "ratio", err_spec / err_port)
    assert np.all(err_port > 0) and np.all(err_spec <= MARGIN * err_port), (err_spec, err_port)


def _ulp_error(got, x64, want64):
    want32 = want64.astype(np.float32)
    ulp = np.spacing(np.abs(want32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want64) / ulp


def test_the_specs_exp_elu_sigmoid_tanh_against_libm():
    """The spec's scalar functions against libm in float64 over a dense grid of the range the layers produce (+-20) and the edges
    (0, subnormals, +-large).  Measured: exp 1.03 ulp, elu 1.33, sigmoid 2.47, tanh 2.65.  Bounds, from the operations:
    exp = (1 + q) 2^n: half an ulp for the last addition, and q's own error (its rounding, the two-step reduction's, the
    dropped r^8 / 8!: together under half an ulp of 1) counts double where 1 + q < 1 -> 1.5 ulp; elu = exp - 1 loses at most
    1 / (1 - 2^-1/2) = 3.4 by cancellation where n != 0 and nothing where n = 0 -> 4 ulp; sigmoid = 1 / (1 + exp): 1.5 + two
    roundings -> 2.5 ulp; tanh = e / (e + 2), e = expm1: e's 4 ulp at most, times 2 / (e + 2) <= 1, + two roundings -> 5 ulp.
    Beyond |x| = 86 exp saturates by construction: its consumers (ELU -> -1, sigmoid -> 0 / 1, tanh -> +-1) are there already."""
    x = np.concatenate([np.linspace(-20.0, 20.0, 2_000_001), np.linspace(-1e-3, 1e-3, 200_001), np.linspace(-85.0, 85.0, 400_001),
                        [0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754944e-38, -1.1754944e-38]]).astype(np.float32)
    x64 = x.astype(np.float64)
    worst = {}
    for name, ref, bound in (("exp", np.exp(x64), 1.5), ("elu", np.where(x64 > 0, x64, np.expm1(np.minimum(x64, 0))), 4.0),
                             ("sigmoid", 1.0 / (1.0 + np.exp(-x64)), 2.5), ("tanh", np.tanh(x64), 5.0)):
        worst[name] = float(_ulp_error(scalar_map(name, x), x64, ref).max())
        assert worst[name] <= bound, (name, worst[name])
    print("largest error in ulp:", worst)
    big = np.float32([100.0, 1e10, 3e38, np.inf])
    assert np.array_equal(scalar_map("tanh", big), np.ones(4, np.float32)) and np.array_equal(scalar_map("tanh", -big), -np.ones(4, np.float32))
    assert np.array_equal(scalar_map("sigmoid", big), np.ones(4, np.float32)) and np.all(scalar_map("sigmoid", -big) < 1e-37)
    assert np.array_equal(scalar_map("elu", -big), -np.ones(4, np.float32)) and np.array_equal(scalar_map("elu", big), big)
    assert scalar_map("exp", np.float32([0.0]))[0] == 1.0 and scalar_map("tanh", np.float32([0.0]))[0] == 0.0


@pytest.mark.parametrize("track,mode", [("austria", ro.RESET_GRID), ("austria", ro.RESET_RANDOM), ("barcelona", ro.RESET_GRID)])
def test_the_spec_drives_like_the_port(track, mode):
    """Closed loops diverge under any rounding change, so facts are compared, not trajectories: the austria agent in the spec's
    arithmetic laps without a wall contact above 3 m/s - the assertion of
    test_reference_austria_agent_from_random_poses_and_on_a_track_it_never_saw."""
    n = 16
    crashes, speed, laps = drive(c_env(track, n), PolicySpec(weights("austria")), n, 400, mode=mode)
    assert crashes == 0 and speed > 3.0, (track, mode, crashes, speed)


def test_policy_symbols_and_shape_refusals(hip_lib):
    """The new entry points are exported and bound on a box without a GPU, and rc_policy_load checks the shapes before it
    touches a handle."""
    from racing_dreamer_amd import _lib as L
    for name in ("rc_policy_load", "rc_policy_unload", "rc_policy_act", "rc_policy_state"):
        assert name in L.SYMBOLS and hasattr(hip_lib, name)
    assert L.K_POLICY == 6 and L.K_COUNT == 7 and L.KERNEL_NAMES[L.K_POLICY] == "rc_policy_kernel"
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "racecar_hip.h")).read()
    assert "RC_K_POLICY = 6, RC_K_COUNT = 7" in header and "#define RC_ABI_VERSION 3" in header
    for name in CHECKPOINTS:
        good, keep = L.policy_weights(weights(name))
        assert hip_lib.rc_policy_load(None, C.byref(good)) == -1 and b"env is NULL" in hip_lib.rc_last_error()     # the shapes passed
    w = dict(weights("austria"))
    w["obs1_w"] = w["obs1_w"][:-1]
    bad, keep = L.policy_weights(w)
    assert hip_lib.rc_policy_load(None, C.byref(bad)) == -1 and b"obs1_w has shape [1279, 200]" in hip_lib.rc_last_error()
    w = dict(weights("treitlstrasse_20210220"))
    del w["hnorm_beta"]
    bad, keep = L.policy_weights(w)
    assert hip_lib.rc_policy_load(None, C.byref(bad)) == -1 and b"hnorm" in hip_lib.rc_last_error()
    w = dict(weights("austria"))
    del w["h2_b"]
    with pytest.raises(KeyError):
        L.policy_weights(w)
    assert hip_lib.rc_policy_load(None, None) == -1
    assert hip_lib.rc_policy_act(None, 1) == -1 and hip_lib.rc_policy_unload(None) == -1
