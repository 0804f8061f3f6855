"""The binary32 specification of imagination (tests/policy_imagine_spec.c): its GRU against the pinned agent
spec bit for bit, its steps and its reward head against a float64 restatement of the reference's formulas (img_step,
ActionDecoder, DenseDecoder) fed the same normals, the head against the NumPy port, the properties of its random stream, and that
a closed-loop rollout is the open-loop rollout of its own actions; the C-ABI's new symbols."""
import ctypes as C

import numpy as np
import pytest

import policy_imagine_spec as pis
import policy_sample_spec as pss
from oracle.dreamer_policy_port import RAW_INIT_STD, DreamerPolicy
from policy_imagine_spec import PolicyImagineSpec
from policy_spec import PolicySpec
from test_golden_policy import weights
from test_policy_sample_spec import CHECKPOINTS, MARGIN, _inputs

H = 15                    # the reference's horizon (dreamer/models.py:213-224)
WITH_HEAD = [name for name in CHECKPOINTS if "reward_h0_w" in weights(name).files]
f32 = np.float32


def _keys(n, step=0, episode=1, first_env=0):
    return np.stack([first_env + np.arange(n), np.full(n, episode), np.full(n, step), np.zeros(n)], 1).astype(np.uint32)


def _reference_step(w, feat, nrm, mode, actions, dtype):
    """One imagined step of the reference in `dtype` from feat [n, 230] = stoch | deter, fed the normals nrm [n, 36] (the spec's
    layout): the actor (models.py:339-364 ActionDecoder: tanh(mu), or one tanh-normal sample) unless `actions` are given,
    RSSM.img_step (models.py:72-84: img1, the GRU cell, img2, img3; stoch = mean, or mean + std n), and the reward head on the new
    feature (models.py:301-318 DenseDecoder) where the checkpoint has one.  Returns action, stoch, deter, reward (or None)."""
    w = {k: np.asarray(w[k], dtype) for k in w.files if k != "source"}
    elu = lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    softplus = lambda x: np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))
    nrm, feat = np.asarray(nrm, dtype), np.asarray(feat, dtype)
    stoch, deter = feat[:, :30], feat[:, 30:]
    if actions is None:
        h = feat
        for i in range(4):
            h = elu(h @ w[f"h{i}_w"] + w[f"h{i}_b"])
        out = h @ w["hout_w"] + w["hout_b"]
        if "hnorm_gamma" in w:
            out = (out - w["hnorm_mean"]) / np.sqrt(w["hnorm_var"] + dtype(1e-3)) * w["hnorm_gamma"] + w["hnorm_beta"]
            mu, sd = out[:, :2], softplus(out[:, 2:]) + dtype(1e-4)
        else:
            mu, sd = dtype(5.0) * np.tanh(out[:, :2] / dtype(5.0)), softplus(out[:, 2:] + dtype(RAW_INIT_STD)) + dtype(1e-4)
        action = np.tanh(mu + sd * nrm[:, 32:34]) if mode == "sample" else np.tanh(mu)
    else:
        action = np.clip(np.asarray(actions, dtype), -1.0, 1.0)
    x = elu(np.concatenate([stoch, action], 1) @ w["img1_w"] + w["img1_b"])
    mx, mh = x @ w["gru_kernel"] + w["gru_bias"][0], deter @ w["gru_recurrent"] + w["gru_bias"][1]
    z, r = sig(mx[:, :200] + mh[:, :200]), sig(mx[:, 200:400] + mh[:, 200:400])
    deter = z * deter + (1 - z) * np.tanh(mx[:, 400:] + r * mh[:, 400:])
    x = elu(deter @ w["img2_w"] + w["img2_b"])
    x = x @ w["img3_w"] + w["img3_b"]
    stoch = x[:, :30] + (softplus(x[:, 30:]) + dtype(0.1)) * nrm[:, :30] if mode == "sample" else x[:, :30]
    return action, stoch, deter, _reference_reward(w, np.concatenate([stoch, deter], 1), dtype)


def _reference_reward(w, feat, dtype):
    if "reward_h0_w" not in (w.files if hasattr(w, "files") else w):
        return None
    elu = lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    h = np.asarray(feat, dtype)
    for i in range(2):
        h = elu(h @ np.asarray(w[f"reward_h{i}_w"], dtype) + np.asarray(w[f"reward_h{i}_b"], dtype))
    return (h @ np.asarray(w["reward_hout_w"], dtype) + np.asarray(w["reward_hout_b"], dtype))[:, 0]


@pytest.mark.parametrize("name", CHECKPOINTS)
def test_the_gru_is_the_pinned_agents_bit_for_bit(name):
    """An open-loop step with action a from (stoch, deter) stores the deter that PolicySpec.act_packed stores from the state
    (stoch, deter, a): both run img1 and the GRU on the same inputs, whatever scan follows.  Actions outside [-1, 1] are clamped
    first, and `action` echoes the clamped value."""
    scan, state, _ = _inputs(name)
    n = len(state)
    rng = np.random.default_rng(5)
    a = rng.uniform(-1.0, 1.0, (n, 2)).astype(f32)
    st = state.copy()
    st[:, 230:] = a
    _, want = PolicySpec(weights(name)).act_packed(scan, st)
    got = PolicyImagineSpec(weights(name)).imagine(state, horizon=1, actions=a[:, None], reward=False, start_reward=False)
    assert np.array_equal(got["feature"][:, 0, 30:], want[:, 30:230]) and np.abs(want[:, 30:230]).max() > 0.1
    assert np.array_equal(got["action"][:, 0], a)
    wild = (3.0 * a).astype(f32)
    got = PolicyImagineSpec(weights(name)).imagine(state, horizon=1, actions=wild[:, None], reward=False, start_reward=False)
    assert np.array_equal(got["action"][:, 0], np.clip(wild, -1.0, 1.0)) and np.abs(wild).max() > 1.0


@pytest.mark.parametrize("name", WITH_HEAD)
def test_the_reward_head_is_the_ports(name):
    """reward_start is the port's predicted_reward(state) to within MARGIN times the port's own (float32) distance from the float64
    restatement, over 16 driven latents."""
    assert len(WITH_HEAD) == 2
    _, state, _ = _inputs(name)
    w = weights(name)
    got = PolicyImagineSpec(w).imagine(state, horizon=1)["reward_start"]
    port = DreamerPolicy(w).predicted_reward(dict(stoch=state[:, :30], deter=state[:, 30:230]))
    want = _reference_reward(w, state[:, :230], np.float64)
    e_spec, e_port = np.abs(got - want).max(), np.abs(port - want).max()
    print(f"{name}: reward_start error against float64: spec {e_spec:.3g}, port {e_port:.3g}, ratio {e_spec / e_port:.2f}; |reward| up to {np.abs(want).max():.3f}")
    assert e_port > 0 and e_spec <= MARGIN * e_port and np.abs(want).max() > 1e-3


@pytest.mark.parametrize("mode", ["mean", "sample"])
def test_imagined_steps_are_the_reference_formulas(mode):
    """16 driven latents per checkpoint, H = 15 steps of the float64 restatement's own rollout; at every step the spec, the
    float64 restatement and the same restatement in float32 take ONE step from the float64 state rounded to binary32 with the
    spec's normals, so a one-step error is measured and nothing compounds.  The spec's largest error (action, stoch, deter over
    four checkpoints; reward over the two with a head) stays within MARGIN times the float32 restatement's own.  The drift of the
    free-running 15-step spec rollout from the free-running float64 one is printed, not asserted.
    Measured (action / stoch / deter / reward): mean - spec 7.9e-06 / 6.6e-06 / 1.2e-05 / 8.2e-07, float32 6.2e-06 / 7.3e-06 /
    7.3e-06 / 4.9e-07, ratios 1.28 / 0.90 / 1.68 / 1.67; sample - spec 7.5e-06 / 5.3e-06 / 1.2e-05 / 1.0e-06, float32 8.0e-06 /
    7.2e-06 / 7.9e-06 / 1.4e-06, ratios 0.93 / 0.73 / 1.52 / 0.74.  Free-running drift at step 15 (feature / reward): mean
    1.2e-04 / 3.6e-07, sample 2.0e-03 / 6.9e-07."""
    err_spec, err_f32, drift = np.zeros(4), np.zeros(4), np.zeros(2)
    for name in CHECKPOINTS:
        w = weights(name)
        pol = PolicyImagineSpec(w)
        _, state, _ = _inputs(name)
        n = len(state)
        feat = state[:, :230].astype(np.float64)
        for t in range(H):
            f_in = feat.astype(f32)
            got = pol.imagine(f_in, _keys(n, step=t), horizon=1, mode=mode, seed=21, start_reward=False)
            nrm = got["normals"][:, 0]
            ref = _reference_step(w, f_in, nrm, mode, None, np.float64)
            r32 = _reference_step(w, f_in, nrm, mode, None, f32)
            mine = (got["action"][:, 0], got["feature"][:, 0, :30], got["feature"][:, 0, 30:], got["reward"][:, 0] if pol.has_head else None)
            for j in range(4 if pol.has_head else 3):
                err_spec[j] = max(err_spec[j], np.abs(mine[j] - ref[j]).max())
                err_f32[j] = max(err_f32[j], np.abs(r32[j] - ref[j]).max())
            feat = np.concatenate([ref[1], ref[2]], 1)
        # free running: the spec's 15 steps against float64's 15 steps under the normals of the spec's rollout
        run = pol.imagine(state, _keys(n), horizon=H, mode=mode, seed=21, start_reward=False)
        f64 = state[:, :230].astype(np.float64)
        for t in range(H):
            a, s, d, r = _reference_step(w, f64, run["normals"][:, t], mode, None, np.float64)
            f64 = np.concatenate([s, d], 1)
        drift[0] = max(drift[0], np.abs(run["feature"][:, -1] - f64).max())
        if pol.has_head:
            drift[1] = max(drift[1], np.abs(run["reward"][:, -1] - r).max())
    print(f"{mode}: largest one-step error against float64 (action, stoch, deter, reward): spec", err_spec, "float32", err_f32, "ratio", err_spec / err_f32)
    print(f"{mode}: free-running drift at step {H} against float64 (feature, reward):", drift)
    assert np.all(err_f32 > 0) and np.all(err_spec <= MARGIN * err_f32), (err_spec, err_f32)


def test_a_cars_draws_do_not_depend_on_the_batch():
    """The normals and every output of (env, slot, episode, agent step) are the same whether the spec is asked for the car alone,
    for a batch with it, for a shard that starts at it (the key carries the GLOBAL env id) or for the batch in another order;
    another seed, env, episode, agent step, slot or imagined step gives other numbers.  The spec has no slot mask: that a masked
    call leaves a car's draws as they are is shown on the device (test_gpu_policy_imagine.py, the slot-mask test)."""
    _, state, _ = _inputs("austria")
    n = len(state)
    pol = PolicyImagineSpec(weights("austria"))
    keys = _keys(n, step=7, episode=3, first_env=40)
    full = pol.imagine(state, keys, horizon=3, mode="sample", seed=9)
    order = np.random.default_rng(1).permutation(n)
    for rows in (np.array([5]), np.arange(5, n), order):
        part = pol.imagine(state[rows], keys[rows], horizon=3, mode="sample", seed=9)
        for k in full:
            assert np.array_equal(part[k], full[k][rows]), k
    base = pis.normals((45, 3, 7, 0), 1, 0, 9, 9)
    assert np.array_equal(base[:32], full["normals"][5, 1, :32]) and np.array_equal(base[32:], full["normals"][5, 1, 32:])
    for key, t, seed in (((46, 3, 7, 0), 1, 9), ((45, 4, 7, 0), 1, 9), ((45, 3, 8, 0), 1, 9), ((45, 3, 7, 1), 1, 9), ((45, 3, 7, 0), 2, 9), ((45, 3, 7, 0), 1, 10)):
        assert not np.any(pis.normals(key, t, 0, 9, seed) == base)


def test_the_stream_is_its_own_and_normal():
    """Tag 5: the blocks of imagined step 0 differ from the agent's (tag 4) blocks of the same key and seed.  2^18 draws
    (1 024 keys x 8 imagined steps x 8 blocks x 4): mean, variance and excess kurtosis within 5 standard errors, lag-1
    correlation within 5 / 512 = 5 standard errors, every draw finite and |n| <= 5.78 (test_policy_sample_spec's checks)."""
    key = (3, 2, 11, 1)
    assert not np.any(pis.normals(key, 0, 0, 9, 77) == pss.normals(key, 0, 9, 77))
    n = np.stack([pis.normals((k % 64, k // 64, 3 * k, k % 4), t, 0, 8, 5) for k in range(1024) for t in range(8)]).reshape(-1).astype(np.float64)
    N = n.size
    assert N == 2 ** 18 and np.all(np.isfinite(n)) and np.abs(n).max() <= 5.78
    mean, var = n.mean(), n.var()
    kurt = ((n - mean) ** 4).mean() / var ** 2 - 3.0
    z = (n - mean) / np.sqrt(var)
    lag1 = float((z[:-1] * z[1:]).mean())
    print(f"mean {mean:.2e} var-1 {var - 1:.2e} kurt {kurt:.2e} lag1 {lag1:.2e}")
    assert abs(mean) <= 5 / np.sqrt(N) and abs(var - 1) <= 5 * np.sqrt(2 / N) and abs(kurt) <= 5 * np.sqrt(24 / N) and abs(lag1) <= 5 / np.sqrt(N)


@pytest.mark.parametrize("name", CHECKPOINTS)
def test_closed_loop_is_open_loop_under_its_own_actions(name):
    """Mode `mean` with the actor's actions equals the open-loop rollout fed the returned actions: features and rewards bit for
    bit (the clamp leaves tanh's values alone); and the input state is not modified."""
    _, state, _ = _inputs(name)
    pol = PolicyImagineSpec(weights(name))
    before = state.copy()
    closed = pol.imagine(state, horizon=H)
    opened = pol.imagine(state, horizon=H, actions=closed["action"])
    assert np.array_equal(state, before)
    for k in closed:
        assert np.array_equal(closed[k], opened[k]), k
    assert np.abs(closed["action"]).max() <= 1.0 and closed["feature"].std(1).max() > 1e-3


def test_imagine_symbols_and_refusals_without_a_handle(hip_lib):
    """The header's new symbols are bound; rc_policy_load_heads checks struct_size and shapes before it looks at the handle and
    names the first wrong array."""
    from racing_dreamer_amd import _lib as L
    for name in ("rc_policy_load_heads", "rc_policy_imagine"):
        assert name in L.SYMBOLS and hasattr(hip_lib, name)
    w = weights("austria")
    h, keep = L.policy_heads(w)
    assert hip_lib.rc_policy_load_heads(None, C.byref(h)) == -1 and b"env is NULL" in hip_lib.rc_last_error()
    h.struct_size = 8
    assert hip_lib.rc_policy_load_heads(None, C.byref(h)) == -1 and b"struct_size" in hip_lib.rc_last_error()
    bad = {k: w[k] for k in L.HEAD_KEYS}
    bad["reward_h1_w"] = np.zeros((400, 399), f32)
    bad["reward_hout_w"] = np.zeros((400, 2), f32)
    h, keep = L.policy_heads(bad)
    assert hip_lib.rc_policy_load_heads(None, C.byref(h)) == -1 and b"reward_h1_w has shape [400, 399]" in hip_lib.rc_last_error()
    assert L.policy_heads(weights("treitlstrasse_20210220")) is None
    a = L.RcPolicyImagineArgs(C.sizeof(L.RcPolicyImagineArgs), 15, 0, 1, 0)
    assert hip_lib.rc_policy_imagine(None, C.byref(a)) == -1
