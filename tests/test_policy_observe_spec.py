"""The binary32 specification of the world model over recorded sequences (tests/policy_observe_spec.c): one
step against the pinned agent spec bit for bit, the hand-over to imagination at `context`, a closed-loop run of the agent
reproduced from its recording, every quantity against a float64 restatement of the reference's obs_step / img_step /
kl_divergence fed the same normals, the KL's sign, the properties of its random stream; the C-ABI's new symbol."""
import ctypes as C
import functools

import numpy as np
import pytest

import policy_imagine_spec as pis
import policy_observe_spec as pos
import policy_sample_spec as pss
from policy_observe_spec import PolicyObserveSpec
from policy_spec import PolicySpec
from test_golden_policy import c_env, weights
from test_policy_sample_spec import CHECKPOINTS, MARGIN, _inputs
from oracle import racecar_oracle as ro

T = 15
WITH_HEAD = [name for name in CHECKPOINTS if "reward_h0_w" in weights(name).files]
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _spec(name):
    return PolicyObserveSpec(weights(name))


@functools.lru_cache(maxsize=None)
def _recorded(name, n=16, steps=T):
    """The checkpoint's own deterministic agent (PolicySpec) closed loop on the C oracle from a reset: per step the scan, the raw
    previous action (0 at step 0) and the agent's state after the step.  The agent is not told of resets, so its latent is one
    chain over the whole recording.  Returns (scan [n, steps, 1080], action [n, steps, 2], states [n, steps, 232])."""
    env, pol = c_env("austria" if name == "austria" else "treitlstrasse_v2", n), PolicySpec(weights(name))
    out = env.reset(mode=ro.RESET_RANDOM, seed=3)
    st = np.zeros((n, 232), f32)
    scans, acts, states = [], [], []
    for _ in range(steps):
        scan = np.asarray(out["lidar"]).reshape(n, 1080).copy()
        scans.append(scan)
        acts.append(st[:, 230:].copy())
        a, st = pol.act_packed(scan, st)
        states.append(st.copy())
        out = env.step(a, repeat=4)
    return np.stack(scans, 1), np.stack(acts, 1), np.stack(states, 1)


@pytest.mark.parametrize("name", CHECKPOINTS)
def test_one_step_is_the_pinned_agents_bit_for_bit(name):
    """T = 1, mode `mean`, from state_in under action[0] = the state's previous action: feature and state_out equal what
    PolicySpec.act_packed stores (stoch | deter), and state_out's action columns are action[0]."""
    assert len(CHECKPOINTS) == 4
    scan, state, _ = _inputs(name)
    _, want = PolicySpec(weights(name)).act_packed(scan, state)
    got = _spec(name).observe(scan[:, None], state[:, None, 230:], state=state, reward=False)
    assert np.array_equal(got["feature"][:, 0], want[:, :230]) and np.array_equal(got["state"][:, :230], want[:, :230])
    assert np.array_equal(got["state"][:, 230:], state[:, 230:]) and np.abs(want[:, 30:230]).max() > 0.1
    assert np.array_equal(got["post_mean"][:, 0], want[:, :30])


@pytest.mark.parametrize("name", CHECKPOINTS)
def test_past_the_context_it_is_imagination_under_the_recorded_actions(name):
    """context = 5 < T = 15, mode `mean`: steps t >= 5 equal PolicyImagineSpec.imagine(state after 5, actions=action[5:]) -
    features, and rewards where a head exists; steps t < 5 equal the context = T run, and post_* / kl stop at the context."""
    scan, act, _ = _recorded(name)
    pol, K = _spec(name), 5
    full, mixed = pol.observe(scan, act), pol.observe(scan, act, context=K)
    head = pol.observe(scan[:, :K], act[:, :K])
    dream = pol.imagine(head["state"], horizon=T - K, actions=act[:, K:], start_reward=False)
    assert np.array_equal(mixed["feature"][:, K:], dream["feature"]) and dream["feature"].std() > 0.01
    if pol.has_head:
        assert np.array_equal(mixed["reward"][:, K:], dream["reward"])
    for k in ("feature", "post_mean", "post_std", "prior_mean", "prior_std", "kl") + (("reward",) if pol.has_head else ()):
        assert np.array_equal(mixed[k][:, :K], full[k][:, :K]), k
    assert np.array_equal(head["feature"], full["feature"][:, :K])
    assert np.all(np.isnan(mixed["kl"][:, K:])) and np.all(np.isnan(mixed["post_std"][:, K:])) and not np.any(np.isnan(full["kl"]))
    assert not np.array_equal(mixed["feature"][:, K:], full["feature"][:, K:])


@pytest.mark.parametrize("name", CHECKPOINTS)
def test_a_recorded_closed_loop_run_is_reproduced_from_zeros(name):
    """The agent's latent after every one of its 15 steps, from the recorded scans and previous actions alone."""
    scan, act, states = _recorded(name)
    got = _spec(name).observe(scan, act, reward=False)
    assert np.array_equal(got["feature"], states[:, :, :230]) and np.array_equal(got["state"][:, :230], states[:, -1, :230])
    assert np.array_equal(got["state"][:, 230:], act[:, -1]) and np.abs(act[:, 1:]).max() > 0.01


def _reference_step(w, scan, action, feat, nrm, observed, mode, dtype):
    """One step of the reference in `dtype` from feat [n, 230] = stoch | deter: RSSM.img_step (dreamer/models.py:72-84: img1 on
    [stoch, action], the GRU cell, img2, img3, std = softplus + 0.1), RSSM.obs_step (models.py:61-71: obs1 on [deter, embed], obs2)
    and tfd.kl_divergence of the two diagonal normals summed over the 30 dimensions (models.py:84-110), fed the normals nrm
    [n, 32].  Returns post_mean, post_std, prior_mean, prior_std, deter, kl, stoch."""
    w = {k: np.asarray(w[k], dtype) for k in w.files if k != "source"}
    elu = lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    softplus = lambda x: np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))
    feat, nrm = np.asarray(feat, dtype), np.asarray(nrm, dtype)[:, :30]
    stoch, deter = feat[:, :30], feat[:, 30:]
    a = np.clip(np.asarray(action, dtype), -1.0, 1.0)
    x = elu(np.concatenate([stoch, a], 1) @ w["img1_w"] + w["img1_b"])
    mx, mh = x @ w["gru_kernel"] + w["gru_bias"][0], deter @ w["gru_recurrent"] + w["gru_bias"][1]
    z, r = sig(mx[:, :200] + mh[:, :200]), sig(mx[:, 200:400] + mh[:, 200:400])
    deter = z * deter + (1 - z) * np.tanh(mx[:, 400:] + r * mh[:, 400:])
    x = elu(deter @ w["img2_w"] + w["img2_b"]) @ w["img3_w"] + w["img3_b"]
    qm, qs = x[:, :30], softplus(x[:, 30:]) + dtype(0.1)
    embed = np.clip(np.asarray(scan, dtype), 0.0, 15.0) / dtype(15.0) - dtype(0.5)
    x = elu(np.concatenate([deter, embed], 1) @ w["obs1_w"] + w["obs1_b"]) @ w["obs2_w"] + w["obs2_b"]
    pm, sp = x[:, :30], softplus(x[:, 30:]) + dtype(0.1)
    kl = (np.log(qs) - np.log(sp) + (sp ** 2 + (pm - qm) ** 2) / (dtype(2.0) * qs ** 2) - dtype(0.5)).sum(1)
    mean, sd = (pm, sp) if observed else (qm, qs)
    return pm, sp, qm, qs, deter, kl, (mean + sd * nrm if mode == "sample" else mean)


def _kl_rounding_bound(pm, sp, qm, qs):
    """By how much the binary32 kl may lie below the exact KL (>= 0) of the normals with the computed parameters, u = 2^-24, per
    dimension: the two logarithms are good to 1 ulp (test_policy_sample_spec: 0.82 measured) = 2 u |log| each and their
    difference rounds once (<= u (|log sq| + |log sp|)): 3 u (|log sq| + |log sp|).  The quotient q = (sp^2 + d^2) / (2 sq^2)
    carries the roundings of d, d d (twice d's, and the fused sum's), sp sp, sq sq and the division: <= 6 u q; the sum with the
    logarithms and the - 1/2 round once each, of values <= |log sq| + |log sp| + q + 1/2.  In all
    u (5 (|log sq| + |log sp|) + 8 q + 1) per dimension.  The ascending sum of 30 terms adds 29 u times the sum of their
    magnitudes.  Second-order terms: a factor 1.01."""
    u = 2.0 ** -24
    pm, sp, qm, qs = (np.asarray(x, np.float64) for x in (pm, sp, qm, qs))
    logs = np.abs(np.log(qs)) + np.abs(np.log(sp))
    q = (sp ** 2 + (pm - qm) ** 2) / (2 * qs ** 2)
    term = np.log(qs) - np.log(sp) + q - 0.5
    return 1.01 * u * ((5 * logs + 8 * q + 1).sum(-1) + 29 * np.abs(term).sum(-1))


@pytest.mark.parametrize("mode", ["mean", "sample"])
def test_observed_steps_are_the_reference_formulas(mode):
    """16 rows x 15 steps per checkpoint, recorded under the checkpoint's own actor on the C oracle.  At every step the spec, the
    float64 restatement and the same restatement in float32 take ONE step from the float64 chain's state rounded to binary32,
    with the spec's normals: a one-step error, nothing compounds.  The spec's largest error over the four checkpoints in
    post_mean, post_std, prior_mean, prior_std, deter and kl stays within MARGIN = 4 times the float32 restatement's own.
    kl >= -(its rounding bound, _kl_rounding_bound) everywhere.  The measured ratios are in DESIGN.md §2 item 17 and
    profiles/policy_observe_spec.txt."""
    names = ("post_mean", "post_std", "prior_mean", "prior_std", "deter", "kl")
    err_spec, err_f32, kl_floor = np.zeros(6), np.zeros(6), np.inf
    for name in CHECKPOINTS:
        w, pol = weights(name), _spec(name)
        scan, act, _ = _recorded(name)
        n = len(scan)
        feat = np.zeros((n, 230), np.float64)
        for t in range(T):
            f_in = feat.astype(f32)
            # (row_offset 4 t: the draws of step 0 of rows 4 t ..: other normals at every step of the chain)
            got = pol.observe(scan[:, t:t + 1], act[:, t:t + 1], mode=mode, seed=21, state=f_in, row_offset=4 * t, reward=False)
            nrm = got["normals"][:, 0]
            ref = _reference_step(w, scan[:, t], act[:, t], f_in, nrm, True, mode, np.float64)
            r32 = _reference_step(w, scan[:, t], act[:, t], f_in, nrm, True, mode, f32)
            mine = (got["post_mean"][:, 0], got["post_std"][:, 0], got["prior_mean"][:, 0], got["prior_std"][:, 0], got["feature"][:, 0, 30:], got["kl"][:, 0])
            for j in range(6):
                err_spec[j] = max(err_spec[j], np.abs(mine[j] - ref[j]).max())
                err_f32[j] = max(err_f32[j], np.abs(r32[j] - ref[j]).max())
            bound = _kl_rounding_bound(*mine[:4])
            assert np.all(got["kl"][:, 0] >= -bound), (name, t)
            kl_floor = min(kl_floor, float((got["kl"][:, 0] + bound).min()))
            feat = np.concatenate([ref[6], ref[4]], 1)
    print(f"{mode}: largest one-step error against float64 ({', '.join(names)}): spec", err_spec, "float32", err_f32, "ratio", err_spec / err_f32)
    print(f"{mode}: smallest kl + rounding bound {kl_floor:.4g}")
    assert np.all(err_f32 > 0) and np.all(err_spec <= MARGIN * err_f32), (err_spec, err_f32)


def test_kl_of_equal_distributions_stays_above_its_rounding_bound():
    """The bound where it matters: post = prior exactly (kl = 0 in exact arithmetic) and post a few ulp from prior, over the range
    of means and stds the checkpoints produce: the binary32 sum of 30 terms is never below -bound."""
    rng = np.random.default_rng(0)
    m = rng.normal(0.0, 2.0, (4096, 30)).astype(f32)
    s = np.exp(rng.uniform(np.log(0.1), np.log(5.0), (4096, 30))).astype(f32)
    m2 = np.nextafter(m, np.where(rng.random(m.shape) < 0.5, -np.inf, np.inf).astype(f32))
    s2 = np.nextafter(s, np.where(rng.random(s.shape) < 0.5, 0, np.inf).astype(f32))
    below = 0
    for case in ((m, s, m, s), (m2, s2, m, s), (m, s, m2, s2)):
        kl = pos.kl(*case)
        below += int((kl < 0).sum())
        assert np.all(kl >= -_kl_rounding_bound(*case)) and np.abs(kl).max() < 1e-4
    print(f"{below} of {3 * 4096} sums of 30 terms are negative")


def test_a_rows_draws_do_not_depend_on_the_batch():
    """Mode `sample`: a row's outputs are the same alone, in a batch, in a shard that starts at it (row_offset compensates) and
    in another order of rows with the same ids - never; ids are positions - but with offsets that put it at the same id; another
    seed, row id or step gives other normals."""
    scan, act, _ = _recorded("austria")
    pol = _spec("austria")
    full = pol.observe(scan, act, context=9, mode="sample", seed=9, row_offset=2 ** 32 - 3)
    for lo, hi in ((5, 6), (5, 16), (0, 7)):
        part = pol.observe(scan[lo:hi], act[lo:hi], context=9, mode="sample", seed=9, row_offset=2 ** 32 - 3 + lo)
        for k in full:
            assert np.array_equal(part[k], full[k][lo:hi], equal_nan=True), k
    base = pos.normals(2 ** 32 + 2, 1, 0, 8, 9)
    assert np.array_equal(base, full["normals"][5, 1])
    for row, t, seed in ((2 ** 32 + 3, 1, 9), (2, 1, 9), (2 ** 32 + 2, 2, 9), (2 ** 32 + 2, 1, 10)):
        assert not np.any(pos.normals(row, t, 0, 8, seed) == base)
    mean = pol.observe(scan, act, context=9)
    assert not np.array_equal(mean["feature"][:, :, :30], full["feature"][:, :, :30]) and np.array_equal(mean["prior_mean"][:, 0], full["prior_mean"][:, 0])


def test_the_stream_is_its_own():
    """Tag 6: the blocks of (row id = env | episode << 32, t = agent step) differ from the agent's (tag 4) and from imagination's
    (tag 5, imagined step 0) blocks of the same counter words, key and seed."""
    env, episode, step = 3, 2, 11
    mine = pos.normals(env | (episode << 32), step, 0, 8, 77)
    assert not np.any(mine == pss.normals((env, episode, step, 0), 0, 8, 77))
    assert not np.any(mine == pis.normals((env, episode, step, 0), 0, 0, 8, 77))
    assert np.all(np.isfinite(mine)) and np.abs(mine).max() <= 5.78


def test_observe_symbol_and_refusals_without_a_handle(hip_lib):
    from racing_dreamer_amd import _lib as L
    assert "rc_policy_observe" in L.SYMBOLS and hasattr(hip_lib, "rc_policy_observe")
    a = L.RcPolicyObserveArgs(C.sizeof(L.RcPolicyObserveArgs), 15, 15, 0, 1)
    assert C.sizeof(L.RcPolicyObserveArgs) == 128
    assert hip_lib.rc_policy_observe(None, C.byref(a)) == -1
    assert L.OBSERVE_MAX_LENGTH == 64 and L.OBSERVE_MODES == {"mean": 0, "sample": 1}
