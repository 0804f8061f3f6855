"""The specification of the critic's fit (tests/policy_fit_spec.c) against NumPy restatements of the reference's
value update (dreamer/models.py:129-137, dreamer/tools.py:421-455): the forward pass, the analytic backward pass, the global-norm clip
and TF's Adam in float64, and the same in plain float32 (NumPy's own summation order) as the yardstick of what binary32 can give.
No GPU: the device is held to the spec bit for bit by tests/test_gpu_policy_fit.py."""
import numpy as np
import pytest

import fit_restatement
from fit_restatement import _elu, _err
from policy_fit_spec import DEFAULTS, LAYERS, PolicyFitSpec, tree_sum
from test_gpu_policy_device import _recorded_inputs

HEADS = ("value", "pcont")
N = 97
_cache = {}

# spec_error <= MARGIN x float32_error per quantity, MARGIN = 2 x the ratio measured on this CPU with these inputs (the inputs are
# fixed, so the ratio is reproducible; the factor 2 leaves room for a later edit of the spec).  Measured ratios, one step at N = 97,
# the larger of the two heads (max |x - float64| over the array; `grad` and `weights` the worst of the eight arrays):
#   grad      x 4.65  (pcont hout_b, ONE number: 3.8e-8 against 8.2e-9; the seven arrays with more than one element: x 0.5 - 1.3)
#   weights   x 2.81  (value h1_b, whose 400 elements moved from zero by lr = 8e-5: 5.0e-10 against 1.8e-10; the kernels: x 0.75 - 1.85)
#   loss      x 8.38  (value: 6.8e-8 against 8.1e-9) and  grad_norm  x 8.29  (value: 8.5e-7 against 1.0e-7)
#   weights after three steps  x 1.46
# The two ratios above the x 1.1 - 3.2 of the earlier specs belong to single numbers, not arrays: the spec's loss (0.904) is off by
# 1.1 ulp and its norm (5.008) by 1.8 ulp - the binary32 roundings of the forward pass and of each term, then one rounding of a
# binary64 sum -, while the float32 restatement's one number happened to land within 0.14 and 0.2 ulp.  The error of one float32 number is anywhere in
# [0, a few ulp]; a ratio of two such draws says little, which is why the arrays (a maximum over thousands of elements) stay at
# x 0.2 - 2.8.  pcont's loss has ratio 1.00, its norm 2.62.
# (There is no test of "N rows presented in two calls' worth of scratch": the spec and the device never chunk a call.)
MARGIN = {"grad": 2 * 4.65, "loss": 2 * 8.38, "grad_norm": 2 * 8.29, "weights": 2 * 2.81, "weights3": 2 * 1.46}


def _critic():
    from racing_dreamer_amd.critic import init_critic
    return init_critic(5)


def _rows(n=N):
    """features [n, 230] of recorded latents, targets and weights of the sizes the reference's have."""
    if "rows" not in _cache:
        state = _recorded_inputs(263, seed=3)[1]
        rng = np.random.default_rng(11)
        _cache["rows"] = (np.ascontiguousarray(state[:, :230]), rng.normal(0.5, 1.0, 263).astype(np.float32),
                          rng.uniform(0.0, 1.0, 263).astype(np.float32), rng.uniform(0.2, 1.0, 263).astype(np.float32))
    feat, value_t, pcont_t, weight = _cache["rows"]
    return feat[:n], {"value": value_t[:n], "pcont": pcont_t[:n]}, weight[:n]


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _loss(W, feat, target, weight, head, dt):
    """(loss, the activations, the output) in dtype dt."""
    a = [feat.astype(dt)]
    for l in range(3):
        a.append(_elu(a[-1] @ W[f"h{l}_w"] + W[f"h{l}_b"]))
    o = (a[3] @ W["hout_w"] + W["hout_b"])[:, 0]
    t, w = target.astype(dt), (np.ones(len(feat), dt) if weight is None else weight.astype(dt))
    if head == "value":
        lp = dt(-0.5) * (o - t) ** 2 - dt(0.5 * np.log(2 * np.pi))
    else:
        lp = -(t * _softplus(-o) + (1 - t) * _softplus(o))
    return -(w * lp).mean(dtype=dt), a, o


def _gradient(W, feat, target, weight, head, dt):
    """The analytic gradient in dtype dt: (loss, the eight arrays by layer name)."""
    loss, a, o = _loss(W, feat, target, weight, head, dt)
    t, w = target.astype(dt), (np.ones(len(feat), dt) if weight is None else weight.astype(dt))
    e = (o - t) if head == "value" else (1 / (1 + np.exp(-o)) - t)
    delta = (w * e / dt(len(feat)))[:, None]
    g = {"hout_w": a[3].T @ delta, "hout_b": delta.sum(0)}
    delta = (delta @ W["hout_w"].T) * np.where(a[3] > 0, 1, a[3] + 1)
    for l in (2, 1, 0):
        g[f"h{l}_w"], g[f"h{l}_b"] = a[l].T @ delta, delta.sum(0)
        if l:
            delta = (delta @ W[f"h{l}_w"].T) * np.where(a[l] > 0, 1, a[l] + 1)
    return loss, {k: g[k].astype(dt) for k in LAYERS}


def Restatement(critic, head, dt, torch=False):
    """fit_restatement.Restatement over one head of the critic."""
    return fit_restatement.Restatement({k: critic[f"{head}_{k}"] for k in LAYERS}, DEFAULTS,
                                       lambda W, feat, target, weight=None: _gradient(W, feat, target, weight, head, dt), dt, torch)


def _ratios(head, steps=1):
    """{quantity: (spec error, float32 error)} against float64 after `steps` steps at N = 97."""
    feat, targets, weight = _rows()
    spec, r64, r32 = PolicyFitSpec(_critic(), head), Restatement(_critic(), head, np.float64), Restatement(_critic(), head, np.float32)
    for _ in range(steps):
        s, d, f = (x.step(feat, targets[head], weight) for x in (spec, r64, r32))
    out = {"loss": (_err(s["loss"], d["loss"]), _err(f["loss"], d["loss"])),
           "grad_norm": (_err(s["grad_norm"], d["grad_norm"]), _err(f["grad_norm"], d["grad_norm"]))}
    for k in LAYERS:
        out["grad/" + k] = (_err(s["grad"][k], d["grad"][k]), _err(f["grad"][k], d["grad"][k]))
        out["weights/" + k] = (_err(spec.arrays[k], r64.W[k]), _err(r32.W[k], r64.W[k]))
    return out


@pytest.mark.parametrize("head", HEADS)
def test_one_step_is_as_close_to_float64_as_float32_can_be(head):
    """Every gradient array, the loss, the norm and the updated weights of one spec step at N = 97 on init_critic(5) and recorded
    latents against the float64 restatement, each within MARGIN x the error of the plain float32 restatement."""
    for k, (spec_err, f32_err) in _ratios(head).items():
        print(f"{head} {k}: spec {spec_err:.3e} float32 {f32_err:.3e} ratio {spec_err / max(f32_err, 1e-300):.2f}")
        assert f32_err > 0 or spec_err == 0, k
        assert spec_err <= MARGIN[k.split("/")[0]] * f32_err, (head, k, spec_err, f32_err)


@pytest.mark.parametrize("head", HEADS)
def test_the_analytic_gradient_is_the_slope_of_the_loss(head):
    """Independent of the formulas: at N = 5, central differences of the float64 loss with respect to 20 randomly chosen weights
    of each layer equal the float64 analytic gradient.  This guards the restatement the spec is measured against."""
    feat, targets, weight = _rows(5)
    W = {k: np.asarray(_critic()[f"{head}_{k}"], np.float64) for k in LAYERS}
    _, g = _gradient(W, feat, targets[head], weight, head, np.float64)
    rng = np.random.default_rng(4)
    for k in LAYERS:
        flat = W[k].reshape(-1)
        for i in rng.choice(flat.size, min(20, flat.size), replace=False):
            keep, h = flat[i], 1e-6
            flat[i] = keep + h
            up = _loss(W, feat, targets[head], weight, head, np.float64)[0]
            flat[i] = keep - h
            dn = _loss(W, feat, targets[head], weight, head, np.float64)[0]
            flat[i] = keep
            slope, want = (up - dn) / (2 * h), g[k].reshape(-1)[i]
            assert abs(slope - want) <= 1e-6 * max(abs(want), 1e-3), (head, k, int(i), slope, want)


@pytest.mark.parametrize("head", HEADS)
def test_three_steps_follow_tfs_adam(head):
    """Three consecutive steps (the carried moments, the bias correction at t = 1, 2, 3) against the float64 restatement of TF's
    formula, within MARGIN x the float32 restatement's error."""
    for k, (spec_err, f32_err) in _ratios(head, steps=3).items():
        if k.startswith("weights/"):
            print(f"{head} {k} after 3 steps: spec {spec_err:.3e} float32 {f32_err:.3e} ratio {spec_err / max(f32_err, 1e-300):.2f}")
            assert spec_err <= MARGIN["weights3"] * f32_err, (head, k, spec_err, f32_err)


def test_epsilon_sits_where_tf_puts_it():
    """TF adds epsilon to sqrt(v), torch to sqrt(v / (1 - beta2^t)): at t = 1 a weight whose gradient is tiny moves measurably
    differently under the two.  The two float64 restatements differ there, and the spec follows TF's."""
    feat, targets, weight = _rows()
    spec, tf, th = PolicyFitSpec(_critic(), "value"), Restatement(_critic(), "value", np.float64), Restatement(_critic(), "value", np.float64, torch=True)
    for x in (spec, tf, th):
        x.step(feat, targets["value"], weight)
    k = "h1_w"
    gap = np.abs(tf.W[k] - th.W[k])
    far = gap > 0.25 * DEFAULTS["lr"]                      # a quarter of the largest move Adam makes in one step
    assert far.sum() >= 10, int(far.sum())
    to_tf, to_torch = np.abs(spec.arrays[k] - tf.W[k])[far], np.abs(spec.arrays[k] - th.W[k])[far]
    assert np.all(to_tf < 0.01 * gap[far]) and np.all(to_torch > 0.9 * gap[far])


def test_clip_scales_above_the_bound_and_is_the_identity_below():
    """Targets scaled so that the norm is >= 2 clip: the applied gradient is g clip / norm (seen in Adam's first moment, m = 0.1 g
    scale).  Norm <= clip / 2: the step equals the step without a clip (clip = 0) bit for bit."""
    feat, targets, weight = _rows()
    big = PolicyFitSpec(_critic(), "value")
    got = big.step(feat, 40 * targets["value"], weight, clip=1.0)
    assert got["grad_norm"] >= 2.0, got["grad_norm"]
    scale = np.float32(1.0) / got["grad_norm"]
    assert np.array_equal(big.m, np.float32(1.0 - np.float32(0.9)) * (got["grad_flat"] * scale))
    small, none = PolicyFitSpec(_critic(), "value"), PolicyFitSpec(_critic(), "value")
    a = small.step(feat, targets["value"], weight, clip=100.0)
    b = none.step(feat, targets["value"], weight, clip=0.0)
    assert 0 < a["grad_norm"] <= 50.0 and a["grad_norm"] == b["grad_norm"]
    assert small.m.tobytes() == none.m.tobytes() and small.v.tobytes() == none.v.tobytes()
    for k in LAYERS:
        assert small.arrays[k].tobytes() == none.arrays[k].tobytes(), k
    assert np.array_equal(small.m, np.float32(1.0 - np.float32(0.9)) * a["grad_flat"])


@pytest.mark.parametrize("head", HEADS)
def test_a_step_whose_norm_is_not_finite_is_skipped(head):
    """One NaN target: skipped = 1, and weights, moments and the step count are byte for byte what they were - after a good step,
    so that the moments are not zero."""
    feat, targets, weight = _rows()
    spec = PolicyFitSpec(_critic(), head)
    assert spec.step(feat, targets[head], weight)["skipped"] == 0 and spec.step_count == 1
    before = {k: a.tobytes() for k, a in spec.arrays.items()}, spec.m.tobytes(), spec.v.tobytes(), spec.opt.b1pow, spec.opt.b2pow
    bad = targets[head].copy()
    bad[13] = np.nan
    got = spec.step(feat, bad, weight)
    assert got["skipped"] == 1 and got["step"] == 1 and spec.step_count == 1 and not np.isfinite(got["grad_norm"])
    assert before == ({k: a.tobytes() for k, a in spec.arrays.items()}, spec.m.tobytes(), spec.v.tobytes(), spec.opt.b1pow, spec.opt.b2pow)
    assert spec.step(feat, targets[head], weight)["step"] == 2


def test_the_tree_is_a_sum():
    """pfs_tree over more elements than one pass of its 32 768 slots, against math.fsum; and of squares."""
    import math
    x = np.random.default_rng(0).normal(size=100_003).astype(np.float32)
    assert abs(tree_sum(x) - math.fsum(x.astype(np.float64))) < 1e-9
    assert abs(tree_sum(x, square=True) - math.fsum((x * x).astype(np.float64))) < 1e-8
