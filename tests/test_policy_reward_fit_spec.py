"""The specification of the reward head's fit (tests/policy_fit_spec.c at two hidden layers) against NumPy restatements of
the update - the head's Normal(o, 1) likelihood of the recorded reward (dreamer/models.py:97-100), the reference's `Optimizer`
(dreamer/tools.py:421-455): the forward pass, the analytic backward pass, the global-norm clip and TF's Adam in float64, and the
same in plain float32 (NumPy's own summation order) as the yardstick of what binary32 can give.  The starting weights are the
austria checkpoint's own reward head, the features recorded latents.  No GPU: the device is held to the spec bit for bit by
tests/test_gpu_reward_fit.py."""
import os

import numpy as np

import fit_restatement
from fit_restatement import _elu, _err
from policy_reward_fit_spec import DEFAULTS, KEYS, LAYERS, N_GRAD, PolicyRewardFitSpec
from test_gpu_policy_device import _recorded_inputs

N = 97
CHECKPOINT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dreamer_policy_austria.npz")
_cache = {}

# spec_error <= MARGIN x float32_error per quantity, MARGIN = 2 x the ratio measured on this CPU with these inputs (the inputs are
# fixed, so the ratio is reproducible; the factor 2 leaves room for a later edit of the spec).  Measured ratios, one step at N = 97
# (max |x - float64| over the array; `grad` and `weights` the worst of the six arrays):
#   grad      x 3.05  (hout_b, ONE number: 2.2e-8 against 7.3e-9; the five arrays with more than one element: x 1.06 - 1.43)
#   weights   x 6.03  (hout_b, ONE number: 4.0e-11 against 6.6e-12; the other five arrays: x 1.00 - 1.66)
#   loss      x 1.00  (2.2e-8 both) and  grad_norm  x 4.32  (3.9e-8 against 9.0e-9, one number)
#   weights after three steps  x 1.65  (h1_w; hout_b there x 0.31)
# As in test_policy_fit_spec.py the ratios above x 2 belong to single numbers, where the float32 restatement's one draw happened to
# land close to the float64 value; the arrays - a maximum over hundreds to 160 000 elements - stay at x 1.0 - 1.7.
MARGIN = {"grad": 2 * 3.05, "loss": 2 * 1.00, "grad_norm": 2 * 4.32, "weights": 2 * 6.03, "weights3": 2 * 1.65}


def _head():
    if "head" not in _cache:
        with np.load(CHECKPOINT) as z:
            _cache["head"] = {k: np.array(z[k], np.float32) for k in KEYS}
    return _cache["head"]


def _rows(n=N):
    """features [n, 230] of recorded latents, reward targets and weights."""
    if "rows" not in _cache:
        state = _recorded_inputs(263, seed=3)[1]
        rng = np.random.default_rng(11)
        _cache["rows"] = (np.ascontiguousarray(state[:, :230]), rng.normal(0.1, 0.5, 263).astype(np.float32),
                          rng.uniform(0.2, 1.0, 263).astype(np.float32))
    feat, target, weight = _cache["rows"]
    return feat[:n], target[:n], weight[:n]


def _loss(W, feat, target, weight, dt):
    """(loss, the activations, the output) in dtype dt."""
    a = [feat.astype(dt)]
    for l in range(2):
        a.append(_elu(a[-1] @ W[f"h{l}_w"] + W[f"h{l}_b"]))
    o = (a[2] @ W["hout_w"] + W["hout_b"])[:, 0]
    t, w = target.astype(dt), (np.ones(len(feat), dt) if weight is None else weight.astype(dt))
    lp = dt(-0.5) * (o - t) ** 2 - dt(0.5 * np.log(2 * np.pi))
    return -(w * lp).mean(dtype=dt), a, o


def _gradient(W, feat, target, weight, dt):
    """The analytic gradient in dtype dt: (loss, the six arrays by layer name)."""
    loss, a, o = _loss(W, feat, target, weight, dt)
    t, w = target.astype(dt), (np.ones(len(feat), dt) if weight is None else weight.astype(dt))
    delta = (w * (o - t) / dt(len(feat)))[:, None]
    g = {"hout_w": a[2].T @ delta, "hout_b": delta.sum(0)}
    delta = (delta @ W["hout_w"].T) * np.where(a[2] > 0, 1, a[2] + 1)
    for l in (1, 0):
        g[f"h{l}_w"], g[f"h{l}_b"] = a[l].T @ delta, delta.sum(0)
        if l:
            delta = (delta @ W[f"h{l}_w"].T) * np.where(a[l] > 0, 1, a[l] + 1)
    return loss, {k: g[k].astype(dt) for k in LAYERS}


def Restatement(head, dt, torch=False):
    """fit_restatement.Restatement over the reward head."""
    return fit_restatement.Restatement({k: head[f"reward_{k}"] for k in LAYERS}, DEFAULTS,
                                       lambda W, feat, target, weight=None: _gradient(W, feat, target, weight, dt), dt, torch)


def _ratios(steps=1):
    """{quantity: (spec error, float32 error)} against float64 after `steps` steps at N = 97."""
    if steps not in _cache:
        feat, target, weight = _rows()
        spec, r64, r32 = PolicyRewardFitSpec(_head()), Restatement(_head(), np.float64), Restatement(_head(), np.float32)
        for _ in range(steps):
            s, d, f = (x.step(feat, target, weight) for x in (spec, r64, r32))
        out = {"loss": (_err(s["loss"], d["loss"]), _err(f["loss"], d["loss"])),
               "grad_norm": (_err(s["grad_norm"], d["grad_norm"]), _err(f["grad_norm"], d["grad_norm"]))}
        for k in LAYERS:
            out["grad/" + k] = (_err(s["grad"][k], d["grad"][k]), _err(f["grad"][k], d["grad"][k]))
            out["weights/" + k] = (_err(spec.arrays[k], r64.W[k]), _err(r32.W[k], r64.W[k]))
        _cache[steps] = out
    return _cache[steps]


def test_the_gradient_has_253201_elements():
    """[231][400] | [401][400] | [401][1], and the arrays of a step's gradient have the head's shapes."""
    spec = PolicyRewardFitSpec(_head())
    assert spec.n_grad == N_GRAD == 231 * 400 + 401 * 400 + 401 == 253201
    feat, target, weight = _rows(5)
    got = spec.step(feat, target, weight)
    assert got["grad_flat"].shape == (253201,)
    assert {k: a.shape for k, a in got["grad"].items()} == {k: a.shape for k, a in spec.arrays.items()}


def test_one_step_is_as_close_to_float64_as_float32_can_be():
    """Every gradient array, the loss, the norm and the updated weights of one spec step at N = 97 on the austria checkpoint's
    reward head and recorded latents against the float64 restatement, each within MARGIN x the error of the plain float32
    restatement."""
    for k, (spec_err, f32_err) in _ratios().items():
        print(f"reward {k}: spec {spec_err:.3e} float32 {f32_err:.3e} ratio {spec_err / max(f32_err, 1e-300):.2f}")
        assert f32_err > 0 or spec_err == 0, k
        assert spec_err <= MARGIN[k.split("/")[0]] * f32_err, (k, spec_err, f32_err)


def test_the_analytic_gradient_is_the_slope_of_the_loss():
    """Independent of the formulas: at N = 5, central differences of the float64 loss with respect to 20 randomly chosen weights
    of each layer equal the float64 analytic gradient.  This guards the restatement the spec is measured against."""
    feat, target, weight = _rows(5)
    W = {k: np.asarray(_head()[f"reward_{k}"], np.float64) for k in LAYERS}
    _, g = _gradient(W, feat, target, weight, np.float64)
    rng = np.random.default_rng(4)
    for k in LAYERS:
        flat = W[k].reshape(-1)
        for i in rng.choice(flat.size, min(20, flat.size), replace=False):
            keep, h = flat[i], 1e-6
            flat[i] = keep + h
            up = _loss(W, feat, target, weight, np.float64)[0]
            flat[i] = keep - h
            dn = _loss(W, feat, target, weight, np.float64)[0]
            flat[i] = keep
            slope, want = (up - dn) / (2 * h), g[k].reshape(-1)[i]
            assert abs(slope - want) <= 1e-6 * max(abs(want), 1e-3), (k, int(i), slope, want)


def test_three_steps_follow_tfs_adam():
    """Three consecutive steps (the carried moments, the bias correction at t = 1, 2, 3) against the float64 restatement of TF's
    formula, within MARGIN x the float32 restatement's error."""
    for k, (spec_err, f32_err) in _ratios(steps=3).items():
        if k.startswith("weights/"):
            print(f"reward {k} after 3 steps: spec {spec_err:.3e} float32 {f32_err:.3e} ratio {spec_err / max(f32_err, 1e-300):.2f}")
            assert spec_err <= MARGIN["weights3"] * f32_err, (k, spec_err, f32_err)


def test_epsilon_sits_where_tf_puts_it():
    """TF adds epsilon to sqrt(v), torch to sqrt(v / (1 - beta2^t)): at t = 1 a weight whose gradient is tiny moves measurably
    differently under the two.  The two float64 restatements differ there, and the spec follows TF's."""
    feat, target, weight = _rows()
    spec, tf, th = PolicyRewardFitSpec(_head()), Restatement(_head(), np.float64), Restatement(_head(), np.float64, torch=True)
    for x in (spec, tf, th):
        x.step(feat, target, weight)
    k = "h1_w"
    gap = np.abs(tf.W[k] - th.W[k])
    far = gap > 0.25 * DEFAULTS["lr"]                      # a quarter of the largest move Adam makes in one step
    assert far.sum() >= 10, int(far.sum())
    to_tf, to_torch = np.abs(spec.arrays[k] - tf.W[k])[far], np.abs(spec.arrays[k] - th.W[k])[far]
    assert np.all(to_tf < 0.01 * gap[far]) and np.all(to_torch > 0.9 * gap[far])


def test_clip_scales_above_the_bound_and_is_the_identity_below():
    """Targets scaled so that the norm is >= 2 clip: the applied gradient is g clip / norm (seen in Adam's first moment, m = 0.1 g
    scale).  Norm <= clip / 2: the step equals the step without a clip (clip = 0) bit for bit."""
    feat, target, weight = _rows()
    big = PolicyRewardFitSpec(_head())
    got = big.step(feat, 40 * target, weight, clip=1.0)
    assert got["grad_norm"] >= 2.0, got["grad_norm"]
    scale = np.float32(1.0) / got["grad_norm"]
    assert np.array_equal(big.m, np.float32(1.0 - np.float32(0.9)) * (got["grad_flat"] * scale))
    small, none = PolicyRewardFitSpec(_head()), PolicyRewardFitSpec(_head())
    a = small.step(feat, target, weight, clip=100.0)
    b = none.step(feat, target, weight, clip=0.0)
    assert 0 < a["grad_norm"] <= 50.0 and a["grad_norm"] == b["grad_norm"]
    assert small.m.tobytes() == none.m.tobytes() and small.v.tobytes() == none.v.tobytes()
    for k in LAYERS:
        assert small.arrays[k].tobytes() == none.arrays[k].tobytes(), k
    assert np.array_equal(small.m, np.float32(1.0 - np.float32(0.9)) * a["grad_flat"])


def test_a_step_whose_norm_is_not_finite_is_skipped():
    """One NaN target: skipped = 1, and weights, moments and the step count are byte for byte what they were - after a good step,
    so that the moments are not zero."""
    feat, target, weight = _rows()
    spec = PolicyRewardFitSpec(_head())
    assert spec.step(feat, target, weight)["skipped"] == 0 and spec.step_count == 1
    before = {k: a.tobytes() for k, a in spec.arrays.items()}, spec.m.tobytes(), spec.v.tobytes(), spec.opt.b1pow, spec.opt.b2pow
    bad = target.copy()
    bad[13] = np.nan
    got = spec.step(feat, bad, weight)
    assert got["skipped"] == 1 and got["step"] == 1 and spec.step_count == 1 and not np.isfinite(got["grad_norm"])
    assert before == ({k: a.tobytes() for k, a in spec.arrays.items()}, spec.m.tobytes(), spec.v.tobytes(), spec.opt.b1pow, spec.opt.b2pow)
    assert spec.step(feat, target, weight)["step"] == 2
