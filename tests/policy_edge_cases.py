"""The numeric edges of the Dreamer units ("where the contract is confirmed"): the comparison rule, the recipes
that take the shipped checkpoints and recorded inputs to the edges of binary32, the spec's answer for each unit, and the guards that
fail a case whose spec answer is ordinary.  tests/test_policy_edge_spec.py runs every case on the CPU (spec + guard),
tests/test_gpu_policy_edges.py runs the device beside it.  Recipes only multiply by powers of two (exact, or one rounding into the
subnormals) or assign special values.

Units: act (modes mean / deploy / explore), imagine, observe, dream, dream_grad, returns (modes mean / sample), value, fit (heads
value / pcont), decode (with its log-likelihood), decode_lidar (with its log-likelihood), reward_fit (the fit engine at two hidden
layers), actor_fit (at four; modes target / grad, eps and weights given), action (the actor's forward alone; modes mean - no eps - and
draw).  `cases(unit)` names a unit's cases,
`make(unit, case)` builds one, `spec(unit, call, mode)` is the spec's answer as {output: float32 array}."""
import functools
from fractions import Fraction

import numpy as np

f32 = np.float32
N, ROW = 33, 17                                # one workgroup and one row; the poisoned row
UNITS = {"act": ("mean", "deploy", "explore"), "imagine": ("mean", "sample"), "observe": ("mean", "sample"), "dream": ("mean", "sample"),
         "dream_grad": ("mean", "sample"), "returns": ("mean", "sample"), "value": ("mean",), "fit": ("value", "pcont"),
         "decode": ("mean",), "decode_lidar": ("mean",), "reward_fit": ("reward",), "actor_fit": ("target", "grad"), "action": ("mean", "draw")}
FIT_UNITS = ("fit", "reward_fit", "actor_fit")     # the units that take optimizer steps: status, weights, moments
PRIVATE = ("m", "v", "out", "grad_hout_w", "grad_hout_b")      # what the spec's answer holds for the guards alone: the device does not offer it
SEED = 77


# ------------------------------------------------------------------ the comparison rule
def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def subnormal(a):
    b = bits(a)
    return ((b & 0x7f800000) == 0) & ((b & 0x007fffff) != 0)


def negzero(a):
    return bits(a) == 0x80000000


def census(a):
    a = np.ascontiguousarray(a, f32)
    return dict(sub=int(subnormal(a).sum()), negzero=int(negzero(a).sum()), inf=int(np.isinf(a).sum()), nan=int(np.isnan(a).sum()),
                zero=int((bits(a) == 0).sum()))


def same(got, want):
    """Two float32 arrays agree when their NaN positions coincide and every other element has the same bytes: +-inf, the sign of
    zero and subnormals are compared exactly, a NaN's sign and payload are not."""
    g, w = np.asarray(got), np.asarray(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    if g.dtype != f32:                                   # (the decoder's uint8 image)
        return bool(np.array_equal(g, w))
    gn, wn = np.isnan(g), np.isnan(w)
    return bool(np.array_equal(gn, wn) and np.array_equal(bits(g).reshape(-1)[~gn.reshape(-1)], bits(w).reshape(-1)[~wn.reshape(-1)]))


def assert_same(got, want, what):
    if same(got, want):
        return
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape and g.dtype == f32, (what, g.shape, w.shape, g.dtype)
    gn, wn = np.isnan(g).reshape(-1), np.isnan(w).reshape(-1)
    bad = np.flatnonzero((gn != wn) | (~gn & ~wn & (bits(g).reshape(-1) != bits(w).reshape(-1))))
    show = [(int(i), f"{bits(g).reshape(-1)[i]:08x}", f"{bits(w).reshape(-1)[i]:08x}") for i in bad[:6]]
    raise AssertionError((what, f"{len(bad)} of {g.size} elements differ (index, device bits, spec bits)", show))


# ------------------------------------------------------------------ exact binary32 arithmetic on the host
def round32(x):
    """A Fraction rounded to binary32 (nearest, ties to even, gradual underflow, overflow to inf), on integers."""
    if x == 0:
        return f32(0.0)
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()          # 2^(e-1) < x < 2^(e+1)
    if Fraction(2) ** e > x:
        e -= 1                                                        # 2^e <= x < 2^(e+1)
    q = max(e, -126) - 23                                              # the last place: 2^q
    scaled = x / Fraction(2) ** q
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m & 1):
        m += 1
    if m * Fraction(2) ** q >= Fraction(2) ** 128:
        return f32(sign * np.inf)
    return f32(sign * float(m * Fraction(2) ** q))                     # (exact in binary64, exact in binary32)


def fma32(a, b, c):
    """fmaf: the exact a b + c, rounded once."""
    a, b, c = float(a), float(b), float(c)
    with np.errstate(all="ignore"):
        plain = np.float64(a) * np.float64(b) + np.float64(c)          # (a b is exact in binary64)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return f32(plain)
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    return f32(plain) if exact == 0 else round32(exact)                # (an exact zero: binary64's sign is IEEE's)


# ------------------------------------------------------------------ racecar_policy_math.h, one binary32 operation per operator
LOG2E, LN2_HI, LN2_LO, LN2, SQRT2 = (f32(float.fromhex(h)) for h in ("0x1.715476p+0", "0x1.62e400p-1", "0x1.7f7d1cp-20", "0x1.62e430p-1", "0x1.6a09e6p+0"))
PC = [f32(v) for v in (0.5, 0.16666667, 0.041666668, 0.0083333338, 0.0013888889, 0.0001984127)]
PL = [f32(v) for v in (3.3333331174e-1, -2.4999993993e-1, 2.0000714765e-1, -1.6668057665e-1, 1.4249322787e-1, -1.2420140846e-1, 1.1676998740e-1,
                       -1.1514610310e-1, 7.0376836292e-2)]


def _exp_parts(x):
    x = f32(x)
    x = x if x > f32(-86.0) else f32(-86.0)                            # (a NaN fails the comparison: -86)
    x = x if x < f32(86.0) else f32(86.0)
    n = f32(np.rint(x * LOG2E))
    r = fma32(n, -LN2_HI, x)
    r = fma32(n, -LN2_LO, r)
    t = fma32(r, PC[5], PC[4])
    for c in (PC[3], PC[2], PC[1], PC[0]):
        t = fma32(r, t, c)
    scale = np.array([(int(n) + 127) << 23], np.uint32).view(f32)[0]
    return fma32(r * r, t, r), n, scale


def m_exp(x):
    q, n, scale = _exp_parts(x)
    return (f32(1.0) + q) * scale


def m_expm1(x):
    q, n, scale = _exp_parts(x)
    return q if n == 0 else (f32(1.0) + q) * scale - f32(1.0)


def m_elu(x):
    x = f32(x)
    return x if x > 0 else m_expm1(x)


def m_sigmoid(x):
    with np.errstate(all="ignore"):
        return f32(1.0) / (f32(1.0) + m_exp(-f32(x)))


def m_tanh(x):
    x = f32(x)
    with np.errstate(all="ignore"):
        e = m_expm1(f32(2.0) * np.abs(x))
        return np.copysign(e / (e + f32(2.0)), x)


def m_log(x):
    b = int(bits(f32(x))[0])
    e = (b >> 23) - 127                                                # (the sign bit enters as the kernel's unsigned shift takes it)
    b = (b & 0x007fffff) | 0x3f800000
    if np.array([b], np.uint32).view(f32)[0] > SQRT2:
        b -= 0x00800000
        e += 1
    f = np.array([b], np.uint32).view(f32)[0] - f32(1.0)
    en = f32(e)
    t = fma32(f, PL[8], PL[7])
    for c in PL[6::-1]:
        t = fma32(f, t, c)
    z = f * f
    y = (f * z) * t
    y = fma32(en, LN2_LO, y)
    y = fma32(f32(-0.5), z, y)
    return fma32(en, LN2_HI, f + y)


def m_log1p(t):
    u = f32(1.0) + f32(t)
    return f32(t) if u == 1 else m_log(u) * (f32(t) / (u - f32(1.0)))


def m_softplus(x):
    x = f32(x)
    return (x if x > 0 else f32(0.0)) + m_log1p(m_exp(-np.abs(x)))


MATH = {"exp": m_exp, "elu": m_elu, "sigmoid": m_sigmoid, "tanh": m_tanh, "log": m_log, "softplus": m_softplus}


def special_arguments():
    """+-0, the smallest and largest subnormal, the smallest normal, +-86 and its neighbours, +-inf, NaN (and the negatives)."""
    one = np.array([0x00000001, 0x007fffff, 0x00800000], np.uint32).view(f32)
    e86 = np.array([86.0, np.nextafter(f32(86.0), f32(np.inf)), np.nextafter(f32(86.0), f32(0.0))], f32)
    return np.concatenate([[f32(0.0), f32(-0.0)], one, -one, e86, -e86, [f32(np.inf), f32(-np.inf), f32(np.nan)]]).astype(f32)


# ------------------------------------------------------------------ recipes
def scaled(a, e):
    """a 2^e, in factors no smaller than 2^-100 (each a normal binary32 number)."""
    out = np.array(a, f32)
    with np.errstate(all="ignore"):
        while e:
            s = max(-100, min(100, e))
            out = out * f32(2.0 ** s)
            e -= s
    return out


def _arrays(npz):
    keys = getattr(npz, "files", None) or npz.keys()
    return {k: np.array(npz[k], f32) for k in keys if k != "source" and np.asarray(npz[k]).dtype.kind == "f"}


@functools.lru_cache(maxsize=None)
def _base():
    from racing_dreamer_amd.critic import init_critic
    from racing_dreamer_amd.decoder import init_lidar_decoder
    from test_golden_policy import weights
    from test_gpu_dream_ahead import _actions, _latents
    from test_gpu_policy_device import _recorded_inputs
    from test_policy_actor_fit_spec import _rows as _actor_rows
    from test_policy_fit_spec import _rows
    from test_policy_reward_fit_spec import _rows as _reward_rows
    scan, state, fresh = _recorded_inputs(2 * N, seed=3)
    feat, targets, weight = _rows(64)
    return dict(reward_rows=_reward_rows(64), actor_rows=_actor_rows(64),
                policy=_arrays(weights("austria")), occ=_arrays(weights("treitlstrasse_occupancy")), critic=_arrays(init_critic(5)),
                ldec=_arrays(init_lidar_decoder(11, -3.0)), scan=scan, state=state, fresh=fresh, latents=_latents(64), actions=_actions(64, 2, 4),
                feat=feat, targets=targets, weight=weight,
                image=(np.random.default_rng(5).integers(0, 2, (N, 64, 64))).astype(np.uint8),
                rec=np.random.default_rng(4).uniform(-1, 1, (N, 2, 2)).astype(f32))


class Call:
    """One case: the weights (policy / critic / ldec, dicts of float32 arrays), the inputs `kw`, the guard's expectations
    {mode: [(output, kind, at least)]} with kind among sub / negzero / inf / nan, an optional custom guard(out, call), an optional
    `clean` twin (the same call without the poison) with the rows that must equal it."""

    def __init__(self, policy=None, critic=None, ldec=None, expect=(), guard=None, clean=None, rows=N, **kw):
        b = _base()
        self.policy = dict(b["policy"]) if policy is None else policy
        self.critic = dict(b["critic"]) if critic is None else critic
        self.ldec = dict(b["ldec"]) if ldec is None else ldec
        self.expect, self.guard, self.clean, self.rows, self.kw = dict(expect), guard, clean, rows, kw


def _edit(src, scale=None, assign=None):
    out = {k: a.copy() for k, a in src.items()}
    for k, e in (scale or {}).items():
        out[k] = scaled(out[k], e)
    for k, v in (assign or {}).items():
        if callable(v):
            v(out[k])
        else:
            out[k][...] = v
    return out


def policy(**kw):
    return _edit(_base()["policy"], **kw)


def occ(**kw):
    return _edit(_base()["occ"], **kw)


def critic(**kw):
    return _edit(_base()["critic"], **kw)


def ldec(**kw):
    return _edit(_base()["ldec"], **kw)


def negzeros(a, step=7):
    """A copy with every `step`-th element of the last axis -0.0."""
    out = np.array(a, f32)
    out[..., ::step] = f32(-0.0)
    return out


BEAMS = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 15.0, np.nextafter(f32(15.0), f32(np.inf)), np.nextafter(f32(15.0), f32(0.0)), 1e30], f32)
BEAMS_AS = np.array([0.0, 15.0, 0.0, 0.0, 0.0, 0.0, 15.0, 15.0, np.nextafter(f32(15.0), f32(0.0)), 15.0], f32)     # what the two selects make of them
RAW = np.array([1.0, -1.0, np.nextafter(f32(1.0), f32(2.0)), np.nextafter(f32(1.0), f32(0.0)), np.nextafter(f32(-1.0), f32(-2.0)),
                np.nextafter(f32(-1.0), f32(0.0)), -0.0, np.nan, np.inf, -np.inf], f32)
RAW_AS = np.array([1.0, -1.0, 1.0, np.nextafter(f32(1.0), f32(0.0)), -1.0, np.nextafter(f32(-1.0), f32(0.0)), -0.0, -1.0, 1.0, -1.0], f32)


def special_scan(scan, values=BEAMS):
    """Row r (over all leading axes) carries values[r % 10] in beams r % 1080, 540 and 1079."""
    out = np.array(scan, f32)
    flat = out.reshape(-1, 1080)
    for r in range(len(flat)):
        flat[r, [r % 1080, 540, 1079]] = values[r % len(values)]
    return out


def special_actions(actions, values=RAW):
    """Row r (over all leading axes but the last two) carries values[r % 10] as its first step's first action and values[(r + 3) % 10] as
    its last step's second."""
    out = np.array(actions, f32)
    flat = out.reshape(-1, out.shape[-2], 2)
    for r in range(len(flat)):
        flat[r, 0, 0] = values[r % len(values)]
        flat[r, -1, 1] = values[(r + 3) % len(values)]
    return out


def poisoned(a, row=ROW):
    out = np.array(a, f32)
    out[row] = np.nan
    return out


def _guard_resolved(unit, clean_kw, resolved_kw):
    """The guard of a case whose special inputs the written selects resolve: the spec's answer equals its answer on the resolved inputs
    in every byte, and differs from its answer on the untouched inputs."""
    def guard(out, call, mode):
        as_resolved = spec(unit, Call(call.policy, call.critic, call.ldec, **{**call.kw, **resolved_kw}), mode)
        untouched = spec(unit, Call(call.policy, call.critic, call.ldec, **{**call.kw, **clean_kw}), mode)
        assert all(same(out[k], as_resolved[k]) for k in out), [k for k in out if not same(out[k], as_resolved[k])]
        assert any(not same(out[k], untouched[k]) for k in out)
    return guard


def _guard_poison(out, call, mode, unit):
    """Row ROW's answer is not the clean twin's (NaN where the row's chain reaches the output; where an ELU or a ReLU stands between,
    `x > 0 ? x : f(x)` takes the NaN to f's clamped end and the row is finite), the other rows hold no NaN and equal the clean
    twin's in every byte."""
    clean = spec(unit, call.clean, mode)
    hit = 0
    for k, a in out.items():
        if a.ndim == 0 or a.shape[0] != call.rows:
            continue
        if a.dtype != f32:                                  # (the decoder's uint8 image)
            assert np.array_equal(np.delete(a, ROW, axis=0), np.delete(clean[k], ROW, axis=0)), k
            continue
        others = np.delete(a, ROW, axis=0)
        hit += int(not same(a[ROW], clean[k][ROW]))
        assert not np.isnan(others).any(), k
        assert same(others, np.delete(clean[k], ROW, axis=0)), k
    assert hit > 0


# ------------------------------------------------------------------ the cases
REWARD_OUT, VALUE_OUT, PCONT_OUT, ACTOR_OUT = ("reward_hout_w", "reward_hout_b"), ("value_hout_w", "value_hout_b"), ("pcont_hout_w", "pcont_hout_b"), ("hout_w", "hout_b")
OCC_OUT, LDEC_OUT = ("dec_h5_k", "dec_h5_b"), ("ldec_params_w", "ldec_params_b")


def _both(keys, e):
    return {k: e for ks in keys for k in ks}


def _inputs(unit, rows=N, horizon=2):
    b = _base()
    if unit == "act":
        return dict(scan=b["scan"][:rows].copy(), state=b["state"][:rows].copy(), fresh=b["fresh"][:rows].copy())
    if unit == "imagine":
        return dict(state=b["state"][:rows].copy(), actions=None, horizon=horizon)
    if unit == "observe":
        return dict(scan=b["scan"][:2 * rows].reshape(rows, 2, 1080).copy(), action=b["rec"][:rows].copy(), state=b["latents"][:rows].copy())
    if unit in ("dream", "dream_grad"):
        return dict(state=b["latents"][:rows].copy(), actions=b["actions"][:rows, :, :horizon].copy())
    if unit == "returns":
        return dict(state=b["latents"][:rows].copy(), actions=None, horizon=horizon)
    if unit == "value":
        return dict(features=b["feat"][:rows].copy())
    if unit == "fit":
        return dict(features=b["feat"][:rows].copy(), target={h: t[:rows].copy() for h, t in b["targets"].items()}, weight=b["weight"][:rows].copy(), steps=1, hyper={})
    if unit == "decode":
        return dict(features=b["feat"][:rows].copy(), target=b["image"][:rows].copy())
    if unit == "decode_lidar":
        return dict(features=b["feat"][:rows].copy(), target=b["scan"][:rows].copy())
    if unit == "reward_fit":                       # (the rows of tests/test_policy_reward_fit_spec.py)
        feat, target, weight = b["reward_rows"]
        return dict(features=feat[:rows].copy(), target={"reward": target[:rows].copy()}, weight=weight[:rows].copy(), steps=1, hyper={})
    if unit in ("actor_fit", "action"):            # (the rows of tests/test_policy_actor_fit_spec.py)
        r = b["actor_rows"]
        if unit == "action":
            return dict(features=r["feat"][:rows].copy(), eps=r["eps"][:rows].copy())
        return dict(features=r["feat"][:rows].copy(), target=r["target"][:rows].copy(), grad_actions=r["grad"][:rows].copy(), eps=r["eps"][:rows].copy(),
                    weight=r["weight"][:rows].copy(), steps=1, hyper={})
    raise KeyError(unit)


LATENT = {"act": "state", "imagine": "state", "observe": "state", "dream": "state", "dream_grad": "state", "returns": "state", "value": "features",
          "fit": "features", "decode": "features", "decode_lidar": "features", "reward_fit": "features", "actor_fit": "features", "action": "features"}
FIRST = {"act": ("policy", "img1"), "imagine": ("policy", "img1"), "observe": ("policy", "img1"), "dream": ("policy", "img1"),
         "dream_grad": ("policy", "img1"), "returns": ("critic", "value_h0"), "value": ("critic", "value_h0"), "fit": ("critic", "value_h0"),
         "decode": ("policy", "dec_h1"), "decode_lidar": ("ldec", "ldec_dense1"), "reward_fit": ("policy", "reward_h0"),
         "actor_fit": ("policy", "h0"), "action": ("policy", "h0")}
OUTPUT_LAYERS = {"act": ("policy", (ACTOR_OUT,)), "imagine": ("policy", (REWARD_OUT, ACTOR_OUT)), "observe": ("policy", (REWARD_OUT,)),
                 "dream": ("policy", (REWARD_OUT,)), "dream_grad": ("policy", (REWARD_OUT,)), "decode": ("policy", (OCC_OUT,)),
                 "decode_lidar": ("ldec", (LDEC_OUT,)), "reward_fit": ("policy", (REWARD_OUT,)), "actor_fit": ("policy", (ACTOR_OUT,)),
                 "action": ("policy", (ACTOR_OUT,))}


def _weights(unit, **edits):
    """{policy=..., critic=..., ldec=...} with `edits` = {which: dict(scale=, assign=)} applied; decode runs the occupancy checkpoint."""
    out = {}
    for which, e in edits.items():
        src = {"policy": occ if unit == "decode" else policy, "critic": critic, "ldec": ldec}[which]
        out[which] = src(**e)
    if unit == "decode" and "policy" not in out:
        out["policy"] = occ()
    return out


def cases(unit):
    """The names of a unit's cases (the table in tests/test_gpu_policy_edges.py says why the others do not apply)."""
    if unit == "reward_fit":                       # the fit unit's, but E2: the likelihood is Normal
        return ["A-zero-layer", "A-negzero-inputs", "B1", "B2", "B3", "B4", "B4-one-row", "C1", "C2", "D3", "D4-target+inf", "D4-target-inf",
                "D4-weight0", "D4-weight-1", "D4-weight-inf", "F"]
    if unit == "actor_fit":
        return ["A-zero-layer", "A-negzero-inputs", "A-no-eps", "B1", "B2", "B1g", "B2g", "B3", "B4", "B4-one-row", "C1", "C2", "D3",
                "D4-target+inf", "D4-target-inf", "D4-weight0+inf-target", "D4-weight-1", "D4-weight-inf", "D5-eps+inf", "D5-eps-inf", "D5-eps-nan",
                "D6-grad-inf", "E2+", "E2-", "E4+", "E4-", "E5-on-target", "F"]
    if unit == "action":
        return ["A-zero-layer", "A-negzero-inputs", "B1", "B2", "B4", "D3", "D5-eps+inf", "D5-eps-inf", "D5-eps-nan", "E2+", "E2-", "E4+", "E4-"]
    names = ["A-zero-layer", "A-negzero-inputs", "B1", "B2", "D3"]
    if unit in ("value", "fit", "decode", "decode_lidar"):
        names.append("B4")
    if unit == "fit":
        names += ["B3", "B4-one-row", "C1", "C2", "D4-target+inf", "D4-target-inf", "D4-weight0", "D4-weight-1", "D4-weight-inf", "E2+", "E2-", "F"]
    if unit in ("returns", "value"):
        names += ["C2", "E2+", "E2-"]
    if unit in ("act", "imagine", "observe", "dream", "dream_grad", "returns"):
        names += ["C3", "C3-inf"]
    if unit in ("act", "observe", "decode_lidar"):
        names.append("D1")
    if unit in ("imagine", "observe", "dream", "dream_grad", "returns"):
        names.append("D2")
    if unit == "act":
        names += ["D3-scan", "E2+", "E2-"]
    if unit == "decode":
        names += ["E2+", "E2-"]
    if unit == "decode_lidar":
        names += ["E1-30", "E1-90", "E1+90", "E1-500"]
    if unit == "observe":
        names += ["E3-same", "E3-far"]
    if unit in ("dream_grad", "returns"):
        names.append("F")
    return names


def _stale_first(unit):
    """Case F's first call for the heads that came after the critic: on ANOTHER head of the same handle, 64 rows, features x 2^127 and
    NaN targets (the fit unit's poison) - an actor step before a reward step, a value-head step before an actor step."""
    big = _inputs("actor_fit" if unit == "reward_fit" else "fit", 64)
    big["features"] = scaled(big["features"], 127)
    if unit == "reward_fit":
        big["target"] = np.full((64, 2), np.nan, f32)
    else:
        big["target"] = {h: np.full(64, np.nan, f32) for h in big["target"]}
    return Call(rows=64, **big)


def _flat_negzeros(a, step=5):
    """A copy with every `step`-th element -0.0, counted over the flattened array."""
    out = np.array(a, f32)
    out.reshape(-1)[::step] = f32(-0.0)
    return out


def _hout_b(lo, hi, v):
    return {"hout_b": lambda a: a.__setitem__(slice(lo, hi), v)}


def _make_actor(unit, case):
    """The cases of actor_fit and action: the actor is the checkpoint's own (Call.policy's h0_w .. hout_b)."""
    kw = _inputs(unit)
    fit = unit == "actor_fit"
    expect, guard = EXPECT.get((unit, case), {}), GUARDS.get((unit, case))
    if case == "A-zero-layer":
        return Call(policy=policy(assign={"h0_w": 0.0, "h0_b": -0.0}), expect=expect, guard=guard, **kw)
    if case == "A-negzero-inputs":
        keys = ("features", "target", "grad_actions", "eps") if fit else ("features", "eps")
        clean = {k: kw[k].copy() for k in keys}
        kw["features"] = negzeros(kw["features"])
        for k in keys[1:]:
            kw[k] = _flat_negzeros(kw[k])
        plus = {k: np.where(negzero(kw[k]), f32(0.0), kw[k]) for k in keys}
        return Call(guard=_guard_resolved(unit, clean, plus), **kw)
    if case == "A-no-eps":
        kw["eps"] = None
        return Call(guard=guard, **kw)
    if case in ("B1", "B2"):
        return Call(policy=policy(scale=_both((ACTOR_OUT,), -135 if case == "B1" else -120)), expect=expect, **kw)
    if case in ("B1g", "B2g"):
        kw["grad_actions"] = scaled(kw["grad_actions"], -135 if case == "B1g" else -120)
        return Call(expect=expect, **kw)
    if case == "B3":
        kw.update(steps=3, hyper=dict(epsilon=float(2.0 ** -80)), weight=scaled(kw["weight"], -60))
        return Call(expect=expect, **kw)
    if case in ("B4", "B4-one-row"):
        rows = 1 if case == "B4-one-row" else N
        kw = _inputs(unit, rows)
        kw["features"] = scaled(kw["features"], -130)
        return Call(policy=policy(assign={"h0_b": 0.0}), expect=expect, guard=guard, rows=rows, **kw)
    if case == "C1":
        # grad: the caller's gradient x 2^100 - every delta and every gradient element is 2^100 times the ordinary one, finite, and its
        # square overflows.  target: targets x 2^100 do the same through act - target (and take the loss to +inf)
        kw["grad_actions"], kw["target"] = scaled(kw["grad_actions"], 100), scaled(kw["target"], 100)
        return Call(expect=expect, **kw)
    if case == "C2":
        return Call(policy=policy(scale={"h1_w": 100, "h2_w": 100}), expect=expect, guard=guard, **kw)
    if case == "D3":
        clean = Call(**kw)
        bad = dict(kw, features=poisoned(kw["features"]))
        return Call(clean=clean, expect=expect, guard=guard or (lambda out, call, mode: _guard_poison(out, call, mode, unit)), **bad)
    if case.startswith("D4"):
        what = case[3:]
        if what.startswith("target"):
            kw["target"][ROW] = np.inf if what == "target+inf" else -np.inf
        elif what == "weight0+inf-target":         # (grad mode takes no target: there the row's action gradient is infinite)
            kw["weight"][ROW], kw["target"][ROW], kw["grad_actions"][ROW] = 0.0, np.inf, np.inf
        else:
            clean = kw["weight"].copy()
            kw["weight"][ROW] = {"weight-1": -1.0, "weight-inf": np.inf}[what]
            guard = None if expect else _guard_differs(unit, dict(weight=clean))
        return Call(expect=expect, guard=guard, **kw)
    if case.startswith("D5"):
        clean = Call(**kw)
        kw["eps"] = kw["eps"].copy()
        kw["eps"][ROW] = {"eps+inf": np.inf, "eps-inf": -np.inf, "eps-nan": np.nan}[case[3:]]
        return Call(clean=None if fit else clean, expect=expect, guard=_guard_eps(unit, clean), **kw)
    if case == "D6-grad-inf":
        kw["grad_actions"][ROW, 1] = np.inf
        return Call(expect=expect, **kw)
    if case in ("E2+", "E2-"):
        return Call(policy=policy(assign=_hout_b(2, 4, 100.0 if case == "E2+" else -100.0)), expect=expect, guard=guard, **kw)
    if case in ("E4+", "E4-"):                     # |o| = 1000: tanh(o / 5) is +-1 exactly (beyond |x| = 9.1)
        return Call(policy=policy(assign=_hout_b(0, 2, 1000.0 if case == "E4+" else -1000.0)), expect=expect, guard=guard, **kw)
    if case == "E5-on-target":
        from policy_actor_fit_spec import PolicyActorFitSpec
        kw["target"] = PolicyActorFitSpec(_base()["policy"]).forward(kw["features"], kw["eps"])["action"]
        return Call(guard=guard, **kw)
    if case == "F":
        return Call(guard=_guard_stale_heads(unit), first=_stale_first(unit), **kw)
    raise KeyError((unit, case))


def make(unit, case):
    """One case of a unit as a Call.  Case F of the fit units and the scratch the four heads share - [2 depth][rows][416] | the output
    delta [rows][nout] | the loss terms [rows], planes at multiples of rows x 416 floats, so the plane offsets depend on the depth AND
    the row count of the call:
      fit (depth 3 after depth 3, the note at its branch below): the 33-row call's six planes [0, 82 368) overlie the 64-row call's a1,
        a2, a3 and the head of delta1.
      reward_fit (depth 2, 33 rows, after an actor step of 64 rows): the actor's eight planes of 26 624 floats are a1 .. a4 [0, 106 496),
        delta1 .. delta4 [106 496, 212 992), then its output deltas [64][4] and loss terms to 213 312.  The reward call's four planes of
        13 728 floats [0, 54 912), its output deltas [54 912, 54 945) and its loss terms [54 945, 54 978) overlie the actor's a1, a2 and
        the head of a3 - +inf and expm1(-86) from the overflowed layers - and are rewritten in full but for the padding columns; all of the
        actor's NaN delta planes lie past the reward call's end, where a row or plane index that ran over would read.
      actor_fit (depth 4, 33 rows, after a value-head step of 64 rows): the value head's six planes are a1, a2, a3 [0, 79 872) and
        delta1, delta2, delta3 [79 872, 159 744), then its output deltas and loss terms to 159 872.  The actor's eight planes [0, 109 824)
        overlie a1, a2, a3, delta1 and the head of delta2: its own delta planes (from 54 912) start inside the value head's a3, its
        output deltas [109 824, 109 956) and loss terms [109 956, 109 989) lie in the value head's NaN delta2.  Stale past its end: the
        rest of delta2, delta3, the output deltas.
    The scratch is not reallocated by the smaller call (it needs fewer floats: 54 978 < 213 312, 109 989 < 159 872) and both heads'
    optimizers stay open, so it is not freed in between."""
    if unit in ("actor_fit", "action"):
        return _make_actor(unit, case)
    kw = _inputs(unit)
    lat = LATENT[unit]
    if case == "A-zero-layer":
        which, layer = FIRST[unit]
        assign = {layer + "_w": 0.0, layer + "_b": -0.0}
        if which == "critic":
            assign.update(pcont_h0_w=0.0, pcont_h0_b=-0.0)
        return Call(**_weights(unit, **{which: dict(assign=assign)}), expect=EXPECT.get((unit, case), {}), guard=GUARDS.get((unit, case)), **kw)
    if case == "A-negzero-inputs":
        clean = {k: (None if v is None else np.array(v)) for k, v in kw.items() if k in (lat, "scan", "actions", "action", "target") and not isinstance(v, dict)}
        kw[lat] = negzeros(kw[lat])
        for k in ("scan", "actions", "action"):
            if kw.get(k) is not None:
                kw[k] = negzeros(kw[k], 5)
        if unit == "decode_lidar":
            kw["target"] = negzeros(kw["target"], 5)
        if unit in ("imagine", "returns"):
            kw["actions"] = negzeros(_base()["actions"][:N, 0, :2], 3)
        # where no output shows a -0 the guard is the definition: a -0 input is worth a +0 in every byte of the answer
        plus = {k: np.where(negzero(v), f32(0.0), v) if v is not None and v.dtype == f32 else v for k, v in kw.items() if k in clean}
        guard = None if EXPECT.get((unit, case)) else _guard_resolved(unit, clean, plus)
        return Call(**_weights(unit), expect=EXPECT.get((unit, case), {}), guard=guard, **kw)
    if case in ("B1", "B2"):
        e = -135 if case == "B1" else -120
        if unit in ("returns", "value"):
            w = dict(policy=policy(scale=_both((REWARD_OUT,), e)), critic=critic(scale=_both((VALUE_OUT, PCONT_OUT), e)))
        elif unit == "fit":
            w = dict(critic=critic(scale=_both((VALUE_OUT, PCONT_OUT), e)))
        else:
            which, layers = OUTPUT_LAYERS[unit]
            w = _weights(unit, **{which: dict(scale=_both(layers, e))})
        return Call(**w, expect=EXPECT.get((unit, case), {}), **kw)
    if case in ("B4", "B4-one-row"):
        rows = 1 if case == "B4-one-row" else N
        kw = _inputs(unit, rows)
        kw["features"] = scaled(kw["features"], -130)
        which, layer = FIRST[unit]
        w = _weights(unit, **{which: dict(assign={layer + "_b": 0.0, **({"pcont_h0_b": 0.0} if which == "critic" else {})})})
        return Call(**w, expect=EXPECT.get((unit, case), {}), guard=GUARDS.get((unit, case)), rows=rows, **kw)
    if case == "B3":
        kw.update(steps=3, hyper=dict(epsilon=float(2.0 ** -80)), weight=scaled(kw["weight"], -60))
        return Call(expect=EXPECT.get((unit, case), {}), **kw)
    if case == "C1" and unit == "reward_fit":
        # the last hidden layer x 2^40: a2, the output and its delta are 2^40 times the trained ones, the output layer's gradient a2^T delta
        # 2^80 times: finite, and every square overflows
        return Call(policy=policy(scale={"reward_h1_w": 40}), expect=EXPECT.get((unit, case), {}), **kw)
    if case == "C2" and unit == "reward_fit":
        # both hidden layers x 2^100: a1 is 2^100 times the trained one, a2 +inf wherever its sum is positive, the output inf - inf
        return Call(policy=policy(scale={"reward_h0_w": 100, "reward_h1_w": 100}), expect=EXPECT.get((unit, case), {}), **kw)
    if case == "C1":
        return Call(critic=critic(scale={"value_h1_w": 40, "pcont_h1_w": 40}), expect=EXPECT.get((unit, case), {}), **kw)
    if case == "C2":
        extra = {"pcont_h1_w": 100, "pcont_h2_w": 100} if unit == "fit" else {}
        return Call(critic=critic(scale={"value_h1_w": 100, "value_h2_w": 100, **extra}), expect=EXPECT.get((unit, case), {}), **kw)
    if case == "C3":
        # (GUARDS holds None for dream_grad: `get` then returns that None, not the default, and the census in EXPECT is the guard)
        return Call(policy=policy(scale={"gru_kernel": 100}), expect=EXPECT.get((unit, case), {}), guard=GUARDS.get((unit, case), _guard_saturated_gru), **kw)
    if case == "C3-inf":
        # +-inf in the carried deter of four rows (none of them a fresh car of act): h R is +-inf where one infinity enters a column and
        # NaN where two of opposite effect do, so sigma and tanh of the GRU meet +-inf and NaN; the trained weights
        st = kw["state"]
        st[4, 30 + 7] = np.inf
        st[9, 30 + 7], st[9, 30 + 150] = np.inf, -np.inf
        st[20, 30 + 199] = -np.inf
        st[32, 30 + 0], st[32, 30 + 100] = np.inf, np.inf
        return Call(expect=EXPECT.get((unit, case), {}), guard=_guard_inf_gru, **kw)
    if case == "D1":
        k = "target" if unit == "decode_lidar" else "scan"
        clean = kw[k]
        kw[k] = special_scan(clean)
        return Call(guard=_guard_resolved(unit, {k: clean}, {k: special_scan(clean, BEAMS_AS)}), **kw)
    if case == "D2":
        k = "action" if unit == "observe" else "actions"
        clean = kw[k] if kw[k] is not None else _base()["actions"][:N, 0, :2].copy()
        kw[k] = special_actions(clean)
        guard = _guard_resolved(unit, {k: clean}, {k: special_actions(clean, RAW_AS)})
        if unit == "dream_grad":
            def guard(out, call, mode, inner=guard):
                inner({k: a for k, a in out.items() if k != "grad_actions"}, call, mode)
                _guard_grad_at_the_clamp(out["grad_actions"], call.kw["actions"])
        return Call(guard=guard, **kw)
    if case == "D3-scan":                      # (the scan's two selects take a NaN to 0: no NaN reaches the latent)
        clean = kw["scan"]
        kw["scan"] = poisoned(clean)
        zero = clean.copy()
        zero[ROW] = 0.0
        return Call(guard=_guard_resolved(unit, dict(scan=clean), dict(scan=zero)), **kw)
    if case == "D3" and unit in ("fit", "reward_fit"):
        kw[lat] = poisoned(kw[lat])
        return Call(expect=EXPECT.get((unit, case), {}), **kw)
    if case == "D3":
        clean = Call(**_weights(unit), **kw)
        key = lat
        bad = dict(kw)
        bad[key] = poisoned(kw[key])
        return Call(**_weights(unit), clean=clean, guard=lambda out, call, mode: _guard_poison(out, call, mode, unit), **bad)
    if case.startswith("D4"):
        what, clean = case[3:], kw["weight"].copy()
        if what.startswith("target"):
            for t in kw["target"].values():
                t[ROW] = np.inf if what == "target+inf" else -np.inf
        else:
            kw["weight"][ROW] = {"weight0": 0.0, "weight-1": -1.0, "weight-inf": np.inf}[what]
        guard = None if EXPECT.get((unit, case)) else _guard_differs(unit, dict(weight=clean))
        return Call(expect=EXPECT.get((unit, case), {}), guard=guard, **kw)
    if case in ("E2+", "E2-"):
        v = 100.0 if case == "E2+" else -100.0
        if unit == "act":
            w = dict(policy=policy(assign={"hout_b": lambda a: a.__setitem__(slice(2, 4), v)}))
        elif unit == "decode":
            w = dict(policy=occ(assign={"dec_h5_b": v}))
        else:
            w = dict(critic=critic(assign={"pcont_hout_b": v}))
        return Call(**w, expect=EXPECT.get((unit, case), {}), guard=GUARDS[unit, case], **kw)
    if case.startswith("E1"):
        v = float(case[2:])
        kw["target"] = kw["target"].copy()
        kw["target"][::2] = 0.0
        kw["target"][1::2] = 15.0
        return Call(ldec=ldec(assign={"ldec_params_b": lambda a: a.__setitem__(slice(1080, 2160), v)}), expect=EXPECT.get((unit, case), {}), guard=GUARDS[unit, case], **kw)
    if case in ("E3-same", "E3-far"):
        # the posterior's two layers made the prior's: no input reaches either (zero kernels), the biases and the second layer copied
        def far(a):
            a[:30] += f32(1e19)
        p = policy(assign={"obs1_w": 0.0, "img2_w": 0.0})
        p["obs1_b"], p["obs2_w"], p["obs2_b"] = p["img2_b"].copy(), p["img3_w"].copy(), p["img3_b"].copy()
        if case == "E3-far":
            far(p["obs2_b"])
        return Call(policy=p, expect=EXPECT.get((unit, case), {}), guard=GUARDS.get((unit, case)), **kw)
    if case == "F" and unit == "reward_fit":       # (the docstring above: an actor step of 64 rows before it)
        return Call(guard=_guard_stale_heads(unit), first=_stale_first(unit), **kw)
    if case == "F":
        # a 64-row call that leaves non-finite values in everything the handle keeps, then the clean 33-row call on the same handle
        big = _inputs(unit, 64, horizon=4 if unit == "dream_grad" else 2)
        if unit == "fit":
            # Neither C2 nor D3 poisons the scratch: an ELU stands behind every layer and takes a NaN or -inf pre-activation to
            # expm1(-86), so the activation planes would hold finite numbers.  Features x 2^127 (some +-inf themselves) overflow the first layer instead: a1,
            # a2, a3 hold +inf wherever the sum is positive; NaN targets make the output delta and with it delta1 .. delta3 NaN, and
            # the step is skipped.  What the smaller call can meet of it: the planes lie at multiples of n x 416 floats, so the 33-row
            # call's six planes [0, 82 368) overlie the larger call's a1, a2, a3 and the head of delta1 and are rewritten in full
            # (but for the 16 padding columns per row, which no call writes or reads); stale and non-finite past them stay the rest
            # of delta1, delta2, delta3 and the output deltas - what a row or plane index that ran past the end would read.
            big["features"] = scaled(big["features"], 127)
            big["target"] = {h: np.full(64, np.nan, f32) for h in big["target"]}
            first = Call(rows=64, **big)
        else:                                      # NaN latents in every row: the stash, the LDS tiles
            big["state"][:] = np.nan
            first = Call(rows=64, **big)
        return Call(guard=lambda out, call, mode: _guard_stale(unit, out, call, mode), first=first, **kw)
    raise KeyError((unit, case))


def _guard_differs(unit, clean_kw):
    """The guard of a case whose edge is the input value itself (a weight of -1): the spec's answer differs from the untouched one."""
    def guard(out, call, mode):
        untouched = spec(unit, Call(call.policy, call.critic, call.ldec, **{**call.kw, **clean_kw}), mode)
        assert any(not same(out[k], untouched[k]) for k in out if out[k].dtype == f32)
    return guard


INF_ROWS = (4, 9, 20, 32)


def _guard_inf_gru(out, call, mode):
    """The recurrent pre-activation h R of the poisoned rows, restated in NumPy's float32, holds +-inf in most columns and NaN in
    many (the classes do not depend on the order of the sum: a column with one infinity is +-inf, one with two of opposite sign NaN);
    the spec's answer for those rows is non-finite where the infinity is carried (z h) and finite elsewhere - sigma and tanh returned
    numbers for +-inf and NaN -, and every other row is finite."""
    deter = call.kw["state"][list(INF_ROWS), 30:230]
    with np.errstate(all="ignore"):
        mh = deter @ call.policy["gru_recurrent"]
    assert int(np.isinf(mh).sum()) >= 1200 and int(np.isnan(mh).sum()) >= 200, (int(np.isinf(mh).sum()), int(np.isnan(mh).sum()))
    shown = 0
    for k, a in out.items():
        if a.ndim < 2 or a.shape[0] != call.rows:
            continue
        rows = a[list(INF_ROWS)]
        others = np.delete(a, list(INF_ROWS), axis=0)
        assert np.isfinite(others).all(), k
        if k in ("state", "feature", "features", "final_feature", "grad_state"):
            shown += 1
            assert (~np.isfinite(rows)).sum() >= len(INF_ROWS), k
            assert k == "grad_state" or np.isfinite(rows).sum() >= len(INF_ROWS), k        # (the backward pass leaves the whole row NaN)
    assert shown >= 1


def _guard_saturated_gru(out, call, mode):
    """A GRU whose input kernel is 2^100 times the trained one: the input pre-activations x K reach 2.5e31 - far beyond +-86, where the
    clamp decides, but finite: no +-inf, no NaN (case C3-inf sends those).  sigma is 0 or 1 and tanh +-1 exactly in most units, so
    the new deter is the candidate +-1 (z = 0) or the old deter (z = 1)."""
    deter = [a for k, a in out.items() if k in ("state", "feature", "features", "final_feature")][0][..., 30:230]
    assert int((np.abs(deter) == 1.0).sum()) >= deter.size // 4, int((np.abs(deter) == 1.0).sum())


def _guard_rows_identical(out, call, mode):
    """No input reaches the output (a zero first layer; features that vanish beside the next bias): every row's answer is the first
    row's, byte for byte - and finite."""
    for k, a in out.items():
        if k in ("value", "value_start", "pcont", "pcont_start", "logits", "image", "mean", "std"):
            assert np.all(a.reshape(call.rows, -1) == a.reshape(call.rows, -1)[0]) and np.isfinite(a).all(), k


def _guard_fit_zero_layer(out, call, mode):
    assert out["step"] == 1 and out["skipped"] == 0 and 0.1 < out["grad_norm"] < 10.0, (out["step"], out["grad_norm"])


def _guard_actor_std(sign):
    def guard(out, call, mode):
        if sign > 0:       # sd = softplus(100 + 4.99) + 1e-4 = 105: tanh(mu + 105 n) is +-1 but for |n| < 0.1
            assert int((np.abs(out["action"]) == 1.0).sum()) >= out["action"].size // 2
        else:              # sd = exp(-86) + 1e-4 = 1e-4 exactly: softplus has saturated, a bias of -200 gives the same bytes
            lower = spec("act", Call(policy(assign={"hout_b": lambda a: a.__setitem__(slice(2, 4), -200.0)}), **call.kw), mode)
            base = spec("act", Call(**call.kw), mode)
            assert same(out["action"], lower["action"]) and not same(out["action"], base["action"])
    return guard


def _guard_pcont(sign):
    def guard(out, call, mode):
        if "pcont" in out:
            p = np.concatenate([out["pcont"].reshape(-1), out.get("pcont_start", out["pcont"]).reshape(-1)])
            assert np.all(p == 1.0) if sign > 0 else np.all((p > 0) & (p < 1e-37)), (p.min(), p.max())      # 1 / (1 + exp(-+86))
        else:              # the fit of the pcont head: softplus(+-100 + o) is that argument itself for every row with target 0 / 1
            assert out["loss"] > 10.0 and out["skipped"] == 0, out["loss"]
    return guard


def _guard_occupancy(sign):
    def guard(out, call, mode):
        if sign > 0:
            assert np.all(out["logits"] > 50.0) and np.isfinite(out["loglik"]).all() and np.all(out["loglik"] < -1e5)
        else:              # the decoder's last ReLU: every logit +0 by bit pattern, the log-likelihood 4096 times -softplus(0)
            assert not bits(out["logits"]).any() and not out["image"].any() and np.all(out["loglik"] == out["loglik"][0]) and -2840 < out["loglik"][0] < -2838
    return guard


def _guard_lidar_scale(bias):
    def guard(out, call, mode):
        sd, ll = out["std"], out["loglik"]
        if bias == -30.0:          # softplus(0.2 (-30 + o)) = 2.5e-3
            assert np.all((sd > 1e-3) & (sd < 1e-2)) and np.isfinite(ll).all()
        elif bias == -90.0:        # softplus(-18) = 1.5e-8: z = 3e7, z^2 = 1e15 - far from overflow, the log-likelihood stays finite
            assert np.all((sd > 1e-9) & (sd < 1e-7)) and np.isfinite(ll).all() and np.all(ll < -1e15)
        elif bias == 90.0:
            assert np.all(sd > 80.0) and np.isfinite(ll).all()
        else:                      # -500: softplus(-100) = exp(-86), the floor; z = 1e37 and z^2 overflows
            assert np.all(sd == m_exp(f32(-86.0))) and int(np.isneginf(ll).sum()) >= call.rows // 2, int(np.isneginf(ll).sum())
    return guard


def _guard_kl_same(out, call, mode):
    """post = prior exactly: every KL term is log s - log s + (s^2 + 0) / (2 s^2) - 1/2 = +0 where s^2 / (2 s^2) rounds to 1/2."""
    assert same(out["post_mean"], out["prior_mean"]) and same(out["post_std"], out["prior_std"])
    assert np.all(np.abs(out["kl"]) < 1e-5)


def _forward(call, eps="given"):
    """The actor's forward under the call's weights: on its eps, or on another (None: the mode action)."""
    from policy_actor_fit_spec import PolicyActorFitSpec
    return PolicyActorFitSpec(call.policy).forward(call.kw["features"], call.kw["eps"] if isinstance(eps, str) else eps)


def _loaded(unit, call):
    """The arrays the unit's optimizer owns, as the call loads them."""
    from policy_actor_fit_spec import KEYS as ACTOR_KEYS
    from policy_reward_fit_spec import KEYS as REWARD_KEYS
    if unit == "fit":
        return dict(call.critic)
    return {k: call.policy[k] for k in (REWARD_KEYS if unit == "reward_fit" else ACTOR_KEYS)}


def _guard_step_taken(unit):
    """A zero first layer: a1 = ELU(-0) = +0 for every row, the next bias takes over - a step is taken, its norm an ordinary number.
    The first kernel starts from zero, so after Adam's first step each element is -lr g / (|g| + epsilon): within lr of zero, and
    not all zero."""
    def guard(out, call, mode):
        from policy_actor_fit_spec import DEFAULTS as ACTOR
        from policy_reward_fit_spec import DEFAULTS as REWARD
        lr = (REWARD if unit == "reward_fit" else ACTOR)["lr"]
        w = out[FIRST[unit][1] + "_w"]
        assert out["step"] == 1 and out["skipped"] == 0 and 1e-3 < out["grad_norm"] < 1e3, (out["step"], out["grad_norm"])
        assert np.all(np.abs(w) <= 1.01 * lr) and int((w != 0).sum()) >= w.size // 2, (float(np.abs(w).max()), int((w != 0).sum()))
    return guard


def _guard_no_eps(out, call, mode):
    """eps absent: d_std is never computed - the raw-std columns of the output layer's gradient are +0 by bit pattern, and so are
    their moments after the step; the mean columns' are not."""
    gw, gb = out["grad_hout_w"], out["grad_hout_b"]
    m, v = (out[k][-401 * 4:].reshape(401, 4) for k in ("m", "v"))
    assert not bits(gw[:, 2:]).any() and not bits(gb[2:]).any() and not bits(m[:, 2:]).any() and not bits(v[:, 2:]).any()
    assert out["step"] == 1 and np.all(gw[:, :2] != 0) and np.all(m[:, :2] != 0)


def _guard_forward_finite(out, call, mode):
    """Hidden layers that overflow: the action, the mean and the standard deviation are still numbers (an ELU takes a NaN and -inf to
    expm1(-86), tanh takes +-inf and NaN to +-1)."""
    fwd = _forward(call)
    assert all(np.isfinite(a).all() for a in fwd.values()) and out["skipped"] == 1


def _guard_actor_poison(out, call, mode):
    """A NaN feature row: the norm is NaN through feat^T delta1 and the step is skipped, but the row's own grad_features are 230 zeros -
    the ELU takes the NaN to expm1(-86) = -1 in every unit of a1 and elu'(a1) = a1 + 1 = 0 - and the other rows' are the clean twin's."""
    clean = spec("actor_fit", call.clean, mode)
    assert np.isnan(out["grad_norm"]) and out["skipped"] == 1 and clean["skipped"] == 0
    assert np.all(out["grad_features"][ROW] == 0) and np.all(clean["grad_features"][ROW] != 0)
    assert same(np.delete(out["grad_features"], ROW, axis=0), np.delete(clean["grad_features"], ROW, axis=0))


def _guard_eps(unit, clean):
    """An infinite or NaN draw in row ROW: u = fmaf(sd, eps, mu) is +-inf or NaN and tanh makes the action +-1 exactly (a NaN: the
    clamped end, under the NaN's sign).  The forward shows that and nothing else; the fit has du = ga 0 = 0 and d_std = (0 eps) sigma =
    NaN, so the norm is NaN and the step skipped, under a finite loss - which for +-inf is not the clean one."""
    def guard(out, call, mode):
        base = spec(unit, clean, mode)
        if unit == "action":
            assert np.all(np.abs(out["action"][ROW]) == 1.0) and not same(out["action"][ROW], base["action"][ROW])
            assert same(out["mean"], base["mean"]) and same(out["std"], base["std"])
            assert same(np.delete(out["action"], ROW, axis=0), np.delete(base["action"], ROW, axis=0))
            return
        assert np.all(np.abs(_forward(call)["action"][ROW]) == 1.0)
        assert np.isnan(out["grad_norm"]) and out["skipped"] == 1 and base["skipped"] == 0 and np.isfinite(out["loss"])
        if mode == "target" and not np.isnan(call.kw["eps"][ROW]).any():
            assert not same(out["loss"], base["loss"])
    return guard


def _guard_actor_fit_std(unit, sign):
    def guard(out, call, mode):
        fwd = out if unit == "action" else _forward(call)
        if sign > 0:       # the trained raw outputs lie in [-77, -14] on these rows: sd = softplus(100 + 4.99 + o) is 28 .. 91, and
            #                tanh(mu + sd n), |mu| <= 5, is +-1 exactly beyond |u| = 9.1: for every |n| > 0.5
            assert np.all(fwd["std"] > 20.0)
            if call.kw["eps"] is not None and mode != "mean":
                assert int((np.abs(fwd["action"]) == 1.0).sum()) >= fwd["action"].size // 2
        else:              # sd = exp(-86) + 1e-4 = 1e-4 exactly: softplus has saturated, a bias of -200 gives the same bytes
            lower = Call(policy=_edit(call.policy, assign=_hout_b(2, 4, -200.0)), **call.kw)
            low = spec(unit, lower, mode) if unit == "action" else _forward(lower)
            assert np.all(fwd["std"] == f32(1e-4)) and all(same(fwd[k], low[k]) for k in ("action", "mean", "std"))
            assert not same(fwd["std"], (spec(unit, Call(**call.kw), mode) if unit == "action" else _forward(Call(**call.kw)))["std"])
        if unit == "actor_fit":
            assert out["skipped"] == 0 and out["step"] == 1
    return guard


def _guard_actor_mean_saturated(unit):
    def guard(out, call, mode):
        if unit == "action":                       # 5 tanh(+-200) = +-5 exactly
            assert np.all(np.abs(out["mean"]) == 5.0)
            return
        # d_mean = du (1 - th th) = du 0 for every row: the mean columns of the output layer's gradient are zeros, the raw-std columns
        # (eps is given) are not, and a step is taken
        assert np.all(np.abs(out["out"][:, :2]) > 46.0)
        assert not np.any(out["grad_hout_w"][:, :2]) and not np.any(out["grad_hout_b"][:2]) and np.all(out["grad_hout_b"][2:] != 0)
        assert out["skipped"] == 0 and out["step"] == 1 and out["grad_norm"] > 0
    return guard


def _guard_on_target(out, call, mode):
    """The targets are the actions themselves: every act - target is +0, the loss a zero (minus the mean of -0 terms summed from +0:
    its sign is compared with the device's), the gradient and its norm +0; the step counts and moves no weight."""
    assert not bits(out["grad_norm"]).any() and out["loss"] == 0 and out["skipped"] == 0 and out["step"] == 1
    assert not np.any(out["grad_features"]) and not bits(out["m"]).any() and not bits(out["v"]).any()
    assert all(same(out[k], a) for k, a in _loaded("actor_fit", call).items())


def _guard_stale_heads(unit):
    """Case F behind another head: the first call's spec answer - the actor's step before a reward step, the value head's before an
    actor step - is skipped on a non-finite norm and its first layer overflows to +inf in at least 2000 of the 25 600 pre-activations;
    the second call's answer is finite throughout."""
    def guard(out, call, mode):
        fk = call.kw["first"].kw
        with np.errstate(all="ignore"):
            if unit == "reward_fit":
                from policy_actor_fit_spec import PolicyActorFitSpec
                got = PolicyActorFitSpec(call.policy).step(fk["features"], target=fk["target"], eps=fk["eps"], weight=fk["weight"])
                pre = fk["features"] @ call.policy["h0_w"] + call.policy["h0_b"]
            else:
                from policy_fit_spec import PolicyFitSpec
                got = PolicyFitSpec(call.critic, "value").step(fk["features"], fk["target"]["value"], fk["weight"])
                pre = fk["features"] @ call.critic["value_h0_w"] + call.critic["value_h0_b"]
        assert got["skipped"] == 1 and not np.isfinite(got["grad_norm"])
        assert int(np.isposinf(pre).sum()) >= 2000, int(np.isposinf(pre).sum())
        assert all(np.isfinite(a).all() for a in out.values())
    return guard


GUARDS = {("reward_fit", "A-zero-layer"): _guard_step_taken("reward_fit"), ("actor_fit", "A-zero-layer"): _guard_step_taken("actor_fit"),
          ("actor_fit", "A-no-eps"): _guard_no_eps, ("actor_fit", "C2"): _guard_forward_finite, ("actor_fit", "D3"): _guard_actor_poison,
          ("actor_fit", "E2+"): _guard_actor_fit_std("actor_fit", 1), ("actor_fit", "E2-"): _guard_actor_fit_std("actor_fit", -1),
          ("action", "E2+"): _guard_actor_fit_std("action", 1), ("action", "E2-"): _guard_actor_fit_std("action", -1),
          ("actor_fit", "E4+"): _guard_actor_mean_saturated("actor_fit"), ("actor_fit", "E4-"): _guard_actor_mean_saturated("actor_fit"),
          ("action", "E4+"): _guard_actor_mean_saturated("action"), ("action", "E4-"): _guard_actor_mean_saturated("action"),
          ("actor_fit", "E5-on-target"): _guard_on_target, ("action", "B4"): _guard_rows_identical, ("action", "A-zero-layer"): _guard_rows_identical,
          ("returns", "A-zero-layer"): _guard_rows_identical, ("value", "A-zero-layer"): _guard_rows_identical,
          ("decode", "A-zero-layer"): _guard_rows_identical, ("decode_lidar", "A-zero-layer"): _guard_rows_identical,
          ("fit", "A-zero-layer"): _guard_fit_zero_layer, ("decode", "B4"): _guard_rows_identical,
          ("act", "E2+"): _guard_actor_std(1), ("act", "E2-"): _guard_actor_std(-1),
          ("returns", "E2+"): _guard_pcont(1), ("returns", "E2-"): _guard_pcont(-1), ("value", "E2+"): _guard_pcont(1), ("value", "E2-"): _guard_pcont(-1),
          ("fit", "E2+"): _guard_pcont(1), ("fit", "E2-"): _guard_pcont(-1), ("decode", "E2+"): _guard_occupancy(1), ("decode", "E2-"): _guard_occupancy(-1),
          ("decode_lidar", "E1-30"): _guard_lidar_scale(-30.0), ("decode_lidar", "E1-90"): _guard_lidar_scale(-90.0),
          ("decode_lidar", "E1+90"): _guard_lidar_scale(90.0), ("decode_lidar", "E1-500"): _guard_lidar_scale(-500.0),
          ("observe", "E3-same"): _guard_kl_same, ("dream_grad", "C3"): None}
# (unit, case[, mode]) that prove nothing and are not run - the table in tests/test_gpu_policy_edges.py says why
NOT_APPLICABLE = {("act", "E2+", "mean"), ("act", "E2-", "mean"), ("fit", "E2+", "value"), ("fit", "E2-", "value"), ("fit", "C1", "pcont"),
                  ("act", "B1", "deploy"), ("act", "B1", "explore"), ("act", "B2", "deploy"), ("act", "B2", "explore"), ("dream", "B2"),
                  ("act", "A-zero-layer"), ("imagine", "A-zero-layer"), ("observe", "A-zero-layer"), ("dream", "A-zero-layer"),
                  ("dream_grad", "A-zero-layer"),
                  ("actor_fit", "B1g", "target"), ("actor_fit", "B2g", "target"), ("actor_fit", "D6-grad-inf", "target"),
                  ("actor_fit", "D4-target+inf", "grad"), ("actor_fit", "D4-target-inf", "grad"), ("actor_fit", "E5-on-target", "grad"),
                  ("action", "D5-eps+inf", "mean"), ("action", "D5-eps-inf", "mean"), ("action", "D5-eps-nan", "mean")}


def _guard_grad_at_the_clamp(grad, actions):
    """At exactly +-1 and at nextafter(-1, 0) the gradient is non-zero; at nextafter(1, 2), NaN and +-inf it is +0 by bit pattern."""
    a, g = bits(actions), bits(grad)
    inside = (a == bits(f32(1.0))) | (a == bits(f32(-1.0))) | (a == bits(np.nextafter(f32(-1.0), f32(0.0))))
    outside = (a == bits(np.nextafter(f32(1.0), f32(2.0)))) | np.isnan(actions) | np.isinf(actions)
    assert inside.sum() >= 12 and outside.sum() >= 16, (int(inside.sum()), int(outside.sum()))
    assert np.all(grad[inside] != 0) and not g[outside].any()


def _guard_stale(unit, out, call, mode):
    """The first call's spec answer is non-finite wherever the handle keeps something; the second's is finite throughout."""
    first = spec(unit, call.kw["first"], mode)
    bad = sum(int((~np.isfinite(a)).sum()) for a in first.values())
    assert bad >= (1 if unit == "fit" else 64), bad
    if unit == "fit":                                   # the first layer of the larger call overflows: +inf in the activation planes
        fk = call.kw["first"].kw
        with np.errstate(all="ignore"):
            pre = fk["features"] @ call.critic[mode + "_h0_w"] + call.critic[mode + "_h0_b"]
        assert int(np.isposinf(pre).sum()) >= 2000, int(np.isposinf(pre).sum())      # (of 25 600; NaN and -inf become expm1(-86))
    assert all(np.isfinite(a).all() for a in out.values())


def applies(unit, case, mode):
    """Whether the case is run in this mode: a lookup in NOT_APPLICABLE, which lists by hand the (unit, case[, mode]) whose spec answer
    is ordinary and for which no guard could be written."""
    if (unit, case, mode) in NOT_APPLICABLE or (unit, case) in NOT_APPLICABLE:
        return False
    return True


def check_guard(unit, case, call, out, mode):
    """Fail unless the spec's answer `out` shows the edge the case is for."""
    assert call.expect.get(mode) or call.guard, (unit, case, mode, "a case without a guard proves nothing")
    for name, kind, least in call.expect.get(mode, ()):
        assert least >= 1
        have = census(out[name])[kind]
        assert have >= least, (unit, case, mode, name, kind, have, least)
    if call.guard:
        call.guard(out, call, mode)


# ------------------------------------------------------------------ the spec's answer
@functools.lru_cache(maxsize=None)
def _keys():
    from policy_sample_spec import EpisodeClock
    clock = EpisodeClock(N)
    clock.reset()
    return clock.keys()


def spec(unit, call, mode):
    """{output: float32 array} of the unit's spec on the call, under the device's output names."""
    kw = call.kw
    if unit == "act":
        from policy_sample_spec import PolicySampleSpec
        from policy_spec import PolicySpec
        if mode == "mean":
            a, s = PolicySpec(call.policy).act_packed(kw["scan"], kw["state"], kw["fresh"])
        else:
            a, s = PolicySampleSpec(call.policy, mode, seed=SEED).act_packed(kw["scan"], kw["state"], kw["fresh"], _keys())
        return dict(action=a, state=s)
    if unit == "imagine":
        from policy_imagine_spec import PolicyImagineSpec
        out = PolicyImagineSpec(call.policy).imagine(kw["state"], _keys(), kw["horizon"], mode, seed=SEED, actions=kw["actions"])
        return {k: out[k] for k in ("action", "feature", "reward", "reward_start")}
    if unit == "observe":
        from policy_observe_spec import PolicyObserveSpec
        out = PolicyObserveSpec(call.policy).observe(kw["scan"], kw["action"], None, mode, seed=SEED, state=kw["state"])
        return {k: out[k] for k in ("feature", "post_mean", "post_std", "prior_mean", "prior_std", "kl", "state", "reward")}
    if unit == "dream":
        from policy_dream_spec import PolicyDreamSpec
        out = PolicyDreamSpec(call.policy).dream(kw["state"], kw["actions"], None, mode, seed=SEED, discount=0.99)
        return {k: out[k] for k in ("return", "reward", "final_feature")}
    if unit == "dream_grad":
        from policy_dream_grad_spec import PolicyDreamGradSpec
        return PolicyDreamGradSpec(call.policy).dream_grad(kw["state"], kw["actions"], None, mode, seed=SEED, discount=0.99)
    if unit == "returns":
        from policy_returns_spec import PolicyReturnsSpec
        out = PolicyReturnsSpec(call.policy, call.critic).returns(kw["state"], None, None, kw["horizon"], mode, seed=SEED, lambda_=0.95, discount=0.99,
                                                                  actions=kw["actions"])
        names = dict(actions="action", features="feature")
        return {k: out[names.get(k, k)] for k in ("reward", "value", "pcont", "returns", "weight", "actions", "features", "reward_start", "value_start", "pcont_start")}
    if unit == "value":
        from policy_returns_spec import PolicyReturnsSpec
        out = PolicyReturnsSpec(call.policy, call.critic).returns(kw["features"], None, None, 0, "mean")
        return {k: out[k + "_start"] for k in ("value", "reward", "pcont")}
    if unit == "fit":
        from policy_fit_spec import PolicyFitSpec
        fit = PolicyFitSpec(call.critic, mode)
        if kw.get("first") is not None:            # (case F: the call before, on the same optimizer)
            fk = kw["first"].kw
            assert fit.step(fk["features"], fk["target"][mode], fk["weight"], **fk["hyper"])["skipped"] == 1
        for _ in range(kw["steps"]):
            got = fit.step(kw["features"], kw["target"][mode], kw["weight"], **kw["hyper"])
        out = {k: np.array(a, f32) for k, a in fit.weights().items()}
        out.update(loss=f32(got["loss"]), grad_norm=f32(got["grad_norm"]), skipped=f32(got["skipped"]), step=f32(got["step"]), m=fit.m.copy(), v=fit.v.copy())
        return out
    if unit == "reward_fit":                       # (case F's first call is the actor's and skipped: it moves nothing of the reward head's)
        from policy_reward_fit_spec import PolicyRewardFitSpec
        fit = PolicyRewardFitSpec(call.policy)
        for _ in range(kw["steps"]):
            got = fit.step(kw["features"], kw["target"]["reward"], kw["weight"], **kw["hyper"])
        out = {k: np.array(a, f32) for k, a in fit.weights().items()}
        out.update(loss=f32(got["loss"]), grad_norm=f32(got["grad_norm"]), skipped=f32(got["skipped"]), step=f32(got["step"]), m=fit.m.copy(), v=fit.v.copy())
        return out
    if unit == "actor_fit":                        # (case F's first call is the value head's)
        from policy_actor_fit_spec import PolicyActorFitSpec
        fit = PolicyActorFitSpec(call.policy)
        given = {("target" if mode == "target" else "grad_actions"): kw["target" if mode == "target" else "grad_actions"]}
        for _ in range(kw["steps"]):
            got = fit.step(kw["features"], eps=kw["eps"], weight=kw["weight"], **given, **kw["hyper"])
        out = {k: np.array(a, f32) for k, a in fit.weights().items()}
        out.update(loss=f32(got["loss"]), grad_norm=f32(got["grad_norm"]), skipped=f32(got["skipped"]), step=f32(got["step"]), m=fit.m.copy(), v=fit.v.copy(),
                   grad_features=got["grad_features"], out=got["out"], grad_hout_w=got["grad"]["hout_w"], grad_hout_b=got["grad"]["hout_b"])
        return out
    if unit == "action":
        from policy_actor_fit_spec import PolicyActorFitSpec
        return PolicyActorFitSpec(call.policy).forward(kw["features"], kw["eps"] if mode == "draw" else None)
    if unit == "decode":
        import policy_decode_loglik_spec as pdl
        from policy_decode_spec import PolicyDecodeSpec
        logits, image = PolicyDecodeSpec(call.policy).decode(kw["features"])
        return dict(logits=logits, image=image, loglik=pdl.loglik(logits, kw["target"]))
    if unit == "decode_lidar":
        from policy_lidar_decode_spec import PolicyLidarDecodeSpec
        return PolicyLidarDecodeSpec(call.ldec).decode(kw["features"], kw["target"])
    raise KeyError(unit)


# What each case's spec answer held on the CPU where the recipes were written, as lower bounds (output, kind, count): the smallest count
# over the unit's modes.  A case is vacuous - and fails - when its spec answer shows fewer.
EXPECT = {('act', 'B1'): {'mean': [('action', 'sub', 66), ('state', 'sub', 66)]},
 ('act', 'B2'): {'mean': [('action', 'sub', 1), ('state', 'sub', 1)]},
 ('act', 'D3'): {'deploy': [('state', 'nan', 200)], 'explore': [('state', 'nan', 200)], 'mean': [('state', 'nan', 200)]},
 ('decode', 'B1'): {'mean': [('logits', 'sub', 23200)]},
 ('decode', 'B2'): {'mean': [('logits', 'sub', 101)]},
 ('decode_lidar', 'B1'): {'mean': [('mean', 'sub', 35631), ('mean', 'negzero', 7)]},
 ('decode_lidar', 'B2'): {'mean': [('mean', 'sub', 4677)]},
 ('decode_lidar', 'B4'): {'mean': [('mean', 'sub', 35640)]},
 ('decode_lidar', 'E1-500'): {'mean': [('loglik', 'inf', 33)]},
 ('dream', 'B1'): {'mean': [('return', 'sub', 66), ('reward', 'sub', 132)], 'sample': [('return', 'sub', 66), ('reward', 'sub', 132)]},
 ('dream', 'D3'): {'mean': [('final_feature', 'nan', 400)], 'sample': [('final_feature', 'nan', 400)]},
 ('dream_grad', 'B1'): {'mean': [('grad_actions', 'sub', 166),
                                 ('grad_state', 'sub', 15133),
                                 ('grad_state', 'negzero', 25),
                                 ('return', 'sub', 66),
                                 ('reward', 'sub', 132)],
                        'sample': [('grad_actions', 'sub', 166),
                                   ('grad_state', 'sub', 15130),
                                   ('grad_state', 'negzero', 23),
                                   ('return', 'sub', 66),
                                   ('reward', 'sub', 132)]},
 ('dream_grad', 'B2'): {'mean': [('grad_actions', 'sub', 151), ('grad_state', 'sub', 8692)],
                        'sample': [('grad_actions', 'sub', 155), ('grad_state', 'sub', 8592)]},
 ('dream_grad', 'C3'): {'mean': [('grad_state', 'sub', 3736)], 'sample': [('grad_state', 'sub', 3687)]},
 ('dream_grad', 'D3'): {'mean': [('grad_actions', 'nan', 4), ('grad_state', 'nan', 460)],
                        'sample': [('grad_actions', 'nan', 4), ('grad_state', 'nan', 460)]},
 ('fit', 'B1'): {'pcont': [('pcont_h0_b', 'sub', 327), ('pcont_h1_b', 'sub', 298), ('pcont_h2_b', 'sub', 273), ('m', 'sub', 257199)],
                 'value': [('value_h0_b', 'sub', 375), ('value_h1_b', 'sub', 382), ('value_h2_b', 'sub', 388), ('m', 'sub', 327295)]},
 ('fit', 'B2'): {'pcont': [('pcont_h0_b', 'sub', 240), ('pcont_h1_b', 'sub', 266), ('pcont_h2_b', 'sub', 230), ('m', 'sub', 413182)],
                 'value': [('value_h0_b', 'sub', 44), ('value_h1_b', 'sub', 25), ('value_h2_b', 'sub', 26), ('m', 'sub', 413190)]},
 ('fit', 'B3'): {'pcont': [('v', 'sub', 297199)], 'value': [('v', 'sub', 338753)]},
 ('fit', 'B4'): {'pcont': [('m', 'sub', 409488)], 'value': [('m', 'sub', 408987)]},
 ('fit', 'B4-one-row'): {'pcont': [('m', 'sub', 410495)], 'value': [('m', 'sub', 410186)]},
 ('fit', 'C1'): {'value': [('grad_norm', 'inf', 1)]},
 ('fit', 'C2'): {'pcont': [('grad_norm', 'nan', 1)], 'value': [('loss', 'nan', 1), ('grad_norm', 'nan', 1)]},
 ('fit', 'D3'): {'pcont': [('grad_norm', 'nan', 1)], 'value': [('grad_norm', 'nan', 1)]},
 ('fit', 'D4-target+inf'): {'pcont': [('loss', 'nan', 1), ('grad_norm', 'nan', 1)], 'value': [('loss', 'inf', 1), ('grad_norm', 'nan', 1)]},
 ('fit', 'D4-target-inf'): {'pcont': [('loss', 'nan', 1), ('grad_norm', 'nan', 1)], 'value': [('loss', 'inf', 1), ('grad_norm', 'nan', 1)]},
 ('fit', 'D4-weight-inf'): {'pcont': [('loss', 'inf', 1), ('grad_norm', 'nan', 1)], 'value': [('loss', 'inf', 1), ('grad_norm', 'nan', 1)]},
 ('imagine', 'A-negzero-inputs'): {'mean': [('action', 'negzero', 66)], 'sample': [('action', 'negzero', 66)]},
 ('imagine', 'B1'): {'mean': [('action', 'sub', 132), ('reward', 'sub', 66), ('reward_start', 'sub', 33)],
                     'sample': [('reward', 'sub', 66), ('reward_start', 'sub', 33)]},
 ('imagine', 'B2'): {'mean': [('action', 'sub', 1), ('reward_start', 'sub', 2)], 'sample': [('reward_start', 'sub', 2)]},
 ('imagine', 'D2'): {'mean': [('action', 'negzero', 6)], 'sample': [('action', 'negzero', 6)]},
 ('imagine', 'D3'): {'mean': [('feature', 'nan', 400)], 'sample': [('feature', 'nan', 400)]},
 ('observe', 'A-negzero-inputs'): {'mean': [('state', 'negzero', 33)], 'sample': [('state', 'negzero', 33)]},
 ('observe', 'B1'): {'mean': [('reward', 'sub', 66)], 'sample': [('reward', 'sub', 66)]},
 ('observe', 'B2'): {'mean': [('reward', 'sub', 3)], 'sample': [('reward', 'sub', 2)]},
 ('observe', 'D2'): {'mean': [('state', 'negzero', 3)], 'sample': [('state', 'negzero', 3)]},
 ('observe', 'D3'): {'mean': [('feature', 'nan', 400), ('state', 'nan', 200)], 'sample': [('feature', 'nan', 400), ('state', 'nan', 200)]},
 ('observe', 'E3-far'): {'mean': [('kl', 'inf', 66)], 'sample': [('kl', 'inf', 66)]},
 ('returns', 'A-negzero-inputs'): {'mean': [('actions', 'negzero', 66)], 'sample': [('actions', 'negzero', 66)]},
 ('returns', 'B1'): {'mean': [('reward', 'sub', 66),
                              ('value', 'sub', 66),
                              ('returns', 'sub', 33),
                              ('reward_start', 'sub', 33),
                              ('value_start', 'sub', 33)],
                     'sample': [('reward', 'sub', 66),
                                ('value', 'sub', 66),
                                ('returns', 'sub', 33),
                                ('reward_start', 'sub', 33),
                                ('value_start', 'sub', 33)]},
 ('returns', 'B2'): {'mean': [('value', 'sub', 2), ('returns', 'sub', 2), ('reward_start', 'sub', 2), ('value_start', 'sub', 2)],
                     'sample': [('value', 'sub', 1), ('returns', 'sub', 2), ('reward_start', 'sub', 2), ('value_start', 'sub', 2)]},
 ('returns', 'C2'): {'mean': [('value', 'nan', 66), ('returns', 'nan', 33), ('value_start', 'nan', 33)],
                     'sample': [('value', 'nan', 66), ('returns', 'nan', 33), ('value_start', 'nan', 33)]},
 ('returns', 'D2'): {'mean': [('actions', 'negzero', 6)], 'sample': [('actions', 'negzero', 6)]},
 ('returns', 'D3'): {'mean': [('features', 'nan', 400)], 'sample': [('features', 'nan', 400)]},
 ('value', 'B1'): {'mean': [('value', 'sub', 33), ('reward', 'sub', 33)]},
 ('value', 'B2'): {'mean': [('value', 'sub', 2), ('reward', 'sub', 2)]},
 ('value', 'B4'): {'mean': [('value', 'sub', 33)]},
 ('value', 'C2'): {'mean': [('value', 'nan', 33)]}}
# case C3-inf: per poisoned row the infinities z h carries and the 30 NaN of a stoch computed from such a deter
_ROLL = lambda k, steps: [(k, "inf", 6 * steps), (k, "nan", 120 * steps)]
EXPECT.update({("act", "C3-inf"): {m: _ROLL("state", 1) for m in UNITS["act"]},
               ("imagine", "C3-inf"): {m: _ROLL("feature", 2) for m in UNITS["imagine"]},
               ("observe", "C3-inf"): {m: _ROLL("feature", 2) + _ROLL("state", 1) + [("kl", "nan", 8)] for m in UNITS["observe"]},
               ("dream", "C3-inf"): {m: _ROLL("final_feature", 2) for m in UNITS["dream"]},
               ("dream_grad", "C3-inf"): {m: [("grad_actions", "nan", 23), ("grad_state", "nan", 1840)] for m in UNITS["dream_grad"]},
               ("returns", "C3-inf"): {m: _ROLL("features", 2) for m in UNITS["returns"]}})
# the fit engine's other heads and the actor's forward: as above, from the spec on the CPU at 33 rows; where a case runs in two modes a
# floor is the smaller of the two counts ("zero" counts +0 by bit pattern: a norm, a skipped flag, every second moment)
_NAN_NORM = [("grad_norm", "nan", 1)]
_BOTH = lambda entries: {"target": list(entries), "grad": list(entries)}
EXPECT.update({
    ("reward_fit", "B1"): {"reward": [("m", "sub", 155057)]},
    ("reward_fit", "B2"): {"reward": [("m", "sub", 252782)]},
    ("reward_fit", "B3"): {"reward": [("v", "sub", 234749)]},
    ("reward_fit", "B4"): {"reward": [("m", "sub", 236051)]},
    ("reward_fit", "B4-one-row"): {"reward": [("m", "sub", 236291)]},
    ("reward_fit", "C1"): {"reward": [("grad_norm", "inf", 1)]},
    ("reward_fit", "C2"): {"reward": [("loss", "nan", 1)] + _NAN_NORM},
    ("reward_fit", "D3"): {"reward": _NAN_NORM},
    ("reward_fit", "D4-target+inf"): {"reward": [("loss", "inf", 1)] + _NAN_NORM},
    ("reward_fit", "D4-target-inf"): {"reward": [("loss", "inf", 1)] + _NAN_NORM},
    ("reward_fit", "D4-weight-inf"): {"reward": [("loss", "inf", 1)] + _NAN_NORM},
    ("actor_fit", "B1"): _BOTH([("m", "sub", 332060), ("grad_features", "sub", 1494), ("grad_features", "negzero", 35)]),
    ("actor_fit", "B2"): _BOTH([("m", "sub", 567853), ("grad_features", "sub", 6595)]),
    ("actor_fit", "B1g"): {"grad": [("grad_norm", "zero", 1), ("skipped", "zero", 1), ("v", "zero", 575204), ("m", "sub", 107024),
                                    ("grad_features", "sub", 694), ("grad_features", "negzero", 59)]},
    ("actor_fit", "B2g"): {"grad": [("grad_norm", "zero", 1), ("skipped", "zero", 1), ("v", "zero", 575204), ("m", "sub", 563787),
                                    ("grad_features", "sub", 6347), ("grad_features", "negzero", 10)]},
    ("actor_fit", "B3"): _BOTH([("v", "sub", 37609)]),
    ("actor_fit", "B4"): _BOTH([("m", "sub", 251190)]),
    ("actor_fit", "B4-one-row"): _BOTH([("m", "sub", 210470)]),
    ("actor_fit", "C1"): {"target": [("loss", "inf", 1), ("grad_norm", "inf", 1)], "grad": [("grad_norm", "inf", 1)]},
    ("actor_fit", "C2"): _BOTH(_NAN_NORM),
    ("actor_fit", "D3"): _BOTH(_NAN_NORM),
    ("actor_fit", "D4-target+inf"): {"target": [("loss", "inf", 1), ("grad_features", "nan", 230)] + _NAN_NORM},
    ("actor_fit", "D4-target-inf"): {"target": [("loss", "inf", 1), ("grad_features", "nan", 230)] + _NAN_NORM},
    ("actor_fit", "D4-weight0+inf-target"): {"target": [("loss", "nan", 1), ("grad_features", "nan", 230)] + _NAN_NORM,
                                             "grad": [("grad_features", "nan", 230)] + _NAN_NORM},
    ("actor_fit", "D4-weight-inf"): {"target": [("loss", "inf", 1), ("grad_features", "nan", 230)] + _NAN_NORM,
                                     "grad": [("grad_features", "nan", 230)] + _NAN_NORM},
    ("actor_fit", "D5-eps+inf"): _BOTH([("grad_features", "nan", 230)] + _NAN_NORM),
    ("actor_fit", "D5-eps-inf"): _BOTH([("grad_features", "nan", 230)] + _NAN_NORM),
    ("actor_fit", "D5-eps-nan"): _BOTH([("grad_features", "nan", 230)] + _NAN_NORM),
    ("actor_fit", "D6-grad-inf"): {"grad": [("grad_features", "nan", 230)] + _NAN_NORM},
    ("actor_fit", "E2+"): _BOTH([("v", "sub", 286)]),
    ("actor_fit", "E2-"): _BOTH([("m", "sub", 802)]),
    ("actor_fit", "E4+"): _BOTH([("v", "sub", 27333)]),
    ("actor_fit", "E4-"): _BOTH([("v", "sub", 30223)]),
    ("action", "B1"): {"mean": [("action", "sub", 66), ("mean", "sub", 66)], "draw": [("mean", "sub", 66)]},
    ("action", "B2"): {"mean": [("action", "sub", 1), ("mean", "sub", 1)], "draw": [("mean", "sub", 1)]}})
