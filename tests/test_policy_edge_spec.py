"""The CPU side of the numeric-edge cases (tests/policy_edge_cases.py; the device side is tests/test_gpu_policy_edges.py): every case's
guard on the spec's own answer - a case whose answer is ordinary proves nothing and fails here -, the spec's dense chain against exact
rational arithmetic on edge operands, and the spec's scalar functions at the special values against a restatement of
racecar_policy_math.h in correctly rounded operations.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import policy_edge_cases as pe
import policy_sample_spec as pss
import policy_spec as ps

f32 = np.float32
ALL = [pytest.param(unit, case, mode, id=f"{unit}-{case}-{mode}") for unit, modes in pe.UNITS.items() for case in pe.cases(unit) for mode in modes
       if pe.applies(unit, case, mode)]


@pytest.mark.parametrize("unit, case, mode", ALL)
def test_the_case_reaches_its_edge(unit, case, mode):
    """The spec's answer shows at least the subnormals, signed zeros, infinities and NaNs the recipe is for (the counts were taken
    from the spec on the CPU where the recipes were written and are lower bounds), or meets the case's own guard."""
    call = pe.make(unit, case)
    pe.check_guard(unit, case, call, pe.spec(unit, call, mode), mode)


def test_every_unit_has_its_cases():
    """A (zero, signed zero), B (subnormals) and D (special inputs) for every unit in every mode, and no case without a guard."""
    for unit, modes in pe.UNITS.items():
        for mode in modes:
            have = {case.split("-")[0][0] for case in pe.cases(unit) if pe.applies(unit, case, mode)}
            assert {"A", "D"} <= have, (unit, mode, have)
            assert "B" in have or (unit == "act" and mode != "mean"), (unit, mode, have)
    for p in ALL:
        unit, case, mode = p.values
        call = pe.make(unit, case)
        assert call.expect.get(mode) or call.guard, p.id


@pytest.mark.parametrize("unit", ["reward_fit", "actor_fit", "action"])
def test_a_guard_fails_on_the_unedited_call(unit):
    """The other half of a guard, for the fit engine's later units: on the spec's answer to the unit's UNEDITED inputs and weights -
    an ordinary answer - every case's guard fails.  (Case F keeps a first call, but a clean one of the same 64 rows.)"""
    for case in pe.cases(unit):
        for mode in pe.UNITS[unit]:
            if not pe.applies(unit, case, mode):
                continue
            call, kw = pe.make(unit, case), pe._inputs(unit)
            if case == "F":
                kw["first"] = pe.Call(rows=64, **pe._inputs("actor_fit" if unit == "reward_fit" else "fit", 64))
            plain = pe.Call(expect=call.expect, guard=call.guard, clean=call.clean, **kw)
            with pytest.raises(AssertionError):
                pe.check_guard(unit, case, plain, pe.spec(unit, plain, mode), mode)
                print("passes on the unedited call:", unit, case, mode)


def test_the_comparison_rule():
    nan2 = np.array([0x7fc00000, 0xffc00001], np.uint32).view(f32)
    assert pe.same(nan2, nan2[::-1].copy())                                                  # a NaN's sign and payload are not compared
    assert not pe.same(np.array([0.0], f32), np.array([-0.0], f32))                          # the sign of zero is
    assert not pe.same(np.array([np.inf], f32), np.array([np.nan], f32)) and not pe.same(np.array([np.inf], f32), np.array([-np.inf], f32))
    sub = np.array([1, 2], np.uint32).view(f32)
    assert pe.same(sub, sub.copy()) and not pe.same(sub, sub[::-1].copy()) and not pe.same(sub[:1], np.zeros(1, f32))
    assert not pe.same(np.zeros(2, f32), np.zeros(3, f32)) and not pe.same(np.zeros(2, f32), np.zeros(2, np.float64))
    with pytest.raises(AssertionError):
        pe.assert_same(np.array([0.0, 1.0], f32), np.array([-0.0, 1.0], f32), "signed zero")


def test_round32_is_binary32s_rounding():
    """The host's rounding against NumPy's own double -> float conversion (one correct rounding of an exactly representable double):
    subnormal results, ties, the overflow threshold."""
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.normal(size=200) * 2.0 ** rng.integers(-160, 130, 200), [2.0 ** -149 * 0.5, 2.0 ** -149 * 1.5, 2.0 ** -150 * 1.0000001,
                        float(np.finfo(f32).max) + 2.0 ** 102, float(np.finfo(f32).max) + 2.0 ** 103, 2.0 ** -126 - 2.0 ** -150, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24]])
    with np.errstate(all="ignore"):
        for v in x:
            assert pe.bits(pe.round32(Fraction(float(v))))[0] == pe.bits(f32(v))[0], v


def _edge_layer():
    """x [4, 230], w [230, 8], bias [8]: column 0 subnormal weights, 1 products that all underflow (a -0 bias), 2 an accumulator that
    climbs from the subnormals into the normal range, 3 a column that overflows, 4 cancellation down into the subnormals, 5 ordinary,
    6 a subnormal bias under products of either sign at half its last place, 7 an overflow that a later term does not undo."""
    rng = np.random.default_rng(12)
    x = rng.normal(0.0, 1.0, (4, 230)).astype(f32)
    w = rng.normal(0.0, 0.1, (230, 8)).astype(f32)
    bias = np.zeros(8, f32)
    w[:, 0] = pe.scaled(w[:, 0], -135)
    w[:, 1] = pe.scaled(w[:, 1], -149)
    bias[1] = -0.0
    w[:, 2] = pe.scaled(np.abs(w[:, 2]) * np.sign(x[0] + f32(1e-3)), -140) * (f32(1.35) ** np.arange(230, dtype=f32)).astype(f32)
    w[:, 3] = pe.scaled(np.abs(w[:, 3]) * np.sign(x[0] + f32(1e-3)), 125)
    w[1::2, 4] = -w[0::2, 4]
    w[:, 4] = pe.scaled(w[:, 4], -120)
    bias[6] = np.array([3], np.uint32).view(f32)[0]
    w[:, 6] = pe.scaled(np.sign(w[:, 6]), -149)
    w[:, 7] = 0.0
    w[10, 7], w[200, 7] = f32(3e38), f32(-3e38)
    x[:, 10], x[:, 200] = f32(2.0), f32(2.0)
    x[1] = pe.scaled(x[1], -20)
    x[2, ::3] = -0.0
    x[3] = np.abs(x[3])
    return x, w, bias


def test_the_dense_chain_is_exact_fmaf_at_the_edges():
    """ps_dense on the edge layer equals, bit for bit, the chain evaluated in exact rational arithmetic with ONE rounding to binary32
    per fmaf (nearest-even on integers, gradual underflow, overflow to inf): the spec's compile flags and fmaf neither flush a
    subnormal operand, product or accumulator nor round twice."""
    x, w, bias = _edge_layer()
    got = ps.dense(x, w, bias)
    want = np.empty_like(got)
    for i in range(len(x)):
        for j in range(w.shape[1]):
            acc = bias[j]
            for k in range(w.shape[0]):
                acc = pe.fma32(x[i, k], w[k, j], acc)
            want[i, j] = acc
    assert pe.subnormal(w).sum() >= 300 and pe.subnormal(want).sum() >= 6 and np.isinf(want[0, 3]) and np.isinf(want[[0, 2, 3], 7]).all()
    assert np.all(want[:, 1] == 0) and np.all(np.abs(want[:, 2]) > 1e-30) and np.all(np.abs(want[:, 6]) < 2.0 ** -126) and pe.subnormal(want[:, 0]).sum() >= 3
    pe.assert_same(got, want, "ps_dense against exact arithmetic")
    assert pe.bits(got).tobytes() == pe.bits(want).tobytes()                                 # (no NaN here: every byte)


@pytest.mark.parametrize("which", ["exp", "elu", "sigmoid", "tanh", "log", "softplus"])
def test_the_scalar_functions_at_the_special_values(which):
    """The spec's scalar functions at +-0, the smallest and largest subnormal, the smallest normal, +-86 and its neighbours, +-inf and
    NaN against racecar_policy_math.h restated with correctly rounded operations (policy_edge_cases.MATH): the same bits, NaN for NaN."""
    x = pe.special_arguments()
    fn = ps.scalar_map if which in ("exp", "elu", "sigmoid", "tanh") else pss.scalar_map
    got = fn(which, x)
    with np.errstate(all="ignore"):
        want = np.array([pe.MATH[which](v) for v in x], f32)
    pe.assert_same(got, want, which)


def test_what_the_definitions_give_at_the_ends():
    """Read off racecar_policy_math.h: the +-86 clamp is two selects `x > -86 ? x : -86`, `x < 86 ? x : 86`, so -inf AND NaN go to -86;
    ELU's `x > 0 ? x : expm1(x)` sends NaN and -0 to expm1: expm1(-0) has n = -0 == 0 and q = fmaf(+0, t, r) with r = fmaf(-0, -ln2, -0) =
    +0 - so ELU(-0) is +0, not -0; tanh is copysign(e / (e + 2), x) with e = expm1(2 |x|) finite for every x: +-1 exactly beyond
    |x| = 9.1, also at +-inf, and copysign(.., NaN) of the finite e(86); softplus(-inf) = log1p(exp(-86)) = exp(-86)."""
    one = lambda which, v: (ps.scalar_map if which in ("exp", "elu", "sigmoid", "tanh") else pss.scalar_map)(which, np.array([v], f32))[0]
    b = lambda v: int(pe.bits(f32(v))[0])
    e86 = one("exp", -86.0)
    assert b(one("tanh", np.inf)) == b(1.0) and b(one("tanh", -np.inf)) == b(-1.0) and b(one("tanh", -0.0)) == b(-0.0)
    assert b(one("elu", -np.inf)) == b(one("elu", -86.0)) == b(one("elu", np.nan)) and -1.0 <= one("elu", -86.0) < -0.9999999
    assert b(one("elu", -0.0)) == b(0.0) and b(one("elu", 0.0)) == b(0.0) and b(one("elu", np.inf)) == b(np.inf)
    assert b(one("softplus", -np.inf)) == b(e86) == b(one("softplus", -100.0)) and 4.4e-38 < e86 < 4.6e-38
    assert b(one("softplus", np.inf)) == b(np.inf) and b(one("softplus", 100.0)) == b(100.0)
    assert b(one("exp", np.nan)) == b(e86) and b(one("exp", np.inf)) == b(one("exp", 86.0)) and np.isfinite(one("exp", 86.0))
    assert b(one("sigmoid", np.inf)) == b(1.0) and b(one("sigmoid", -np.inf)) == b(f32(1.0) / (f32(1.0) + one("exp", 86.0)))
    assert b(one("sigmoid", np.nan)) == b(1.0)                                               # exp(-NaN) = exp(-86): 1 / (1 + 4.5e-38)
    tiny = np.array([1], np.uint32).view(f32)[0]
    assert b(one("elu", -tiny)) == b(-tiny) and b(one("tanh", tiny)) == b(tiny) and b(one("exp", tiny)) == b(1.0)
