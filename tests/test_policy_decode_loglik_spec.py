"""The binary32 specification of the observation decoder's Bernoulli log-likelihood (tests/policy_decode_loglik_spec.c, DESIGN.md §2
item 22) against float64 on the golden decoders' logits, and its documented order of summation."""
import numpy as np
import pytest

import policy_decode_loglik_spec as pdl
import policy_sample_spec as pss
from test_policy_decode_spec import DECODERS, decoded

f32 = np.float32


@pytest.mark.parametrize("name", DECODERS)
def test_loglik_is_the_float64_sum_within_the_rounding_bound(name):
    """x logit - softplus(logit) summed over the 4096 pixels of each of the 162 inputs, logits up to 562: within 1080 x 2^-24 x
    sum |terms| of the float64 sum over the same binary32 logits, for a random target, all ones and all zeros."""
    _, logits, image, _, _, _ = decoded(name)
    rng = np.random.default_rng(1)
    for target in ((rng.random(logits.shape) > 0.5).astype(np.uint8), np.ones_like(image), np.zeros_like(image), image):
        got = pdl.loglik(logits, target)
        lg = logits.astype(np.float64)
        terms = (np.where(target != 0, lg, 0.0) - (lg + np.log1p(np.exp(-lg)))).reshape(len(lg), -1)
        err, bound = np.abs(got - terms.sum(1)), 1080 * 2.0 ** -24 * np.abs(terms).sum(1)
        print(f"{name}: largest error / bound {np.max(err / bound):.3e}")
        assert got.shape == (len(lg),) and got.dtype == f32 and np.all(err <= bound) and np.all(got < 0)


def test_the_summation_order_is_the_documented_one():
    rng = np.random.default_rng(2)
    logits = (np.abs(rng.normal(size=(64, 64))) * 10.0 ** rng.uniform(-2, 2, (64, 64))).astype(f32)
    target = (rng.random((64, 64)) > 0.5).astype(np.uint8)
    terms = (np.where(target != 0, logits, f32(0)) - pss.scalar_map("softplus", logits)).astype(f32)
    total = f32(0)
    for wave in range(8):
        v = np.zeros(64, f32)
        for lane in range(64):
            t, s = 64 * wave + lane, f32(0)
            for item in (t, t + 512):
                Y, X = item >> 5, item & 31
                for py in range(2):
                    for px in range(2):
                        s = f32(s + terms[2 * Y + py, 2 * X + px])
            v[lane] = s
        for m in (1, 2, 4, 8, 16, 32):
            v[::2 * m] = v[::2 * m] + v[m::2 * m]
        total = f32(total + v[0])
    assert pdl.loglik(logits, target).view(np.uint32) == total.view(np.uint32)
