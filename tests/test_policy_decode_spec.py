"""The binary32 specification of the observation decoder (tests/policy_decode_spec.c) against a float64
restatement of the reference's scatter-form formulas (LidarOccupancyDecoder, dreamer/models.py:444-465; the loops of
oracle.dreamer_policy_port.DreamerPolicy.decoded_occupancy in float64): logits, mode, independence of the batch, encoding; and
the host side of rc_policy_load_decoder that needs no GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle.racecar_oracle as ro
from oracle.dreamer_policy_port import DreamerPolicy
from policy_decode_spec import DECODER_KEYS, PolicyDecodeSpec
from test_golden_policy import GOLDEN, c_env, weights

DECODERS = ("treitlstrasse_occupancy", "treitlstrasse_20210220")          # the two checkpoints with a LidarOccupancyDecoder
MARGIN = 4.0              # spec error / the float32 port's own, as items 12, 14 and 15
f32 = np.float32


@functools.lru_cache(maxsize=None)
def live_features(name, n=16):
    """The decoder's inputs as G11 produces them: n cars on treitlstrasse_v2 under the checkpoint's own deterministic actor
    (the NumPy port), 60 agent steps, the feature [stoch | deter] of every 4th step from step 20: 10 n rows; then an all-zero
    feature and row 0 scaled by 8.  Read only."""
    env, policy = c_env("treitlstrasse_v2", n), DreamerPolicy(weights(name), sample=False)
    out = env.reset(mode=ro.RESET_RANDOM, seed=1)
    state, rows = policy.initial(n), []
    for k in range(60):
        action, state = policy.act(np.asarray(out["lidar"]).reshape(n, ro.N_BEAMS), state,
                                   reset=(np.asarray(out["fresh"]).reshape(n) != 0) if k else None)
        if k >= 20 and k % 4 == 0:
            rows.append(np.concatenate([state["stoch"], state["deter"]], 1).astype(f32))
        out = env.step(action, repeat=4)
    live = np.concatenate(rows)
    feats = np.concatenate([live, np.zeros((1, 230), f32), 8.0 * live[:1]]).astype(f32)
    feats.setflags(write=False)
    return feats


def reference_float64(w, feat):
    """The reference's decoder in float64, scatter form: (logits after the last ReLU, the last layer BEFORE its ReLU), [n, 64, 64]."""
    x = (np.asarray(feat, np.float64) @ np.asarray(w["dec_h1_w"], np.float64) + np.asarray(w["dec_h1_b"], np.float64)).reshape(-1, 1, 1, 64)
    pre = None
    for name in ("dec_h2", "dec_h3", "dec_h4", "dec_h5"):
        k, b = np.asarray(w[name + "_k"], np.float64), np.asarray(w[name + "_b"], np.float64)
        n, hh, ww, _ = x.shape
        out = np.zeros((n, (hh - 1) * 2 + k.shape[0], (ww - 1) * 2 + k.shape[1], k.shape[2]))
        for u in range(k.shape[0]):
            for v in range(k.shape[1]):
                out[:, u:u + 2 * hh:2, v:v + 2 * ww:2, :] += np.einsum("bhwc,oc->bhwo", x, k[u, v])
        pre = out + b
        x = np.maximum(pre, 0.0)
    return x[..., 0], pre[..., 0]


@functools.lru_cache(maxsize=None)
def decoded(name):
    """(features, spec logits, spec image, float64 logits, float64 pre-ReLU, float32 port logits) of a checkpoint's inputs."""
    w, feat = weights(name), live_features(name)
    logits, image = PolicyDecodeSpec(w).decode(feat)
    ref, pre = reference_float64(w, feat)
    port = DreamerPolicy(w, sample=False).decoded_occupancy(dict(stoch=feat[:, :30], deter=feat[:, 30:]))
    for a in (logits, image, ref, pre, port):
        a.setflags(write=False)
    return feat, logits, image, ref, pre, port


@pytest.mark.parametrize("name", DECODERS)
def test_spec_logits_are_the_references_within_the_float32_ports_own_error(name):
    """Gather form in binary32 chains against scatter form in float64, every pixel (the border ones with fewer than 3 x 3 taps
    included): the spec's largest logit error is at most MARGIN times the float32 port's own on the same 162 inputs.
    Measured (spec / port): treitlstrasse_occupancy 1.77e-04 / 1.35e-04, treitlstrasse_20210220 1.50e-04 / 1.53e-04, on logits up to
    562 - the x 8 row's (profiles/policy_decode_spec.txt)."""
    feat, logits, _, ref, _, port = decoded(name)
    assert logits.shape == (len(feat), 64, 64) and port.shape == logits.shape and len(feat) == 162
    err_spec, err_port = np.abs(logits - ref).max(), np.abs(port - ref).max()
    print(f"{name}: spec {err_spec:.3e} port {err_port:.3e} ratio {err_spec / err_port:.2f} max logit {ref.max():.1f}")
    assert err_port > 0 and err_spec <= MARGIN * err_port, (err_spec, err_port)


@pytest.mark.parametrize("name", DECODERS)
def test_spec_image_is_the_float64_mode_away_from_zero(name):
    """image = Bernoulli.mode() = logit > 0 equals float64's at every pixel whose float64 pre-ReLU value is at least
    MARGIN x (the float32 port's largest error) away from 0; at most 0.1 % of the pixels are closer than that."""
    _, _, image, ref, pre, port = decoded(name)
    bound = MARGIN * np.abs(port - ref).max()
    sure = np.abs(pre) >= bound
    print(f"{name}: bound {bound:.3e}, excluded {100.0 * (1.0 - sure.mean()):.4f} % of {sure.size} pixels")
    assert 1.0 - sure.mean() <= 1e-3
    assert np.array_equal(image[sure], (pre > 0)[sure].astype(np.uint8))


@pytest.mark.parametrize("name", DECODERS)
def test_a_row_does_not_depend_on_its_batch_and_the_encoding(name):
    feat, logits, image, _, _, _ = decoded(name)
    spec = PolicyDecodeSpec(weights(name), threads=1)
    for i in (0, 77, 160, 161):
        lg, im = spec.decode(feat[i:i + 1])
        assert np.array_equal(lg[0].view(np.uint32), logits[i].view(np.uint32)) and np.array_equal(im[0], image[i])
    assert image.dtype == np.uint8 and np.array_equal(image, (logits > 0).astype(np.uint8))
    assert np.all(logits >= 0) and not np.any(np.signbit(logits))
    assert 0 < image.mean() < 1                    # (neither all drivable nor all wall)


def test_policy_decoder_fills_the_struct_or_returns_none():
    """racing_dreamer_amd._lib.policy_decoder: None for a checkpoint without dec_* arrays; else the ten arrays, a 4-D kernel passed
    as [kh kw out, in]."""
    from racing_dreamer_amd import _lib as L
    assert L.policy_decoder(os.path.join(GOLDEN, "dreamer_policy_austria.npz")) is None
    assert L.DECODER_KEYS == DECODER_KEYS
    want = {"dec_h1_w": (230, 64), "dec_h1_b": (1, 64), "dec_h2_k": (800, 64), "dec_h2_b": (1, 32), "dec_h3_k": (400, 32),
            "dec_h3_b": (1, 16), "dec_h4_k": (288, 16), "dec_h4_b": (1, 8), "dec_h5_k": (36, 8), "dec_h5_b": (1, 1)}
    for name in DECODERS:
        d, keep = L.policy_decoder(weights(name))
        assert d.struct_size == C.sizeof(L.RcPolicyDecoder) == 8 + 10 * 16 and len(keep) == 10
        for k, arr in zip(DECODER_KEYS, keep):
            a = getattr(d, k)
            assert (a.rows, a.cols) == want[k] and a.data == arr.ctypes.data and arr.dtype == np.float32 and arr.flags.c_contiguous
            assert np.array_equal(arr.reshape(-1), np.asarray(weights(name)[k]).reshape(-1))


def test_abi_symbols_refuse_before_they_look_at_the_handle(hip_lib):
    """The two new symbols are bound; rc_policy_load_decoder checks struct_size and shapes first and names the first wrong array."""
    from racing_dreamer_amd import _lib as L
    for name in ("rc_policy_load_decoder", "rc_policy_decode"):
        assert name in L.SYMBOLS and hasattr(hip_lib, name)
    d, keep = L.policy_decoder(weights(DECODERS[0]))
    assert hip_lib.rc_policy_load_decoder(None, C.byref(d)) == -1 and b"env is NULL" in hip_lib.rc_last_error()
    d.struct_size -= 4
    assert hip_lib.rc_policy_load_decoder(None, C.byref(d)) == -1 and b"struct_size" in hip_lib.rc_last_error()
    d.struct_size += 4
    d.dec_h3_k.cols, d.dec_h4_b.cols = 31, 9
    assert hip_lib.rc_policy_load_decoder(None, C.byref(d)) == -1 and b"dec_h3_k has shape [400, 31]" in hip_lib.rc_last_error()
    a = L.RcPolicyDecodeArgs()
    assert hip_lib.rc_policy_decode(None, C.byref(a)) == -1
