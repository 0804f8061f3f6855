"""The binary32 specification of the LiDAR distance decoder (tests/policy_lidar_decode_spec.c) against a
float64 NumPy restatement of the reference's LidarDistanceDecoder (dreamer/models.py:424-441) and tfpl.IndependentNormal's
log_prob; the fixed summation order; the partial tile's beams; the decoder module; the host side of
rc_policy_load_lidar_decoder / rc_policy_decode_lidar that needs no GPU; world_model.model_loss on a spec-backed env."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import policy_lidar_decode_spec as pls
from policy_lidar_decode_spec import PolicyLidarDecodeSpec
from racing_dreamer_amd import decoder as dec
from test_golden_policy import weights
from test_policy_observe_spec import WITH_HEAD, _recorded
from test_policy_observe_spec import _spec as observe_spec

MARGIN = 4.0              # spec error / a plain float32 restatement's own, as items 12, 14, 15 and 16
SCALE_BIASES = (0.0, -30.0)
CHECKPOINTS = ("austria", "treitlstrasse_occupancy")
f32, f64 = np.float32, np.float64
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


@functools.lru_cache(maxsize=None)
def observed(name):
    """(features [16, 15, 230], scans [16, 15, 1080] metres) of the checkpoint's recorded closed-loop run: the posterior features of
    policy_observe's spec in mode `sample`, as training decodes them.  Read only."""
    scan, act, _ = _recorded(name)
    feat = observe_spec(name).observe(scan, act, mode="sample", seed=1)["feature"]
    scan = np.ascontiguousarray(scan, f32)
    feat.setflags(write=False)
    scan.setflags(write=False)
    return feat, scan


def restated(w, feat, scan, dtype):
    """models.py:424-441 and IndependentNormal(1080).log_prob in NumPy at `dtype`: (mean, std [n, 1080], loglik [n], terms)."""
    a = lambda k: np.asarray(w[k], dtype)
    x = np.asarray(feat, dtype).reshape(-1, 230)
    x = x @ a("ldec_dense1_w") + a("ldec_dense1_b")
    x = np.maximum(x @ a("ldec_dense2_w") + a("ldec_dense2_b"), dtype(0))
    x = x @ a("ldec_params_w") + a("ldec_params_b")
    x = np.where(x > 0, x, dtype(0.2) * x)
    loc, raw = x[:, :1080], x[:, 1080:]
    sd = np.maximum(raw, dtype(0)) + np.log1p(np.exp(-np.abs(raw)))
    y = np.clip(np.asarray(scan, dtype).reshape(-1, 1080), dtype(0), dtype(15)) / dtype(15) - dtype(0.5)
    z = (y - loc) / sd
    terms = dtype(-0.5) * z * z - np.log(sd) - dtype(HALF_LOG_2PI)
    return loc, sd, terms.sum(axis=1, dtype=dtype), terms


@functools.lru_cache(maxsize=None)
def decoded(name, scale_bias):
    """(weights, spec outputs, float64, float32) on the checkpoint's features, all flattened to [240, ...]."""
    w = dec.init_lidar_decoder(7, scale_bias)
    feat, scan = observed(name)
    spec = PolicyLidarDecodeSpec(w).decode(feat.reshape(-1, 230), scan.reshape(-1, 1080))
    return w, spec, restated(w, feat, scan, f64), restated(w, feat, scan, f32)


@pytest.mark.parametrize("scale_bias", SCALE_BIASES)
@pytest.mark.parametrize("name", CHECKPOINTS)
def test_spec_is_the_reference_within_a_float32_restatements_own_error(name, scale_bias):
    """k-ordered binary32 chains, pm_softplus / pm_log and the fixed-order sum against float64, on 240 posterior features per
    checkpoint: the spec's largest error in mean, std and loglik is at most MARGIN times that of a plain float32 NumPy restatement
    (BLAS matmuls, libm, pairwise sums) against the same float64.  With scale_bias -30 the scale is about 2.5e-3 and loglik about
    -1e8: where it is most sensitive.  Measured factors (spec / float32), austria and treitlstrasse_occupancy:
    scale_bias 0: mean 1.65 and 1.87, std 1.51 and 1.35, loglik 1.01 and 1.92; scale_bias -30: mean 1.65 and 1.87, std 0.96 and 1.06,
    loglik 1.00 and 1.16.  With the last layer's bias at the head of its chain, as in the other layers, the
    std factor at scale_bias -30 was 7.6: each of the 512 steps then rounds at magnitude 30.  So that layer adds its bias last."""
    _, spec, ref, port = decoded(name, scale_bias)
    assert spec["mean"].shape == (240, 1080) and spec["loglik"].shape == (240,)
    for i, k in enumerate(("mean", "std", "loglik")):
        err_spec, err_port = np.abs(spec[k] - ref[i]).max(), np.abs(port[i] - ref[i]).max()
        print(f"{name} scale_bias {scale_bias} {k}: spec {err_spec:.3e} float32 {err_port:.3e} factor {err_spec / err_port:.2f} "
              f"largest |value| {np.abs(ref[i]).max():.3e}")
        assert err_port > 0 and err_spec <= MARGIN * err_port, (k, err_spec, err_port)
    if scale_bias:
        assert 2.0e-3 < np.median(ref[1]) < 3.0e-3 and ref[1].max() < 1e-2          # (the narrow case is narrow: softplus(-6) = 2.5e-3)


@pytest.mark.parametrize("scale_bias", SCALE_BIASES)
def test_loglik_is_the_float64_sum_of_its_terms_within_the_rounding_bound(scale_bias):
    """loglik against the terms recomputed in float64 from the spec's own mean and std and the preprocessed target: the binary32
    terms and their fixed-order sum stay within 1080 x 2^-24 x sum |terms| of it."""
    _, spec, _, _ = decoded("austria", scale_bias)
    _, scan = observed("austria")
    y = np.clip(scan.reshape(-1, 1080).astype(f64), 0.0, 15.0) / 15.0 - 0.5
    z = (y - spec["mean"].astype(f64)) / spec["std"].astype(f64)
    terms = -0.5 * z * z - np.log(spec["std"].astype(f64)) - HALF_LOG_2PI
    bound = 1080 * 2.0 ** -24 * np.abs(terms).sum(axis=1)
    err = np.abs(spec["loglik"].astype(f64) - terms.sum(axis=1))
    print(f"scale_bias {scale_bias}: largest error / bound {np.max(err / bound):.3e}")
    assert np.all(err <= bound)


def test_the_summation_order_is_the_documented_one():
    """34 groups of 32 (the last one 24 terms and 8 zeros), a binary tree inside a group, the groups in ascending order from +0."""
    rng = np.random.default_rng(3)
    terms = (rng.normal(size=1080) * 10.0 ** rng.uniform(-3, 5, 1080)).astype(f32)
    padded = np.concatenate([terms, np.zeros(8, f32)]).reshape(34, 32)
    v = padded.copy()
    for m in (1, 2, 4, 8, 16):
        v[:, ::2 * m] = v[:, ::2 * m] + v[:, m::2 * m]
    total = f32(0)
    for g in range(34):
        total = f32(total + v[g, 0])
    assert pls.ordered_sum(terms).view(np.uint32) == total.view(np.uint32)
    assert pls.ordered_sum(terms) != f32(np.cumsum(terms, dtype=f32)[-1])          # (and not a plain running sum)
    tail = np.zeros(1080, f32)
    tail[1056:] = terms[1056:]
    assert pls.ordered_sum(tail).view(np.uint32) == v[33, 0].view(np.uint32)


@pytest.mark.parametrize("scale_bias", SCALE_BIASES)
def test_beams_1056_to_1079_on_their_own(scale_bias):
    """The 24 beams of the partial tile: mean and std within MARGIN of the float32 restatement's error ON THOSE BEAMS, every one
    finite and the scale positive; a decoder changed in the columns of beam 1079 alone changes beam 1079 alone, and loglik by that
    beam's term."""
    w, spec, ref, port = decoded("austria", scale_bias)
    for i, k in enumerate(("mean", "std")):
        err_spec, err_port = np.abs(spec[k][:, 1056:] - ref[i][:, 1056:]).max(), np.abs(port[i][:, 1056:] - ref[i][:, 1056:]).max()
        assert err_port > 0 and err_spec <= MARGIN * err_port, (k, err_spec, err_port)
    assert np.all(np.isfinite(spec["mean"][:, 1056:])) and np.all(spec["std"][:, 1056:] > 0)
    feat, scan = observed("austria")
    other = {k: v.copy() for k, v in w.items()}
    other["ldec_params_w"][:, 1079] *= 1.5
    other["ldec_params_w"][:, 2159] += 0.01
    got = PolicyLidarDecodeSpec(other).decode(feat[:2], scan[:2])
    base = {k: v.reshape(16, 15, -1)[:2] for k, v in spec.items()}
    for k in ("mean", "std"):
        assert np.array_equal(got[k][..., :1079].view(np.uint32), base[k][..., :1079].view(np.uint32))
        assert np.all(got[k][..., 1079] != base[k][..., 1079])
    assert np.all(got["loglik"] != base["loglik"][..., 0])


def test_a_row_does_not_depend_on_its_batch():
    _, spec, _, _ = decoded("austria", 0.0)
    feat, scan = observed("austria")
    one = PolicyLidarDecodeSpec(dec.init_lidar_decoder(7, 0.0), threads=1)
    for i in (0, 77, 239):
        got = one.decode(feat.reshape(-1, 230)[i:i + 1], scan.reshape(-1, 1080)[i:i + 1])
        for k in ("mean", "std", "loglik"):
            assert np.array_equal(got[k][0].view(np.uint32), spec[k][i].view(np.uint32)), k
    assert "loglik" not in one.decode(feat[0])


def test_the_unit_and_its_kernel_are_built_and_checked():
    from racing_dreamer_amd import build
    assert "racecar_decode_lidar.hip" in build.SOURCES
    assert "rc_policy_decode_lidar_kernel" in build.NO_SPILL_KERNELS
    assert "rc_policy_decode_lidar_kernel" in build.required_kernels("shipped")


def test_init_save_load_and_from_variables(tmp_path):
    from racing_dreamer_amd import _lib as L
    w = dec.init_lidar_decoder(3, scale_bias=-2.5)
    assert tuple(w) == L.LIDAR_DECODER_KEYS == pls.KEYS and L.LIDAR_DECODER_SHAPES == pls.SHAPES
    for k, shape in zip(L.LIDAR_DECODER_KEYS, L.LIDAR_DECODER_SHAPES):
        assert w[k].shape == shape and w[k].dtype == f32
        if len(shape) == 2:
            limit = math.sqrt(6.0 / sum(shape))
            assert np.abs(w[k]).max() <= limit and np.abs(w[k]).max() > 0.99 * limit and abs(float(w[k].mean())) < 0.01 * limit
    assert not w["ldec_dense1_b"].any() and not w["ldec_dense2_b"].any() and not w["ldec_params_b"][:1080].any()
    assert np.all(w["ldec_params_b"][1080:] == f32(-2.5))
    again = dec.init_lidar_decoder(3, scale_bias=-2.5)
    assert all(np.array_equal(w[k], again[k]) for k in w) and not np.array_equal(w["ldec_dense1_w"], dec.init_lidar_decoder(4)["ldec_dense1_w"])
    path = tmp_path / "ldec.npz"
    dec.save_lidar_decoder(path, w)
    back = dec.load_lidar_decoder_file(path)
    assert tuple(back) == L.LIDAR_DECODER_KEYS and all(np.array_equal(w[k], back[k]) and back[k].dtype == f32 for k in w)
    rng = np.random.default_rng(0)
    encoder = [rng.normal(size=s).astype(f32) for s in ((200, 600), (2, 600), (32, 200), (200,))]
    reward = [rng.normal(size=s).astype(f32) for s in ((230, 400), (400,), (400, 400), (400,), (400, 1), (1,))]
    mine = [w[k] for k in L.LIDAR_DECODER_KEYS]
    got = dec.lidar_decoder_from_variables(encoder + mine + reward)
    assert tuple(got) == L.LIDAR_DECODER_KEYS and all(np.array_equal(got[k], w[k]) for k in w)
    with pytest.raises(ValueError):
        dec.lidar_decoder_from_variables(encoder + reward)
    with pytest.raises(ValueError):
        dec.lidar_decoder_from_variables(encoder + mine[:5] + [np.zeros(2161, f32)] + reward)
    with pytest.raises(ValueError):
        dec.lidar_decoder_from_variables(mine + encoder + mine)


def test_abi_symbols_structs_and_refusals_without_a_handle(hip_lib):
    """The two new symbols are bound; the structs have the header's sizes; rc_policy_load_lidar_decoder checks struct_size and shapes
    before it looks at the handle and names the first wrong array."""
    from racing_dreamer_amd import _lib as L
    for name in ("rc_policy_load_lidar_decoder", "rc_policy_decode_lidar"):
        assert name in L.SYMBOLS and hasattr(hip_lib, name)
    assert L.policy_lidar_decoder(weights("austria")) is None
    d, keep = L.policy_lidar_decoder(dec.init_lidar_decoder(1))
    assert d.struct_size == C.sizeof(L.RcPolicyLidarDecoder) == 8 + 6 * 16 and len(keep) == 6
    assert C.sizeof(L.RcPolicyDecodeLidarArgs) == 64 and C.sizeof(L.RcPolicyDecodeArgs) == 56          # (the old struct keeps its size)
    assert (d.ldec_params_w.rows, d.ldec_params_w.cols, d.ldec_params_b.rows, d.ldec_params_b.cols) == (512, 2160, 1, 2160)
    assert hip_lib.rc_policy_load_lidar_decoder(None, C.byref(d)) == -1 and b"env is NULL" in hip_lib.rc_last_error()
    d.struct_size -= 4
    assert hip_lib.rc_policy_load_lidar_decoder(None, C.byref(d)) == -1 and b"struct_size" in hip_lib.rc_last_error()
    d.struct_size += 4
    d.ldec_dense2_w.cols, d.ldec_params_b.cols = 511, 2161
    assert hip_lib.rc_policy_load_lidar_decoder(None, C.byref(d)) == -1 and b"ldec_dense2_w has shape [256, 511]" in hip_lib.rc_last_error()
    d.ldec_dense2_w.cols, d.ldec_dense1_b.data = 512, None
    assert hip_lib.rc_policy_load_lidar_decoder(None, C.byref(d)) == -1 and b"ldec_dense1_b is missing" in hip_lib.rc_last_error()
    a = L.RcPolicyDecodeLidarArgs()
    assert hip_lib.rc_policy_decode_lidar(None, C.byref(a)) == -1
    assert hip_lib.rc_abi_version() == 3


class _SpecEnv:
    """A CPU stand-in for BatchedRaceEnv whose three calls are the binary32 specifications: policy_observe, policy_decode_lidar and
    (the pcont head) policy_value, on torch CPU tensors."""

    def __init__(self, name, ldec, critic):
        import torch
        from policy_returns_spec import PolicyReturnsSpec
        self.torch, self.device = torch, torch.device("cpu")
        self.obs, self.dec = observe_spec(name), PolicyLidarDecodeSpec(ldec)
        self.ret = PolicyReturnsSpec(weights(name), critic) if critic is not None else None
        self.policy_has_reward_head, self.policy_has_lidar_decoder, self.policy_has_pcont_head = True, True, critic is not None
        self.calls = []

    def policy_observe(self, lidar, action, context=None, mode="mean", seed=0, outputs=("feature",)):
        self.calls.append(("observe", mode, seed, context))
        got = self.obs.observe(lidar.numpy(), action.numpy(), context=context, mode=mode, seed=seed)
        return {k: self.torch.from_numpy(np.ascontiguousarray(got[k])) for k in outputs}

    def policy_decode_lidar(self, features=None, slots=None, target=None, outputs=("mean",), out=None):
        self.calls.append(("decode_lidar", tuple(outputs)))
        got = self.dec.decode(features.numpy(), None if target is None else target.numpy())
        return {k: self.torch.from_numpy(got[k]) for k in outputs}

    def policy_value(self, features=None, slots=None, outputs=("value",)):
        self.calls.append(("value", tuple(outputs)))
        lead = features.shape[:-1]
        got = self.ret.returns(features.reshape(-1, 230).numpy(), horizon=0)
        return {k: self.torch.from_numpy(np.ascontiguousarray(got[k + "_start"])).reshape(lead) for k in outputs}


@pytest.mark.parametrize("pcont", (False, True))
def test_model_loss_is_the_formula_of_the_reference(pcont):
    """world_model.model_loss on a spec-backed env: kl_scale max(div, free_nats) - (image + reward + pcont_scale pcont), each term
    recomputed here in float64 from the specs' outputs; free nats above and below div; image_loglik and lidar_open_loop_summary
    agree with the same calls."""
    import torch
    from racing_dreamer_amd import world_model
    from racing_dreamer_amd.critic import init_critic
    name = WITH_HEAD[0]
    scan, act, _ = _recorded(name)
    rng = np.random.default_rng(5)
    B, T = 3, 6
    batch = dict(lidar=torch.from_numpy(scan[:B, :T].copy()), action=torch.from_numpy(act[:B, :T].copy()),
                 reward=torch.from_numpy(rng.normal(size=(B, T)).astype(f32)), discount=torch.from_numpy((rng.random((B, T)) > 0.2).astype(f32)))
    ldec = dec.init_lidar_decoder(2, -3.0)
    env = _SpecEnv(name, ldec, init_critic(4) if pcont else None)
    got = world_model.model_loss(env, batch, seed=9)
    assert env.calls[0] == ("observe", "sample", 9, None)
    obs = observe_spec(name).observe(scan[:B, :T], act[:B, :T], mode="sample", seed=9)
    div = obs["kl"].astype(f64).mean()
    image = PolicyLidarDecodeSpec(ldec).decode(obs["feature"], scan[:B, :T])["loglik"].astype(f64).mean()
    reward = (-0.5 * (batch["reward"].numpy().astype(f64) - obs["reward"].astype(f64)) ** 2 - HALF_LOG_2PI).mean()
    likes = image + reward
    assert set(got) == {"div", "image_loglik", "reward_loglik", "model_loss"} | ({"pcont_loglik"} if pcont else set())
    if pcont:
        p = env.ret.returns(obs["feature"].reshape(-1, 230), horizon=0)["pcont_start"].astype(f64).reshape(B, T)
        t = 0.99 * batch["discount"].numpy().astype(f64)
        pc = 10.0 * (t * np.log(p) + (1 - t) * np.log1p(-p)).mean()
        likes += pc
        assert float(got["pcont_loglik"]) == pytest.approx(pc, rel=1e-12)
    assert all(v.dtype == torch.float64 and v.dim() == 0 for v in got.values())
    assert float(got["div"]) == pytest.approx(div, rel=1e-12) and float(got["image_loglik"]) == pytest.approx(image, rel=1e-12)
    assert float(got["reward_loglik"]) == pytest.approx(reward, rel=1e-12)
    assert float(got["model_loss"]) == pytest.approx(max(div, 3.0) - likes, rel=1e-12)
    low = world_model.model_loss(env, batch, kl_scale=0.5, free_nats=div / 2, seed=9)
    assert float(low["model_loss"]) == pytest.approx(0.5 * div - likes, rel=1e-12)
    high = world_model.model_loss(env, batch, kl_scale=0.5, free_nats=2 * div + 1, seed=9)
    assert float(high["model_loss"]) == pytest.approx(0.5 * (2 * div + 1) - likes, rel=1e-12)
    assert float(world_model.image_loglik(env, batch, seed=9)) == pytest.approx(image, rel=1e-12)
    s = world_model.lidar_open_loop_summary(env, batch, context=4)
    assert env.calls[-2] == ("observe", "mean", 0, 4) and s["model"].shape == (B, T, 1080)
    mean = PolicyLidarDecodeSpec(ldec).decode(observe_spec(name).observe(scan[:B, :T], act[:B, :T], context=4)["feature"])["mean"]
    assert torch.equal(s["model"], (torch.from_numpy(mean) + 0.5) * 15.0) and torch.equal(s["truth"], batch["lidar"])
    assert torch.equal(s["error"], s["model"] - s["truth"])
    env.policy_has_lidar_decoder = False
    with pytest.raises(RuntimeError, match="LidarDistanceDecoder"):
        world_model.model_loss(env, batch)
