"""rc_policy_decode_lidar / policy_decode_lidar against its binary32 specification (tests/policy_lidar_decode_spec.c), bit for bit:
the live latents of short runs (one car, a partial workgroup, several cars per env, one row more than a workgroup, three
workgroups), the features of an imagined rollout, a zero and a large feature; each output alone; the partial tile; that nothing
but the outputs changes; slot masks, mixed tracks, the refusals and the decoder's life; world_model.model_loss against the
separate device calls."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from policy_lidar_decode_spec import PolicyLidarDecodeSpec
from racing_dreamer_amd import decoder as dec
from test_golden_policy import weights

pytestmark = pytest.mark.gpu
TRACK = "treitlstrasse_v2"
NAME = "treitlstrasse"          # a `lidar` agent with a reward head
OUTPUTS = ("mean", "std", "loglik")


@functools.lru_cache(maxsize=None)
def _ldec(scale_bias=-3.0):
    return dec.init_lidar_decoder(11, scale_bias)


@functools.lru_cache(maxsize=None)
def _spec(scale_bias=-3.0):
    return PolicyLidarDecodeSpec(_ldec(scale_bias))


def _cpu(d):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _env(num_envs, cars=1, steps=3, scale_bias=-3.0):
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv(TRACK, num_envs, cars, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=3)
    env.load_policy({**dict(weights(NAME)), **_ldec(scale_bias)})           # (load_policy picks the ldec_* arrays up)
    assert env.policy_has_lidar_decoder
    for _ in range(steps):
        env.policy_act()
        env.step(None, repeat=4)
    return env


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what=""):
    for k in got:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float32, (what, k, got[k].shape)
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k, float(np.abs(got[k] - want[k]).max()))


@pytest.mark.parametrize("num_envs, cars", [(1, 1), (5, 1), (2, 3), (33, 1), (67, 1)])
def test_live_latents_are_the_spec_bit_for_bit(num_envs, cars):
    """Three agent steps, then one policy_decode_lidar of the live latents: mean, std and loglik - against the car's own live
    scan - equal the spec fed the same latents and scans, as bit patterns."""
    env = _env(num_envs, cars)
    n = env.n_cars
    state = env.policy_state.cpu().numpy()
    scan = env.views["lidar"].cpu().numpy().reshape(n, 1080)
    assert np.abs(state[:, 30:230]).max() > 0.1 and scan.max() > 1.0
    got = _cpu(env.policy_decode_lidar(outputs=OUTPUTS))
    want = _spec().decode(state[:, :230], scan)
    assert got["mean"].shape == (n, 1080) and got["std"].shape == (n, 1080) and got["loglik"].shape == (n,)
    _same(got, want)
    assert np.all(got["std"] > 0) and np.all(np.isfinite(got["loglik"])) and np.all(got["loglik"] < 0)
    env.close()


def test_imagined_features_keep_their_leading_dimensions():
    """policy_imagine(horizon=3, features=True) on 67 cars, its [67, 3, 230] tensor straight into policy_decode_lidar with a
    [67, 3, 1080] target: [67, 3, 1080] and [67, 3] outputs that equal the spec on the same 201 rows; then an all-zero feature and
    a live one scaled by 8."""
    import torch
    env = _env(67)
    feat = env.policy_imagine(3, "mean", features=True)["feature"]
    assert feat.shape == (67, 3, 230)
    rng = np.random.default_rng(2)
    target = rng.uniform(-1.0, 17.0, (67, 3, 1080)).astype(np.float32)          # (both clips of the preprocessing are met)
    got = _cpu(env.policy_decode_lidar(features=feat, target=torch.from_numpy(target), outputs=OUTPUTS))
    assert got["mean"].shape == (67, 3, 1080) and got["std"].shape == (67, 3, 1080) and got["loglik"].shape == (67, 3)
    _same(got, _spec().decode(feat.cpu().numpy(), target))
    odd = np.stack([np.zeros(230, np.float32), 8.0 * env.policy_state.cpu().numpy()[0, :230]])
    got = _cpu(env.policy_decode_lidar(features=torch.from_numpy(odd), target=torch.from_numpy(target[0, :2]), outputs=OUTPUTS))
    want = _spec().decode(odd, target[0, :2])
    _same(got, want, "odd")
    assert np.abs(want["mean"][1]).max() > 4 * np.abs(want["mean"][0]).max()
    env.close()


def test_each_output_alone_is_itself_among_the_others():
    import torch
    env = _env(33)
    both = _cpu(env.policy_decode_lidar(outputs=OUTPUTS))
    for k in OUTPUTS:
        alone = _cpu(env.policy_decode_lidar(outputs=(k,)))
        assert set(alone) == {k} and alone[k].tobytes() == both[k].tobytes(), k
    feat = env.policy_imagine(2, features=True)["feature"]
    target = torch.full((33, 2, 1080), 3.0, device=env.device)
    both = _cpu(env.policy_decode_lidar(features=feat, target=target, outputs=OUTPUTS))
    for k in OUTPUTS:
        alone = _cpu(env.policy_decode_lidar(features=feat, target=target, outputs=(k,)))
        assert alone[k].tobytes() == both[k].tobytes(), k
    assert set(env.policy_decode_lidar(features=feat)) == {"mean"}          # (the default; no target needed)
    env.close()


def test_the_last_beam_is_its_own_columns():
    """Two decoders that differ only in ldec_params_w[:, 1079] and [:, 2159] - the last columns of the partial loc and scale
    tiles - give the same mean and std at beams 0 .. 1078, as bit patterns, and different ones at beam 1079; both equal the spec."""
    env = _env(35)
    base = _cpu(env.policy_decode_lidar(outputs=OUTPUTS))
    other = {k: v.copy() for k, v in _ldec().items()}
    other["ldec_params_w"][:, 1079] *= 1.5
    other["ldec_params_w"][:, 2159] += 0.01
    env.load_lidar_decoder(other)
    got = _cpu(env.policy_decode_lidar(outputs=OUTPUTS))
    for k in ("mean", "std"):
        assert np.array_equal(_bits(got[k][:, :1079]), _bits(base[k][:, :1079])), k
        assert np.all(got[k][:, 1079] != base[k][:, 1079]), k
    assert np.all(got["loglik"] != base["loglik"])
    n = env.n_cars
    _same(got, PolicyLidarDecodeSpec(other).decode(env.policy_state.cpu().numpy()[:, :230], env.views["lidar"].cpu().numpy().reshape(n, 1080)))
    env.close()


def test_nothing_else_changes_and_two_calls_agree():
    import torch
    env = _env(5)
    env.enable_episode_log(64)

    def snapshot():
        torch.cuda.synchronize()
        return [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes(),
                sorted(env.episode_counters.items())]
    before = snapshot()
    got = _cpu(env.policy_decode_lidar(outputs=OUTPUTS))
    again = _cpu(env.policy_decode_lidar(outputs=OUTPUTS))
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    feat = torch.from_numpy(np.random.default_rng(1).normal(0, 0.5, (9, 230)).astype(np.float32))
    env.policy_decode_lidar(features=feat, target=torch.ones((9, 1080)), outputs=OUTPUTS)
    assert before == snapshot()
    env.close()


def test_slot_mask_leaves_the_other_rows_alone():
    """slots=(1, 2) of three cars per env: slot 0's rows keep the caller's sentinel (zero without `out`), the others equal the full call."""
    import torch
    env = _env(2, 3)
    n = env.n_cars
    full = _cpu(env.policy_decode_lidar(outputs=OUTPUTS))
    out = dict(mean=torch.full((n, 1080), 7.0, device=env.device), std=torch.full((n, 1080), 7.0, device=env.device),
               loglik=torch.full((n,), 7.0, device=env.device))
    got = env.policy_decode_lidar(slots=(1, 2), outputs=OUTPUTS, out=out)
    assert all(got[k] is out[k] for k in out)
    got = _cpu(got)
    others = np.flatnonzero(np.arange(n) % 3 != 0)
    for k in full:
        assert np.array_equal(_bits(got[k][others]), _bits(full[k][others])) and np.all(got[k][::3] == 7), k
    got = _cpu(env.policy_decode_lidar(slots=(1, 2), outputs=OUTPUTS))
    for k in full:
        assert np.array_equal(_bits(got[k][others]), _bits(full[k][others])) and np.all(got[k][::3] == 0), k
    env.close()


def test_mixed_tracks_equal_their_parts():
    """A MixedTrackEnv of two tracks decodes each block's latents, against each block's own scans, into its rows: what each part
    gives on its own; given features go through the first part."""
    from racing_dreamer_amd.batched_env import MixedTrackEnv
    env = MixedTrackEnv([TRACK, "austria"], [5, 3], auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=4)
    env.load_policy(weights(NAME))
    assert not env.policy_has_lidar_decoder
    env.load_lidar_decoder(_ldec())
    assert env.policy_has_lidar_decoder
    for _ in range(3):
        env.policy_act()
        env.step(None, repeat=4)
    got = _cpu(env.policy_decode_lidar(outputs=OUTPUTS))
    lo = 0
    for p in env.parts:
        part = _cpu(p.policy_decode_lidar(outputs=OUTPUTS))
        for k in part:
            assert np.array_equal(_bits(got[k][lo:lo + p.n_cars]), _bits(part[k])), k
        lo += p.n_cars
    assert lo == 8
    _same(got, _spec().decode(env.policy_state.cpu().numpy()[:, :230], env.views["lidar"].cpu().numpy().reshape(8, 1080)))
    feat = env.policy_imagine(2, features=True)["feature"]
    out = _cpu(env.policy_decode_lidar(features=feat, outputs=("mean", "std")))
    want = _spec().decode(feat.cpu().numpy())
    assert out["mean"].shape == (8, 2, 1080)
    _same(out, want)
    env.close()


def test_refusals_and_the_decoders_life():
    """Every refusal names its cause; the decoder goes with NULL, with a load of a checkpoint without one and with unload."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv(TRACK, 2, 2, auto_reset=True, remap_actions=True)
    env.reset(mode="grid", seed=1)
    lib, n = env._lib, env.n_cars
    buf = dict(mean=torch.zeros((n, 1080), device=env.device), loglik=torch.zeros(n, device=env.device),
               features=torch.zeros((n, 230), device=env.device), target=torch.ones((n, 1080), device=env.device))

    def call(**kw):
        a = L.RcPolicyDecodeLidarArgs(C.sizeof(L.RcPolicyDecodeLidarArgs))
        a.slot_mask, a.mean = 3, buf["mean"].data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.rc_policy_decode_lidar(env._h, C.byref(a))
        return rc, lib.rc_last_error()

    def refused(text, **kw):
        with pytest.raises(L.RacecarHipError, match=text):
            env.policy_decode_lidar(**kw)

    d, keep = L.policy_lidar_decoder(_ldec())
    rc, msg = call()
    assert rc == -1 and b"no policy loaded" in msg
    refused("no policy loaded")
    assert lib.rc_policy_load_lidar_decoder(env._h, C.byref(d)) == -1 and b"no policy loaded" in lib.rc_last_error()
    env.load_policy(weights(NAME))
    assert not env.policy_has_lidar_decoder
    rc, msg = call()
    assert rc == -1 and b"no LiDAR decoder loaded" in msg
    refused("no LiDAR decoder loaded")
    wrong = {k: v for k, v in _ldec().items()}
    wrong["ldec_params_w"] = wrong["ldec_params_w"][:, :2159]
    with pytest.raises(L.RacecarHipError, match=r"ldec_params_w has shape \[512, 2159\]"):
        env.load_lidar_decoder(wrong)
    with pytest.raises(KeyError):
        env.load_lidar_decoder(dict(weights(NAME)))
    env.load_lidar_decoder(_ldec())
    assert env.policy_has_lidar_decoder and call()[0] == 0
    feats, loglik, target = buf["features"].data_ptr(), buf["loglik"].data_ptr(), buf["target"].data_ptr()
    for kw, text in ((dict(struct_size=8), b"struct_size"), (dict(mean=None), b"no output"), (dict(slot_mask=0), b"mask is empty"),
                     (dict(slot_mask=4), b"beyond cars_per_env"), (dict(features=feats, rows=n), b"slot mask"),
                     (dict(features=feats, rows=0, slot_mask=0), b"rows"), (dict(features=feats, rows=n, slot_mask=0, loglik=loglik), b"needs a target"),
                     (dict(target=target), b"target must be NULL")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, kw
    assert call(features=feats, rows=n, slot_mask=0, loglik=loglik, target=target)[0] == 0
    assert call(mean=None, loglik=loglik)[0] == 0
    refused("no output", outputs=())
    refused("slot mask", features=buf["features"], slots=(1,))
    refused("needs a target", features=buf["features"], outputs=("loglik",))
    refused("target must be NULL", target=buf["target"])
    with pytest.raises(ValueError):
        env.policy_decode_lidar(features=torch.zeros((n, 232), device=env.device))
    with pytest.raises(ValueError):
        env.policy_decode_lidar(outputs=("logits",))
    with pytest.raises(ValueError):
        env.policy_decode_lidar(features=buf["features"], target=torch.ones((n, 1081)))
    # the decoder goes with NULL, with a new load without ldec_* arrays, and with unload
    env.load_lidar_decoder(None)
    assert not env.policy_has_lidar_decoder and b"no LiDAR decoder loaded" in call()[1]
    assert lib.rc_policy_load_lidar_decoder(env._h, C.byref(d)) == 0 and call()[0] == 0
    env.load_policy(weights(NAME))
    assert not env.policy_has_lidar_decoder and b"no LiDAR decoder loaded" in call()[1]
    env.load_policy({**dict(weights(NAME)), **_ldec()})
    assert env.policy_has_lidar_decoder and call()[0] == 0
    env.unload_policy()
    assert not env.policy_has_lidar_decoder and b"no policy loaded" in call()[1]
    torch.cuda.synchronize()
    env.close()


def test_model_loss_is_the_formula_over_the_separate_device_calls():
    """world_model.model_loss on a batch of B = 3 windows of T = 6 steps: every term recomputed here in float64 from the separate
    device calls - policy_observe in mode `sample` under the same seed, policy_decode_lidar, policy_value - and combined as
    dreamer/models.py:99-110 does; with and without a pcont head; image_loglik and lidar_open_loop_summary use the same calls."""
    import torch
    from racing_dreamer_amd import world_model
    from racing_dreamer_amd.critic import init_critic
    env = _env(3, steps=0)
    scans, acts = [], []
    for _ in range(6):
        scans.append(env.views["lidar"].reshape(3, 1080).clone())
        acts.append(env.policy_state[:, 230:].clone())
        env.policy_act()
        env.step(None, repeat=4)
    rng = np.random.default_rng(8)
    batch = dict(lidar=torch.stack(scans, 1), action=torch.stack(acts, 1),
                 reward=torch.from_numpy(rng.normal(size=(3, 6)).astype(np.float32)).to(env.device),
                 discount=torch.from_numpy((rng.random((3, 6)) > 0.2).astype(np.float32)).to(env.device))
    half_log_2pi = 0.5 * math.log(2.0 * math.pi)
    for pcont in (False, True):
        if pcont:
            env.load_critic(init_critic(4))
        got = {k: float(v) for k, v in world_model.model_loss(env, batch, seed=9).items()}
        obs = env.policy_observe(batch["lidar"], batch["action"], mode="sample", seed=9, outputs=("feature", "kl", "reward"))
        div = float(obs["kl"].double().mean())
        image = float(env.policy_decode_lidar(features=obs["feature"], target=batch["lidar"], outputs=("loglik",))["loglik"].double().mean())
        reward = float((-0.5 * (batch["reward"].double() - obs["reward"].double()) ** 2 - half_log_2pi).mean())
        likes = image + reward
        assert set(got) == {"div", "image_loglik", "reward_loglik", "model_loss"} | ({"pcont_loglik"} if pcont else set())
        if pcont:
            p = env.policy_value(features=obs["feature"], outputs=("pcont",))["pcont"].double()
            t = 0.99 * batch["discount"].double()
            pc = 10.0 * float((t * torch.log(p) + (1 - t) * torch.log1p(-p)).mean())
            likes += pc
            assert got["pcont_loglik"] == pytest.approx(pc, rel=1e-12)
        assert got["div"] == pytest.approx(div, rel=1e-12) and got["image_loglik"] == pytest.approx(image, rel=1e-12)
        assert got["reward_loglik"] == pytest.approx(reward, rel=1e-12)
        assert got["model_loss"] == pytest.approx(max(div, 3.0) - likes, rel=1e-12)
        low = float(world_model.model_loss(env, batch, kl_scale=0.5, free_nats=div / 2, seed=9)["model_loss"])
        assert low == pytest.approx(0.5 * div - likes, rel=1e-12)
        assert float(world_model.image_loglik(env, batch, seed=9)) == pytest.approx(image, rel=1e-12)
    s = world_model.lidar_open_loop_summary(env, batch, context=4)
    feat = env.policy_observe(batch["lidar"], batch["action"], context=4)["feature"]
    assert s["model"].shape == (3, 6, 1080) and torch.equal(s["model"], (env.policy_decode_lidar(features=feat)["mean"] + 0.5) * 15.0)
    assert torch.equal(s["truth"], batch["lidar"]) and torch.equal(s["error"], s["model"] - s["truth"])
    env.close()


# ---- the occupancy decoder's Bernoulli log-likelihood (rc_policy_decode_loglik)
OCC = "treitlstrasse_occupancy"


@functools.lru_cache(maxsize=None)
def _occ_spec():
    from policy_decode_spec import PolicyDecodeSpec
    return PolicyDecodeSpec(weights(OCC))


def _occ_env(num_envs, cars=1, steps=3):
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv(TRACK, num_envs, cars, obs_type="lidar_occupancy", auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=3)
    env.load_policy(weights(OCC))
    assert env.policy_has_decoder and not env.policy_has_lidar_decoder
    for _ in range(steps):
        env.policy_act()
        env.step(None, repeat=4)
    return env


def _float64_loglik(logits, target):
    lg = logits.astype(np.float64)
    terms = np.where(target != 0, lg, 0.0) - (np.maximum(lg, 0.0) + np.log1p(np.exp(-np.abs(lg))))
    flat = terms.reshape(terms.shape[:-2] + (-1,))
    return flat.sum(-1), 1080 * 2.0 ** -24 * np.abs(flat).sum(-1)


@pytest.mark.parametrize("num_envs, cars", [(1, 1), (5, 1), (2, 3), (33, 1), (67, 1)])
def test_occupancy_loglik_of_live_latents_is_its_spec_bit_for_bit(num_envs, cars):
    """policy_decode_loglik on the live latents against each car's own rendered lidar_occupancy: loglik equals the spec's
    fixed-order sum over the spec's logits as a bit pattern, logits and image from the same launch are policy_decode's, and
    loglik is the float64 sum over policy_decode(logits=True) within 1080 x 2^-24 x sum |terms|."""
    import policy_decode_loglik_spec as pdl
    env = _occ_env(num_envs, cars)
    n = env.n_cars
    seen = env.views["lidar_occupancy"].cpu().numpy().reshape(n, 64, 64)
    got = _cpu(env.policy_decode_loglik(outputs=("loglik", "logits", "image")))
    plain = _cpu(env.policy_decode(logits=True, image=True))
    assert got["loglik"].shape == (n,) and got["loglik"].dtype == np.float32
    assert got["logits"].tobytes() == plain["logits"].tobytes() and got["image"].tobytes() == plain["image"].tobytes()
    want_logits, _ = _occ_spec().decode(env.policy_state.cpu().numpy()[:, :230])
    assert np.array_equal(_bits(got["logits"]), _bits(want_logits))
    assert np.array_equal(_bits(got["loglik"]), _bits(pdl.loglik(want_logits, seen)))
    ref, bound = _float64_loglik(plain["logits"], seen)
    assert np.all(np.abs(got["loglik"] - ref) <= bound) and np.all(got["loglik"] < 0)
    alone = _cpu(env.policy_decode_loglik())
    assert set(alone) == {"loglik"} and alone["loglik"].tobytes() == got["loglik"].tobytes()
    env.close()


def test_occupancy_loglik_of_imagined_features_masks_and_refusals():
    """[67, 3, 230] imagined features against a [67, 3, 64, 64] target: [67, 3] loglik equal to the spec; a slot mask leaves the
    other rows alone; the refusals of the new entry point; world_model.image_loglik uses this decoder when it is the loaded one."""
    import torch
    import policy_decode_loglik_spec as pdl
    from racing_dreamer_amd import _lib as L, world_model
    env = _occ_env(67)
    feat = env.policy_imagine(3, "mean", features=True)["feature"]
    target = (np.random.default_rng(4).random((67, 3, 64, 64)) > 0.4).astype(np.uint8)
    got = _cpu(env.policy_decode_loglik(target=torch.from_numpy(target), features=feat))
    want_logits, _ = _occ_spec().decode(feat.cpu().numpy())
    assert got["loglik"].shape == (67, 3) and np.array_equal(_bits(got["loglik"]), _bits(pdl.loglik(want_logits, target)))
    ref, bound = _float64_loglik(want_logits, target)
    assert np.all(np.abs(got["loglik"] - ref) <= bound)
    with pytest.raises(L.RacecarHipError, match="needs a target"):
        env.policy_decode_loglik(features=feat)
    with pytest.raises(L.RacecarHipError, match="target must be NULL"):
        env.policy_decode_loglik(target=torch.zeros((67, 64, 64), dtype=torch.uint8))
    with pytest.raises(L.RacecarHipError, match="slot mask"):
        env.policy_decode_loglik(target=torch.from_numpy(target), features=feat, slots=(0,))
    with pytest.raises(L.RacecarHipError, match="no output"):
        env.policy_decode_loglik(outputs=())
    a = L.RcPolicyDecodeLoglikArgs(8)
    assert env._lib.rc_policy_decode_loglik(env._h, C.byref(a)) == -1 and b"struct_size" in env._lib.rc_last_error()
    batch = dict(lidar=torch.rand((2, 4, 1080), device=env.device) * 10, action=torch.zeros((2, 4, 2), device=env.device),
                 lidar_occupancy=torch.from_numpy(target[:2, 0:1].repeat(4, 1)).to(env.device))
    f = env.policy_observe(batch["lidar"], batch["action"], mode="sample", seed=2)["feature"]
    want = env.policy_decode_loglik(target=batch["lidar_occupancy"], features=f)["loglik"].double().mean()
    assert float(world_model.image_loglik(env, batch, seed=2)) == pytest.approx(float(want), rel=1e-12)
    env.close()
    masked = _occ_env(2, 3)
    full = _cpu(masked.policy_decode_loglik())["loglik"]
    part = _cpu(masked.policy_decode_loglik(slots=(1, 2)))["loglik"]
    assert np.all(part[::3] == 0) and np.array_equal(_bits(part[np.arange(6) % 3 != 0]), _bits(full[np.arange(6) % 3 != 0]))
    masked.close()
    plain = _env(2)
    with pytest.raises(L.RacecarHipError, match="no decoder loaded"):
        plain.policy_decode_loglik()
    plain.close()
