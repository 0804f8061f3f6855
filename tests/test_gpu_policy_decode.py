"""rc_policy_decode / policy_decode against its binary32 specification (tests/policy_decode_spec.c), bit for bit: the live latents of
short runs (one car, a partial workgroup, several cars per env, more rows than any workgroup takes), the features of an imagined
rollout, a zero and a large feature; the mismatch count against the env's own render; that nothing but the outputs changes; slot
masks, mixed tracks, the refusals and the decoder's life."""
import ctypes as C
import functools

import numpy as np
import pytest

from policy_decode_spec import PolicyDecodeSpec
from test_golden_policy import weights
from test_policy_decode_spec import DECODERS

pytestmark = pytest.mark.gpu
TRACK = "treitlstrasse_v2"


@functools.lru_cache(maxsize=None)
def _spec(name):
    return PolicyDecodeSpec(weights(name))


def _cpu(d):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _env(name, num_envs, cars=1, obs_type="lidar_occupancy", steps=3):
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv(TRACK, num_envs, cars, obs_type=obs_type, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=3)
    env.load_policy(weights(name))
    assert env.policy_has_decoder
    for _ in range(steps):
        env.policy_act()
        env.step(None, repeat=4)
    return env


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("num_envs, cars", [(1, 1), (5, 1), (2, 3), (67, 1)])
@pytest.mark.parametrize("name", DECODERS)
def test_live_latents_are_the_spec_bit_for_bit(name, num_envs, cars):
    """Three agent steps, then one policy_decode of the live latents: the logits equal the spec's as bit patterns, the image is
    logits > 0, and mismatch is the host's count of pixels in which the image differs from the env's own lidar_occupancy."""
    env = _env(name, num_envs, cars)
    n = env.n_cars
    state = env.policy_state.cpu().numpy()
    assert np.abs(state[:, 30:230]).max() > 0.1
    got = _cpu(env.policy_decode(logits=True, image=True, mismatch=True))
    want_logits, want_image = _spec(name).decode(state[:, :230])
    assert got["logits"].shape == (n, 64, 64) and got["image"].shape == (n, 64, 64) and got["mismatch"].shape == (n,)
    assert got["logits"].dtype == np.float32 and got["image"].dtype == np.uint8 and got["mismatch"].dtype == np.int32
    assert np.array_equal(_bits(got["logits"]), _bits(want_logits)), float(np.abs(got["logits"] - want_logits).max())
    assert np.array_equal(got["image"], (got["logits"] > 0).astype(np.uint8)) and np.array_equal(got["image"], want_image)
    seen = env.views["lidar_occupancy"].cpu().numpy().reshape(n, 64, 64)
    assert np.array_equal(got["mismatch"], (got["image"] != seen).reshape(n, -1).sum(1))
    assert 0 < got["mismatch"].max() < 4096 and 0 < got["image"].mean() < 1
    only = _cpu(env.policy_decode(image=False, mismatch=True))            # (the count does not need the image)
    assert set(only) == {"mismatch"} and np.array_equal(only["mismatch"], got["mismatch"])
    env.close()


@pytest.mark.parametrize("name", DECODERS)
def test_imagined_features_keep_their_leading_dimensions(name):
    """policy_imagine(horizon=3, features=True) on 67 cars, its [67, 3, 230] tensor straight into policy_decode: [67, 3, 64, 64]
    outputs that equal the spec on the same 201 rows; then an all-zero feature and a live one scaled by 8."""
    import torch
    env = _env(name, 67)
    feat = env.policy_imagine(3, "mean", features=True)["feature"]
    assert feat.shape == (67, 3, 230)
    got = _cpu(env.policy_decode(features=feat, logits=True, image=True))
    want_logits, want_image = _spec(name).decode(feat.cpu().numpy())
    assert got["logits"].shape == (67, 3, 64, 64) and got["image"].shape == (67, 3, 64, 64)
    assert np.array_equal(_bits(got["logits"]), _bits(want_logits)) and np.array_equal(got["image"], want_image)
    odd = np.stack([np.zeros(230, np.float32), 8.0 * env.policy_state.cpu().numpy()[0, :230]])
    got = _cpu(env.policy_decode(features=torch.from_numpy(odd), logits=True))
    want_logits, _ = _spec(name).decode(odd)
    assert set(got) == {"logits", "image"} and got["logits"].shape == (2, 64, 64)
    assert np.array_equal(_bits(got["logits"]), _bits(want_logits)) and want_logits[1].max() > 100.0
    env.close()


def test_nothing_else_changes_and_two_calls_agree():
    import torch
    env = _env(DECODERS[0], 5)
    env.enable_episode_log(64)

    def snapshot():
        torch.cuda.synchronize()
        return [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes(),
                sorted(env.episode_counters.items())]
    before = snapshot()
    got = _cpu(env.policy_decode(logits=True, image=True, mismatch=True))
    again = _cpu(env.policy_decode(logits=True, image=True, mismatch=True))
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    feat = torch.from_numpy(np.random.default_rng(1).normal(0, 0.5, (9, 230)).astype(np.float32))
    env.policy_decode(features=feat)
    assert before == snapshot()
    env.close()


def test_slot_mask_leaves_the_other_rows_alone():
    """slots=(1, 2) of three cars per env: slot 0's rows keep the caller's sentinel (zero without `out`), the others equal the full call."""
    import torch
    env = _env(DECODERS[0], 2, 3)
    n = env.n_cars
    full = _cpu(env.policy_decode(logits=True, image=True, mismatch=True))
    out = dict(logits=torch.full((n, 64, 64), 7.0, device=env.device), image=torch.full((n, 64, 64), 7, dtype=torch.uint8, device=env.device),
               mismatch=torch.full((n,), 7, dtype=torch.int32, device=env.device))
    got = env.policy_decode(slots=(1, 2), logits=True, image=True, mismatch=True, out=out)
    assert all(got[k] is out[k] for k in out)
    got = _cpu(got)
    others = np.flatnonzero(np.arange(n) % 3 != 0)
    for k in full:
        assert np.array_equal(got[k][others], full[k][others]) and np.all(got[k][::3] == 7), k
    got = _cpu(env.policy_decode(slots=(1, 2), logits=True, mismatch=True))
    for k in full:
        assert np.array_equal(got[k][others], full[k][others]) and np.all(got[k][::3] == 0), k
    env.close()


def test_mixed_tracks_equal_their_parts():
    """A MixedTrackEnv of two tracks decodes each block's latents into its rows: what each part gives on its own; given features
    go through the first part."""
    from racing_dreamer_amd.batched_env import MixedTrackEnv
    name = DECODERS[0]
    env = MixedTrackEnv([TRACK, "austria"], [5, 3], obs_type="lidar_occupancy", auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=4)
    env.load_policy(weights(name))
    assert env.policy_has_decoder
    for _ in range(3):
        env.policy_act()
        env.step(None, repeat=4)
    got = _cpu(env.policy_decode(logits=True, image=True, mismatch=True))
    lo = 0
    for p in env.parts:
        part = _cpu(p.policy_decode(logits=True, image=True, mismatch=True))
        for k in part:
            assert np.array_equal(got[k][lo:lo + p.n_cars], part[k]), k
        lo += p.n_cars
    assert lo == 8 and np.array_equal(_bits(got["logits"]), _bits(_spec(name).decode(env.policy_state.cpu().numpy()[:, :230])[0]))
    seen = env.views["lidar_occupancy"].cpu().numpy().reshape(8, -1)
    assert np.array_equal(got["mismatch"], (got["image"].reshape(8, -1) != seen).sum(1))
    feat = env.policy_imagine(2, features=True)["feature"]
    dec = _cpu(env.policy_decode(features=feat, logits=True))
    assert dec["logits"].shape == (8, 2, 64, 64) and np.array_equal(_bits(dec["logits"]), _bits(_spec(name).decode(feat.cpu().numpy())[0]))
    env.close()


def test_refusals_and_the_decoders_life():
    """Every refusal names its cause; the decoder goes with NULL, with a load of a checkpoint without one and with unload."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    name = DECODERS[0]
    env = BatchedRaceEnv(TRACK, 2, 2, obs_type="lidar_occupancy", auto_reset=True, remap_actions=True)
    env.reset(mode="grid", seed=1)
    lib, n = env._lib, env.n_cars
    buf = dict(logits=torch.zeros((n, 64, 64), device=env.device), image=torch.zeros((n, 64, 64), dtype=torch.uint8, device=env.device),
               mismatch=torch.zeros(n, dtype=torch.int32, device=env.device), features=torch.zeros((n, 230), device=env.device))

    def call(**kw):
        a = L.RcPolicyDecodeArgs(C.sizeof(L.RcPolicyDecodeArgs))
        a.slot_mask, a.image = 3, buf["image"].data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.rc_policy_decode(env._h, C.byref(a))
        return rc, lib.rc_last_error()

    def refused(text, **kw):
        with pytest.raises(L.RacecarHipError, match=text):
            env.policy_decode(**kw)

    dec, keep = L.policy_decoder(weights(name))
    rc, msg = call()
    assert rc == -1 and b"no policy loaded" in msg
    refused("no policy loaded")
    assert lib.rc_policy_load_decoder(env._h, C.byref(dec)) == -1 and b"no policy loaded" in lib.rc_last_error()
    env.load_policy(weights("austria"))
    assert not env.policy_has_decoder
    rc, msg = call()
    assert rc == -1 and b"no decoder loaded" in msg
    refused("no decoder loaded")
    wrong = dict(weights(name))
    wrong["dec_h4_k"] = wrong["dec_h4_k"][:, :, :, :15]
    wrong["dec_h5_b"] = np.zeros(2, np.float32)
    with pytest.raises(L.RacecarHipError, match=r"dec_h4_k has shape \[288, 15\]"):
        env.load_policy(wrong)
    env.load_policy(weights(name))
    assert env.policy_has_decoder and call()[0] == 0
    feats = buf["features"].data_ptr()
    for kw, text in ((dict(struct_size=8), b"struct_size"), (dict(image=None), b"no output"), (dict(slot_mask=0), b"mask is empty"),
                     (dict(slot_mask=4), b"beyond cars_per_env"), (dict(features=feats, rows=n), b"slot mask"),
                     (dict(features=feats, rows=0, slot_mask=0), b"rows"), (dict(features=feats, rows=n, slot_mask=0, mismatch=buf["mismatch"].data_ptr()), b"mismatch")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, kw
    assert call(features=feats, rows=n, slot_mask=0, logits=buf["logits"].data_ptr())[0] == 0
    assert call(image=None, mismatch=buf["mismatch"].data_ptr())[0] == 0
    refused("no output", image=False)
    refused("slot mask", features=buf["features"], slots=(1,))
    refused("mismatch", features=buf["features"], mismatch=True)
    with pytest.raises(ValueError):
        env.policy_decode(features=torch.zeros((n, 232), device=env.device))
    # under obs_type lidar there is no render to compare with
    plain = BatchedRaceEnv(TRACK, 2, 1, auto_reset=True, remap_actions=True)
    plain.reset(mode="grid", seed=1)
    plain.load_policy(weights(name))
    with pytest.raises(L.RacecarHipError, match="mismatch needs the rendered"):
        plain.policy_decode(mismatch=True)
    assert plain.policy_decode()["image"].shape == (2, 64, 64)
    plain.close()
    # the decoder goes with NULL, with a new load without dec_* arrays, and with unload
    assert lib.rc_policy_load_decoder(env._h, None) == 0 and b"no decoder loaded" in call()[1]
    assert lib.rc_policy_load_decoder(env._h, C.byref(dec)) == 0 and call()[0] == 0
    env.load_policy({k: weights(name)[k] for k in weights(name).files if not k.startswith("dec_")})
    assert not env.policy_has_decoder and b"no decoder loaded" in call()[1]
    env.load_policy(weights(name))
    env.unload_policy()
    assert not env.policy_has_decoder and b"no policy loaded" in call()[1]
    torch.cuda.synchronize()
    env.close()
