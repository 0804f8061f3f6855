"""rc_policy_imagine / policy_imagine against its binary32 specification (tests/policy_imagine_spec.c), bit for bit: one call for
every kind of checkpoint, both action conventions, partial and several workgroups, both modes; open loop; from the live latents of
a run with resets; that nothing but the outputs changes; slot masks, mixed tracks, shards; the refusals."""
import ctypes as C

import numpy as np
import pytest

from policy_imagine_spec import PolicyImagineSpec
from policy_sample_spec import EpisodeClock
from test_golden_policy import weights
from test_gpu_policy_device import _recorded_inputs

pytestmark = pytest.mark.gpu
MODES = ("mean", "sample")


def _cpu(d):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(got, want, what, rows=slice(None)):
    for k, g in got.items():
        assert g[rows].tobytes() == want[k][rows].tobytes(), (what, k, float(np.abs(g[rows] - want[k][rows]).max()))


@pytest.mark.parametrize("remap", [True, False])
@pytest.mark.parametrize("name", ["austria", "treitlstrasse", "treitlstrasse_20210220"])
def test_one_call_is_the_spec_bit_for_bit(name, remap):
    """Recorded latents written into policy_state, one policy_imagine: action, feature, reward and reward_start (the two plain
    checkpoints carry a head; the normalized one gives actions and features only) equal the spec in every row for 1 and 33 cars
    (a partial workgroup, and a second one) x H = 1, 2, 15 and for 4 097 cars x H = 2, in both modes.  The outputs are raw: the
    env's action convention does not enter."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    spec_pol = PolicyImagineSpec(weights(name))
    assert spec_pol.has_head == (name != "treitlstrasse_20210220")
    for n, horizons in ((1, (1, 2, 15)), (33, (1, 2, 15)), (4097, (2,))):
        _, state, _ = _recorded_inputs(min(n, 97), seed=3)
        state = np.concatenate([state] * -(-n // len(state)))[:n]
        state = state * (1.0 + 0.001 * (np.arange(n) // 97))[:, None].astype(np.float32)
        env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=remap)
        env.reset(mode="random", seed=1)
        env.load_policy(weights(name))
        assert env.policy_has_reward_head == spec_pol.has_head
        env.policy_state.copy_(torch.from_numpy(state))
        clock = EpisodeClock(n)
        clock.reset()
        for h in horizons:
            for mode in MODES:
                got = _cpu(env.policy_imagine(h, mode, seed=77, features=True, start_reward=spec_pol.has_head))
                want = spec_pol.imagine(state, clock.keys(), h, mode, seed=77)
                assert set(got) == {"action", "feature"} | ({"reward", "reward_start"} if spec_pol.has_head else set())
                _same(got, want, (name, n, h, mode))
                assert np.abs(want["action"]).max() <= 1.0 and np.abs(want["action"]).max() > 0.01
        env.close()


@pytest.mark.parametrize("mode, name, h, start", [pytest.param(mode, *case, id=mode + tag) for tag, case in
                                                  (("", ("austria", 5, True)), ("-no-head", ("treitlstrasse_20210220", 2, False))) for mode in MODES])
def test_open_loop_follows_the_given_actions(mode, name, h, start):
    """Actions given from outside, a third of them beyond +-1: the outputs equal the spec's, `action` echoes the clamped input.
    Also on the normalized checkpoint, which has no reward head, without the starting reward: the prior's three layers alone."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n = 33
    _, state, _ = _recorded_inputs(n, seed=3)
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=1)
    env.load_policy(weights(name))
    assert env.policy_has_reward_head == start
    env.policy_state.copy_(torch.from_numpy(state))
    clock = EpisodeClock(n)
    clock.reset()
    acts = np.random.default_rng(2).uniform(-1.5, 1.5, (n, h, 2)).astype(np.float32)
    got = _cpu(env.policy_imagine(h, mode, seed=5, actions=torch.from_numpy(acts), features=True, start_reward=start))
    assert set(got) == {"action", "feature"} | ({"reward", "reward_start"} if start else set())
    _same(got, PolicyImagineSpec(weights(name)).imagine(state, clock.keys(), h, mode, seed=5, actions=acts), (name, mode))
    assert np.array_equal(got["action"], np.clip(acts, -1.0, 1.0)) and np.abs(acts).max() > 1.0
    env.close()


def test_after_a_real_run_with_resets_and_nothing_else_changes():
    """30 closed-loop agent steps on austria (random starts, terminate_on_collision, a time limit of 7 agent steps: every env is
    reset at least four times, so the keys carry episodes > 1 and the latents a non-zero deter), then imagination from the live
    latents in both modes: the spec's, keyed by the counters the last step left.  policy_state, action_in and the whole arena are
    byte for byte what they were, and a second call returns the same bytes."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n = 48
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True, terminate_on_collision=True, time_limit_steps=7)
    env.reset(mode="random", seed=5)
    env.load_policy(weights("austria"))
    clock = EpisodeClock(n)
    clock.reset()
    _drive(env, 30, clock)
    assert clock.episode.min() >= 4
    state = env.policy_state.cpu().numpy()
    assert np.abs(state[:, 30:230]).max() > 0.1
    spec_pol = PolicyImagineSpec(weights("austria"))
    before = [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes()]
    for mode in MODES:
        got = _cpu(env.policy_imagine(15, mode, seed=11, features=True, start_reward=True))
        _same(got, spec_pol.imagine(state, clock.keys(), 15, mode, seed=11), mode)
        again = _cpu(env.policy_imagine(15, mode, seed=11, features=True, start_reward=True))
        assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    torch.cuda.synchronize()
    assert before == [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes()]
    env.close()


def _drive(env, steps, clock=None):
    """`steps` closed-loop agent steps; `clock` follows the env's episode and agent-step counters."""
    import torch
    for _ in range(steps):
        env.policy_act()
        env.step(None, repeat=4)
        if clock is not None:
            torch.cuda.synchronize()
            clock.step(env.views["fresh"].reshape(-1).cpu().numpy())


def test_slot_mask_leaves_the_other_rows_alone():
    """slots=(1, 2, 3) of four cars per env: slot A's rows keep the caller's sentinel (zero without `out`), the others equal the
    spec, whose draws carry the slot."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n_envs, cars, h = 19, 4, 3
    env = BatchedRaceEnv("austria", n_envs, cars, auto_reset=True, remap_actions=True)
    env.reset(mode="grid", seed=2)
    env.load_policy(weights("austria"))
    n = env.n_cars
    clock = EpisodeClock(n_envs, cars)
    clock.reset()
    _drive(env, 3, clock)
    state = env.policy_state.cpu().numpy()
    want = PolicyImagineSpec(weights("austria")).imagine(state, clock.keys(), h, "sample", seed=14)
    others = np.flatnonzero(np.arange(n) % cars != 0)
    out = {k: torch.full(s, 7.0, device=env.device) for k, s in (("action", (n, h, 2)), ("reward", (n, h)), ("feature", (n, h, 230)), ("reward_start", (n,)))}
    got = env.policy_imagine(h, "sample", seed=14, slots=(1, 2, 3), features=True, start_reward=True, out=out)
    assert all(got[k] is out[k] for k in out)
    got = _cpu(got)
    _same(got, want, "mask", others)
    assert all(np.all(g[::cars] == 7.0) for g in got.values())
    got = _cpu(env.policy_imagine(h, "sample", seed=14, slots=(1, 2, 3)))
    _same(got, want, "mask, own tensors", others)
    assert all(np.all(g[::cars] == 0.0) for g in got.values())
    env.close()


def test_mixed_tracks_and_two_shards():
    """A MixedTrackEnv of three tracks writes its blocks' slices of one tensor per output: the spec's, keyed by global env ids.
    Envs [0, 40) on one handle, and [0, 17) and [17, 40) on two handles with first_env offsets, give the same rows in `sample`."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    env = MixedTrackEnv(["columbia", "austria", "barcelona"], [13, 20, 7], auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=4)
    env.load_policy(weights("austria"))
    assert env.policy_has_reward_head
    clock = EpisodeClock(40)
    clock.reset()
    _drive(env, 3, clock)
    state = env.policy_state.cpu().numpy()
    got = _cpu(env.policy_imagine(4, "sample", seed=21, features=True, start_reward=True))
    _same(got, PolicyImagineSpec(weights("austria")).imagine(state, clock.keys(), 4, "sample", seed=21), "mixed")
    env.close()

    def run(n, first):
        env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True, terminate_on_collision=True, time_limit_steps=4, first_env=first)
        env.reset(mode="random", seed=5)
        env.load_policy(weights("austria"))
        _drive(env, 6)
        out = _cpu(env.policy_imagine(6, "sample", seed=31, features=True, start_reward=True))
        env.close()
        return out
    full = run(40, 0)
    for lo, hi in ((0, 17), (17, 40)):
        part = run(hi - lo, lo)
        assert all(np.array_equal(part[k], full[k][lo:hi]) for k in full)


def test_refusals():
    """Every RC_ERR_INVALID of rc_policy_imagine, and the head's life: dropped by NULL, by a new rc_policy_load and by unload."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 4, 2, auto_reset=True)
    env.reset(mode="grid", seed=1)
    lib, n = env._lib, env.n_cars
    buf = {k: torch.zeros(s, device=env.device) for k, s in (("reward", (n, 15)), ("actions", (n, 15, 2)), ("features", (n, 15, 230)), ("reward_start", (n,)))}

    def call(**kw):
        a = L.RcPolicyImagineArgs(C.sizeof(L.RcPolicyImagineArgs), 15, 0, 3, 0)
        a.actions = buf["actions"].data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.rc_policy_imagine(env._h, C.byref(a))
        return rc, lib.rc_last_error()

    heads, keep = L.policy_heads(weights("austria"))
    rc, msg = call()
    assert rc == -1 and b"no policy loaded" in msg
    assert lib.rc_policy_load_heads(env._h, C.byref(heads)) == -1 and b"no policy loaded" in lib.rc_last_error()
    w = {k: weights("austria")[k] for k in weights("austria").files if not k.startswith(("img2", "img3"))}
    env.load_policy(w)
    assert env.policy_has_reward_head
    rc, msg = call()
    assert rc == -1 and b"img2 / img3" in msg
    env.policy_act()                                               # (the agent itself works without the prior's layers)
    env.load_policy(weights("austria"))
    assert call()[0] == 0
    for kw, text in ((dict(struct_size=8), b"struct_size"), (dict(horizon=0), b"horizon"), (dict(horizon=65), b"horizon"), (dict(mode=2), b"unknown mode"),
                     (dict(mode=-1), b"unknown mode"), (dict(slot_mask=0), b"mask is empty"), (dict(slot_mask=4), b"beyond cars_per_env"),
                     (dict(actions=None), b"no output")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, kw
    assert call(horizon=64, actions=None, reward_start=buf["reward_start"].data_ptr())[0] == 0
    assert call(reward=buf["reward"].data_ptr(), features=buf["features"].data_ptr())[0] == 0
    with pytest.raises(ValueError):
        env.policy_imagine(mode="deploy")
    with pytest.raises(ValueError):
        env.policy_imagine(horizon=65)
    # the head goes with NULL, with a new load of a checkpoint without one, and with unload
    assert lib.rc_policy_load_heads(env._h, None) == 0
    for field in ("reward", "reward_start"):
        rc, msg = call(**{field: buf[field].data_ptr()})
        assert rc == -1 and b"no reward head" in msg
    assert call()[0] == 0
    assert lib.rc_policy_load_heads(env._h, C.byref(heads)) == 0 and call(reward=buf["reward"].data_ptr())[0] == 0
    env.load_policy({k: weights("austria")[k] for k in weights("austria").files if not k.startswith("reward_")})
    assert not env.policy_has_reward_head and call(reward=buf["reward"].data_ptr())[0] == -1 and "reward" not in env.policy_imagine(2)
    with pytest.raises(L.RacecarHipError):
        env.policy_imagine(2, start_reward=True)
    env.load_policy(weights("austria"))
    env.unload_policy()
    assert not env.policy_has_reward_head and b"no policy loaded" in call()[1]
    env.load_policy({k: weights("austria")[k] for k in weights("austria").files if not k.startswith("reward_")})
    assert call(reward=buf["reward"].data_ptr())[0] == -1 and call()[0] == 0
    torch.cuda.synchronize()
    env.close()
