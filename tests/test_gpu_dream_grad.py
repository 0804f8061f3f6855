"""rc_policy_dream_grad / dream_ahead_grad against its binary32 specification (tests/policy_dream_grad_spec.c), bit for bit on all
four outputs: the two checkpoints with a reward head, both modes, the row mappings of dream_ahead's test and the longest stash;
`return` and `reward` against the device's own dream_ahead; chunks; a given state, shards and row offsets beyond 2^32; the choice of
outputs; purity after a real run; slot masks and mixed tracks; the refusals; dream_gradient_act on a live env."""
import ctypes as C

import numpy as np
import pytest

from policy_dream_grad_spec import PolicyDreamGradSpec
from test_golden_policy import weights
from test_gpu_dream_ahead import _actions, _latents
from test_gpu_policy_device import _recorded_inputs
from test_gpu_policy_imagine import _cpu, _drive

pytestmark = pytest.mark.gpu
MODES = ("mean", "sample")
WITH_HEAD = ("austria", "treitlstrasse")
ALL = ("grad_actions", "grad_state", "return", "reward")
_cache = {}


def _spec(name):
    if name not in _cache:
        _cache[name] = PolicyDreamGradSpec(weights(name))
    return _cache[name]


def _same(got, want, what, rows=slice(None)):
    for k, g in got.items():
        assert g[rows].tobytes() == want[k][rows].tobytes(), (what, k, float(np.abs(g[rows] - want[k][rows]).max()))


def _env(n, cars=1, name="austria", **kw):
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", n, cars, auto_reset=True, remap_actions=True, **kw)
    env.reset(mode="random", seed=1)
    env.load_policy(weights(name))
    return env


# (starts, candidates, horizon, discount): one start's rows straddling two workgroups; three starts in one workgroup; H = 1; exactly
# three full workgroups; the longest stash
CASES = ((1, 33, 15, 0.99), (3, 5, 2, 1.0), (33, 1, 1, 0.99), (3, 32, 2, 0.99), (1, 2, 64, 0.99))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", WITH_HEAD)
def test_one_call_is_the_spec_bit_for_bit(name, mode):
    """Recorded latents written into policy_state, one dream_ahead_grad from them: grad_actions, grad_state, return and reward equal
    the spec in every row, a third of the actions beyond +-1 (their gradient +0 by bit pattern)."""
    import torch
    envs = {}
    for s, k, h, discount in CASES:
        state = _latents(s)
        if s not in envs:
            envs[s] = _env(s, name=name)
            envs[s].policy_state.copy_(torch.from_numpy(state))
        acts = _actions(s, k, h, seed=s + k + h)
        got = _cpu(envs[s].dream_ahead_grad(torch.from_numpy(acts), mode, seed=77, discount=discount, outputs=ALL))
        want = _spec(name).dream_grad(state, acts, None, mode, seed=77, discount=discount)
        assert set(got) == set(ALL)
        _same(got, want, (name, mode, s, k, h))
        outside = np.abs(acts) > 1.0
        assert outside.any() and not got["grad_actions"].view(np.uint32)[outside].any()
        assert np.all(got["grad_actions"][~outside] != 0.0) and np.abs(got["grad_state"]).max() > 1e-3
    for env in envs.values():
        env.close()


@pytest.mark.parametrize("mode", MODES)
def test_return_and_reward_are_dream_aheads_own(mode):
    """From the same latents, seed, mode and discount: byte for byte what dream_ahead returns."""
    import torch
    n, k, h = 35, 3, 15
    env = _env(n)
    env.policy_state.copy_(torch.from_numpy(_latents(n)))
    acts = torch.from_numpy(_actions(n, k, h, seed=9)).to(env.device)
    got = _cpu(env.dream_ahead_grad(acts, mode, seed=5, discount=0.99, outputs=("return", "reward", "grad_actions")))
    own = _cpu(env.dream_ahead(acts, mode, seed=5, discount=0.99, outputs=("return", "reward")))
    assert got["return"].tobytes() == own["return"].tobytes() and got["reward"].tobytes() == own["reward"].tobytes()
    assert np.abs(own["return"]).max() > 1e-3
    env.close()


def test_chunks_do_not_change_the_results():
    """3 x 32 rows in `sample`: one launch per 32 rows (chunk_rows=32; 20 is rounded up to it) and one launch for all give the same
    bytes - also right after each other on the one stash."""
    import torch
    s, k, h = 3, 32, 4
    env = _env(s)
    env.policy_state.copy_(torch.from_numpy(_latents(s)))
    acts = torch.from_numpy(_actions(s, k, h, seed=21)).to(env.device)
    whole = _cpu(env.dream_ahead_grad(acts, "sample", seed=4, discount=0.99, outputs=ALL, chunk_rows=0))
    for chunk in (32, 20, 64, 1 << 40, (1 << 63) - 1):
        part = _cpu(env.dream_ahead_grad(acts, "sample", seed=4, discount=0.99, outputs=ALL, chunk_rows=chunk))
        _same(part, whole, chunk)
    _same(whole, _spec("austria").dream_grad(_latents(s), acts.cpu().numpy(), None, "sample", seed=4, discount=0.99), "spec")
    with pytest.raises(ValueError):
        env.dream_ahead_grad(acts, chunk_rows=-1)
    env.close()


def test_from_an_observed_window_and_in_shards():
    """policy_observe's `state` as the starts, keyed by row_offset + row beyond 2^32: the spec's answer.  Two shards with their
    row_offset reproduce the whole batch in `sample`.  The env's own cars do not enter: it has two."""
    import torch
    rows, t_len, k, h = 7, 3, 5, 3
    scan = _recorded_inputs(rows * t_len, seed=3)[0].reshape(rows, t_len, 1080)
    rec = np.random.default_rng(4).uniform(-1, 1, (rows, t_len, 2)).astype(np.float32)
    env = _env(2)
    state = env.policy_observe(torch.from_numpy(scan), torch.from_numpy(rec), outputs=("state",))["state"]
    host = _cpu({"s": state})["s"]
    acts = _actions(rows, k, h, seed=6)
    dev_acts = torch.from_numpy(acts).to(env.device)
    offset = (1 << 33) + 11
    for mode in MODES:
        got = _cpu(env.dream_ahead_grad(dev_acts, mode, seed=8, state=state, row_offset=offset, discount=0.99, outputs=ALL))
        want = _spec("austria").dream_grad(host, acts, offset + np.arange(rows, dtype=np.uint64), mode, seed=8, discount=0.99)
        _same(got, want, mode)
    full = _cpu(env.dream_ahead_grad(dev_acts, "sample", seed=8, state=state, row_offset=offset, outputs=ALL))
    for lo, hi in ((0, 2), (2, rows)):
        part = _cpu(env.dream_ahead_grad(dev_acts[lo:hi], "sample", seed=8, state=state[lo:hi], row_offset=offset + lo, outputs=ALL))
        assert all(part[key].tobytes() == full[key][lo:hi].tobytes() for key in full)
    wrong = _cpu(env.dream_ahead_grad(dev_acts[2:], "sample", seed=8, state=state[2:], row_offset=offset, outputs=("grad_actions",)))
    assert not np.array_equal(wrong["grad_actions"], full["grad_actions"][2:])
    env.close()


def test_each_output_alone_is_what_all_together_give():
    import torch
    s, k, h = 5, 9, 3
    env = _env(s)
    env.policy_state.copy_(torch.from_numpy(_latents(s)))
    acts = torch.from_numpy(_actions(s, k, h, seed=13)).to(env.device)
    for mode in MODES:
        whole = _cpu(env.dream_ahead_grad(acts, mode, seed=2, discount=0.99, outputs=ALL))
        for name in ALL:
            alone = _cpu(env.dream_ahead_grad(acts, mode, seed=2, discount=0.99, outputs=(name,)))
            assert set(alone) == {name} and alone[name].tobytes() == whole[name].tobytes(), (mode, name)
    assert set(env.dream_ahead_grad(acts)) == {"grad_actions", "return"}
    env.close()


def test_after_a_real_run_nothing_else_changes():
    """30 closed-loop agent steps with resets, then the gradient from the live latents in both modes: the spec's.  policy_state,
    action_in, the whole arena and the episode counters are byte for byte what they were; a second call returns the same bytes."""
    import torch
    n, k, h = 48, 3, 4
    env = _env(n, terminate_on_collision=True, time_limit_steps=7)
    env.enable_episode_log(4096)
    _drive(env, 30)
    torch.cuda.synchronize()
    state = env.policy_state.cpu().numpy()
    assert np.abs(state[:, 30:230]).max() > 0.1
    acts = _actions(n, k, h, seed=3)
    dev_acts = torch.from_numpy(acts).to(env.device)

    def snapshot():
        torch.cuda.synchronize()
        return [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes(),
                sorted(env.episode_counters.items())]
    before = snapshot()
    assert dict(before[3])["written"] > 0 and dict(before[3])["calls"] > 0
    for mode in MODES:
        got = _cpu(env.dream_ahead_grad(dev_acts, mode, seed=11, discount=0.99, outputs=ALL))
        _same(got, _spec("austria").dream_grad(state, acts, None, mode, seed=11, discount=0.99), mode)
        again = _cpu(env.dream_ahead_grad(dev_acts, mode, seed=11, discount=0.99, outputs=ALL))
        assert all(got[key].tobytes() == again[key].tobytes() for key in got)
    torch.cuda.synchronize()
    assert before == snapshot()
    env.close()


def test_slot_mask_and_mixed_tracks():
    """slots=(1, 2, 3) of four cars per env: slot 0's rows keep the caller's sentinel, the others equal the spec, whose draws carry
    the global car id.  A MixedTrackEnv's blocks write their slices of one tensor per output: the rows of single-env calls from the
    same latents, and a given state goes through its first block."""
    import torch
    from racing_dreamer_amd.batched_env import MixedTrackEnv
    n_envs, cars, k, h = 19, 4, 3, 2
    env = _env(n_envs, cars)
    n = env.n_cars
    _drive(env, 3)
    torch.cuda.synchronize()
    state = env.policy_state.cpu().numpy()
    acts = _actions(n, k, h, seed=5)
    dev_acts = torch.from_numpy(acts).to(env.device)
    want = _spec("austria").dream_grad(state, acts, None, "sample", seed=14)
    others = np.flatnonzero(np.arange(n) % cars != 0)
    shapes = {"grad_actions": (n, k, h, 2), "grad_state": (n, k, 230), "return": (n, k), "reward": (n, k, h)}
    out = {key: torch.full(shape, 7.0, device=env.device) for key, shape in shapes.items()}
    got = env.dream_ahead_grad(dev_acts, "sample", seed=14, slots=(1, 2, 3), outputs=ALL, out=out)
    assert all(got[key] is out[key] for key in out)
    got = _cpu(got)
    _same(got, want, "mask", others)
    assert all(np.all(g[::cars] == 7.0) for g in got.values())
    env.close()

    mixed = MixedTrackEnv(["columbia", "austria", "barcelona"], [13, 20, 7], auto_reset=True, remap_actions=True)
    mixed.reset(mode="random", seed=4)
    mixed.load_policy(weights("austria"))
    _drive(mixed, 3)
    torch.cuda.synchronize()
    state = mixed.policy_state.cpu().numpy()
    acts = _actions(40, 5, 3, seed=7)
    got = _cpu(mixed.dream_ahead_grad(torch.from_numpy(acts), "sample", seed=21, discount=0.99, outputs=ALL))
    _same(got, _spec("austria").dream_grad(state, acts, None, "sample", seed=21, discount=0.99), "mixed")
    given = _cpu(mixed.dream_ahead_grad(torch.from_numpy(acts), "sample", seed=21, state=torch.from_numpy(state), discount=0.99, outputs=ALL))
    _same(given, got, "mixed, given state")
    single = _env(40)
    single.policy_state.copy_(torch.from_numpy(state))
    own = _cpu(single.dream_ahead_grad(torch.from_numpy(acts), "sample", seed=21, discount=0.99, outputs=ALL))
    _same(own, got, "the blocks' rows against a single env's")
    single.close()
    mixed.close()


def test_refusals():
    """Every RC_ERR_INVALID of rc_policy_dream_grad; each raises (or returns -1) and leaves the outputs untouched."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 4, 2, auto_reset=True)
    env.reset(mode="grid", seed=1)
    lib, n, k, h = env._lib, env.n_cars, 3, 15
    buf = {key: torch.full(shape, 7.0, device=env.device) for key, shape in (("grad_actions", (n, k, 64, 2)), ("grad_state", (n, k, 230)), ("ret", (n, k)),
                                                                             ("reward", (n, k, 64)))}
    acts_in, state_in = torch.zeros((n, k, 64, 2), device=env.device), torch.zeros((n, 232), device=env.device)

    def call(**kw):
        a = L.RcPolicyDreamGradArgs(C.sizeof(L.RcPolicyDreamGradArgs), h, 0, k, 3, 1.0, 0, 0, 0, 0)
        a.actions_in = acts_in.data_ptr()
        for key, t in buf.items():
            setattr(a, key, t.data_ptr())
        for key, v in kw.items():
            setattr(a, key, v)
        rc = lib.rc_policy_dream_grad(env._h, C.byref(a))
        return rc, lib.rc_last_error()

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == 7.0).all()) for t in buf.values())

    rc, msg = call()
    assert rc == -1 and b"no policy loaded" in msg
    w = {key: weights("austria")[key] for key in weights("austria").files if not key.startswith(("img2", "img3"))}
    env.load_policy(w)
    rc, msg = call()
    assert rc == -1 and b"img2 / img3" in msg
    env.load_policy(weights("treitlstrasse_20210220"))
    assert not env.policy_has_reward_head
    for kw in ({}, dict(ret=None, reward=None), dict(grad_actions=None, grad_state=None)):
        rc, msg = call(**kw)
        assert rc == -1 and b"no reward head" in msg
    with pytest.raises(L.RacecarHipError, match="no reward head"):
        env.dream_ahead_grad(acts_in[:, :, :h])
    env.load_policy(weights("austria"))
    state = state_in.data_ptr()
    for kw, text in ((dict(struct_size=8), b"struct_size"), (dict(horizon=0), b"horizon"), (dict(horizon=65), b"horizon"), (dict(candidates=0), b"candidates"),
                     (dict(candidates=1 << 30), b"not below 2^31"), (dict(mode=2), b"unknown mode"), (dict(discount=1.5), b"discount"),
                     (dict(discount=float("nan")), b"discount"), (dict(chunk_rows=-32), b"chunk_rows"), (dict(actions_in=None), b"actions_in is NULL"),
                     (dict(grad_actions=None, grad_state=None, ret=None, reward=None), b"no output"),
                     (dict(state_in=state, starts=n), b"slot mask"), (dict(state_in=state, slot_mask=0, starts=0), b"starts"),
                     (dict(state_in=state, slot_mask=0, starts=1 << 40), b"not below 2^31"),
                     (dict(slot_mask=0), b"mask is empty"), (dict(slot_mask=4), b"beyond cars_per_env")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    assert untouched()
    acts = torch.zeros((n, k, h, 2), device=env.device)
    for bad in (dict(mode="deploy"), dict(discount=1.01), dict(outputs=("final_feature",)), dict(state=state_in[:2]), dict(state=state_in[:, :230]),
                dict(out={"return": torch.zeros((n, k), dtype=torch.float64, device=env.device)}),
                dict(out={"grad_actions": torch.zeros((n, k, h), device=env.device)})):
        with pytest.raises(ValueError):
            env.dream_ahead_grad(acts, **bad)
    with pytest.raises(ValueError):
        env.dream_ahead_grad(torch.zeros(n, k, 65, 2))
    with pytest.raises(ValueError):
        env.dream_ahead_grad(torch.zeros(n, k, 0, 2))
    with pytest.raises(L.RacecarHipError, match="slot mask"):
        env.dream_ahead_grad(acts, state=state_in, slots=(0,))
    assert untouched()
    assert call(horizon=64, discount=0.0, slot_mask=2)[0] == 0 and not untouched()
    # new weights drop the transposed images and the stash; the next call makes them again
    env.load_policy(weights("treitlstrasse"))
    assert call()[0] == 0
    env.unload_policy()
    assert b"no policy loaded" in call()[1]
    torch.cuda.synchronize()
    env.close()


def test_new_weights_rebuild_the_transposed_images():
    """austria, then treitlstrasse on the same handle: each call equals its checkpoint's spec."""
    import torch
    s, k, h = 3, 5, 2
    state, acts = _latents(s), _actions(s, k, h, seed=12)
    env = _env(s)
    for name in ("austria", "treitlstrasse", "austria"):
        env.load_policy(weights(name))
        env.policy_state.copy_(torch.from_numpy(state))
        got = _cpu(env.dream_ahead_grad(torch.from_numpy(acts), "mean", discount=0.99, outputs=ALL))
        _same(got, _spec(name).dream_grad(state, acts, None, "mean", discount=0.99), name)
    env.close()


def test_dream_gradient_act_on_a_live_env():
    """austria, 64 envs, after a few policy_act steps: for every car the planner's imagined return is at least dream_shooting_act's
    on the same candidates, seed and discount, and strictly greater for at least half the cars; action_in holds the chosen first
    actions."""
    import torch
    from racing_dreamer_amd.planning import dream_gradient_act, dream_shooting_act, shooting_candidates
    n, k, h, discount = 64, 8, 15, 0.99
    env = _env(n)
    _drive(env, 4)
    env.policy_act()
    cand = shooting_candidates(env, k, h, hold=5, seed=9)
    before = env.views["action_in"].clone()
    dream_shooting_act(env, candidates=k, horizon=h, hold=5, seed=9, discount=discount)
    shot_first = env.views["action_in"].reshape(n, 2).clone()
    acts = cand.reshape(n, k, h, 2)
    ret = env.dream_ahead(acts, discount=discount)["return"]
    picked = (acts[:, :, 0] == shot_first[:, None]).all(dim=2).float().argmax(dim=1)
    shot_ret = ret[torch.arange(n, device=ret.device), picked]
    env.views["action_in"].copy_(before)                        # the same candidates: candidate 0 repeats action_in
    info = {}
    out = dream_gradient_act(env, candidates=k, horizon=h, iterations=10, step=0.2, hold=5, seed=9, discount=discount, info=info)
    assert out is env.views["action_in"]
    torch.cuda.synchronize()
    assert torch.equal(info["initial_return"], ret)
    gain = (info["return"] - shot_ret).cpu().numpy()
    print(f"dream_gradient_act: gain over shooting-{k} min {gain.min():.4f} mean {gain.mean():.4f} max {gain.max():.4f}, "
          f"strictly greater for {(gain > 0).sum()} of {n} cars")
    assert np.all(gain >= 0.0)
    assert (gain > 0).sum() >= n // 2
    again = env.dream_ahead(info["actions"][:, None].contiguous(), discount=discount)["return"][:, 0]
    assert torch.equal(again, info["return"])
    assert torch.equal(out.reshape(n, 2), info["actions"][:, 0])
    env.close()
