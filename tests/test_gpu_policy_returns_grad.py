"""rc_policy_returns_grad / policy_returns_grad against its binary32 specification (tests/policy_returns_grad_spec.c), bit for bit:
the two checkpoints with a reward head and the synthetic critic of tests/test_gpu_policy_returns.py, both modes, with and without the
pcont head, closed loop and under given actions, from live latents and from a given state; the forward against the device's own
policy_returns; chunks, shards and row offsets beyond 2^32; a real run under a slot mask and purity; MixedTrackEnv; output subsets;
staleness after the fits and the loaders; world_model's two learning steps against the chain of specs; the readers; the refusals."""
import ctypes as C

import numpy as np
import pytest

from policy_actor_fit_spec import PolicyActorFitSpec
from policy_fit_spec import PolicyFitSpec
from policy_observe_spec import PolicyObserveSpec
from policy_returns_grad_spec import PolicyReturnsGradSpec
from policy_sample_spec import EpisodeClock
from test_golden_policy import weights
from test_gpu_actor_fit import _same_status, _same_weights
from test_gpu_policy_device import _recorded_inputs
from test_gpu_policy_imagine import _cpu, _drive
from test_gpu_policy_returns import STARTS, WITH_HEAD, _critic, _env, _latents

pytestmark = pytest.mark.gpu
MODES = ("mean", "sample")
FORWARD = ("reward", "value", "pcont", "returns", "weight", "actions", "features")
GRADS = ("grad_actions", "actor_features", "grad_state")
NAMES = {"actions": "action", "features": "feature"}          # the device's output names -> the spec's
_cache = {}


def _spec(name, pcont=True):
    if (name, pcont) not in _cache:
        _cache[name, pcont] = PolicyReturnsGradSpec(weights(name), _critic(pcont))
    return _cache[name, pcont]


def _same(got, want, what, rows=slice(None)):
    for k, g in got.items():
        w = want[NAMES.get(k, k)]
        diff = np.flatnonzero(g[rows].reshape(-1).view(np.uint32) != w[rows].reshape(-1).view(np.uint32))
        assert g.shape == w.shape and not len(diff), (what, k, len(diff), diff[:4], float(np.abs(g[rows] - w[rows]).max()))


def _outputs(mode, pcont, closed):
    return FORWARD + STARTS[:3 if pcont else 2] + GRADS + (("eps",) if mode == "sample" and closed else ())


def _actions(s, h, seed=2):
    """[s, h, 2] raw, a third of the entries beyond +-1."""
    return np.random.default_rng(seed).uniform(-1.5, 1.5, (s, h, 2)).astype(np.float32)


# (rows, horizon, lambda_, pcont head): one row; one row past a workgroup at the shortest horizon; two workgroups and a partial one;
# the longest horizon; lambda 0 and 1 are the recursion's two ends
CASES = ((1, 15, 0.95, True), (33, 2, 0.0, True), (67, 3, 1.0, False), (3, 64, 0.95, True), (67, 3, 0.95, True))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", WITH_HEAD)
def test_one_call_is_the_spec_bit_for_bit(name, mode):
    """Recorded latents written into policy_state (closed loop), and the same latents given as `state` under a row_offset beyond
    2^32 (closed loop, and open loop under actions a third of which lie outside [-1, 1]): every output of one policy_returns_grad
    equals the spec in every row, and every forward output is byte for byte policy_returns' from the same arguments."""
    import torch
    for s, h, lam, pcont in CASES:
        state = _latents(s)
        env = _env(name, s, pcont=pcont, state=state)
        spec = _spec(name, pcont)
        clock = EpisodeClock(s)
        clock.reset()
        kw = dict(horizon=h, mode=mode, seed=77, lambda_=lam, discount=0.97)
        outputs = _outputs(mode, pcont, True)
        got = _cpu(env.policy_returns_grad(outputs=outputs, **kw))
        assert set(got) == set(outputs)
        _same(got, spec.returns_grad(state, keys=clock.keys(), **kw), (name, mode, s, h, "live"))
        own = _cpu(env.policy_returns(outputs=FORWARD + STARTS[:3 if pcont else 2], **kw))
        assert all(got[k].tobytes() == v.tobytes() for k, v in own.items()), (name, mode, s, h, "forward, live")
        assert np.all(np.abs(got["grad_actions"]).max(axis=2) > 0) and np.abs(got["grad_state"]).max() > 0
        offset = (1 << 33) + 5
        ids = offset + np.arange(s, dtype=np.uint64)
        dev = torch.from_numpy(state)
        got = _cpu(env.policy_returns_grad(state=dev, row_offset=offset, outputs=outputs, **kw))
        _same(got, spec.returns_grad(state, ids=ids, **kw), (name, mode, s, h, "given"))
        acts = _actions(s, h)
        outputs = _outputs(mode, pcont, False)
        got = _cpu(env.policy_returns_grad(state=dev, row_offset=offset, actions=torch.from_numpy(acts), outputs=outputs, **kw))
        _same(got, spec.returns_grad(state, ids=ids, actions=acts, **kw), (name, mode, s, h, "open loop"))
        outside = np.abs(acts) > 1.0
        assert outside.any() and not got["grad_actions"].view(np.uint32)[outside].any() and np.all(got["grad_actions"][~outside] != 0)
        own = _cpu(env.policy_returns(state=dev, row_offset=offset, actions=torch.from_numpy(acts), outputs=FORWARD, **kw))
        assert all(got[k].tobytes() == v.tobytes() for k, v in own.items()), (name, mode, s, h, "forward, open loop")
        env.close()


def test_chunks_shards_and_a_subset_of_the_outputs():
    """chunk_rows = 32 (three launches over 67 rows, the last partial) against one chunk; two shards of a given state with their
    row_offset against the full batch; grad_actions alone, grad_state alone, and the actor's rows alone: the bytes of the call that
    asks for everything.  With and without the pcont head."""
    import torch
    for pcont in (True, False):
        s, h = 67, 5
        env = _env("austria", 4, pcont=pcont)
        dev = torch.from_numpy(_latents(s)).to(env.device)
        outputs = _outputs("sample", pcont, True)
        kw = dict(horizon=h, mode="sample", seed=8, state=dev)
        full = _cpu(env.policy_returns_grad(outputs=outputs, **kw))
        part = _cpu(env.policy_returns_grad(outputs=outputs, chunk_rows=32, **kw))
        assert all(part[k].tobytes() == full[k].tobytes() for k in full), pcont
        for lo, hi in ((0, 7), (7, 67)):
            shard = _cpu(env.policy_returns_grad(h, "sample", seed=8, state=dev[lo:hi], row_offset=lo, scale=-1.0 / (s * (h - 1)), outputs=outputs))
            assert all(shard[k].tobytes() == full[k][lo:hi].tobytes() for k in full), (pcont, lo)
        wrong = _cpu(env.policy_returns_grad(h, "sample", seed=8, state=dev[7:], scale=-1.0 / (s * (h - 1)), outputs=("grad_actions",)))
        assert not np.array_equal(wrong["grad_actions"], full["grad_actions"][7:])
        for names in (("grad_actions",), ("grad_state",), ("grad_actions", "actor_features", "eps"), ("grad_state", "returns", "weight")):
            sub = _cpu(env.policy_returns_grad(outputs=names, **kw))
            assert set(sub) == set(names) and all(sub[k].tobytes() == full[k].tobytes() for k in names), (pcont, names)
        env.close()


def test_after_a_real_run_under_a_slot_mask_nothing_else_changes():
    """30 closed-loop agent steps with resets on a 2-car env, then policy_returns_grad from the live latents of slot 1 in both modes:
    the spec's rows, keyed by the counters the last step left; the rows of slot 0 keep the caller's sentinel.  policy_state,
    action_in, the whole arena and every weight image are byte for byte what they were, and the next policy_act equals that of a twin
    env that never made the call."""
    import torch
    n = 24
    kw = dict(terminate_on_collision=True, time_limit_steps=7)
    env, twin = _env("austria", n, cars=2, **kw), _env("austria", n, cars=2, **kw)
    for e in (env, twin):
        e.reset(mode="random", seed=5)
    clock = EpisodeClock(n, 2)
    clock.reset()
    clock.reset()                        # (_env's reset, and the one above)
    _drive(env, 30, clock)
    _drive(twin, 30)
    torch.cuda.synchronize()
    state = env.policy_state.cpu().numpy()
    assert clock.episode.min() >= 3 and np.abs(state[:, 30:230]).max() > 0.1

    def held():
        torch.cuda.synchronize()
        images = {**env.critic_weights(), **env.actor_weights(), **env.reward_head_weights()}
        return [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes(),
                {k: v.tobytes() for k, v in images.items()}]

    before = held()
    for mode in MODES:
        outputs = _outputs(mode, True, True)
        want = _spec("austria").returns_grad(state, keys=clock.keys(), horizon=6, mode=mode, seed=11, scale=-1.0 / (n * 5))
        out = {k: torch.full(want[NAMES.get(k, k)].shape, 7.0, device=env.device) for k in outputs}
        got = env.policy_returns_grad(6, mode, seed=11, slots=(1,), outputs=outputs, out=out)
        assert all(got[k] is out[k] for k in out)
        got = _cpu(got)
        _same(got, want, mode, np.arange(1, 2 * n, 2))
        assert all(np.all(g[::2] == 7.0) for g in got.values())
    assert before == held()
    a, b = env.policy_act().cpu().numpy(), twin.policy_act().cpu().numpy()
    assert a.tobytes() == b.tobytes() and env.policy_state.cpu().numpy().tobytes() == twin.policy_state.cpu().numpy().tobytes()
    env.close()
    twin.close()


def test_mixed_tracks():
    """A MixedTrackEnv writes its blocks' rows of one tensor per output, from live latents and - through its first block - from a
    given state; the default scale counts the rows of all blocks."""
    import torch
    from racing_dreamer_amd.batched_env import MixedTrackEnv
    h = 4
    mixed = MixedTrackEnv(["columbia", "austria", "barcelona"], [13, 20, 7], auto_reset=True, remap_actions=True)
    mixed.reset(mode="random", seed=4)
    mixed.load_policy(weights("austria"))
    mixed.load_critic(_critic())
    clock = EpisodeClock(40)
    clock.reset()
    _drive(mixed, 3, clock)
    torch.cuda.synchronize()
    st = mixed.policy_state.cpu().numpy()
    outputs = _outputs("sample", True, True)
    got = _cpu(mixed.policy_returns_grad(h, "sample", seed=21, outputs=outputs))
    _same(got, _spec("austria").returns_grad(st, keys=clock.keys(), horizon=h, mode="sample", seed=21), "mixed")
    given = _cpu(mixed.policy_returns_grad(h, "sample", seed=21, state=torch.from_numpy(st), outputs=outputs, chunk_rows=32))
    _same(given, _spec("austria").returns_grad(st, horizon=h, mode="sample", seed=21), "mixed, given state")
    mixed.close()


def test_the_images_follow_the_fits_and_the_loaders():
    """After critic_fit (value, pcont), reward_fit, load_critic and load_reward_head the next call equals that of a fresh env loaded
    with the moved weights: the transposed images are remade in stream order."""
    import torch
    s, h = 33, 4
    state = _latents(s)
    dev = torch.from_numpy(state)
    kw = dict(horizon=h, mode="sample", seed=3, state=dev, outputs=("grad_actions", "grad_state", "returns"))
    env = _env("austria", 4)
    first = _cpu(env.policy_returns_grad(**kw))                       # (the images exist from here on)
    rng = np.random.default_rng(1)
    feat = torch.from_numpy(state[:, :230].copy())
    target = torch.from_numpy(rng.normal(0, 1, s).astype(np.float32))
    soft = torch.from_numpy(rng.uniform(0, 1, s).astype(np.float32))

    def fresh():
        other = _env("austria", 4)
        other.load_reward_head(env.reward_head_weights())
        other.load_critic(env.critic_weights())
        res = _cpu(other.policy_returns_grad(**kw))
        other.close()
        return res

    last = first
    steps = (("critic_fit value", lambda: (env.critic_fit_begin("value"), env.critic_fit(feat, target, head="value", lr=1e-2))),
             ("critic_fit pcont", lambda: (env.critic_fit_begin("pcont"), env.critic_fit(feat, soft, head="pcont", lr=1e-2))),
             ("reward_fit", lambda: (env.reward_fit_begin(), env.reward_fit(feat, target, lr=1e-2))),
             ("load_critic", lambda: env.load_critic(_critic_of(9))),
             ("load_reward_head", lambda: env.load_reward_head({k: (v * np.float32(0.5)) for k, v in env.reward_head_weights().items()})))
    for what, move in steps:
        move()
        got = _cpu(env.policy_returns_grad(**kw))
        assert got["grad_actions"].tobytes() != last["grad_actions"].tobytes(), what
        want = fresh()
        assert all(got[k].tobytes() == want[k].tobytes() for k in want), what
        last = got
    env.close()


def _critic_of(seed):
    from racing_dreamer_amd.critic import init_critic
    return init_critic(seed)


def test_the_learning_steps_are_the_chain_of_specs_and_the_agent_reads_the_fitted_actor():
    """world_model.actor_learning_step and behaviour_learning_step on a batch shaped as TrajectoryRing.sample returns it (B = 3,
    T = 5, H = 4): the posterior features of PolicyObserveSpec in `sample` without each window's last step, the starts of
    PolicyReturnsGradSpec, whose rows go through PolicyActorFitSpec in grad mode (the ten actor arrays, loss, norm and step) and,
    for the pair, through PolicyFitSpec on the value head.  Afterwards policy_action and policy_act read the fitted actor."""
    import torch
    from racing_dreamer_amd.world_model import actor_learning_step, behaviour_learning_step
    b, t, h = 3, 5, 4
    scan = _recorded_inputs(b * t, seed=3)[0].reshape(b, t, 1080)
    rec = np.random.default_rng(4).uniform(-1, 1, (b, t, 2)).astype(np.float32)
    batch = dict(lidar=torch.from_numpy(scan), action=torch.from_numpy(rec))
    w = weights("austria")
    feat = PolicyObserveSpec(w).observe(scan, rec, mode="sample", seed=13)["feature"][:, :-1].reshape(-1, 230)
    dream = _spec("austria").returns_grad(feat, horizon=h, mode="sample", seed=13, lambda_=0.95, discount=0.99)
    assert dream["scale"] == np.float32(-1.0 / (b * (t - 1) * (h - 1)))
    loss = -(dream["weight"].astype(np.float64) * dream["returns"].astype(np.float64)).mean()

    def actor_spec():
        spec = PolicyActorFitSpec(w)
        return spec, spec.step(dream["actor_features"].reshape(-1, 230), grad_actions=dream["grad_actions"].reshape(-1, 2),
                               eps=dream["eps"].reshape(-1, 2), clip=100.0)

    env = _env("austria", 4)
    env.actor_fit_begin()
    got = actor_learning_step(env, batch, horizon=h, seed=13, clip=100.0)
    spec, want = actor_spec()
    status = {k: v.item() for k, v in _cpu(got).items()}
    _same_status(status, want, "actor_learning_step")
    assert want["step"] == 1 and want["grad_norm"] > 0 and abs(status["actor_loss"] - loss) <= 1e-6 * abs(loss)
    _same_weights(env, spec, "actor_learning_step")
    # the readers: the actor on given features, and the agent's own step in mode mean
    probe = _latents(5)[:, :230]
    act = _cpu(env.policy_action(torch.from_numpy(probe)))["action"]
    assert act.tobytes() == spec.forward(probe)["action"].tobytes()
    env.policy_act()
    torch.cuda.synchronize()
    st = env.policy_state.cpu().numpy()
    assert st[:, 230:].tobytes() == spec.forward(st[:, :230])["action"].tobytes()
    env.close()

    env = _env("austria", 4)
    env.actor_fit_begin()
    env.critic_fit_begin("value")
    got = behaviour_learning_step(env, batch, horizon=h, seed=13, actor_fit=dict(clip=100.0), value_fit=dict(clip=100.0))
    spec, want = actor_spec()
    vspec = PolicyFitSpec(_critic(), "value")
    vwant = vspec.step(dream["feature"][:, :-1].reshape(-1, 230), dream["returns"].reshape(-1), dream["weight"].reshape(-1), clip=100.0)
    _same_status({k: v.item() for k, v in _cpu(got["actor"]).items()}, want, "behaviour_learning_step, actor")
    _same_status({k: v.item() for k, v in _cpu(got["value"]).items()}, vwant, "behaviour_learning_step, value")
    _same_weights(env, spec, "behaviour_learning_step")
    critic = env.critic_weights()
    assert all(critic[k].tobytes() == a.tobytes() for k, a in vspec.weights().items())
    assert abs(float(got["actor_loss"]) - loss) <= 1e-6 * abs(loss) and float(got["value_loss"]) == float(got["value"]["loss"])
    env.close()


def test_refusals():
    """Every RC_ERR_INVALID of rc_policy_returns_grad names its cause; nothing is launched."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 4, 2, auto_reset=True)
    env.reset(mode="grid", seed=1)
    lib, n, h = env._lib, env.n_cars, 15
    buf = {k: torch.zeros((n, 64 * 230), device=env.device) for k in ("a", "b", "state")}
    ptr = {k: v.data_ptr() for k, v in buf.items()}

    def call(**kw):
        a = L.RcPolicyReturnsGradArgs(C.sizeof(L.RcPolicyReturnsGradArgs), h, 1, 3, 0.95, 0.99, -0.01)
        a.grad_actions = ptr["a"]
        for key, v in kw.items():
            setattr(a, key, v)
        rc = lib.rc_policy_returns_grad(env._h, C.byref(a))
        return rc, lib.rc_last_error()

    rc, msg = call()
    assert rc == -1 and b"no policy loaded" in msg
    env.load_policy(weights("treitlstrasse_20210220"))
    rc, msg = call()
    assert rc == -1 and b"no reward head" in msg
    env.load_policy(weights("austria"))
    rc, msg = call()
    assert rc == -1 and b"no value head" in msg
    env.load_critic(_critic(pcont=False))
    rc, msg = call(pcont_start=ptr["b"])
    assert rc == -1 and b"no pcont head" in msg
    assert call()[0] == 0
    env.load_critic(_critic())
    assert call()[0] == 0 and call(eps=ptr["b"], grad_state=ptr["state"])[0] == 0
    for kw, text in ((dict(struct_size=8), b"struct_size"), (dict(horizon=1), b"horizon"), (dict(horizon=0), b"horizon"), (dict(horizon=65), b"horizon"),
                     (dict(mode=2), b"unknown mode"), (dict(lambda_=1.5), b"lambda_"), (dict(lambda_=float("nan")), b"lambda_"),
                     (dict(discount=-0.5), b"discount"), (dict(scale=float("inf")), b"scale"), (dict(scale=float("nan")), b"scale"),
                     (dict(chunk_rows=-1), b"chunk_rows"),
                     (dict(grad_actions=None), b"no gradient output"), (dict(grad_actions=None, actor_features=ptr["a"], returns=ptr["b"]), b"no gradient output"),
                     (dict(mode=0, eps=ptr["b"]), b"eps"), (dict(eps=ptr["b"], actions_in=ptr["state"]), b"eps"),
                     (dict(state_in=ptr["state"], starts=n), b"slot mask"), (dict(state_in=ptr["state"], slot_mask=0, starts=0), b"starts"),
                     (dict(state_in=ptr["state"], slot_mask=0, starts=1 << 40), b"starts"), (dict(starts=n), b"state_in is NULL"),
                     (dict(slot_mask=0), b"mask is empty"), (dict(slot_mask=4), b"beyond cars_per_env")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    assert call(horizon=64, lambda_=0.0, discount=0.0, slot_mask=2, mode=0)[0] == 0
    assert call(state_in=ptr["state"], slot_mask=0, starts=n, horizon=2, grad_actions=None, grad_state=ptr["a"])[0] == 0
    for bad in (dict(mode="deploy"), dict(lambda_=1.01), dict(outputs=("return",)), dict(horizon=1), dict(horizon=65), dict(chunk_rows=-1),
                dict(state=buf["state"][:, :230])):
        with pytest.raises(ValueError):
            env.policy_returns_grad(**bad)
    with pytest.raises(L.RacecarHipError, match="eps"):
        env.policy_returns_grad(mode="mean")
    with pytest.raises(L.RacecarHipError, match="no gradient output"):
        env.policy_returns_grad(outputs=("actor_features", "eps"))
    env.unload_policy()
    assert b"no policy loaded" in call()[1]
    torch.cuda.synchronize()
    env.close()
