"""rc_policy_actor_fit_step / actor_fit and rc_policy_actor_forward / policy_action against their binary32 specification
(tests/policy_actor_fit_spec.c), bit for bit: both loss modes, with and without eps and weights, row counts that reach every path of
the kernels; consecutive steps; the forward against policy_act's own action; that every reader of the actor - the sampled modes'
pair image among them - sees the fitted weights; purity; neutral and edge rows; MixedTrackEnv; the round trip through actor_weights
and load_actor; planning.distil_step; the refusals.  The env is austria with 4 envs, the actor the checkpoint's own; the rows are
recorded latents, not the env's."""
import numpy as np
import pytest

from policy_actor_fit_spec import KEYS, PolicyActorFitSpec
from test_golden_policy import weights
from test_gpu_policy_imagine import _cpu
from test_policy_actor_fit_spec import _actor, _inputs, _rows
from test_policy_fit_spec import _critic

pytestmark = pytest.mark.gpu


def _env(n=4, checkpoint=None, critic=False):
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=1)
    env.load_policy(weights("austria") if checkpoint is None else checkpoint)
    if critic:
        env.load_critic(_critic())
    return env


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _fit(env, feat, grad_features=False, **kw):
    """actor_fit on NumPy inputs (the keyword arguments of PolicyActorFitSpec.step): the status as Python numbers, grad_features."""
    got = _cpu(env.actor_fit(_t(feat), grad_features=grad_features, **{k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}))
    out = {k: got[k].item() for k in ("loss", "grad_norm", "skipped", "step")}
    if grad_features:
        out["grad_features"] = got["grad_features"]
    return out


def _same_status(got, want, what):
    assert np.float32(got["loss"]).tobytes() == np.float32(want["loss"]).tobytes(), (what, got["loss"], want["loss"])
    assert np.float32(got["grad_norm"]).tobytes() == np.float32(want["grad_norm"]).tobytes(), (what, got["grad_norm"], want["grad_norm"])
    assert (got["skipped"], got["step"]) == (want["skipped"], want["step"]), (what, got, want["skipped"], want["step"])


def _same_weights(env, spec, what):
    got = env.actor_weights()
    assert tuple(got) == KEYS
    for k, a in spec.weights().items():
        diff = np.flatnonzero(got[k].reshape(-1) != a.reshape(-1))
        assert got[k].shape == a.shape and got[k].tobytes() == a.tobytes(), (what, k, len(diff), diff[:4])


def _bytes(d):
    return {k: v.tobytes() for k, v in d.items()}


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("with_eps", [True, False])
@pytest.mark.parametrize("mode", ["target", "grad"])
def test_one_step_is_the_spec_bit_for_bit(mode, with_eps, weighted):
    """One step from the checkpoint's actor: all ten arrays, loss, grad_norm, step and grad_features equal the spec for N = 1 and 2
    (a single row, one row pair), 33 (one row past a workgroup), 97 (three workgroups and a partial one, the four chains of unequal
    length) and 263 (every chain several pairs long).  (At most a quarter of these rows are saturated:
    tests/test_policy_actor_fit_spec.py.)"""
    env = _env()
    for n in (1, 2, 33, 97, 263):
        feat, kw = _inputs(mode, with_eps, n, weighted)
        env.load_actor(_actor())
        env.actor_fit_begin()
        spec = PolicyActorFitSpec(_actor())
        want = spec.step(feat, **kw)
        got = _fit(env, feat, grad_features=True, **kw)
        print(mode, with_eps, weighted, n, {k: got[k] for k in ("loss", "grad_norm", "step")})
        _same_status(got, want, (mode, with_eps, weighted, n))
        diff = np.flatnonzero(got["grad_features"].reshape(-1) != want["grad_features"].reshape(-1))
        assert got["grad_features"].shape == (n, 230) and got["grad_features"].tobytes() == want["grad_features"].tobytes(), (n, len(diff), diff[:4])
        _same_weights(env, spec, (mode, with_eps, weighted, n))
        assert want["step"] == 1 and want["grad_norm"] > 0
    env.close()


def test_three_steps_are_the_specs_three_steps():
    """The carried moments and the bias correction: three consecutive steps at N = 97, status and weights after each; the second
    without grad_features (the kernel's other path), in grad mode."""
    env = _env()
    env.actor_fit_begin()
    spec = PolicyActorFitSpec(_actor())
    feat, kw = _inputs("target", True, 97)
    _, kg = _inputs("grad", True, 97)
    for i, k in enumerate((kw, kg, kw)):
        want = spec.step(feat, **k)
        _same_status(_fit(env, feat, grad_features=i != 1, **k), want, i)
        _same_weights(env, spec, i)
    assert spec.step_count == 3
    env.close()


def test_policy_action_is_the_agents_action():
    """After policy_act in mode mean, policy_action(policy_state[:, :230]) equals policy_state[:, 230:232] - the action the agent
    wrote - byte for byte; with eps, and for mean and std, it equals the spec."""
    env = _env(8)
    for _ in range(3):
        env.policy_act()
        env.step(None, repeat=4)
    env.policy_act()
    state = env.policy_state.clone()
    got = _cpu(env.policy_action(state[:, :230], outputs=("action", "mean", "std")))
    state = state.cpu().numpy()
    assert got["action"].tobytes() == np.ascontiguousarray(state[:, 230:232]).tobytes()
    assert got["action"].tobytes() == env.views["action_in"].reshape(-1, 2).cpu().numpy().tobytes()
    spec = PolicyActorFitSpec(_actor())
    r = _rows(263)
    assert _bytes(spec.forward(state[:, :230])) == _bytes(got)
    for n in (1, 33, 263):
        want = spec.forward(r["feat"][:n], r["eps"][:n])
        drawn = _cpu(env.policy_action(_t(r["feat"][:n]), eps=_t(r["eps"][:n]), outputs=("action", "mean", "std")))
        assert _bytes(drawn) == _bytes(want), n
    lead = _cpu(env.policy_action(_t(r["feat"][:6].reshape(2, 3, 230))))
    assert tuple(lead) == ("action",) and lead["action"].shape == (2, 3, 2)
    env.close()


def _readers(env):
    """Every call that reads the actor, from the env's live latents: policy_act in its three modes (each from the same latents and
    observation), policy_imagine and policy_returns closed loop, mean and sampled."""
    import torch
    state = env.policy_state.clone()
    out = {}
    for mode in ("mean", "deploy", "explore"):
        env.policy_state.copy_(state)
        env.set_policy_sampling(mode, seed=5)
        out["act_" + mode] = env.policy_act().clone()
        out["state_" + mode] = env.policy_state.clone()
    env.set_policy_sampling("mean")
    env.policy_state.copy_(state)
    for mode in ("mean", "sample"):
        out["imagine_" + mode] = env.policy_imagine(5, mode, seed=3)["action"]
        got = env.policy_returns(4, mode, seed=3, outputs=("actions", "value"))
        out["returns_actions_" + mode], out["returns_value_" + mode] = got["actions"], got["value"]
    torch.cuda.synchronize()
    return _bytes(_cpu(out))


def test_every_reader_sees_the_fitted_actor():
    """After two steps policy_act in mean, deploy and explore (the sampled modes read hout's pair image), policy_imagine and
    policy_returns are byte-identical to those of a fresh env loaded with the checkpoint whose actor arrays are replaced by
    actor_weights() - with no reload and no latent reset on the fitted env."""
    feat, kw = _inputs("target", True, 97)
    env = _env(critic=True)

    driven = []
    for _ in range(3):
        driven.append(env.policy_act().clone())
        env.step(None, repeat=4)
    state = env.policy_state.clone()
    before = _readers(env)
    env.policy_state.copy_(state)
    env.actor_fit_begin()
    for _ in range(2):
        _fit(env, feat, lr=1e-3, **kw)
    fitted = env.actor_weights()
    assert all(fitted[k].tobytes() != _actor()[k].tobytes() for k in KEYS)
    assert env.policy_state.cpu().numpy().tobytes() == state.cpu().numpy().tobytes()
    after = _readers(env)
    twin = _env(checkpoint={**dict(weights("austria")), **fitted}, critic=True)
    for a in driven:                                          # the same cars at the same places: the checkpoint's own actor drove env
        twin.step(a, repeat=4)
    assert twin.views["lidar"].cpu().numpy().tobytes() == env.views["lidar"].cpu().numpy().tobytes()
    twin.policy_state.copy_(state)
    want = _readers(twin)
    for k in want:
        assert after[k] == want[k], k
    changed = [k for k in want if after[k] != before[k]]
    assert {"act_mean", "act_deploy", "act_explore", "imagine_mean", "imagine_sample", "returns_actions_mean"} <= set(changed), changed
    env.close()
    twin.close()


def test_a_fit_changes_nothing_else():
    """An actor step leaves the RSSM, the reward head, the critic, policy_state, action_in and the whole arena byte for byte as they
    were: the checkpoint's other arrays are seen through calls that read them and not the actor."""
    import torch
    feat, kw = _inputs("grad", True, 263)
    env = _env(critic=True)
    for _ in range(3):
        env.policy_act()
        env.step(None, repeat=4)
    acts = torch.from_numpy(np.random.default_rng(6).uniform(-1, 1, (4, 3, 5, 2)).astype(np.float32))

    def others():
        torch.cuda.synchronize()
        open_loop = env.policy_returns(5, "sample", seed=2, actions=acts[:, 0], outputs=("reward", "value", "features"))
        return [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes(),
                _bytes(env.critic_weights()), _bytes(env.reward_head_weights()), _bytes(_cpu(open_loop)),
                _bytes(_cpu(env.dream_ahead(acts, "mean", outputs=("return", "final_feature"))))]
    before = others()
    env.actor_fit_begin()
    assert _fit(env, feat, **kw)["step"] == 1
    assert before == others()
    assert all(env.actor_weights()[k].tobytes() != _actor()[k].tobytes() for k in KEYS)
    env.close()


def test_neutral_and_edge_rows():
    """Rows of weight zero contribute nothing, whatever their finite targets (0 inf is NaN: tests/test_gpu_policy_edges.py); a NaN target or action gradient skips the step and changes no
    weight; a fully saturated batch (draws that push tanh to +-1) gives norm 0 and leaves the weights as they are."""
    feat, kw = _inputs("target", True, 97)
    env = _env()
    w = kw["weight"].copy()
    w[::3] = 0.0
    wild = kw["target"].copy()
    wild[::3] = 1e6
    results = []
    for t in (wild, kw["target"]):
        env.load_actor(_actor())
        env.actor_fit_begin()
        spec = PolicyActorFitSpec(_actor())
        want = spec.step(feat, target=t, eps=kw["eps"], weight=w)
        got = _fit(env, feat, target=t, eps=kw["eps"], weight=w)
        assert np.float32(got["grad_norm"]).tobytes() == np.float32(want["grad_norm"]).tobytes()
        _same_weights(env, spec, "zero weights")
        results.append(env.actor_weights())
    assert all(results[0][k].tobytes() == results[1][k].tobytes() for k in KEYS)
    # a NaN: after a good step, so that the moments are not zero
    held, _, kg = _bytes(env.actor_weights()), *_inputs("grad", True, 97)
    bad_t, bad_g = kw["target"].copy(), kg["grad_actions"].copy()
    bad_t[13, 1] = bad_g[5, 0] = np.nan
    for bad in (dict(kw, target=bad_t), dict(kg, grad_actions=bad_g)):
        want = spec.step(feat, **bad)
        got = _fit(env, feat, **bad)
        assert got["skipped"] == 1 and got["step"] == 1 and want["skipped"] == 1 and np.isnan(got["grad_norm"])
        assert _bytes(env.actor_weights()) == held
    _same_status(_fit(env, feat, **kw), spec.step(feat, **kw), "after the skips")
    _same_weights(env, spec, "after the skips")
    assert spec.step_count == 2
    # saturated: the standard deviations are about 1e-4, so draws of +-1e6 move u by +-100.  On a new optimizer: with moments
    # carried over from earlier steps Adam would go on moving the weights under a zero gradient, as it should
    env.load_actor(_actor())
    env.actor_fit_begin()
    spec = PolicyActorFitSpec(_actor())
    sat = dict(kw, eps=np.where(kw["eps"] > 0, 1e6, -1e6).astype(np.float32))
    want = spec.step(feat, **sat)
    got = _fit(env, feat, grad_features=True, **sat)
    _same_status(got, want, "saturated")
    assert got["grad_norm"] == 0.0 and got["step"] == 1 and got["loss"] > 0 and not np.any(got["grad_features"])
    assert _bytes(env.actor_weights()) == _bytes(_actor())
    env.close()


def test_mixed_track_blocks_end_with_identical_actors():
    from racing_dreamer_amd.batched_env import MixedTrackEnv
    feat, kw = _inputs("target", True, 33)
    mixed = MixedTrackEnv(["columbia", "austria"], [3, 4], auto_reset=True, remap_actions=True)
    mixed.reset(mode="random", seed=4)
    mixed.load_policy(weights("austria"))
    mixed.actor_fit_begin()
    spec = PolicyActorFitSpec(_actor())
    for _ in range(2):
        want = spec.step(feat, **kw)
        got = _fit(mixed, feat, grad_features=True, **kw)
    _same_status(got, want, "mixed")
    assert got["grad_features"].tobytes() == want["grad_features"].tobytes()
    a, b = (p.actor_weights() for p in mixed.parts)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    _same_weights(mixed, spec, "mixed")
    assert _bytes(_cpu(mixed.policy_action(_t(feat)))) == {"action": spec.forward(feat)["action"].tobytes()}
    mixed.actor_fit_end()
    mixed.close()


def test_round_trip_and_distil_step():
    """load_actor(actor_weights()) after a step gives the same bytes back and resets no latent; planning.distil_step is the spec's
    step on the live features against the expert's actions, and leaves action_in as the actor wrote it."""
    import torch
    from racing_dreamer_amd.planning import distil_actor, distil_step, shooting_act
    feat, kw = _inputs("target", True, 33)
    env = _env(critic=True)
    for _ in range(3):
        env.policy_act()
        env.step(None, repeat=4)
    env.actor_fit_begin()
    _fit(env, feat, **kw)
    held = env.actor_weights()
    assert any(held[k].tobytes() != _actor()[k].tobytes() for k in KEYS)
    torch.cuda.synchronize()
    state, critic = env.policy_state.cpu().numpy().tobytes(), _bytes(env.critic_weights())
    assert np.any(env.policy_state.cpu().numpy() != 0)
    env.load_actor(held)
    assert _bytes(env.actor_weights()) == _bytes(held)
    assert env.policy_state.cpu().numpy().tobytes() == state and _bytes(env.critic_weights()) == critic
    # distil_step: the expert is the planner on the true dynamics
    env.actor_fit_begin()
    spec = PolicyActorFitSpec(held)
    env.policy_act()
    drove = env.views["action_in"].clone()
    expert = lambda e: shooting_act(e, candidates=8, horizon=5, seed=2)
    got = distil_step(env, expert, lr=1e-3)
    label = shooting_act(env, candidates=8, horizon=5, seed=2).clone().reshape(-1, 2)
    env.views["action_in"].copy_(drove)
    assert got["target"].cpu().numpy().tobytes() == label.cpu().numpy().tobytes()
    assert torch.equal(env.views["action_in"], drove)
    want = spec.step(env.policy_state[:, :230].cpu().numpy(), target=label.cpu().numpy(), lr=1e-3)
    _same_status({k: got[k].item() for k in ("loss", "grad_norm", "skipped", "step")}, want, "distil_step")
    _same_weights(env, spec, "distil_step")
    losses = distil_actor(env, expert, 2, act="mean", lr=1e-3)
    assert losses.shape == (2,) and bool(torch.isfinite(losses).all()) and env.policy_sampling["mode"] == "mean"
    env.close()


def test_refusals():
    """Wrong struct_size; no policy loaded; a normalized actor (both checkpoints with hnorm_* arrays); no optimizer open; both or
    neither of target and grad; rows outside [1, 2^31); null features; bad hyper-parameters; load_actor, load_policy and
    unload_policy close the optimizer."""
    import ctypes as C
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    INVALID = -1                                               # RC_ERR_INVALID (include/racecar_hip.h)
    feat, kw = _inputs("target", True, 2)
    f, t, g = _t(feat), _t(kw["target"]), _t(_rows(2)["grad"])
    bare = BatchedRaceEnv("austria", 2, 1, auto_reset=True, remap_actions=True)
    bare.reset(mode="random", seed=1)
    with pytest.raises(L.RacecarHipError, match="no policy loaded"):
        bare.actor_fit_begin()
    with pytest.raises(L.RacecarHipError, match="no policy loaded"):
        bare.policy_action(f)
    with pytest.raises(L.RacecarHipError, match="no policy loaded"):
        bare.actor_weights()
    for name in ("treitlstrasse_20210220", "treitlstrasse_occupancy"):
        bare.load_policy(weights(name))
        with pytest.raises(L.RacecarHipError, match="normalized"):
            bare.actor_fit_begin()
        with pytest.raises(L.RacecarHipError, match="normalized"):
            bare.policy_action(f)
    bare.close()
    env = _env()
    with pytest.raises(L.RacecarHipError, match="no optimizer is open for the actor"):
        env.actor_fit(f, target=t)
    env.actor_fit_begin()
    dev = f.to(env.device)
    args = L.RcPolicyActorFitArgs(C.sizeof(L.RcPolicyActorFitArgs), 2, dev.data_ptr())
    args.lr, args.clip, args.beta1, args.beta2, args.epsilon = 8e-5, 1.0, 0.9, 0.999, 1e-7
    step = lambda: env._lib.rc_policy_actor_fit_step(env._h, C.byref(args))
    assert step() == INVALID and b"neither" in env._lib.rc_last_error()
    args.target = args.grad = t.to(env.device).data_ptr()
    assert step() == INVALID and b"both" in env._lib.rc_last_error()
    args.grad = None
    for rows in (0, -1, 2 ** 31):
        args.rows = rows
        assert step() == INVALID and b"outside [1, 2^31)" in env._lib.rc_last_error()
    args.rows, args.features = 2, None
    assert step() == INVALID and b"features is NULL" in env._lib.rc_last_error()
    args.features, args.struct_size = dev.data_ptr(), C.sizeof(L.RcPolicyActorFitArgs) - 8
    assert step() == INVALID and b"struct_size" in env._lib.rc_last_error()
    fwd = L.RcPolicyActorForwardArgs(C.sizeof(L.RcPolicyActorForwardArgs) + 8, 2, dev.data_ptr())
    assert env._lib.rc_policy_actor_forward(env._h, C.byref(fwd)) == INVALID and b"struct_size" in env._lib.rc_last_error()
    fwd.struct_size = C.sizeof(L.RcPolicyActorForwardArgs)
    assert env._lib.rc_policy_actor_forward(env._h, C.byref(fwd)) == INVALID and b"no output" in env._lib.rc_last_error()
    with pytest.raises(ValueError):
        env.actor_fit(f, target=t, grad_actions=g)
    with pytest.raises(ValueError):
        env.actor_fit(f)
    with pytest.raises(ValueError):
        env.actor_fit(f[:0], target=t[:0])
    with pytest.raises(ValueError):
        env.actor_fit(f, target=t[:1])
    with pytest.raises(ValueError):
        env.policy_action(f, outputs=("logits",))
    for bad in (dict(lr=-1.0), dict(lr=float("nan")), dict(clip=float("inf")), dict(beta1=1.0), dict(beta2=1.5), dict(epsilon=-1e-7)):
        with pytest.raises(L.RacecarHipError, match="rc_policy_actor_fit_step"):
            env.actor_fit(f, target=t, **bad)
    assert _cpu(env.actor_fit(f, target=t))["step"].item() == 1.0           # (none of the refused calls counted)
    assert _cpu(env.actor_fit(f, grad_actions=g))["step"].item() == 2.0
    env.load_actor(env.actor_weights())                                      # replaces the actor: its optimizer is closed
    with pytest.raises(L.RacecarHipError, match="no optimizer is open for the actor"):
        env.actor_fit(f, target=t)
    with pytest.raises(KeyError):
        env.load_actor({})
    env.actor_fit_begin()
    env.load_policy(weights("austria"))
    with pytest.raises(L.RacecarHipError, match="no optimizer is open for the actor"):
        env.actor_fit(f, target=t)
    env.actor_fit_begin()
    env.actor_fit_end()
    with pytest.raises(L.RacecarHipError, match="no optimizer is open for the actor"):
        env.actor_fit(f, target=t)
    env.actor_fit_begin()
    env.unload_policy()
    with pytest.raises(L.RacecarHipError, match="no policy loaded"):
        env.actor_fit(f, target=t)
    env.close()
