"""rc_policy_fit_* / critic_fit against its binary32 specification (tests/policy_fit_spec.c), bit for bit: both heads, with and
without weights, row counts that reach every path of the three kernels; consecutive steps; the clip; that the fitted head is the one
the other kernels read; purity; zero weights; a NaN target; MixedTrackEnv; world_model.value_learning_step; the refusals; the .npz
round trip.  The env is austria with 4 envs; the rows are recorded latents, not the env's."""
import numpy as np
import pytest

from policy_fit_spec import LAYERS, PolicyFitSpec
from policy_observe_spec import PolicyObserveSpec
from policy_returns_spec import PolicyReturnsSpec
from test_golden_policy import weights
from test_gpu_policy_device import _recorded_inputs
from test_gpu_policy_imagine import _cpu
from test_policy_fit_spec import _critic, _rows

pytestmark = pytest.mark.gpu
HEADS = ("value", "pcont")


def _env(n=4, critic=None):
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=1)
    env.load_policy(weights("austria"))
    env.load_critic(_critic() if critic is None else critic)
    return env


def _fit(env, head, feat, target, weight=None, **hyper):
    import torch
    got = env.critic_fit(torch.from_numpy(feat), torch.from_numpy(target), None if weight is None else torch.from_numpy(weight), head=head, **hyper)
    return {k: v.item() for k, v in _cpu(got).items()}


def _same_status(got, want, what):
    assert np.float32(got["loss"]).tobytes() == np.float32(want["loss"]).tobytes(), (what, got["loss"], want["loss"])
    assert np.float32(got["grad_norm"]).tobytes() == np.float32(want["grad_norm"]).tobytes(), (what, got["grad_norm"], want["grad_norm"])
    assert (got["skipped"], got["step"]) == (want["skipped"], want["step"]), (what, got, want["skipped"], want["step"])


def _same_weights(env, spec, what, other=None):
    got = env.critic_weights()
    for k, a in spec.weights().items():
        diff = np.flatnonzero(got[k].reshape(-1) != a.reshape(-1))
        assert got[k].shape == a.shape and got[k].tobytes() == a.tobytes(), (what, k, len(diff), diff[:4])
    if other is not None:                                   # the head that was not fitted
        for k, a in other.items():
            assert got[k].tobytes() == a.tobytes(), (what, k)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("head", HEADS)
def test_one_step_is_the_spec_bit_for_bit(head, weighted):
    """One step from init_critic(5): all eight arrays, loss, grad_norm and step equal the spec for N = 1 and 2 (a single row, one
    row pair), 33 (one row past a workgroup), 97 (three workgroups and a partial one, the four chains of unequal length) and 263
    (every chain several pairs long)."""
    env = _env()
    other = {k: a for k, a in _critic().items() if not k.startswith(head)}
    for n in (1, 2, 33, 97, 263):
        feat, targets, weight = _rows(n)
        w = weight if weighted else None
        env.load_critic(_critic())
        env.critic_fit_begin(head)
        spec = PolicyFitSpec(_critic(), head)
        want = spec.step(feat, targets[head], w)
        got = _fit(env, head, feat, targets[head], w)
        print(head, weighted, n, got)
        _same_status(got, want, (head, weighted, n))
        _same_weights(env, spec, (head, weighted, n), other)
        assert want["step"] == 1 and want["grad_norm"] > 0
    env.close()


@pytest.mark.parametrize("head", HEADS)
def test_three_steps_are_the_specs_three_steps(head):
    """The carried moments and the bias correction: three consecutive steps at N = 97, status and weights after each."""
    env = _env()
    env.critic_fit_begin(head)
    spec = PolicyFitSpec(_critic(), head)
    feat, targets, weight = _rows(97)
    for i in range(3):
        want = spec.step(feat, targets[head], weight)
        _same_status(_fit(env, head, feat, targets[head], weight), want, (head, i))
        _same_weights(env, spec, (head, i))
    assert spec.step_count == 3
    env.close()


def test_clip_cases():
    """The CPU test's clipped case (norm >= 2 clip) and unclipped case (norm <= clip / 2), and clip = 0."""
    feat, targets, weight = _rows(97)
    env = _env()
    for scale, clip in ((40.0, 1.0), (1.0, 100.0), (1.0, 0.0)):
        env.load_critic(_critic())
        env.critic_fit_begin("value")
        spec = PolicyFitSpec(_critic(), "value")
        t = (np.float32(scale) * targets["value"]).astype(np.float32)
        want = spec.step(feat, t, weight, clip=clip)
        assert want["grad_norm"] >= 2 * clip if scale > 1 else (clip == 0 or want["grad_norm"] <= clip / 2)
        _same_status(_fit(env, "value", feat, t, weight, clip=clip), want, (scale, clip))
        _same_weights(env, spec, (scale, clip))
    env.close()


def test_the_fitted_head_is_what_the_other_kernels_read():
    """After two steps policy_value(features) and policy_returns(...)["value"] are byte-identical to those of a second env into
    which the spec's weights were loaded: no stale forward image, no missed repack."""
    import torch
    feat, targets, weight = _rows(97)
    env = _env()
    spec = {h: PolicyFitSpec(_critic(), h) for h in HEADS}
    for h in HEADS:
        env.critic_fit_begin(h)
        for _ in range(2):
            spec[h].step(feat, targets[h], weight)
            _fit(env, h, feat, targets[h], weight)
    twin = _env(critic={**spec["value"].weights(), **spec["pcont"].weights()})
    state = torch.from_numpy(np.pad(feat[:33], ((0, 0), (0, 2))))
    a = _cpu(env.policy_value(torch.from_numpy(feat), outputs=("value", "pcont")))
    b = _cpu(twin.policy_value(torch.from_numpy(feat), outputs=("value", "pcont")))
    assert a["value"].tobytes() == b["value"].tobytes() and a["pcont"].tobytes() == b["pcont"].tobytes()
    unfitted = _env()
    assert not np.array_equal(a["value"], _cpu(unfitted.policy_value(torch.from_numpy(feat)))["value"])
    unfitted.close()
    ra = _cpu(env.policy_returns(4, "sample", seed=3, state=state, outputs=("value", "returns", "weight")))
    rb = _cpu(twin.policy_returns(4, "sample", seed=3, state=state, outputs=("value", "returns", "weight")))
    assert all(ra[k].tobytes() == rb[k].tobytes() for k in ra)
    env.close()
    twin.close()


@pytest.mark.parametrize("head", HEADS)
def test_a_fit_changes_nothing_else(head):
    """Fitting one head leaves the other head's arrays, policy_state, action_in and the whole arena (observation views, episode
    counters) byte for byte as they were, and the next policy_act equals that of a twin env that never fitted."""
    import torch
    feat, targets, weight = _rows(97)
    env, twin = _env(), _env()
    for e in (env, twin):
        for _ in range(3):
            e.policy_act()
            e.step(None, repeat=4)
    torch.cuda.synchronize()
    before = [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes()]
    other = {k: a for k, a in env.critic_weights().items() if not k.startswith(head)}
    env.critic_fit_begin(head)
    _fit(env, head, feat, targets[head], weight)
    after = [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes()]
    assert before == after
    now = env.critic_weights()
    assert all(now[k].tobytes() == a.tobytes() for k, a in other.items())
    assert any(now[k].tobytes() != a.tobytes() for k, a in _critic().items() if k.startswith(head))
    env.critic_fit_end(head)
    for e in (env, twin):
        e.policy_act()
    torch.cuda.synchronize()
    assert env.views["action_in"].cpu().numpy().tobytes() == twin.views["action_in"].cpu().numpy().tobytes()
    assert env.policy_state.cpu().numpy().tobytes() == twin.policy_state.cpu().numpy().tobytes()
    env.close()
    twin.close()


def test_rows_of_weight_zero_contribute_nothing():
    """Every third row's weight is 0 and its target wild: the spec's step (1 / N counts all rows) bit for bit, and the same
    weights as with tame targets in those rows."""
    feat, targets, weight = _rows(97)
    w = weight.copy()
    w[::3] = 0.0
    wild = targets["value"].copy()
    wild[::3] = 1e6
    env = _env()
    results = []
    for t in (wild, targets["value"]):
        env.load_critic(_critic())
        env.critic_fit_begin("value")
        spec = PolicyFitSpec(_critic(), "value")
        want = spec.step(feat, t, w)
        got = _fit(env, "value", feat, t, w)
        assert np.float32(got["grad_norm"]).tobytes() == np.float32(want["grad_norm"]).tobytes()
        _same_weights(env, spec, "zero weights")
        results.append(env.critic_weights())
    assert all(results[0][k].tobytes() == results[1][k].tobytes() for k in results[0])
    env.close()


def test_a_nan_target_skips_the_step():
    """Arithmetic, not a fault: skipped = 1, the weights and the step count stay, and the next good step is step 2."""
    feat, targets, weight = _rows(97)
    env = _env()
    env.critic_fit_begin("value")
    spec = PolicyFitSpec(_critic(), "value")
    _same_status(_fit(env, "value", feat, targets["value"], weight), spec.step(feat, targets["value"], weight), "good")
    bad = targets["value"].copy()
    bad[13] = np.nan
    want = spec.step(feat, bad, weight)
    got = _fit(env, "value", feat, bad, weight)
    assert got["skipped"] == 1 and got["step"] == 1 and want["skipped"] == 1 and np.isnan(got["grad_norm"])
    _same_weights(env, spec, "skipped")
    _same_status(_fit(env, "value", feat, targets["value"], weight), spec.step(feat, targets["value"], weight), "after")
    _same_weights(env, spec, "after the skip")
    assert spec.step_count == 2
    env.close()


def test_mixed_track_blocks_end_with_identical_critics():
    from racing_dreamer_amd.batched_env import MixedTrackEnv
    import torch
    feat, targets, weight = _rows(33)
    mixed = MixedTrackEnv(["columbia", "austria"], [3, 4], auto_reset=True, remap_actions=True)
    mixed.reset(mode="random", seed=4)
    mixed.load_policy(weights("austria"))
    mixed.load_critic(_critic())
    mixed.critic_fit_begin("value")
    spec = PolicyFitSpec(_critic(), "value")
    for _ in range(2):
        want = spec.step(feat, targets["value"], weight)
        got = mixed.critic_fit(torch.from_numpy(feat), torch.from_numpy(targets["value"]), torch.from_numpy(weight))
    _same_status({k: v.item() for k, v in _cpu(got).items()}, want, "mixed")
    a, b = (p.critic_weights() for p in mixed.parts)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    _same_weights(mixed, spec, "mixed")
    mixed.critic_fit_end("value")
    mixed.close()


def test_value_learning_step_is_the_composition_of_the_specs():
    """world_model.value_learning_step on a batch shaped as TrajectoryRing.sample returns it (B = 3, T = 5, H = 3): the posterior
    features of PolicyObserveSpec in `sample` without each window's last step, the starts of PolicyReturnsSpec, whose features
    [:, :-1], returns and weight are the rows of PolicyFitSpec's step."""
    import torch
    from racing_dreamer_amd.world_model import value_learning_step
    b, t, h = 3, 5, 3
    scan = _recorded_inputs(b * t, seed=3)[0].reshape(b, t, 1080)
    rec = np.random.default_rng(4).uniform(-1, 1, (b, t, 2)).astype(np.float32)
    env = _env()
    env.critic_fit_begin("value")
    got = value_learning_step(env, dict(lidar=torch.from_numpy(scan), action=torch.from_numpy(rec)), horizon=h, seed=13, clip=100.0)
    feat = PolicyObserveSpec(weights("austria")).observe(scan, rec, mode="sample", seed=13)["feature"][:, :-1].reshape(-1, 230)
    dream = PolicyReturnsSpec(weights("austria"), _critic()).returns(feat, horizon=h, mode="sample", seed=13, lambda_=0.95, discount=0.99)
    spec = PolicyFitSpec(_critic(), "value")
    want = spec.step(dream["feature"][:, :-1].reshape(-1, 230), dream["returns"].reshape(-1), dream["weight"].reshape(-1), clip=100.0)
    status = {k: v.item() for k, v in _cpu(got).items()}
    _same_status(status, want, "value_learning_step")
    assert status["value_loss"] == status["loss"]
    _same_weights(env, spec, "value_learning_step")
    env.close()


def test_pcont_learning_step_fits_the_pcont_head_alone():
    """world_model.pcont_learning_step (B = 2, T = 4) with weight=10: the spec's pcont step on the posterior features of
    PolicyObserveSpec against discount * batch["discount"]; the value head does not move."""
    import torch
    from racing_dreamer_amd.world_model import pcont_learning_step
    b, t = 2, 4
    scan = _recorded_inputs(b * t, seed=3)[0].reshape(b, t, 1080)
    rec = np.random.default_rng(4).uniform(-1, 1, (b, t, 2)).astype(np.float32)
    alive = np.ones((b, t), np.float32)
    alive[1, 3] = 0.0                                       # (a terminal step: target 0)
    env = _env()
    env.critic_fit_begin("pcont")
    batch = dict(lidar=torch.from_numpy(scan), action=torch.from_numpy(rec), discount=torch.from_numpy(alive))
    got = pcont_learning_step(env, batch, discount=0.99, seed=13, weight=10, clip=100.0)
    feat = PolicyObserveSpec(weights("austria")).observe(scan, rec, mode="sample", seed=13)["feature"].reshape(-1, 230)
    spec = PolicyFitSpec(_critic(), "pcont")
    want = spec.step(feat, (np.float32(0.99) * alive).reshape(-1), np.full(b * t, 10.0, np.float32), clip=100.0)
    _same_status({k: v.item() for k, v in _cpu(got).items()}, want, "pcont_learning_step")
    _same_weights(env, spec, "pcont_learning_step", {k: a for k, a in _critic().items() if k.startswith("value_")})
    env.close()


def test_refusals():
    """A step without begin; a head that is not loaded; bad hyper-parameters; no rows; NULL inputs; load_critic closes the optimizer."""
    import ctypes as C
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.critic import init_critic
    feat, targets, weight = _rows(2)
    f, t = torch.from_numpy(feat), torch.from_numpy(targets["value"])
    env = _env(critic=init_critic(5, pcont=False))
    with pytest.raises(L.RacecarHipError, match="no optimizer is open"):
        env.critic_fit(f, t)
    with pytest.raises(L.RacecarHipError, match="no pcont head is loaded"):
        env.critic_fit_begin("pcont")
    with pytest.raises(ValueError):
        env.critic_fit_begin("reward")
    env.critic_fit_begin("value")
    for bad in (dict(lr=-1.0), dict(lr=float("nan")), dict(clip=float("inf")), dict(beta1=1.0), dict(beta2=1.5), dict(epsilon=-1e-7)):
        with pytest.raises(L.RacecarHipError, match="rc_policy_fit_step"):
            env.critic_fit(f, t, **bad)
    with pytest.raises(ValueError):
        env.critic_fit(f[:0], t[:0])
    with pytest.raises(ValueError):
        env.critic_fit(f, t[:1])
    dev_f, dev_t = f.to(env.device), t.to(env.device)
    a = L.RcPolicyFitArgs(C.sizeof(L.RcPolicyFitArgs), 0, 0, dev_f.data_ptr(), dev_t.data_ptr(), None, 8e-5, 1.0, 0.9, 0.999, 1e-7, None)
    assert env._lib.rc_policy_fit_step(env._h, C.byref(a)) == -1 and b"rows" in env._lib.rc_last_error()
    a.rows, a.features = 2, None
    assert env._lib.rc_policy_fit_step(env._h, C.byref(a)) == -1 and b"features is NULL" in env._lib.rc_last_error()
    a.features, a.target = dev_f.data_ptr(), None
    assert env._lib.rc_policy_fit_step(env._h, C.byref(a)) == -1 and b"target is NULL" in env._lib.rc_last_error()
    a.target, a.struct_size = dev_t.data_ptr(), 8
    assert env._lib.rc_policy_fit_step(env._h, C.byref(a)) == -1 and b"struct_size" in env._lib.rc_last_error()
    assert _cpu(env.critic_fit(f, t))["step"].item() == 1.0          # (none of the refused calls counted)
    env.load_critic(init_critic(5, pcont=False))
    with pytest.raises(L.RacecarHipError, match="no optimizer is open"):
        env.critic_fit(f, t)
    env.critic_fit_begin("value")
    env.critic_fit_end("value")
    with pytest.raises(L.RacecarHipError, match="no optimizer is open"):
        env.critic_fit(f, t)
    env.close()


def test_save_and_load_round_trip(tmp_path):
    """critic.save_critic after a step, critic.load_critic_file into a second env: the same arrays, byte for byte."""
    from racing_dreamer_amd.critic import load_critic_file, save_critic
    feat, targets, weight = _rows(33)
    env = _env()
    env.critic_fit_begin("pcont")
    _fit(env, "pcont", feat, targets["pcont"], weight)
    save_critic(tmp_path / "critic.npz", env)
    loaded = load_critic_file(tmp_path / "critic.npz")
    assert set(loaded) == set(_critic())
    twin = _env(critic=loaded)
    a, b = env.critic_weights(), twin.critic_weights()
    assert all(a[k].tobytes() == b[k].tobytes() == loaded[k].tobytes() for k in a)
    assert any(a[k].tobytes() != v.tobytes() for k, v in _critic().items())
    env.close()
    twin.close()
