"""rc_policy_fit_* with RC_POLICY_FIT_REWARD / reward_fit against its binary32 specification (tests/policy_fit_spec.c at two hidden layers), bit for
bit: with and without weights, row counts that reach every path of the kernels; consecutive steps; that every reader of the reward
head - the dream's backward pass with its transposed images among them - sees the fitted weights; purity; zero weights; a NaN
target; MixedTrackEnv; world_model.reward_learning_step; the refusals; the round trip through reward_head_weights and
load_reward_head.  The env is austria with 4 envs, the head the checkpoint's own; the rows are recorded latents, not the env's."""
import numpy as np
import pytest

from policy_fit_spec import PolicyFitSpec
from policy_observe_spec import PolicyObserveSpec
from policy_reward_fit_spec import KEYS, PolicyRewardFitSpec
from test_golden_policy import weights
from test_gpu_policy_device import _recorded_inputs
from test_gpu_policy_imagine import _cpu
from test_policy_fit_spec import _critic
from test_policy_fit_spec import _rows as _critic_rows
from test_policy_reward_fit_spec import _head, _rows

pytestmark = pytest.mark.gpu


def _env(n=4, checkpoint=None, critic=True):
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=1)
    env.load_policy(weights("austria") if checkpoint is None else checkpoint)
    if critic:
        env.load_critic(_critic())
    return env


def _fit(env, feat, target, weight=None, **hyper):
    import torch
    got = env.reward_fit(torch.from_numpy(feat), torch.from_numpy(target), None if weight is None else torch.from_numpy(weight), **hyper)
    return {k: v.item() for k, v in _cpu(got).items()}


def _same_status(got, want, what):
    assert np.float32(got["loss"]).tobytes() == np.float32(want["loss"]).tobytes(), (what, got["loss"], want["loss"])
    assert np.float32(got["grad_norm"]).tobytes() == np.float32(want["grad_norm"]).tobytes(), (what, got["grad_norm"], want["grad_norm"])
    assert (got["skipped"], got["step"]) == (want["skipped"], want["step"]), (what, got, want["skipped"], want["step"])


def _same_weights(env, spec, what):
    got = env.reward_head_weights()
    assert tuple(got) == KEYS
    for k, a in spec.weights().items():
        diff = np.flatnonzero(got[k].reshape(-1) != a.reshape(-1))
        assert got[k].shape == a.shape and got[k].tobytes() == a.tobytes(), (what, k, len(diff), diff[:4])


def _bytes(d):
    return {k: v.tobytes() for k, v in d.items()}


@pytest.mark.parametrize("weighted", [False, True])
def test_one_step_is_the_spec_bit_for_bit(weighted):
    """One step from the checkpoint's head: all six arrays, loss, grad_norm and step equal the spec for N = 1 and 2 (a single row,
    one row pair), 33 (one row past a workgroup), 97 (three workgroups and a partial one, the four chains of unequal length) and
    263 (every chain several pairs long)."""
    env = _env(critic=False)
    for n in (1, 2, 33, 97, 263):
        feat, target, weight = _rows(n)
        w = weight if weighted else None
        env.load_reward_head(_head())
        env.reward_fit_begin()
        spec = PolicyRewardFitSpec(_head())
        want = spec.step(feat, target, w)
        got = _fit(env, feat, target, w)
        print(weighted, n, got)
        _same_status(got, want, (weighted, n))
        _same_weights(env, spec, (weighted, n))
        assert want["step"] == 1 and want["grad_norm"] > 0
    env.close()


def test_three_steps_are_the_specs_three_steps():
    """The carried moments and the bias correction: three consecutive steps at N = 97, status and weights after each."""
    env = _env(critic=False)
    env.reward_fit_begin()
    spec = PolicyRewardFitSpec(_head())
    feat, target, weight = _rows(97)
    for i in range(3):
        want = spec.step(feat, target, weight)
        _same_status(_fit(env, feat, target, weight), want, i)
        _same_weights(env, spec, i)
    assert spec.step_count == 3
    env.close()


@pytest.mark.gpu_slow          # (the spec's step on 32 769 rows takes 13 s on the CPU, the device's milliseconds: `pytest -m gpu_slow`)
def test_the_loss_sum_takes_a_second_term_per_lane():
    """rc_policy_fit_sums_kernel adds the N loss terms by lanes 32 768 apart (128 workgroups of 256): up to N = 32 768 every lane
    has at most one term, at N = 32 769 lane 0 of workgroup 0 takes a second one - the loop's second pass over the loss terms, which
    no other test reaches.  One reward-head step at that N: the recorded latents tiled, each row scaled by its own factor in
    [0.5, 1.5], fresh targets and weights; the last row's target is 40, so its loss term (0.5 w (o - 40)^2, several hundred among
    terms below 10) moves the mean by one part in a hundred and not by a few ulps.  loss, grad_norm, step and the six arrays equal
    the spec - whose sum is pfs_tree, the same tree on the host - byte for byte."""
    n = 32 * 1024 + 1
    feat, _, _ = _rows(263)
    rng = np.random.default_rng(23)
    big = np.ascontiguousarray(feat[np.arange(n) % 263] * rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32))
    target, weight = rng.normal(0.1, 0.5, n).astype(np.float32), rng.uniform(0.2, 1.0, n).astype(np.float32)
    target[-1] = 40.0
    spec = PolicyRewardFitSpec(_head())
    want = spec.step(big, target, weight)
    assert want["step"] == 1 and want["skipped"] == 0 and want["loss"] > 0.63
    env = _env(critic=False)
    env.reward_fit_begin()
    got = _fit(env, big, target, weight)
    print(n, got)
    _same_status(got, want, n)
    _same_weights(env, spec, n)
    env.close()


def _readers(env, scan, rec, acts):
    """Every call that reads the reward head, on the env's live latents (and a recorded window)."""
    import torch
    out = {"imagine": env.policy_imagine(5, "mean", seed=3)["reward"],
           "observe": env.policy_observe(torch.from_numpy(scan), torch.from_numpy(rec), outputs=("reward",))["reward"],
           "dream": env.dream_ahead(acts, "mean", discount=0.99, outputs=("return",))["return"],
           "returns": env.policy_returns(4, "mean", seed=3, outputs=("reward",))["reward"]}
    grad = env.dream_ahead_grad(acts, "mean", discount=0.99, outputs=("grad_actions", "return"))
    out["grad_actions"], out["grad_return"] = grad["grad_actions"], grad["return"]
    return _bytes(_cpu(out))


def test_every_reader_sees_the_fitted_head():
    """After two steps policy_imagine, policy_observe, dream_ahead, policy_returns and dream_ahead_grad are byte-identical to those of
    a fresh env loaded with the checkpoint and the fitted head.  dream_ahead_grad ran once BEFORE the fit, so its transposed images
    of the head exist and are stale after it: they must be made again."""
    import torch
    feat, target, weight = _rows(97)
    scan = _recorded_inputs(2 * 6, seed=3)[0].reshape(2, 6, 1080)
    rec = np.random.default_rng(4).uniform(-1, 1, (2, 6, 2)).astype(np.float32)
    acts = torch.from_numpy(np.random.default_rng(6).uniform(-1, 1, (4, 3, 5, 2)).astype(np.float32))
    env = _env()

    def drive(e):
        for _ in range(3):
            e.policy_act()
            e.step(None, repeat=4)
    drive(env)
    before = _readers(env, scan, rec, acts)
    env.reward_fit_begin()
    for _ in range(2):
        _fit(env, feat, target, weight)
    fitted = env.reward_head_weights()
    assert any(fitted[k].tobytes() != _head()[k].tobytes() for k in KEYS)
    after = _readers(env, scan, rec, acts)
    twin = _env(checkpoint={**dict(weights("austria")), **fitted})
    drive(twin)
    want = _readers(twin, scan, rec, acts)
    for k in want:
        assert after[k] == want[k], k
        assert after[k] != before[k], k
    env.close()
    twin.close()


def test_a_fit_changes_nothing_else():
    """A reward step leaves policy_state, action_in, the critic and the whole arena (observation views, episode counters) byte for
    byte as they were; and a value-head optimizer that was open before it - the two share the scratch - takes its next step exactly
    as the spec's."""
    import torch
    feat, target, weight = _rows(263)
    cfeat, ctargets, cweight = _critic_rows(97)
    env = _env()
    for _ in range(3):
        env.policy_act()
        env.step(None, repeat=4)
    env.critic_fit_begin("value")
    value_spec = PolicyFitSpec(_critic(), "value")
    value_spec.step(cfeat, ctargets["value"], cweight)
    env.critic_fit(torch.from_numpy(cfeat), torch.from_numpy(ctargets["value"]), torch.from_numpy(cweight))
    torch.cuda.synchronize()
    before = [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes(),
              _bytes(env.critic_weights())]
    env.reward_fit_begin()
    assert _fit(env, feat, target, weight)["step"] == 1
    after = [env.policy_state.cpu().numpy().tobytes(), env.views["action_in"].cpu().numpy().tobytes(), env.arena.cpu().numpy().tobytes(),
             _bytes(env.critic_weights())]
    assert before == after
    assert any(env.reward_head_weights()[k].tobytes() != _head()[k].tobytes() for k in KEYS)
    want = value_spec.step(cfeat, ctargets["value"], cweight)
    got = env.critic_fit(torch.from_numpy(cfeat), torch.from_numpy(ctargets["value"]), torch.from_numpy(cweight))
    _same_status({k: v.item() for k, v in _cpu(got).items()}, want, "the value head's second step")
    now = env.critic_weights()
    for k, a in value_spec.weights().items():
        assert now[k].tobytes() == a.tobytes(), k
    env.close()


def test_rows_of_weight_zero_contribute_nothing():
    """Every third row's weight is 0 and its target wild: the spec's step (1 / N counts all rows) bit for bit, and the same
    weights as with tame targets in those rows."""
    feat, target, weight = _rows(97)
    w = weight.copy()
    w[::3] = 0.0
    wild = target.copy()
    wild[::3] = 1e6
    env = _env(critic=False)
    results = []
    for t in (wild, target):
        env.load_reward_head(_head())
        env.reward_fit_begin()
        spec = PolicyRewardFitSpec(_head())
        want = spec.step(feat, t, w)
        got = _fit(env, feat, t, w)
        assert np.float32(got["grad_norm"]).tobytes() == np.float32(want["grad_norm"]).tobytes()
        _same_weights(env, spec, "zero weights")
        results.append(env.reward_head_weights())
    assert all(results[0][k].tobytes() == results[1][k].tobytes() for k in results[0])
    env.close()


def test_a_nan_target_skips_the_step():
    """Arithmetic, not a fault: skipped = 1, the weights and the step count stay, and the next good step is step 2."""
    feat, target, weight = _rows(97)
    env = _env(critic=False)
    env.reward_fit_begin()
    spec = PolicyRewardFitSpec(_head())
    _same_status(_fit(env, feat, target, weight), spec.step(feat, target, weight), "good")
    held = _bytes(env.reward_head_weights())
    bad = target.copy()
    bad[13] = np.nan
    want = spec.step(feat, bad, weight)
    got = _fit(env, feat, bad, weight)
    assert got["skipped"] == 1 and got["step"] == 1 and want["skipped"] == 1 and np.isnan(got["grad_norm"])
    assert _bytes(env.reward_head_weights()) == held
    _same_weights(env, spec, "skipped")
    _same_status(_fit(env, feat, target, weight), spec.step(feat, target, weight), "after")
    _same_weights(env, spec, "after the skip")
    assert spec.step_count == 2
    env.close()


def test_mixed_track_blocks_end_with_identical_reward_heads():
    from racing_dreamer_amd.batched_env import MixedTrackEnv
    import torch
    feat, target, weight = _rows(33)
    mixed = MixedTrackEnv(["columbia", "austria"], [3, 4], auto_reset=True, remap_actions=True)
    mixed.reset(mode="random", seed=4)
    mixed.load_policy(weights("austria"))
    mixed.reward_fit_begin()
    spec = PolicyRewardFitSpec(_head())
    for _ in range(2):
        want = spec.step(feat, target, weight)
        got = mixed.reward_fit(torch.from_numpy(feat), torch.from_numpy(target), torch.from_numpy(weight))
    _same_status({k: v.item() for k, v in _cpu(got).items()}, want, "mixed")
    a, b = (p.reward_head_weights() for p in mixed.parts)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    _same_weights(mixed, spec, "mixed")
    mixed.reward_fit_end()
    mixed.close()


def test_reward_learning_step_is_the_composition_of_the_specs():
    """world_model.reward_learning_step on a [2, 6] window batch: the posterior features of PolicyObserveSpec in `sample` are the
    rows of PolicyRewardFitSpec's step against the recorded rewards."""
    import torch
    from racing_dreamer_amd.world_model import reward_learning_step
    b, t = 2, 6
    scan = _recorded_inputs(b * t, seed=3)[0].reshape(b, t, 1080)
    rng = np.random.default_rng(4)
    rec = rng.uniform(-1, 1, (b, t, 2)).astype(np.float32)
    reward = rng.normal(0.1, 0.5, (b, t)).astype(np.float32)
    env = _env(critic=False)
    env.reward_fit_begin()
    batch = dict(lidar=torch.from_numpy(scan), action=torch.from_numpy(rec), reward=torch.from_numpy(reward))
    got = reward_learning_step(env, batch, seed=13, clip=100.0)
    feat = PolicyObserveSpec(weights("austria")).observe(scan, rec, mode="sample", seed=13)["feature"].reshape(-1, 230)
    spec = PolicyRewardFitSpec(_head())
    want = spec.step(feat, reward.reshape(-1), None, clip=100.0)
    status = {k: v.item() for k, v in _cpu(got).items()}
    _same_status(status, want, "reward_learning_step")
    assert status["reward_loss"] == status["loss"]
    _same_weights(env, spec, "reward_learning_step")
    env.close()


def test_refusals():
    """A step without begin; begin with no reward head loaded; bad hyper-parameters; no rows; a mismatched target; load_reward_head
    closes the optimizer and load_critic does not; "reward" is still no head of critic_fit_begin."""
    import torch
    from racing_dreamer_amd import _lib as L
    feat, target, weight = _rows(2)
    f, t = torch.from_numpy(feat), torch.from_numpy(target)
    env = _env()
    with pytest.raises(L.RacecarHipError, match="no optimizer is open for the reward head"):
        env.reward_fit(f, t)
    with pytest.raises(ValueError):
        env.critic_fit_begin("reward")
    L.check(env._lib.rc_policy_load_heads(env._h, None))
    with pytest.raises(L.RacecarHipError, match="no reward head is loaded"):
        env.reward_fit_begin()
    with pytest.raises(L.RacecarHipError, match="no reward head is loaded"):
        env.reward_head_weights()
    env.load_reward_head(_head())
    env.reward_fit_begin()
    for bad in (dict(lr=-1.0), dict(lr=float("nan")), dict(clip=float("inf")), dict(beta1=1.0), dict(beta2=1.5), dict(epsilon=-1e-7)):
        with pytest.raises(L.RacecarHipError, match="rc_policy_fit_step"):
            env.reward_fit(f, t, **bad)
    with pytest.raises(ValueError):
        env.reward_fit(f[:0], t[:0])
    with pytest.raises(ValueError):
        env.reward_fit(f, t[:1])
    assert _cpu(env.reward_fit(f, t))["step"].item() == 1.0           # (none of the refused calls counted)
    env.load_critic(_critic())                                        # replaces the critic: the reward optimizer stays open
    assert _cpu(env.reward_fit(f, t))["step"].item() == 2.0
    env.load_reward_head(env.reward_head_weights())                   # replaces the reward head: its optimizer is closed
    with pytest.raises(L.RacecarHipError, match="no optimizer is open for the reward head"):
        env.reward_fit(f, t)
    env.reward_fit_begin()
    env.reward_fit_end()
    with pytest.raises(L.RacecarHipError, match="no optimizer is open for the reward head"):
        env.reward_fit(f, t)
    with pytest.raises(KeyError):
        env.load_reward_head({})
    env.close()


def test_read_and_load_round_trip():
    """load_reward_head(reward_head_weights()) after a step gives the same bytes back, and resets no latent."""
    import torch
    feat, target, weight = _rows(33)
    env = _env()
    for _ in range(3):
        env.policy_act()
        env.step(None, repeat=4)
    env.reward_fit_begin()
    _fit(env, feat, target, weight)
    held = env.reward_head_weights()
    assert any(held[k].tobytes() != _head()[k].tobytes() for k in KEYS)
    torch.cuda.synchronize()
    state, critic = env.policy_state.cpu().numpy().tobytes(), _bytes(env.critic_weights())
    assert np.any(env.policy_state.cpu().numpy() != 0)
    env.load_reward_head(held)
    assert _bytes(env.reward_head_weights()) == _bytes(held)
    assert env.policy_state.cpu().numpy().tobytes() == state and _bytes(env.critic_weights()) == critic
    assert env.policy_has_reward_head
    env.close()
