"""Every Dreamer unit on the device against its binary32 spec at the numeric edges (tests/policy_edge_cases.py has the recipes, the
comparison rule and the guards; tests/test_policy_edge_spec.py runs the guards on the CPU): zero and signed zero, subnormal weights,
operands, products, accumulators and Adam moments, overflow to inf and inf - inf, the +-86 clamp under a GRU scaled by 2^100, special
scan beams and raw actions, one poisoned row among 33, saturated output layers, and memory a handle keeps from a larger, poisoned
call.  The rule: NaN positions coincide, every other element has the same bytes (`same`).  One env of 33 cars - a full workgroup and
one row, so padded rows exist -, H = T = 2, K = 2; every output a call offers is compared.

Which case applies to which unit (x: run; the modes are the unit's own - act: mean / deploy / explore, the rollouts: mean / sample,
fit: value / pcont, reward_fit: reward, actor_fit: target / grad with eps and weights given, action: mean (no eps) / draw):

    case                act  imagine observe dream dream_grad returns value fit decode decode_lidar reward_fit actor_fit action
    A-zero-layer         -      -       -      -       -         x      x    x    x       x            x         x       x    (1)
    A-negzero-inputs     x      x       x      x       x         x      x    x    x       x            x         x       x
    A-no-eps                                                                                                     x            (11)
    B1, B2 (out 2^-135,  x(2)   x       x      x(3)    x         x      x    x    x       x            x         x       x
            2^-120)
    B1g, B2g (action                                                                                             x(12)
            gradient 2^-135, 2^-120)
    B3 (Adam moments)                                                        x                         x         x            (4)
    B4 (features 2^-130)                                                x    x    x       x            x         x       x    (4)
    C1 (infinite norm)                                                       x(5)                      x         x            (13)
    C2 (inf - inf)                                               x      x    x                         x         x       -    (6)
    C3 (GRU 2^100)       x      x       x      x       x         x                                                            (7)
    C3-inf (+-inf deter) x      x       x      x       x         x                                                            (7)
    D1 (beams)           x              x                                                 x                                   (8)
    D2 (raw actions)            x       x      x       x         x                                                            (8)
    D3 (poisoned row)    x      x       x      x       x         x      x    x    x       x            x         x       x    (14)
    D4 (fit inputs)                                                          x                         x         x(15)
    D5 (eps +-inf, NaN)                                                                                          x       x(16)
    D6 (action gradient inf)                                                                                     x(12)
    E1 (raw scale bias)                                                                   x
    E2 (+-100 biases)    x(9)                                    x      x    x(9) x                    -         x       x    (9)
    E3 (KL)                             x
    E4 (mean saturated)                                                                                          x       x    (17)
    E5 (on target)                                                                                               x(18)
    F  (stale memory)                                  x         x           x                         x         x            (10)

 (1) the rollout units' first layer is img1: a zero kernel with a -0 bias gives ELU(-0) = +0 and the next bias takes over - the spec's
     answer is ordinary in every output, the case proves nothing there.  The heads and decoders answer with identical rows.  So does the
     actor's forward (mean and std; a draw's action differs by its eps).  The fits take a step whose first kernel starts from zero.
 (2) `mean` only: in deploy / explore the draw's noise makes the action a normal number.  (3) B1 only: the dream has no gradient and
     its rewards at 2^-120 are normal.  (4) units that take features.  (5) the value head: a sigmoid bounds the pcont head's delta.
 (6) units that read the value head, and the other fits (the hidden layers x 2^100); action: the forward stays finite there, which
     actor_fit's C2 guard asserts.  (7) units with a GRU: C3's pre-activations are beyond +-86 but finite (2.5e31), C3-inf carries +-inf
     in the deter of four rows, so sigma and tanh meet +-inf and NaN.  (8) units that take scans / raw actions (the LiDAR decoder: its target).
 (9) act: the sampled modes (the mean does not read the raw std); fit: the pcont head; reward_fit: its likelihood is Normal(o, 1), no
     output is squashed; action: in mode mean the std output shows it.  (10) units whose handle keeps memory between
     calls: the fit's scratch, dream_ahead_grad's stash; policy_returns for its LDS rows past the last row.  The fit's first call is
     neither C2 nor D3 (an ELU takes their NaN to a finite number) but features x 2^127 with NaN targets: +inf in the activation
     planes, NaN in the delta planes; policy_edge_cases.make says what of it the smaller call's planes overlie.  reward_fit and
     actor_fit: the first call is on ANOTHER head of the same handle (an actor step; a value-head step), both optimizers open - the four
     heads share one scratch whose plane offsets depend on the depth.
 (11) eps None: the raw-std columns of the gradient and their moments are +0 by bit pattern.  (12) `grad` only (`target` takes no
     action gradient): at 2^-135 every square underflows, the norm is exactly +0, the step is taken with v = +0 and den = epsilon.
 (13) reward_fit: the last hidden layer x 2^40; actor_fit: the action gradient (grad) or the targets (target) x 2^100.
 (14) actor_fit: the norm is NaN and the step skipped, the poisoned row's own grad_features are 230 zeros (ELU(NaN) = -1, elu' = 0), the
     other rows' are the clean twin's.  (15) D4-target+-inf in `target` only; D4-weight0+inf-target: 0 inf = NaN in the loss (target)
     and in the action gradient (grad: the row's gradient is infinite there).  (16) action: `draw` only.  (17) hout_b[0:2] = +-1000:
     tanh(o / 5) = +-1 exactly, d_mean = 0 for every row; action: the mean is +-5 exactly.  (18) `target` only: every act - target is +0.
 A unit has no single-row path of its own but the fits (a lone row is half a row pair): B4-one-row (fit, reward_fit, actor_fit).
 A skipped step (C1, C2, D3 .. D6) leaves every weight byte as LOADED: `_compare` holds the device to the loaded arrays as well as to
 the spec's.  After every actor_fit case that takes a step the actor's readers are checked once (`_actor_readers`), after reward_fit's B1
 the reward head's (`_reward_readers`).

Addresses and loop bounds derived from float data - read before the first run of cases C, D and F: there are none.  The only
float -> integer conversions in the twelve kernels (the fit engine's instances at two and four hidden layers and the actor's
forward-only instance among them) and their shared headers are `(int32_t)n` in pm_exp_parts, where n = rint(x log2 e)
of an x that two selects have put into [-86, 86] (a NaN fails `x > -86` and becomes -86), which builds the exponent bits of 2^n, never
an address; and pm_log's exponent field, used as a number.  deploy's best-of-100 keeps an index: it starts at the lane's first
candidate (`best_i < 0 ||`), every comparison with a NaN score is false, so it stays in [0, 100) and only selects a Philox block.
Rows, columns and time steps are integers of the call.  The fit engine (fit_rows, fit_dense, fit_grad_features, the wgrad, sums,
scale and apply kernels) indexes by blockIdx, threadIdx, n and compile-time tables alone; on the host fit_run sizes the scratch
(n (2 depth 416 + nout + 1) floats), its plane offsets, the wgrad tile table and every grid from n, the head's depth and constants,
and reads no device memory: a NaN or infinite norm only sets FitCtl.skipped, which makes apply return before it touches a weight.  Padded rows are selected to zero on the way in (`q < n ? x : 0`), not
multiplied; outputs of rows past the end are never stored."""
import numpy as np
import pytest

import policy_edge_cases as pe

pytestmark = pytest.mark.gpu
f32 = np.float32
OBSERVE = ("feature", "post_mean", "post_std", "prior_mean", "prior_std", "kl", "state", "reward")
RETURNS = ("reward", "value", "pcont", "returns", "weight", "actions", "features", "reward_start", "value_start", "pcont_start")


def _new_env():
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", pe.N, 1, auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=1)                    # (episode 1, agent step 0: the keys of policy_edge_cases._keys; no test steps the env)
    return env


@pytest.fixture(scope="module")
def env():
    e = _new_env()
    yield e
    e.close()


def _cpu(d):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _load(env, unit, call):
    weights = dict(call.policy)
    if unit == "decode_lidar":
        weights.update(call.ldec)
    env.load_policy(weights)
    if unit in ("returns", "value", "fit", "reward_fit", "actor_fit"):      # (the new heads' case F and readers take the critic)
        env.load_critic(call.critic)


def _t(env, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


def _device(env, unit, call, mode, loaded=False, after=None):
    """The device's answer under the spec's output names.  Leaves the env's views as it found them.  `after(env, out)` runs behind the
    steps of reward_fit and actor_fit, while their optimizers are open."""
    import torch
    kw = call.kw
    if not loaded:
        _load(env, unit, call)
    if unit == "act":
        n = pe.N
        keep = {k: env.views[k].clone() for k in ("lidar", "fresh", "action_in")}
        env.views["lidar"].view(n, 1080).copy_(_t(env, kw["scan"]))
        env.views["fresh"].view(n).copy_(_t(env, kw["fresh"]))
        env.policy_state.copy_(_t(env, kw["state"]))
        env.set_policy_sampling(mode, seed=pe.SEED)
        env.policy_act()
        torch.cuda.synchronize()
        out = dict(action=env.views["action_in"].view(n, 2).cpu().numpy(), state=env.policy_state.cpu().numpy())
        for k, v in keep.items():                           # (a NaN action never reaches env.step)
            env.views[k].copy_(v)
        return out
    if unit == "imagine":
        env.policy_state.copy_(_t(env, kw["state"]))
        return _cpu(env.policy_imagine(kw["horizon"], mode, seed=pe.SEED, actions=_t(env, kw["actions"]), features=True, start_reward=True))
    if unit == "observe":
        return _cpu(env.policy_observe(_t(env, kw["scan"]), _t(env, kw["action"]), None, mode, seed=pe.SEED, state=_t(env, kw["state"]), outputs=OBSERVE))
    if unit == "dream":
        return _cpu(env.dream_ahead(_t(env, kw["actions"]), mode, seed=pe.SEED, state=_t(env, kw["state"]), discount=0.99,
                                    outputs=("return", "reward", "final_feature")))
    if unit == "dream_grad":
        return _cpu(env.dream_ahead_grad(_t(env, kw["actions"]), mode, seed=pe.SEED, state=_t(env, kw["state"]), discount=0.99,
                                         outputs=("grad_actions", "grad_state", "return", "reward")))
    if unit == "returns":
        return _cpu(env.policy_returns(kw["horizon"], mode, seed=pe.SEED, lambda_=0.95, discount=0.99, actions=_t(env, kw["actions"]),
                                       state=_t(env, kw["state"]), outputs=RETURNS))
    if unit == "value":
        return _cpu(env.policy_value(_t(env, kw["features"]), outputs=("value", "reward", "pcont")))
    if unit == "fit":
        env.critic_fit_begin(mode)
        calls = ([kw["first"].kw] if kw.get("first") is not None else []) + [kw] * kw["steps"]
        for k in calls:
            status = env.critic_fit(_t(env, k["features"]), _t(env, k["target"][mode]), _t(env, k["weight"]), head=mode, **k["hyper"])
        out = {k: f32(v.item()) for k, v in _cpu(status).items()}
        out.update(env.critic_weights())                    # (both heads: the one that was not fitted is compared with what was loaded)
        env.critic_fit_end(mode)
        return out
    if unit == "reward_fit":
        env.reward_fit_begin()
        if kw.get("first") is not None:                     # case F: an actor step of 64 rows first; both optimizers stay open
            fk = kw["first"].kw
            env.actor_fit_begin()
            status = env.actor_fit(_t(env, fk["features"]), target=_t(env, fk["target"]), eps=_t(env, fk["eps"]), weight=_t(env, fk["weight"]))
            assert _cpu(status)["skipped"].item() == 1.0
        for _ in range(kw["steps"]):
            status = env.reward_fit(_t(env, kw["features"]), _t(env, kw["target"][mode]), _t(env, kw["weight"]), **kw["hyper"])
        out = {k: f32(v.item()) for k, v in _cpu(status).items()}
        out.update(env.reward_head_weights())
        if after is not None:
            after(env, out)
        env.reward_fit_end()
        if kw.get("first") is not None:
            env.actor_fit_end()
        return out
    if unit == "actor_fit":
        env.actor_fit_begin()
        if kw.get("first") is not None:                     # case F: a value-head step of 64 rows first; both optimizers stay open
            fk = kw["first"].kw
            env.critic_fit_begin("value")
            status = env.critic_fit(_t(env, fk["features"]), _t(env, fk["target"]["value"]), _t(env, fk["weight"]), head="value")
            assert _cpu(status)["skipped"].item() == 1.0
        given = {("target" if mode == "target" else "grad_actions"): _t(env, kw["target" if mode == "target" else "grad_actions"])}
        for _ in range(kw["steps"]):
            status = env.actor_fit(_t(env, kw["features"]), eps=_t(env, kw["eps"]), weight=_t(env, kw["weight"]), grad_features=True, **given, **kw["hyper"])
        got = _cpu(status)
        out = {k: f32(got[k].item()) for k in ("loss", "grad_norm", "skipped", "step")}
        out["grad_features"] = got["grad_features"]
        out.update(env.actor_weights())
        if after is not None:
            after(env, out)
        env.actor_fit_end()
        if kw.get("first") is not None:
            env.critic_fit_end("value")
        return out
    if unit == "action":
        return _cpu(env.policy_action(_t(env, kw["features"]), eps=_t(env, kw["eps"]) if mode == "draw" else None, outputs=("action", "mean", "std")))
    if unit == "decode":
        out = _cpu(env.policy_decode_loglik(_t(env, kw["target"]), _t(env, kw["features"]), outputs=("loglik", "logits", "image")))
        plain = _cpu(env.policy_decode(_t(env, kw["features"]), logits=True, image=True))
        assert all(pe.same(plain[k], out[k]) for k in plain), "policy_decode and policy_decode_loglik disagree"
        return out
    if unit == "decode_lidar":
        return _cpu(env.policy_decode_lidar(_t(env, kw["features"]), target=_t(env, kw["target"]), outputs=("mean", "std", "loglik")))
    raise KeyError(unit)


def _compare(unit, case, mode, got, want, call):
    offered = set(got)
    expected = set(want) - set(pe.PRIVATE)                  # (the moments stay on the device: the weights after three steps show them)
    if unit == "fit":
        other = {k: a for k, a in call.critic.items() if not k.startswith(mode)}
        want = {**want, **other}
        expected |= set(other)
    assert offered == expected, (unit, case, mode, sorted(offered ^ expected))
    for k in sorted(offered):
        pe.assert_same(np.asarray(got[k]), np.asarray(want[k]), (unit, case, mode, k))
    if unit in pe.FIT_UNITS and want["skipped"] == 1:       # a skipped step: every weight byte as loaded, not only as the spec has it
        assert got["skipped"] == 1
        for k, a in pe._loaded(unit, call).items():
            pe.assert_same(np.asarray(got[k]), a, (unit, case, mode, k, "a skipped step moved a weight"))


def _actor_readers(call, want):
    """After an actor step that was taken, while the optimizer is open: policy_action without and with eps equals the spec's forward
    under the spec's updated weights AND under what actor_weights() returned (`out`); and hout's two images have not come apart -
    rc_policy_actor_forward and rc_policy_read_actor read the pair image, policy_act in mode mean reads the mean image, so the action
    policy_act writes for the env's own observation must be policy_action's for the feature it left in policy_state."""
    from policy_actor_fit_spec import KEYS, PolicyActorFitSpec
    feat = call.kw["features"]
    eps = call.kw["eps"] if call.kw["eps"] is not None else pe._inputs("action", call.rows)["eps"]

    def after(env, out):
        fitted, read = PolicyActorFitSpec({k: want[k] for k in KEYS}), PolicyActorFitSpec({k: out[k] for k in KEYS})
        for e in (None, eps):
            got = _cpu(env.policy_action(_t(env, feat), eps=_t(env, e), outputs=("action", "mean", "std")))
            for k, a in fitted.forward(feat, e).items():
                pe.assert_same(got[k], a, ("policy_action under the spec's fitted actor", k, e is not None))
            for k, a in read.forward(feat, e).items():
                pe.assert_same(got[k], a, ("policy_action under actor_weights()", k, e is not None))
        keep = env.views["action_in"].clone()
        env.set_policy_sampling("mean")
        env.policy_act()
        state = env.policy_state.clone()
        env.views["action_in"].copy_(keep)
        mode_action = _cpu(env.policy_action(state[:, :230]))["action"]
        pe.assert_same(mode_action, np.ascontiguousarray(state[:, 230:232].cpu().numpy()), "hout's mean image against its pair image")
    return after


def _reward_readers(call, want):
    """After the reward head's B1 step: policy_value's reward equals the spec under the fitted head, and one dream_ahead_grad call
    (K = 2, H = 2) equals PolicyDreamGradSpec under it - its transposed images of the head existed before the step (`_run` calls it
    once) and are made again on the stream."""
    from policy_returns_spec import PolicyReturnsSpec
    from policy_reward_fit_spec import KEYS
    feat = call.kw["features"]

    def after(env, out):
        fitted = {**call.policy, **{k: want[k] for k in KEYS}}
        got = _cpu(env.policy_value(_t(env, feat), outputs=("reward",)))["reward"]
        pe.assert_same(got, PolicyReturnsSpec(fitted, call.critic).returns(feat, None, None, 0, "mean")["reward_start"], "policy_value under the fitted head")
        dream = pe.Call(policy=fitted, **pe._inputs("dream_grad"))
        have, ref = _device(env, "dream_grad", dream, "mean", loaded=True), pe.spec("dream_grad", dream, "mean")
        for k in sorted(have):
            pe.assert_same(have[k], ref[k], ("dream_ahead_grad under the fitted head", k))
    return after


def _run(env, unit, case, mode):
    call = pe.make(unit, case)
    want = pe.spec(unit, call, mode)
    pe.check_guard(unit, case, call, want, mode)
    first = call.kw.get("first")
    if first is not None and unit not in pe.FIT_UNITS:      # case F: the larger, poisoned call on the same handle (a fit's is part of its loop)
        _load(env, unit, call)
        _device(env, unit, first, mode, loaded=True)
        got = _device(env, unit, call, mode, loaded=True)
    elif unit == "actor_fit" and want["skipped"] == 0:
        got = _device(env, unit, call, mode, after=_actor_readers(call, want))
    elif unit == "reward_fit" and case == "B1":
        _load(env, unit, call)
        _device(env, "dream_grad", pe.Call(policy=call.policy, **pe._inputs("dream_grad")), "mean", loaded=True)
        got = _device(env, unit, call, mode, loaded=True, after=_reward_readers(call, want))
    else:
        got = _device(env, unit, call, mode)
    _compare(unit, case, mode, got, want, call)
    if call.clean is not None:                              # case D3: the other 32 rows are those of the call without the poisoned row
        clean = _device(env, unit, call.clean, mode)
        for k, a in got.items():
            if np.ndim(a) and a.shape[0] == call.rows:
                assert pe.same(np.delete(a, pe.ROW, axis=0), np.delete(clean[k], pe.ROW, axis=0)), (unit, case, mode, k)
    if first is not None:                                   # case F: and the same call on a handle that never saw the first
        fresh = _new_env()
        try:
            twin = pe.make(unit, case)
            twin.kw.pop("first")
            again = _device(fresh, unit, twin, mode)
        finally:
            fresh.close()
        for k in got:
            assert pe.same(np.asarray(got[k]), np.asarray(again[k])), (unit, case, mode, k, "differs from a fresh handle")


def _params(unit):
    return [pytest.param(case, mode, id=f"{case}-{mode}") for case in pe.cases(unit) for mode in pe.UNITS[unit] if pe.applies(unit, case, mode)]


@pytest.mark.parametrize("case, mode", _params("act"))
def test_policy_act(env, case, mode):
    _run(env, "act", case, mode)


@pytest.mark.parametrize("case, mode", _params("imagine"))
def test_policy_imagine(env, case, mode):
    _run(env, "imagine", case, mode)


@pytest.mark.parametrize("case, mode", _params("observe"))
def test_policy_observe(env, case, mode):
    _run(env, "observe", case, mode)


@pytest.mark.parametrize("case, mode", _params("dream"))
def test_dream_ahead(env, case, mode):
    _run(env, "dream", case, mode)


@pytest.mark.parametrize("case, mode", _params("dream_grad"))
def test_dream_ahead_grad(env, case, mode):
    _run(env, "dream_grad", case, mode)


@pytest.mark.parametrize("case, mode", _params("returns"))
def test_policy_returns(env, case, mode):
    _run(env, "returns", case, mode)


@pytest.mark.parametrize("case, mode", _params("value"))
def test_policy_value(env, case, mode):
    _run(env, "value", case, mode)


@pytest.mark.parametrize("case, mode", _params("fit"))
def test_critic_fit(env, case, mode):
    _run(env, "fit", case, mode)


@pytest.mark.parametrize("case, mode", _params("reward_fit"))
def test_reward_fit(env, case, mode):
    _run(env, "reward_fit", case, mode)


@pytest.mark.parametrize("case, mode", _params("actor_fit"))
def test_actor_fit(env, case, mode):
    _run(env, "actor_fit", case, mode)


@pytest.mark.parametrize("case, mode", _params("action"))
def test_policy_action(env, case, mode):
    _run(env, "action", case, mode)


@pytest.mark.parametrize("case, mode", _params("decode"))
def test_policy_decode_and_loglik(env, case, mode):
    _run(env, "decode", case, mode)


@pytest.mark.parametrize("case, mode", _params("decode_lidar"))
def test_policy_decode_lidar_and_loglik(env, case, mode):
    _run(env, "decode_lidar", case, mode)


def test_the_nan_the_device_returns(env):
    """Not compared by `same`, pinned here: the bit patterns of the NaNs the device produces where the spec's x86 answer is the
    default NaN 0xffc00000 (inf - inf; a negative quiet NaN).  DESIGN.md §2 item 12 records what was seen."""
    call = pe.make("value", "C2")
    got = _device(env, "value", call, "mean")["value"]
    want = pe.spec("value", call, "mean")["value"]
    assert np.isnan(got).all() and np.isnan(want).all()
    print("device NaN bit patterns:", sorted({f"{b:08x}" for b in pe.bits(got)}), "spec:", sorted({f"{b:08x}" for b in pe.bits(want)}))
    assert all(int(b) & 0x7fc00000 == 0x7fc00000 for b in pe.bits(got))             # quiet NaNs
