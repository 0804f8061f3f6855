"""Every Dreamer unit on the device against its binary32 spec at the numeric edges (tests/policy_edge_cases.py has the recipes, the
comparison rule and the guards; tests/test_policy_edge_spec.py runs the guards on the CPU): zero and signed zero, subnormal weights,
operands, products, accumulators and Adam moments, overflow to inf and inf - inf, the +-86 clamp under a GRU scaled by 2^100, special
scan beams and raw actions, one poisoned row among 33, saturated output layers, and memory a handle keeps from a larger, poisoned
call.  The rule: NaN positions coincide, every other element has the same bytes (`same`).  One env of 33 cars - a full workgroup and
one row, so padded rows exist -, H = T = 2, K = 2; every output a call offers is compared.

Which case applies to which unit (x: run; the modes are the unit's own - act: mean / deploy / explore, the rollouts: mean / sample,
fit: value / pcont):

    case                act  imagine observe dream dream_grad returns value fit decode decode_lidar
    A-zero-layer         -      -       -      -       -         x      x    x    x       x      (1)
    A-negzero-inputs     x      x       x      x       x         x      x    x    x       x
    B1, B2 (out 2^-135,  x(2)   x       x      x(3)    x         x      x    x    x       x
            2^-120)
    B3 (Adam moments)                                                        x                   (4)
    B4 (features 2^-130)                                                x    x    x       x      (4)
    C1 (infinite norm)                                                       x(5)
    C2 (inf - inf)                                               x      x    x                   (6)
    C3 (GRU 2^100)       x      x       x      x       x         x                               (7)
    C3-inf (+-inf deter) x      x       x      x       x         x                               (7)
    D1 (beams)           x              x                                                 x      (8)
    D2 (raw actions)            x       x      x       x         x                               (8)
    D3 (poisoned row)    x      x       x      x       x         x      x    x    x       x
    D4 (fit inputs)                                                          x
    E1 (raw scale bias)                                                                   x
    E2 (+-100 biases)    x(9)                                    x      x    x(9) x
    E3 (KL)                             x
    F  (stale memory)                                  x         x           x                   (10)

 (1) the rollout units' first layer is img1: a zero kernel with a -0 bias gives ELU(-0) = +0 and the next bias takes over - the spec's
     answer is ordinary in every output, the case proves nothing there.  The heads and decoders answer with identical rows.
 (2) `mean` only: in deploy / explore the draw's noise makes the action a normal number.  (3) B1 only: the dream has no gradient and
     its rewards at 2^-120 are normal.  (4) units that take features.  (5) the value head: a sigmoid bounds the pcont head's delta.
 (6) units that read the value head.  (7) units with a GRU: C3's pre-activations are beyond +-86 but finite (2.5e31), C3-inf carries +-inf
     in the deter of four rows, so sigma and tanh meet +-inf and NaN.  (8) units that take scans / raw actions (the LiDAR decoder: its target).
 (9) act: the sampled modes (the mean does not read the raw std); fit: the pcont head.  (10) units whose handle keeps memory between
     calls: the fit's scratch, dream_ahead_grad's stash; policy_returns for its LDS rows past the last row.  The fit's first call is
     neither C2 nor D3 (an ELU takes their NaN to a finite number) but features x 2^127 with NaN targets: +inf in the activation
     planes, NaN in the delta planes; policy_edge_cases.make says what of it the smaller call's planes overlie.
 A unit has no single-row path of its own but the fit (a lone row is half a row pair): B4-one-row.

Addresses and loop bounds derived from float data - read before the first run of cases C, D and F: there are none.  The only
float -> integer conversions in the nine kernels and their shared headers are `(int32_t)n` in pm_exp_parts, where n = rint(x log2 e)
of an x that two selects have put into [-86, 86] (a NaN fails `x > -86` and becomes -86), which builds the exponent bits of 2^n, never
an address; and pm_log's exponent field, used as a number.  deploy's best-of-100 keeps an index: it starts at the lane's first
candidate (`best_i < 0 ||`), every comparison with a NaN score is false, so it stays in [0, 100) and only selects a Philox block.
Rows, columns and time steps are integers of the call.  Padded rows are selected to zero on the way in (`q < n ? x : 0`), not
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
    if unit in ("returns", "value", "fit"):
        env.load_critic(call.critic)


def _t(env, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


def _device(env, unit, call, mode, loaded=False):
    """The device's answer under the spec's output names.  Leaves the env's views as it found them."""
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
    expected = set(want) - {"m", "v"}                       # (the moments stay on the device: the weights after three steps show them)
    if unit == "fit":
        other = {k: a for k, a in call.critic.items() if not k.startswith(mode)}
        want = {**want, **other}
        expected |= set(other)
    assert offered == expected, (unit, case, mode, sorted(offered ^ expected))
    for k in sorted(offered):
        pe.assert_same(np.asarray(got[k]), np.asarray(want[k]), (unit, case, mode, k))


def _run(env, unit, case, mode):
    call = pe.make(unit, case)
    want = pe.spec(unit, call, mode)
    pe.check_guard(unit, case, call, want, mode)
    first = call.kw.get("first")
    if first is not None and unit != "fit":                 # case F: the larger, poisoned call on the same handle (the fit's is part of its loop)
        _load(env, unit, call)
        _device(env, unit, first, mode, loaded=True)
        got = _device(env, unit, call, mode, loaded=True)
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
