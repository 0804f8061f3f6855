"""The binary32 specification of the critic and the lambda-return (tests/policy_returns_spec.c): its rollout
is PolicyImagineSpec's bit for bit under the same keys; its value and pcont heads against a float64 restatement of the reference's
DenseDecoder; its returns and weights against a float64 restatement of dreamer/tools.py `lambda_return` and the cumprod of
dreamer/models.py:121-125 fed the spec's own r, v, p; the recursion's exact identities; a row's independence of batch, shard and
outputs; the tag-8 stream; racing_dreamer_amd.critic; the planners' `bootstrap` flag against a stub env; the C-ABI's new symbols.
The critic is synthetic (critic.init_critic): no shipped checkpoint holds one."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import policy_dream_spec as pds
import policy_imagine_spec as pis
import policy_returns_spec as prs
from policy_imagine_spec import PolicyImagineSpec
from policy_returns_spec import PolicyReturnsSpec
from test_golden_policy import weights
from test_policy_dream_spec import _round_f32
from test_policy_imagine_spec import WITH_HEAD, _keys
from test_policy_sample_spec import MARGIN, _inputs

f32 = np.float32
H = 15
_cache = {}


def _critic(pcont=True, seed=5):
    from racing_dreamer_amd.critic import init_critic
    return init_critic(seed, pcont=pcont)


def _spec(name, pcont=True):
    if (name, pcont) not in _cache:
        _cache[name, pcont] = PolicyReturnsSpec(weights(name), _critic(pcont))
    return _cache[name, pcont]


def _head64(critic, prefix, feat, dtype):
    """DenseDecoder((), 3, 400) (dreamer/models.py:301-318) in `dtype`: three ELU layers and the one output column."""
    elu = lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    h = np.asarray(feat, dtype)
    for i in range(3):
        h = elu(h @ np.asarray(critic[f"{prefix}_h{i}_w"], dtype) + np.asarray(critic[f"{prefix}_h{i}_b"], dtype))
    return (h @ np.asarray(critic[f"{prefix}_hout_w"], dtype) + np.asarray(critic[f"{prefix}_hout_b"], dtype))[..., 0]


def _lambda_return64(reward, value, pcont, bootstrap, lambda_):
    """dreamer/tools.py:396-418 over axis 1 of [n, T] float64 arrays: inputs = reward + pcont next_values (1 - lambda), then
    static_scan(lambda agg, cur: cur[0] + cur[1] lambda agg, reverse=True) from the bootstrap."""
    next_values = np.concatenate([value[:, 1:], bootstrap[:, None]], 1)
    inputs = reward + pcont * next_values * (1 - lambda_)
    agg, out = bootstrap, np.empty_like(reward)
    for t in range(reward.shape[1] - 1, -1, -1):
        agg = inputs[:, t] + pcont[:, t] * lambda_ * agg
        out[:, t] = agg
    return out


def _fma(a, b, c):
    """fmaf(a, b, c): the binary32 number nearest to the exact a b + c."""
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _abs_terms(r, v, p, lambda_):
    """The sum of the absolute values of the terms a return is made of, by the same recursion over absolute values."""
    r, v, p = (np.abs(x.astype(np.float64)) for x in (r, v, p))
    agg, out = v[:, -1], np.empty_like(r[:, :-1])
    for t in range(r.shape[1] - 2, -1, -1):
        agg = r[:, t] + p[:, t] * v[:, t + 1] * (1 - lambda_) + p[:, t] * lambda_ * agg
        out[:, t] = agg
    return out


@pytest.mark.parametrize("mode", ["mean", "sample"])
@pytest.mark.parametrize("name", WITH_HEAD)
def test_the_rollout_is_the_imagination_specs_bit_for_bit(name, mode):
    """Under PolicyImagineSpec's keys reward, action, feature, reward_start and the normals are PolicyImagineSpec's, closed loop
    and open loop; the critic does not enter the rollout."""
    assert len(WITH_HEAD) == 2
    _, state, _ = _inputs(name)
    keys = _keys(len(state), step=3, episode=2, first_env=7)
    acts = np.random.default_rng(2).uniform(-1.5, 1.5, (len(state), H, 2)).astype(f32)
    before = state.copy()
    for a in (None, acts):
        got = _spec(name).returns(state, keys=keys, horizon=H, mode=mode, seed=21, actions=a)
        want = PolicyImagineSpec(weights(name)).imagine(state, keys, H, mode, seed=21, actions=a)
        for k in ("reward", "action", "feature", "reward_start", "normals"):
            assert np.array_equal(got[k], want[k]), (k, a is None)
    assert np.array_equal(state, before)


def test_value_and_pcont_are_the_reference_heads():
    """value, pcont and their _start forms on the spec's own features (both checkpoints, both modes, 16 latents x 15 steps) against
    the float64 restatement of DenseDecoder (pcont: the Bernoulli's mean, sigmoid of the logit): the spec's largest error stays
    within MARGIN times that of the same restatement in float32.
    Measured (value / pcont): spec 1.5e-06 / 3.3e-07, float32 1.3e-06 / 1.0e-07, ratios 1.12 / 3.20."""
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    err_spec, err_f32 = np.zeros(2), np.zeros(2)
    critic = _critic()
    for name in WITH_HEAD:
        _, state, _ = _inputs(name)
        for mode in ("mean", "sample"):
            got = _spec(name).returns(state, keys=_keys(len(state)), horizon=H, mode=mode, seed=3)
            feat = np.concatenate([state[:, None, :230], got["feature"]], 1)
            mine = (np.concatenate([got["value_start"][:, None], got["value"]], 1), np.concatenate([got["pcont_start"][:, None], got["pcont"]], 1))
            for j, (prefix, fn) in enumerate((("value", lambda x: x), ("pcont", sig))):
                ref = fn(_head64(critic, prefix, feat, np.float64))
                r32 = fn(_head64(critic, prefix, feat, f32))
                err_spec[j] = max(err_spec[j], np.abs(mine[j] - ref).max())
                err_f32[j] = max(err_f32[j], np.abs(r32 - ref).max())
            assert 0.8 < got["pcont"].min() and got["pcont"].max() < 0.99 and np.abs(got["value"]).max() > 0.05
    print("largest error against float64 (value, pcont): spec", err_spec, "float32", err_f32, "ratio", err_spec / err_f32)
    assert np.all(err_f32 > 0) and np.all(err_spec <= MARGIN * err_f32), (err_spec, err_f32)


@pytest.mark.parametrize("pcont", [True, False])
def test_returns_and_weights_are_the_reference_recursion(pcont):
    """returns against the float64 restatement of tools.lambda_return (reward[:-1], value[:-1], pcont[:-1], bootstrap value[-1])
    and weight against cumprod([1, pcont[:-2]]), both fed the spec's own r, v, p, for H in {2, 3, 15, 64} and lambda in {0, 0.95,
    1}.  A return is a sum of products of at most H - 1 factors p lambda with an r, a p v (1 - lambda) or the bootstrap; every
    binary32 step of the recursion rounds once or twice, fewer than 64 steps lie above any term, so the error is at most
    64 x 2^-24 of the sum of the terms' absolute values.  A weight is a product of at most 63 factors: 64 x 2^-24 of itself."""
    name = WITH_HEAD[0]
    _, state, _ = _inputs(name)
    worst = 0.0
    for h in (2, 3, 15, 64):
        for lam in (0.0, 0.95, 1.0):
            got = _spec(name, pcont).returns(state, keys=_keys(len(state)), horizon=h, mode="sample", seed=8, lambda_=lam, discount=0.99)
            r, v, p = (got[k].astype(np.float64) for k in ("reward", "value", "pcont"))
            lam64 = float(f32(lam))
            want = _lambda_return64(r[:, :-1], v[:, :-1], p[:, :-1], v[:, -1], lam64)
            bound = 64 * 2.0 ** -24 * _abs_terms(got["reward"], got["value"], got["pcont"], lam64)
            err = np.abs(got["returns"] - want)
            worst = max(worst, float((err / bound).max()))
            assert got["returns"].shape == (len(state), h - 1) and np.all(err <= bound), (h, lam, float((err / bound).max()))
            weight = np.cumprod(np.concatenate([np.ones_like(p[:, :1]), p[:, :-2]], 1), 1)
            assert got["weight"].shape == weight.shape and np.all(np.abs(got["weight"] - weight) <= 64 * 2.0 ** -24 * weight)
            assert np.array_equal(got["returns"], prs.lambda_return(got["reward"], got["value"], got["pcont"], lam)[0])
    print(f"pcont head {pcont}: largest error of a return over its bound {worst:.3f}")


def test_exact_identities():
    """lambda = 0: R_t = fmaf(p_t v_{t+1}, 1, r_t), the correctly rounded r_t + fl(p_t v_{t+1}); H = 2: one step from the bootstrap;
    no pcont head: weight[t] is the repeated binary32 product of `discount` and pcont the constant; discount = 0 without a pcont
    head: returns == reward[:, :-1] exactly."""
    name = WITH_HEAD[0]
    _, state, _ = _inputs(name)
    keys = _keys(len(state))
    got = _spec(name).returns(state, keys=keys, horizon=5, mode="sample", seed=2, lambda_=0.0)
    r, v, p = got["reward"], got["value"], got["pcont"]
    pv = (p[:, :-1] * v[:, 1:]).astype(f32)
    for i in range(len(state)):
        for t in range(4):
            assert got["returns"][i, t] == _fma(pv[i, t], f32(1.0), r[i, t]), (i, t)
    two = _spec(name).returns(state, keys=keys, horizon=2, mode="sample", seed=2, lambda_=0.95)
    lam = f32(0.95)
    assert two["returns"].shape == (len(state), 1) and np.all(two["weight"] == 1.0)
    for i in range(len(state)):
        r0, p0, v1 = two["reward"][i, 0], two["pcont"][i, 0], two["value"][i, 1]
        inner = _fma(f32(p0 * v1), f32(f32(1.0) - lam), r0)
        assert two["returns"][i, 0] == _fma(f32(p0 * lam), v1, inner), i
    const = _spec(name, False).returns(state, keys=keys, horizon=6, mode="mean", discount=0.97)
    w = np.ones(len(state), f32)
    for t in range(5):
        assert np.array_equal(const["weight"][:, t], w)
        w = w * f32(0.97)
    assert np.all(const["pcont"] == f32(0.97)) and "pcont_start" not in const
    zero = _spec(name, False).returns(state, keys=keys, horizon=6, mode="mean", discount=0.0)
    assert np.array_equal(zero["returns"], zero["reward"][:, :-1]) and np.abs(zero["reward"]).max() > 1e-3
    assert np.all(zero["weight"][:, 0] == 1.0) and not zero["weight"][:, 1:].any()


def test_a_row_does_not_depend_on_the_batch_the_shard_or_the_horizon_outputs():
    """Given states: a row's outputs are the same alone, in a batch, in a shard that passes its ids (row_offset + row, also beyond
    2^32) or in another order; other ids give other draws.  The stream is tag 8, keyed by (id, t): not imagination's, not
    planning's."""
    name = WITH_HEAD[0]
    _, state, _ = _inputs(name)
    n = len(state)
    ids = (1 << 33) + 11 + np.arange(n, dtype=np.uint64)
    full = _spec(name).returns(state, ids=ids, horizon=4, mode="sample", seed=9)
    order = np.random.default_rng(1).permutation(n)
    for rows in (np.array([5]), np.arange(5, n), order):
        part = _spec(name).returns(state[rows], ids=ids[rows], horizon=4, mode="sample", seed=9)
        for k in full:
            assert np.array_equal(part[k], full[k][rows]), k
    other = _spec(name).returns(state[5:], horizon=4, mode="sample", seed=9)
    assert not np.array_equal(other["returns"], full["returns"][5:])
    base = prs.normals(int(ids[5]), 1, 0, 9, 9)
    assert np.array_equal(base, full["normals"][5, 1])
    for sid, t, seed in ((int(ids[5]) + 1, 1, 9), (int(ids[5]) - (1 << 33), 1, 9), (int(ids[5]), 2, 9), (int(ids[5]), 1, 10)):
        assert not np.any(prs.normals(sid, t, 0, 9, seed) == base)
    assert not np.any(prs.normals(3, 1, 0, 8, 9) == pis.normals((3, 0, 0, 0), 1, 0, 8, 9))
    assert not np.any(prs.normals(3, 1, 0, 8, 9) == pds.normals(3, 0, 1, 0, 8, 9))
    # open loop draws no action block
    acts = np.zeros((n, 4, 2), f32)
    assert not _spec(name).returns(state, ids=ids, horizon=4, mode="sample", seed=9, actions=acts)["normals"][:, :, 32:].any()


def test_init_critic_and_critic_from_variables():
    """init_critic: Glorot-uniform weights, zero biases, the pcont bias; deterministic under its seed.  critic_from_variables picks
    the sixteen (or eight) arrays behind the reward head out of a variables.pkl-ordered list and checks their shapes."""
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.critic import critic_from_variables, init_critic
    c = init_critic(3)
    assert tuple(c) == L.VALUE_KEYS + L.PCONT_KEYS and all(v.dtype == f32 for v in c.values())
    assert c["value_h0_w"].shape == (230, 400) and c["pcont_hout_w"].shape == (400, 1) and c["value_hout_b"].shape == (1,)
    assert np.abs(c["value_h1_w"]).max() <= np.sqrt(6 / 800) and np.abs(c["value_h1_w"]).max() > 0.9 * np.sqrt(6 / 800)
    assert not c["value_h2_b"].any() and c["pcont_hout_b"][0] == 3.0 and not c["value_hout_b"].any()
    assert all(np.array_equal(c[k], init_critic(3)[k]) for k in c) and not np.array_equal(c["value_h0_w"], init_critic(4)["value_h0_w"])
    assert tuple(init_critic(3, pcont=False)) == L.VALUE_KEYS
    rng = np.random.default_rng(0)
    shapes = [(230, 400), (400,), (400, 400), (400,), (400, 400), (400,), (400, 1), (1,)]
    rssm = [rng.normal(size=s).astype(f32) for s in ((200, 600), (2, 600), (32, 200), (200,))]
    reward = [rng.normal(size=s).astype(f32) for s in ((230, 400), (400,), (400, 400), (400,), (400, 1), (1,))]
    pcont, value = ([rng.normal(size=s).astype(f32) for s in shapes] for _ in range(2))
    actor = [rng.normal(size=s).astype(f32) for s in ((230, 400), (400,), (400, 4), (4,))]
    got = critic_from_variables(rssm + reward + pcont + value + actor)
    assert all(np.array_equal(got[k], a) for k, a in zip(L.PCONT_KEYS, pcont)) and all(np.array_equal(got[k], a) for k, a in zip(L.VALUE_KEYS, value))
    alone = critic_from_variables(rssm + reward + value + actor)
    assert tuple(alone) == L.VALUE_KEYS and np.array_equal(alone["value_hout_b"], value[7])
    with pytest.raises(ValueError):
        critic_from_variables(rssm + actor)
    with pytest.raises(ValueError):
        critic_from_variables(rssm + reward + actor)
    assert PolicyReturnsSpec(weights(WITH_HEAD[0]), got).has_pcont


class _StubEnv:
    """One car per env; the dream's return of a candidate is minus its squared distance from a goal, the final feature carries the
    candidate's last action, and the value head reads it: torch functions with known answers, every call recorded."""

    def __init__(self, E, goal, value_goal):
        import torch
        self.num_envs, self.cars_per_env, self.n_cars, self.device = E, 1, E, torch.device("cpu")
        self.views = {"action_in": torch.full((E, 1, 2), 0.25)}
        self.goal = torch.as_tensor(goal, dtype=torch.float32).reshape(E, 1, 1, 2)
        self.value_goal = torch.as_tensor(value_goal, dtype=torch.float32).reshape(E, 1, 2)
        self.policy_has_reward_head = self.policy_has_value_head = True
        self.calls = []

    def dream_ahead(self, actions, **kw):
        import torch
        self.calls.append(("dream", dict(kw)))
        out = {"return": -((actions.clamp(-1, 1) - self.goal) ** 2).sum(dim=(2, 3))}
        if "final_feature" in kw.get("outputs", ()):
            out["final_feature"] = torch.nn.functional.pad(actions[:, :, -1], (0, 228))
        return out

    def policy_value(self, features=None, slots=None, outputs=("value",)):
        self.calls.append(("value", tuple(features.shape)))
        return {"value": -100.0 * ((features[..., :2] - self.value_goal) ** 2).sum(-1)}


def test_the_planners_bootstrap_flag():
    """Flag off: dream_shooting_act and dream_cem_act make the calls they always made - dream_ahead with `slots` (shooting) or
    nothing (CEM) and outputs ("return",), no discount, no policy_value.  Flag on: one dream_ahead with the discount and the final
    feature, one policy_value on it, and the choice follows return + discount^H value."""
    import torch
    from racing_dreamer_amd.planning import dream_cem_act, dream_shooting_act
    E, K, Hs = 2, 3, 2
    seq = torch.zeros((E, K, Hs, 1, 2))
    seq[:, 0] = 0.5                                       # the dream's favourite: on the goal
    seq[:, 1] = 0.4                                       # a little off the goal, but it ends where the value head wants it
    seq[:, 2] = -0.9
    env = _StubEnv(E, torch.full((E, 2), 0.5), torch.full((E, 2), 0.4))
    out = dream_shooting_act(env, seq)
    assert env.calls == [("dream", dict(slots=None, outputs=("return",)))] and torch.equal(out, torch.full((E, 1, 2), 0.5))
    env.calls.clear()
    out = dream_shooting_act(env, seq, slots=(0,), bootstrap=True, discount=0.9)
    assert env.calls == [("dream", dict(slots=(0,), discount=0.9, outputs=("return", "final_feature"))), ("value", (E, K, 230))]
    assert torch.equal(out, torch.full((E, 1, 2), 0.4))
    env.calls.clear()
    dream_cem_act(env, candidates=8, horizon=3, iterations=2, elites=2, seed=1)
    assert env.calls == [("dream", dict(outputs=("return",)))] * 2
    env.calls.clear()
    dream_cem_act(env, candidates=8, horizon=3, iterations=2, elites=2, seed=1, bootstrap=True)
    assert [c[0] for c in env.calls] == ["dream", "value"] * 2 and env.calls[0][1] == dict(discount=0.99, outputs=("return", "final_feature"))
    env.policy_has_value_head = False
    with pytest.raises(RuntimeError, match="value head"):
        dream_shooting_act(env, seq, bootstrap=True)


def test_returns_symbols_structs_and_refusals_without_a_handle(hip_lib):
    """The header's new symbols are bound; the ctypes structs have the header's fields in order; rc_policy_load_critic checks
    struct_size and shapes before it looks at the handle and names the first wrong array; the new kernels are among those the
    build refuses to ship with a spill; the unit is part of the build."""
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd import build
    for name in ("rc_policy_load_critic", "rc_policy_returns"):
        assert name in L.SYMBOLS and hasattr(hip_lib, name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "racecar_hip.h")).read()
    for struct, cls in (("rc_policy_returns_args", L.RcPolicyReturnsArgs), ("rc_policy_critic", L.RcPolicyCritic)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n for decl in body.split(";") for n in re.findall(r"\*?(\w+)", re.sub(r"^.*?\s(?=\*?\w+(\s*,|\s*$))", "", decl.strip(), flags=re.S))]
        assert fields == [f[0] for f in cls._fields_], struct
    assert C.sizeof(L.RcPolicyReturnsArgs) == 144 and C.sizeof(L.RcPolicyCritic) == 8 + 16 * 16
    critic, keep = L.policy_critic(_critic())
    assert hip_lib.rc_policy_load_critic(None, C.byref(critic)) == -1 and b"env is NULL" in hip_lib.rc_last_error()
    assert hip_lib.rc_policy_load_critic(None, None) == -1 and b"env is NULL" in hip_lib.rc_last_error()
    critic.struct_size = 8
    assert hip_lib.rc_policy_load_critic(None, C.byref(critic)) == -1 and b"struct_size" in hip_lib.rc_last_error()
    bad = _critic()
    bad["value_h1_w"] = np.zeros((400, 399), f32)
    bad["pcont_hout_w"] = np.zeros((400, 2), f32)
    critic, keep = L.policy_critic(bad)
    assert hip_lib.rc_policy_load_critic(None, C.byref(critic)) == -1 and b"value_h1_w has shape [400, 399]" in hip_lib.rc_last_error()
    bad = _critic()
    bad["pcont_h0_b"] = np.zeros(401, f32)
    critic, keep = L.policy_critic(bad)
    assert hip_lib.rc_policy_load_critic(None, C.byref(critic)) == -1 and b"pcont_h0_b has shape [1, 401]" in hip_lib.rc_last_error()
    half = _critic()
    del half["pcont_hout_b"]
    critic = L.RcPolicyCritic(C.sizeof(L.RcPolicyCritic))
    keep = L._fill_arrays(critic, half, [k for k in L.CRITIC_KEYS if k in half])
    assert hip_lib.rc_policy_load_critic(None, C.byref(critic)) == -1 and b"7 of the eight pcont_* arrays" in hip_lib.rc_last_error()
    missing = {k: v for k, v in _critic(pcont=False).items() if k != "value_h2_b"}
    critic = L.RcPolicyCritic(C.sizeof(L.RcPolicyCritic))
    keep = L._fill_arrays(critic, missing, list(missing))
    assert hip_lib.rc_policy_load_critic(None, C.byref(critic)) == -1 and b"value_h2_b is missing" in hip_lib.rc_last_error()
    assert L.policy_critic(weights(WITH_HEAD[0])) is None
    a = L.RcPolicyReturnsArgs(C.sizeof(L.RcPolicyReturnsArgs), 15, 0, 1, 0.95, 0.99)
    assert hip_lib.rc_policy_returns(None, C.byref(a)) == -1 and hip_lib.rc_policy_returns(None, None) == -1
    for k in ("rc_policy_returns_kernel", "rc_policy_returns_sampled_kernel"):
        assert k in build.NO_SPILL_KERNELS and k in build.required_kernels("shipped")
    assert "racecar_returns.hip" in build.SOURCES
