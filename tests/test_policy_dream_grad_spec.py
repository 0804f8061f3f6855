"""The binary32 specification of the dream's backward pass (tests/policy_dream_grad_spec.c): the NumPy
restatement of forward and backward against central differences of its own float64 forward; the spec against that float64
restatement, as close as a plain float32 restatement gets; the clamp's exact zeros; the forward's identity with PolicyDreamSpec;
H = 1 and discount 0; the C-ABI's new symbol; `planning.dream_gradient_act` against a stub env with a quadratic return."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from policy_dream_grad_spec import PolicyDreamGradSpec, restated
from policy_dream_spec import PolicyDreamSpec
from test_golden_policy import weights
from test_policy_observe_spec import WITH_HEAD, _recorded
from test_policy_observe_spec import _spec as observe_spec

f32, f64 = np.float32, np.float64
MODES = ("mean", "sample")
H, DISCOUNT, SEED = 15, 0.99, 5
# spec error <= MARGIN x float32 error per output, both against the float64 restatement (max |x - float64| over the array, 64 rows x
# 1 candidate, H = 15, discount 0.99): MARGIN = 2 x the largest ratio measured on these fixed inputs over (checkpoint, mode), the
# rule of item 21.  Measured ratios, austria mean / sample, treitlstrasse mean / sample:
#   grad_actions  0.53 / 2.68, 0.10 / 1.50
#   grad_state    1.46 / 2.14, 0.10 / 0.85
#   return        1.54 / 2.21, 0.82 / 1.09
#   reward        0.99 / 2.47, 0.67 / 0.68
# austria in `sample` is the one case above x 1.6, in the forward (`reward`, item 19's arithmetic unchanged) as much as in the
# backward: its sampled rollouts amplify a rounding difference of either restatement ~40-fold over 15 steps (errors of 3e-5
# against 1e-6 in `mean`), and the ratio of two such amplified errors is a draw.  Relative to the largest entry the spec is off by
# 3.6e-5 there (grad_actions), 2.8e-6 in austria `mean`.
MARGIN = {"grad_actions": 2 * 2.68, "grad_state": 2 * 2.14, "return": 2 * 2.21, "reward": 2 * 2.47}


@functools.lru_cache(maxsize=None)
def _gspec(name):
    return PolicyDreamGradSpec(weights(name))


@functools.lru_cache(maxsize=None)
def _latents(name):
    """[64, 232]: posterior latents of the checkpoint's recorded closed-loop run - policy_observe's spec in mode `sample`, steps 3, 6,
    9 and 12 of its 16 windows, as item 22's test takes its features.  Read only."""
    scan, act, _ = _recorded(name)
    feat = observe_spec(name).observe(scan, act, mode="sample", seed=1)["feature"]
    st = np.zeros((64, 232), f32)
    st[:, :230] = feat[:, 3:13:3].reshape(64, 230)
    st.setflags(write=False)
    return st


def _actions(s, k, h, seed=2):
    """[s, k, h, 2], a third of the entries beyond +-1."""
    return np.random.default_rng(seed).uniform(-1.5, 1.5, (s, k, h, 2)).astype(f32)


@functools.lru_cache(maxsize=None)
def _case(name, mode):
    """(state, actions, normals, the spec's outputs) of the 64-row case; computed once, read only."""
    state, acts = _latents(name), _actions(64, 1, H, seed=11)
    got = _gspec(name).dream_grad(state, acts, None, mode, seed=SEED, discount=DISCOUNT)
    nrm = PolicyDreamSpec(weights(name)).dream(state, acts, None, mode, seed=SEED, discount=DISCOUNT)["normals"]
    for v in list(got.values()) + [acts, nrm]:
        v.setflags(write=False)
    return state, acts, nrm, got


@pytest.mark.parametrize("mode", MODES)
def test_the_restatement_agrees_with_central_differences(mode):
    """The float64 restatement's backward against central differences (eps = 1e-6) of its own forward: per probed row, 3 action
    entries inside the clamp at each of t = 0, the middle and H - 1 (9 >= 8) and 8 start-latent entries (stoch and deter), to 1e-6 of
    the row's largest gradient entry."""
    name = WITH_HEAD[0]
    state, acts, nrm, _ = _case(name, mode)
    w = weights(name)
    rows = (0, 21, 63)
    st, ac, nr = state[list(rows)].astype(f64), acts[list(rows)].astype(f64), nrm[list(rows)]
    full = restated(w, st, ac, nr, mode, DISCOUNT, f64)
    eps, checked_a, checked_s = 1e-6, 0, 0
    for i in range(len(rows)):
        scale = max(np.abs(full["grad_actions"][i]).max(), np.abs(full["grad_state"][i]).max())
        assert scale > 0

        def ret_of(s1, a1):
            return restated(w, s1[None], a1[None], nr[i:i + 1], mode, DISCOUNT, f64, backward=False)["return"][0, 0]

        for t in (0, H // 2, H - 1):
            inside = [(t, j) for j in range(2) if abs(ac[i, 0, t, j]) < 1.0 - 1e-3]
            for (tt, j) in inside + ([] if len(inside) == 2 else [(t + (1 if t == 0 else -1), 0)]):
                if abs(ac[i, 0, tt, j]) >= 1.0 - 1e-3:
                    continue
                up, dn = ac[i].copy(), ac[i].copy()
                up[0, tt, j] += eps
                dn[0, tt, j] -= eps
                fd = (ret_of(st[i], up) - ret_of(st[i], dn)) / (2 * eps)
                assert abs(fd - full["grad_actions"][i, 0, tt, j]) <= 1e-6 * scale, (mode, i, tt, j, fd, full["grad_actions"][i, 0, tt, j])
                checked_a += 1
        for col in (0, 7, 29, 30, 31, 100, 177, 229):
            up, dn = st[i].copy(), st[i].copy()
            up[col] += eps
            dn[col] -= eps
            fd = (ret_of(up, ac[i]) - ret_of(dn, ac[i])) / (2 * eps)
            assert abs(fd - full["grad_state"][i, 0, col]) <= 1e-6 * scale, (mode, i, col, fd, full["grad_state"][i, 0, col])
            checked_s += 1
    assert checked_a >= 8 and checked_s >= 8


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", WITH_HEAD)
def test_the_spec_is_as_close_to_float64_as_float32_can_be(name, mode):
    """64 rows, H = 15, posterior latents of the recorded run: every output of the spec against the float64 restatement within
    MARGIN x the error of the plain float32 restatement."""
    assert len(WITH_HEAD) == 2
    state, acts, nrm, got = _case(name, mode)
    w = weights(name)
    ref = restated(w, state, acts, nrm, mode, DISCOUNT, f64)
    own = restated(w, state, acts, nrm, mode, DISCOUNT, f32)
    missed = []
    for key in ("grad_actions", "grad_state", "return", "reward"):
        assert own[key].dtype == f32
        spec_err = float(np.abs(got[key].astype(f64) - ref[key]).max())
        f32_err = float(np.abs(own[key].astype(f64) - ref[key]).max())
        print(f"{name} {mode} {key}: spec {spec_err:.3e} float32 {f32_err:.3e} ratio {spec_err / max(f32_err, 1e-300):.2f} "
              f"largest {float(np.abs(ref[key]).max()):.3e}")
        assert f32_err > 0
        if not spec_err <= MARGIN[key] * f32_err:
            missed.append((name, mode, key, spec_err, f32_err))
    assert not missed, missed


@pytest.mark.parametrize("mode", MODES)
def test_the_clamp_passes_inside_and_gives_positive_zero_outside(mode):
    """grad_actions is +0.0f by bit pattern wherever |raw action| > 1 and non-zero somewhere inside; an action at exactly +-1
    passes its gradient (the inclusive range of tf.clip_by_value)."""
    name = WITH_HEAD[0]
    state = _latents(name)[:4]
    acts = _actions(4, 3, 5, seed=4)
    acts[0, 0, 0] = (1.0, -1.0)
    acts[1, 1, 2] = (-1.0, 1.0)
    got = _gspec(name).dream_grad(state, acts, None, mode, seed=3, discount=DISCOUNT)["grad_actions"]
    outside = np.abs(acts) > 1.0
    assert outside.any() and not outside.all()
    assert not got.view(np.uint32)[outside].any()
    assert np.all(got[~outside] != 0.0)
    assert np.all(got[0, 0, 0] != 0.0) and np.all(got[1, 1, 2] != 0.0)
    # the edge is the clamp's, not the gradient's: just inside +-1 the same row has nearly the same gradient
    near = acts.copy()
    near[0, 0, 0] = (np.nextafter(f32(1), f32(0)), np.nextafter(f32(-1), f32(0)))
    other = _gspec(name).dream_grad(state[:1], near[:1], None, mode, seed=3, discount=DISCOUNT)["grad_actions"]
    assert np.allclose(other[0, 0, 0], got[0, 0, 0], rtol=1e-3, atol=1e-7)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", WITH_HEAD)
def test_the_forward_is_the_dreams_bit_for_bit(name, mode):
    """`return` and `reward` of the gradient's spec are PolicyDreamSpec.dream's, bit for bit, with ids beyond 2^32."""
    state = _latents(name)[:5]
    acts = _actions(5, 3, 4, seed=8)
    ids = np.array([7, 8, (1 << 33) + 1, 9, 10], np.uint64)
    for discount in (1.0, 0.99):
        got = _gspec(name).dream_grad(state, acts, ids, mode, seed=12, discount=discount)
        want = PolicyDreamSpec(weights(name)).dream(state, acts, ids, mode, seed=12, discount=discount)
        assert got["return"].tobytes() == want["return"].tobytes() and got["reward"].tobytes() == want["reward"].tobytes()


def test_horizon_one_and_discount_zero():
    """H = 1: no recurrence is involved, grad_state's deter part is non-zero (through the GRU's z h term and gru_recurrent) and
    equals the float64 restatement to float32 accuracy.  Discount 0: only step 0's reward contributes, so grad_actions[t >= 1] is
    exactly zero while grad_actions[0] is not."""
    name = WITH_HEAD[0]
    state = _latents(name)[:6]
    w = weights(name)
    acts = np.random.default_rng(3).uniform(-0.9, 0.9, (6, 2, 1, 2)).astype(f32)
    one = _gspec(name).dream_grad(state, acts, None, "mean", discount=DISCOUNT)
    assert np.all(np.abs(one["grad_state"][..., 30:]).max(axis=-1) > 0) and np.all(np.abs(one["grad_state"][..., :30]).max(axis=-1) > 0)
    ref = restated(w, state, acts, None, "mean", DISCOUNT, f64)
    assert np.abs(one["grad_state"] - ref["grad_state"]).max() <= 1e-5 * np.abs(ref["grad_state"]).max()
    assert np.abs(one["grad_actions"] - ref["grad_actions"]).max() <= 1e-5 * np.abs(ref["grad_actions"]).max()
    acts = np.random.default_rng(4).uniform(-0.9, 0.9, (6, 2, 4, 2)).astype(f32)
    for mode in MODES:
        zero = _gspec(name).dream_grad(state, acts, None, mode, seed=2, discount=0.0)
        assert not zero["grad_actions"][:, :, 1:].any() and np.all(zero["grad_actions"][:, :, 0] != 0.0)
        assert np.array_equal(zero["return"], zero["reward"][:, :, 0])


def test_abi_symbol_and_struct(hip_lib):
    """rc_policy_dream_grad is declared, exported and bound on a box without a GPU; the ctypes struct has the header's fields in
    order and its size; the paths that need no device refuse; rc_policy_dream_ahead_args and the ABI version are what they were."""
    import os
    from racing_dreamer_amd import _lib as L
    assert "rc_policy_dream_grad" in L.SYMBOLS and hasattr(hip_lib, "rc_policy_dream_grad")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "racecar_hip.h")).read()
    body = re.search(r"typedef struct rc_policy_dream_grad_args \{(.*?)\} rc_policy_dream_grad_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"\*?(\w+)\s*$", decl.strip())]
    assert fields == [f[0] for f in L.RcPolicyDreamGradArgs._fields_] and fields[0] == "struct_size"
    # 6 x 4 bytes, 4 x 8 bytes, 6 pointers
    assert C.sizeof(L.RcPolicyDreamGradArgs) == 24 + 32 + 48
    assert set(L.DREAM_GRAD_OUTPUTS) == {"grad_actions", "grad_state", "return", "reward"}
    assert hip_lib.rc_policy_dream_grad(None, None) == -1 and b"NULL" in hip_lib.rc_last_error()
    a = L.RcPolicyDreamGradArgs(C.sizeof(L.RcPolicyDreamGradArgs), 15, 0, 4, 1, 0.99, 0, 0, 0, 0)
    assert hip_lib.rc_policy_dream_grad(None, C.byref(a)) == -1 and b"NULL" in hip_lib.rc_last_error()
    assert C.sizeof(L.RcPolicyDreamAheadArgs) == 88
    assert hip_lib.rc_abi_version() == 3
    assert re.search(r"RC_K_COUNT = 7\b", header)
    from racing_dreamer_amd import build
    assert "racecar_dream_grad.hip" in build.SOURCES
    assert {"rc_policy_dream_grad_kernel", "rc_policy_dream_grad_sampled_kernel"} <= set(build.required_kernels("shipped"))


# ---- dream_gradient_act against a stub env whose dream is a torch function with a known gradient
class _QuadraticEnv:
    """E envs of A cars; a step's reward is -(a0 - goal0)^2 - (a1 - goal1)^2 with a goal per car, discounted; the gradient is
    autograd-free: -2 discount^t (clamp(a) - goal) inside the clamp, zero outside."""

    def __init__(self, E, A, goal):
        import torch
        self.num_envs, self.cars_per_env, self.n_cars, self.device = E, A, E * A, torch.device("cpu")
        self.views = {"action_in": torch.full((E, A, 2), 0.25)}
        self.goal = torch.as_tensor(goal, dtype=torch.float32).reshape(E * A, 1, 1, 2)
        self.policy_has_reward_head = True
        self.calls = []

    def _keep(self, slots):
        import torch
        if slots is None:
            return torch.ones(self.n_cars, dtype=torch.bool)
        return torch.tensor([a in slots for a in range(self.cars_per_env)]).repeat(self.num_envs)

    def _ret(self, actions, discount):
        import torch
        w = float(discount) ** torch.arange(actions.shape[2], dtype=torch.float32).reshape(1, 1, -1, 1)
        return -(w * (actions.clamp(-1, 1) - self.goal) ** 2).sum(dim=(2, 3)), w

    def dream_ahead(self, actions, mode="mean", seed=0, state=None, row_offset=0, slots=None, discount=1.0, outputs=("return",), out=None):
        import torch
        assert tuple(outputs) == ("return",) and mode == "mean" and state is None
        self.calls.append(("dream", slots, actions.clone()))
        ret, _ = self._ret(actions, discount)
        return {"return": torch.where(self._keep(slots)[:, None], ret, torch.zeros_like(ret))}

    def dream_ahead_grad(self, actions, mode="mean", seed=0, state=None, row_offset=0, slots=None, discount=1.0,
                         outputs=("grad_actions", "return"), out=None, chunk_rows=0):
        import torch
        assert tuple(outputs) == ("grad_actions", "return") and mode == "mean" and state is None and chunk_rows == 0
        self.calls.append(("grad", slots, actions.clone()))
        ret, w = self._ret(actions, discount)
        g = -2.0 * w * (actions.clamp(-1, 1) - self.goal)
        g = torch.where((actions >= -1) & (actions <= 1), g, torch.zeros_like(g))
        keep = self._keep(slots)
        return {"return": torch.where(keep[:, None], ret, torch.zeros_like(ret)),
                "grad_actions": torch.where(keep[:, None, None, None], g, torch.zeros_like(g))}


def test_dream_gradient_act_on_a_quadratic_dream():
    """Iterates move toward the optimum; the best iterate seen is kept (a step so large that later iterates overshoot and score
    worse does not lose it); the chosen return is never below the initial best; only the first action is written; `slots` is
    respected; a checkpoint without a head is refused."""
    import torch
    from racing_dreamer_amd.planning import dream_gradient_act, dream_shooting_act, first_best, shooting_candidates, to_dream_actions
    E, A, K, Hh = 3, 2, 4, 5
    goal = torch.tensor([[0.5, 0.5], [-0.5, 0.0], [0.0, 0.0], [0.5, -0.9], [0.3, 0.3], [-0.7, 0.6]])
    env = _QuadraticEnv(E, A, goal)
    cand = shooting_candidates(env, K, Hh, 2, 5)
    info = {}
    out = dream_gradient_act(env, candidates=K, horizon=Hh, iterations=10, step=0.1, hold=2, seed=5, discount=0.9, info=info)
    assert out is env.views["action_in"]
    kinds = [c[0] for c in env.calls]
    assert kinds == ["grad"] * 10 + ["dream"] and torch.equal(env.calls[0][2], to_dream_actions(cand))
    # iterates move toward the optimum: the distance of every sequence to its goal shrinks from call to call until it is there
    dist = [float(((c[2].clamp(-1, 1) - env.goal) ** 2).sum()) for c in env.calls]
    print("distance to the goals per call:", [round(d, 3) for d in dist])
    assert all(b < a for a, b in zip(dist[:4], dist[1:4])) and dist[-1] < 0.5 * dist[0]
    first_ret = env._ret(to_dream_actions(cand), 0.9)[0]
    assert torch.equal(info["initial_return"], first_ret)
    assert bool((info["return"] >= first_ret.max(dim=1).values).all()) and bool((info["return"] > first_ret.max(dim=1).values).any())
    assert torch.equal(env._ret(info["actions"][:, None], 0.9)[0][:, 0], info["return"])
    assert torch.equal(out.reshape(E * A, 2), info["actions"][:, 0])                  # the first action, nothing else
    # never below dream_shooting_act's choice among the same candidates under the same discount
    shoot = _QuadraticEnv(E, A, goal)
    dream_shooting_act(shoot, cand)
    acts0 = to_dream_actions(cand)
    picked = acts0[torch.arange(E * A), first_best(env._ret(acts0, 1.0)[0])]
    assert torch.equal(shoot.views["action_in"].reshape(-1, 2), picked[:, 0])
    assert bool((info["return"] >= env._ret(picked[:, None], 0.9)[0][:, 0]).all())
    # the best iterate is kept: with a huge step the iterates jump between the clamp's walls and never beat the start again where
    # the start is good - one candidate is the goal itself
    env = _QuadraticEnv(E, A, goal)
    seq = cand.clone()
    seq[:, 1] = goal.reshape(E, 1, A, 2)
    info = {}
    dream_gradient_act(env, seq, iterations=3, step=5.0, discount=0.9, info=info)
    assert torch.equal(info["return"], torch.zeros(E * A)) and torch.equal(info["actions"], goal.reshape(E * A, 1, 2).expand(E * A, Hh, 2))
    assert torch.equal(env.views["action_in"].reshape(-1, 2), goal)
    # iterations = 0 is dream_shooting_act under the same discount
    env = _QuadraticEnv(E, A, goal)
    dream_gradient_act(env, cand, iterations=0, discount=0.9)
    assert [c[0] for c in env.calls] == ["dream"]
    best = first_ret.argmax(dim=1)
    assert torch.equal(env.views["action_in"].reshape(-1, 2), to_dream_actions(cand)[torch.arange(E * A), best, 0])
    # slots: only slot 1's cars are planned for and written
    env = _QuadraticEnv(E, A, goal)
    out = dream_gradient_act(env, candidates=K, horizon=Hh, iterations=2, hold=2, seed=5, slots=(1,))
    assert all(c[1] == (1,) for c in env.calls)
    assert torch.equal(out[:, 0], torch.full((E, 2), 0.25)) and not torch.equal(out[:, 1], torch.full((E, 2), 0.25))
    env.policy_has_reward_head = False
    with pytest.raises(RuntimeError):
        dream_gradient_act(env, 4, 3)
    with pytest.raises(ValueError):
        dream_gradient_act(_QuadraticEnv(E, A, goal), 4, 3, step=0.0)
