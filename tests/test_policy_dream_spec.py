"""The binary32 specification of planning in the latent (tests/policy_dream_spec.c): in `mean` mode it is
PolicyImagineSpec's open-loop rollout of every candidate from the replicated start, bit for bit, and its return is the fmaf
recurrence over those rewards; the properties of its tag-7 random stream; the planners of racing_dreamer_amd/planning.py and
`world_model.dream_vs_truth` against a stub env whose dream and simulator are torch functions with known answers; the C-ABI's new
symbol."""
import ctypes as C
import re
from fractions import Fraction

import numpy as np
import pytest

import policy_dream_spec as pds
import policy_observe_spec as pos
import policy_sample_spec as pss
from policy_dream_spec import PolicyDreamSpec
from policy_imagine_spec import PolicyImagineSpec
from test_golden_policy import weights
from test_policy_imagine_spec import WITH_HEAD
from test_policy_sample_spec import CHECKPOINTS, _inputs

f32 = np.float32


def _actions(s, k, h, seed=2):
    """[s, k, h, 2], a third of the entries beyond +-1."""
    return np.random.default_rng(seed).uniform(-1.5, 1.5, (s, k, h, 2)).astype(f32)


def _round_f32(x: Fraction) -> np.float32:
    """The binary32 number nearest to the exact x, ties to even."""
    c = f32(float(x))
    near = sorted({c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(-np.inf))}, key=lambda v: abs(Fraction(float(v)) - x))
    a, b = near[0], near[1]
    if abs(Fraction(float(a)) - x) == abs(Fraction(float(b)) - x) and (a.view(np.uint32) & 1):
        return b
    return a


@pytest.mark.parametrize("name", CHECKPOINTS)
def test_mean_mode_is_the_open_loop_rollout_of_every_candidate(name):
    """reward and final_feature of (start s, candidate k) equal PolicyImagineSpec.imagine from start s under actions[s, k], bit for
    bit; the return is acc = fmaf(w, r_t, acc), w = w * discount over those rewards: for discount 1 the plain binary32 sum in step
    order, for 0.99 the correctly rounded exact fused operation."""
    _, state, _ = _inputs(name, n=3)
    s, k, h = 3, 5, 4
    acts = _actions(s, k, h)
    spec = PolicyDreamSpec(weights(name))
    assert spec.has_head == (name in WITH_HEAD)
    rep = np.repeat(state, k, axis=0)
    want = PolicyImagineSpec(weights(name)).imagine(rep, None, h, "mean", actions=acts.reshape(s * k, h, 2), start_reward=False)
    for discount in (1.0, 0.99):
        got = spec.dream(state, acts, mode="mean", discount=discount)
        assert np.array_equal(got["final_feature"].reshape(s * k, 230), want["feature"][:, -1])
        assert not got["normals"].any()
        if not spec.has_head:
            assert "return" not in got and "reward" not in got
            continue
        assert np.array_equal(got["reward"].reshape(s * k, h), want["reward"]) and np.abs(want["reward"]).max() > 1e-3
        assert np.array_equal(got["return"], pds.discounted_return(got["reward"], discount))
        if discount == 1.0:
            acc = np.zeros(s * k, f32)
            for t in range(h):
                acc = acc + want["reward"][:, t]
            assert np.array_equal(got["return"].reshape(-1), acc)
        for q in range(s * k):
            acc, w = f32(0.0), f32(1.0)
            for t in range(h):
                acc = _round_f32(Fraction(float(w)) * Fraction(float(want["reward"][q, t])) + Fraction(float(acc)))
                w = f32(w * f32(discount))
            assert got["return"].reshape(-1)[q] == acc, (q, discount)


def test_the_stream_is_tag_7_keyed_by_start_candidate_step():
    """The normals of (start id, candidate, t): counter (id lo, id hi, candidate, block | t << 8 | 7 << 24) - restated here through
    the sampled agent's stream, whose word 3 is block | slot << 8 | 4 << 24 (7 | 4 = 7) -; other numbers for another start (also
    one that differs in the high word only), candidate, step or seed, and none of the streams of tags 5 and 6."""
    base = pds.normals(5, 3, 2, 0, 8, seed=9)
    assert np.array_equal(base, pss.normals((5, 0, 3, 0), 2 << 8 | 7 << 24, 8, 9))
    big = (1 << 40) + 5
    assert np.array_equal(pds.normals(big, 3, 2, 0, 8, seed=9), pss.normals((5, 1 << 8, 3, 0), 2 << 8 | 7 << 24, 8, 9))
    others = [pds.normals(6, 3, 2, 0, 8, 9), pds.normals(big, 3, 2, 0, 8, 9), pds.normals(5, 4, 2, 0, 8, 9), pds.normals(5, 3, 1, 0, 8, 9),
              pds.normals(5, 3, 2, 0, 8, 10), pds.normals(5, 3, 2, 0, 8, 9 + (1 << 32)), pos.normals(5, 3, 0, 8, 9), pos.normals(5, 2, 0, 8, 9)]
    for o in [base] + others:
        assert np.isfinite(o).all() and len(np.unique(o)) == 32
    for i, o in enumerate(others):
        assert not np.intersect1d(base, o).size, i
    many = np.concatenate([pds.normals(s, k, t, 0, 8, 1) for s in range(4) for k in range(8) for t in range(8)])
    assert abs(many.mean()) < 0.05 and abs(many.std() - 1.0) < 0.05


def test_a_rows_draws_do_not_depend_on_the_batch():
    """The normals and the outputs of (start id, candidate) are the same whether the spec is asked for all K candidates, for a
    range of them, for K + 1 candidates, or for one start alone under its id."""
    name = WITH_HEAD[0]
    _, state, _ = _inputs(name, n=3)
    s, k, h = 3, 4, 3
    acts = _actions(s, k + 1, h)
    ids = np.array([7, 8, (1 << 33) + 1], np.uint64)
    spec = PolicyDreamSpec(weights(name))
    full = spec.dream(state, acts[:, :k], ids, "sample", seed=12, discount=0.99)
    assert len(np.unique(full["normals"][..., :30])) == s * k * h * 30            # start, candidate and t all enter
    wider = spec.dream(state, acts, ids, "sample", seed=12, discount=0.99)
    part = spec.dream(state, acts[:, :k], ids, "sample", seed=12, discount=0.99, candidates=(1, 3))
    alone = spec.dream(state[2:], acts[2:, :k], ids[2:], "sample", seed=12, discount=0.99)
    for key, v in full.items():
        assert np.array_equal(v, wider[key][:, :k]), key
        assert np.array_equal(v[:, 1:3], part[key][:, 1:3]), key
        assert np.array_equal(v[2:], alone[key]), key
    other = spec.dream(state, acts[:, :k], ids, "sample", seed=13, discount=0.99)
    assert not np.intersect1d(full["normals"][..., :30], other["normals"][..., :30]).size
    assert not np.array_equal(full["return"], other["return"])


def test_sample_mode_moves_stoch_alone_by_std_times_normal():
    """At H = 1 the sampled deter is the mean mode's (the draw enters stoch' only).  Two candidates with the same action have
    the same prior: (stoch' - mean) / normal gives each the same std >= 0.1, to a few ulps of the fused operation."""
    name = WITH_HEAD[0]
    _, state, _ = _inputs(name, n=2)
    acts = _actions(2, 3, 1)
    acts[:, 1] = acts[:, 0]
    spec = PolicyDreamSpec(weights(name))
    mean = spec.dream(state, acts, mode="mean")
    samp = spec.dream(state, acts, mode="sample", seed=4)
    assert np.array_equal(samp["final_feature"][..., 30:], mean["final_feature"][..., 30:])
    assert np.array_equal(samp["mean"][:, :, 0], mean["final_feature"][..., :30])
    assert np.array_equal(samp["mean"][:, 0], samp["mean"][:, 1]) and np.array_equal(samp["std"][:, 0], samp["std"][:, 1])
    assert samp["std"].min() >= f32(0.1)
    n = samp["normals"][:, :, 0, :30]
    assert not np.array_equal(n[:, 0], n[:, 1])
    stoch = samp["final_feature"][..., :30].astype(np.float64)
    m, sd = samp["mean"][:, :, 0].astype(np.float64), samp["std"][:, :, 0].astype(np.float64)
    # stoch' = fl(mean + std n): its error is half an ulp of stoch', which the division by n carries into the std
    tol = 2.0 ** -23 * np.maximum(np.abs(stoch), 2.0 ** -126) / np.abs(n) + 4 * 2.0 ** -24 * sd
    assert np.all(np.abs((stoch - m) / n - sd) <= tol)


# ---- the planners and the diagnostic against a stub env with known answers
class _StubEnv:
    """E envs of A cars; the dream's reward of a step is -(a0 - goal0)^2 - (a1 - goal1)^2 with a goal per car, the simulator's the
    same around `true_goal`: torch functions, so every choice is known."""

    def __init__(self, E, A, goal, true_goal=None):
        import torch
        self.num_envs, self.cars_per_env, self.n_cars, self.device = E, A, E * A, torch.device("cpu")
        self.views = {"action_in": torch.full((E, A, 2), 0.25)}
        self.goal = torch.as_tensor(goal, dtype=torch.float32).reshape(E * A, 1, 1, 2)
        self.true_goal = self.goal if true_goal is None else torch.as_tensor(true_goal, dtype=torch.float32).reshape(E * A, 1, 1, 2)
        self.policy_has_reward_head = True
        self.calls = []

    def dream_ahead(self, actions, mode="mean", seed=0, state=None, row_offset=0, slots=None, discount=1.0, outputs=("return",), out=None):
        import torch
        assert tuple(actions.shape[::3]) == (self.n_cars, 2) and tuple(outputs) == ("return",) and mode == "mean" and state is None
        self.calls.append(("dream", slots, actions.clone()))
        ret = -((actions.clamp(-1, 1) - self.goal) ** 2).sum(dim=(2, 3))
        if slots is not None:
            keep = torch.tensor([a in slots for a in range(self.cars_per_env)]).repeat(self.num_envs)
            ret = torch.where(keep[:, None], ret, torch.zeros_like(ret))
        return {"return": ret}

    def look_ahead(self, actions, repeat=None, outputs=("return",), out=None):
        E, K, H, A, _ = actions.shape
        assert (E, A) == (self.num_envs, self.cars_per_env) and tuple(outputs) == ("return",)
        self.calls.append(("truth", repeat, actions.clone()))
        a = actions.permute(0, 3, 1, 2, 4).reshape(E * A, K, H, 2)
        return {"return": (-((a - self.true_goal) ** 2).sum(dim=(2, 3))).reshape(E, A, K).permute(0, 2, 1)}


def test_to_dream_actions_is_the_one_conversion():
    import torch
    from racing_dreamer_amd.planning import to_dream_actions
    E, K, H, A = 3, 4, 5, 2
    seq = torch.arange(E * K * H * A * 2, dtype=torch.float32).reshape(E, K, H, A, 2)
    d = to_dream_actions(seq)
    assert d.shape == (E * A, K, H, 2) and d.is_contiguous()
    for e, a, k, t in ((0, 0, 0, 0), (2, 1, 3, 4), (1, 0, 2, 3)):
        assert torch.equal(d[e * A + a, k, t], seq[e, k, t, a])


def test_dream_shooting_takes_the_first_best_and_writes_its_first_action():
    """Explicit candidates with a tie for the best: the lower index wins; candidate 0 of generated candidates repeats action_in;
    with `slots` only those cars' rows of action_in change."""
    import torch
    from racing_dreamer_amd.planning import dream_shooting_act, shooting_candidates
    E, A, K, H = 2, 2, 4, 3
    goal = torch.tensor([[0.5, 0.5], [-0.5, 0.0], [0.0, 0.0], [0.5, -1.0]])
    g = goal.reshape(E, 1, A, 2)
    seq = torch.zeros((E, K, H, A, 2))
    seq[:, 0] = 0.9
    seq[:, 1] = g                                        # candidates 1 and 2 miss the goal by 0.25 in one step each: a tie that
    seq[:, 1, 0, :, 0] += 0.25                           # goes to 1, whose first action is the one that is off
    seq[:, 2] = g
    seq[:, 2, 1, :, 0] += 0.25
    seq[:, 3] = -0.9
    seq[1, 1, :, 1] = 0.7                                # car (1, 1): candidate 1 is far off, candidate 2 wins alone
    env = _StubEnv(E, A, goal)
    out = dream_shooting_act(env, seq)
    assert out is env.views["action_in"]
    want = goal.reshape(E, A, 2).clone()
    want[:, :, 0] += 0.25
    want[1, 1, 0] -= 0.25
    assert torch.equal(out, want)
    kind, slots, acts = env.calls[-1]
    assert kind == "dream" and slots is None and acts.shape == (E * A, K, H, 2)
    ret = env.dream_ahead(acts)["return"]
    assert torch.equal(ret.argmax(dim=1), torch.tensor([1, 1, 1, 2])) and ret[0, 1] == ret[0, 2]
    # slots: only slot 1's cars are planned for and written
    env = _StubEnv(E, A, goal)
    out = dream_shooting_act(env, seq, slots=(1,))
    assert env.calls[-1][1] == (1,)
    assert torch.equal(out[:, 0], torch.full((E, 2), 0.25)) and torch.equal(out[:, 1], want[:, 1])
    # generated candidates: shooting_candidates', whose candidate 0 repeats action_in - the goal of every car here
    env = _StubEnv(E, A, torch.full((E * A, 2), 0.25))
    out = dream_shooting_act(env, candidates=16, horizon=7, hold=3, seed=5)
    _, _, acts = env.calls[-1]
    gen = shooting_candidates(env, 16, 7, 3, 5)
    assert torch.equal(acts, gen.permute(0, 3, 1, 2, 4).reshape(E * A, 16, 7, 2))
    assert torch.equal(out, torch.full((E, A, 2), 0.25))
    env.policy_has_reward_head = False
    with pytest.raises(RuntimeError):
        dream_shooting_act(env, 4, 3)


def test_dream_cem_is_deterministic_under_a_seed_and_finds_the_goal():
    import torch
    from racing_dreamer_amd.planning import dream_cem_act
    E, A = 3, 1
    goal = torch.tensor([[0.6, -0.3], [-0.8, 0.8], [0.0, 0.2]])
    runs = []
    for seed in (1, 1, 2):
        env = _StubEnv(E, A, goal)
        out = dream_cem_act(env, candidates=64, horizon=4, iterations=4, elites=8, seed=seed)
        assert out is env.views["action_in"] and len(env.calls) == 4
        assert all(c[2].shape == (E, 64, 4, 2) and float(c[2].abs().max()) <= 1.0 for c in env.calls)
        runs.append(out.clone())
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    # 4 refits of 64 draws to their 8 best: the mean's first action has moved from 0 most of the way to the goal
    assert float((runs[0].reshape(E, 2) - goal).abs().max()) < 0.25
    with pytest.raises(ValueError):
        dream_cem_act(_StubEnv(E, A, goal), candidates=4, elites=5)


def test_dream_vs_truth_statistics():
    """Candidates whose imagined and true returns are known: equal goals give correlation 1, agreement and regret 0; a dream
    with the opposite goal ranks the candidates backwards."""
    import torch
    from racing_dreamer_amd.world_model import dream_vs_truth, rank_correlation
    E, K, H = 2, 5, 3
    level = torch.tensor([-0.8, -0.4, 0.0, 0.4, 0.8])
    seq = level.reshape(1, K, 1, 1, 1).expand(E, K, H, 1, 2).clone()
    same = dream_vs_truth(_StubEnv(E, 1, torch.full((E, 2), 0.8)), seq)
    assert same["imagined"].shape == same["true"].shape == (E, K) and torch.equal(same["imagined"], same["true"])
    assert torch.allclose(same["rank_correlation"], torch.ones(E, dtype=torch.float64)) and bool(same["argmax_agree"].all())
    assert torch.equal(same["regret"], torch.zeros(E))
    env = _StubEnv(E, 1, torch.full((E, 2), -1.0), true_goal=torch.full((E, 2), 1.0))
    opposite = dream_vs_truth(env, seq.reshape(E, K, H, 2), repeat=2)
    assert [c[0] for c in env.calls] == ["dream", "truth"] and env.calls[1][1] == 2
    assert torch.allclose(opposite["rank_correlation"], -torch.ones(E, dtype=torch.float64)) and not bool(opposite["argmax_agree"].any())
    true = opposite["true"]
    assert torch.equal(opposite["regret"], true[:, 4] - true[:, 0]) and float(opposite["regret"].min()) > 0
    # ties share the mean rank; a constant row has no correlation
    a = torch.tensor([[1.0, 2.0, 2.0, 3.0], [1.0, 1.0, 1.0, 1.0]])
    b = torch.tensor([[1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0]])
    rho = rank_correlation(a, b)
    ra, rb = np.array([0.0, 1.5, 1.5, 3.0]), np.array([0.0, 1.0, 2.0, 3.0])
    assert abs(float(rho[0]) - np.corrcoef(ra, rb)[0, 1]) < 1e-12 and bool(torch.isnan(rho[1]))
    with pytest.raises(ValueError):
        dream_vs_truth(_StubEnv(1, 2, torch.zeros(2, 2)), torch.zeros(1, 2, 2, 2, 2))


def test_abi_symbol_and_struct(hip_lib):
    """rc_policy_dream_ahead is declared, exported and bound on a box without a GPU; the ctypes struct has the header's fields in
    order; the paths that need no device refuse."""
    import os
    from racing_dreamer_amd import _lib as L
    assert "rc_policy_dream_ahead" in L.SYMBOLS and hasattr(hip_lib, "rc_policy_dream_ahead")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "racecar_hip.h")).read()
    body = re.search(r"typedef struct rc_policy_dream_ahead_args \{(.*?)\} rc_policy_dream_ahead_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"\*?(\w+)\s*$", decl.strip())]
    assert fields == [f[0] for f in L.RcPolicyDreamAheadArgs._fields_]
    assert C.sizeof(L.RcPolicyDreamAheadArgs) == 88
    assert hip_lib.rc_policy_dream_ahead(None, None) == -1 and b"NULL" in hip_lib.rc_last_error()
    assert hip_lib.rc_abi_version() == 3
