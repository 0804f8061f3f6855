"""The binary32 specification of the actor loss's gradient through the dream (tests/policy_returns_grad_spec.c, DESIGN.md §2 item
26): the NumPy restatement of forward and backward against central differences of its own float64 forward; the clamp's exact zeros;
closed loop = open loop on its own actions; the forward's identity with PolicyReturnsSpec; the rows fed through the actor's fit spec
against a float64 total derivative of actor_loss (torch autograd, the actor's input detached); the spec against the float64
restatement, as close as a plain float32 restatement gets; non-vacuity; H = 2, lambda 0 and 1, discount 0, scale 0; the C-ABI's new
symbol."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import policy_returns_grad_spec as prg
from policy_actor_fit_spec import KEYS as ACTOR_KEYS
from policy_actor_fit_spec import PolicyActorFitSpec
from policy_returns_grad_spec import PolicyReturnsGradSpec, restated
from policy_returns_spec import PolicyReturnsSpec
from test_golden_policy import weights
from test_policy_dream_grad_spec import _latents
from test_policy_observe_spec import WITH_HEAD

f32, f64 = np.float32, np.float64
MODES = ("mean", "sample")
H, LAMBDA, DISCOUNT, SEED = 15, 0.95, 0.99, 5
CRITIC_SEED = 5                # tests/test_gpu_policy_returns.py's synthetic critic; test_every_action_gradient_is_nonzero pins the choice
# spec error <= MARGIN x float32 error per output, both against the float64 restatement (max |x - float64| over the array; 64 rows,
# H = 15, lambda 0.95, a pcont head, the closed loop's own actions given to both restatements): MARGIN = 2 x the largest ratio
# measured on these fixed inputs over (checkpoint, mode), the rule of items 21-25.  Measured ratios, austria mean / sample,
# treitlstrasse mean / sample:
#   grad_actions  1.30 / 1.13, 2.08 / 1.31
#   grad_state    2.64 / 0.86, 1.97 / 1.47
#   returns       1.95 / 2.19, 0.81 / 1.34
# Relative to the largest entry the spec is off by at most 5.1e-5 (grad_state, austria `mean`), 8e-6 in grad_actions.
MARGIN = {"grad_actions": 2 * 2.08, "grad_state": 2 * 2.64, "returns": 2 * 2.19}
# the same rule for the actor's ten gradient arrays (max |x - float64| over all of them; austria, `sample`, 16 rows, H = 6, a pcont
# head): the spec chain (returns-grad spec -> actor-fit spec) and torch's float32 autograd against torch's float64.  Measured ratio:
# 1.51 (9.2e-6 against 6.1e-6, the largest entry 4.1).
ACTOR_MARGIN = 2 * 1.51


def _critic(pcont=True):
    from racing_dreamer_amd.critic import init_critic
    return init_critic(CRITIC_SEED, pcont=pcont)


@functools.lru_cache(maxsize=None)
def _gspec(name, pcont=True):
    return PolicyReturnsGradSpec(weights(name), _critic(pcont))


@functools.lru_cache(maxsize=None)
def _case(name, mode, pcont=True, lambda_=LAMBDA):
    """(state, the spec's outputs) of the 64-row closed-loop case; computed once, read only."""
    state = _latents(name)
    got = _gspec(name, pcont).returns_grad(state, horizon=H, mode=mode, seed=SEED, lambda_=lambda_, discount=DISCOUNT)
    for v in got.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return state, got


def _fd_check(w, critic, st, ac, nr, mode, lambda_, discount, scale, probes_t, cols):
    """Central differences (eps = 1e-6) of the float64 restatement's own J, weight held constant, against its backward: the action
    entries inside the clamp at the steps `probes_t` and the start-latent entries `cols`, to 1e-6 of the row's largest gradient entry.
    Returns the counts checked."""
    # (converted once: `restated` takes arrays that already have its dtype as they are)
    w = {k: np.asarray(w[k], f64) for k in (getattr(w, "files", None) or w.keys()) if k != "source" and np.asarray(w[k]).dtype.kind == "f"}
    critic = {k: np.asarray(v, f64) for k, v in critic.items()}
    full = restated(w, critic, st, ac, nr, mode, lambda_, discount, scale, f64)
    eps, n_a, n_s = 1e-6, 0, 0
    for i in range(len(st)):
        big = max(np.abs(full["grad_actions"][i]).max(), np.abs(full["grad_state"][i]).max())
        assert big > 0
        wgt = full["weight"][i:i + 1]

        def j_of(s1, a1):
            return restated(w, critic, s1[None], a1[None], None if nr is None else nr[i:i + 1], mode, lambda_, discount, scale, f64, weight=wgt,
                            backward=False)["J"][0]

        for t in probes_t:
            for j in range(2):
                if abs(ac[i, t, j]) >= 1.0 - 1e-3:
                    continue
                up, dn = ac[i].copy(), ac[i].copy()
                up[t, j] += eps
                dn[t, j] -= eps
                fd = (j_of(st[i], up) - j_of(st[i], dn)) / (2 * eps)
                assert abs(fd - full["grad_actions"][i, t, j]) <= 1e-6 * big, (mode, lambda_, i, t, j, fd, full["grad_actions"][i, t, j])
                n_a += 1
        for col in cols:
            up, dn = st[i].copy(), st[i].copy()
            up[col] += eps
            dn[col] -= eps
            fd = (j_of(up, ac[i]) - j_of(dn, ac[i])) / (2 * eps)
            assert abs(fd - full["grad_state"][i, col]) <= 1e-6 * big, (mode, lambda_, i, col, fd, full["grad_state"][i, col])
            n_s += 1
    return n_a, n_s, full


@pytest.mark.parametrize("lambda_", (0.0, 0.95, 1.0))
@pytest.mark.parametrize("pcont", (True, False))
@pytest.mark.parametrize("mode", MODES)
def test_the_restatement_agrees_with_central_differences(mode, pcont, lambda_):
    """The float64 restatement's backward against central differences of its own open-loop forward: J perturbed in an action entry
    at t = 0, the middle and H - 1 and in start-latent entries (stoch and deter), the project's criterion (eps = 1e-6, 1e-6 of the
    row's largest entry), in both modes, with and without a pcont head, at lambda 0, 0.95 and 1."""
    name = WITH_HEAD[0]
    state, got = _case(name, mode, pcont)
    rows = [0, 41]
    # (open loop under actions of its own: the actor's, for these latents, sit too close to the clamp's kink at +-1 to be probed)
    st, ac, nr = state[rows].astype(f64), np.random.default_rng(6).uniform(-0.9, 0.9, (2, H, 2)), got["normals"][rows]
    n_a, n_s, _ = _fd_check(weights(name), _critic(pcont), st, ac, nr, mode, lambda_, DISCOUNT, got["scale"], (0, H // 2, H - 1), (0, 29, 30, 177, 229))
    assert n_a >= 8 and n_s >= 8


@pytest.mark.parametrize("mode", MODES)
def test_the_clamp_passes_inside_and_gives_positive_zero_outside(mode):
    """actions_in drawn uniformly from [-1.5, 1.5] - a third of the entries outside [-1, 1]: the spec's grad_actions is +0.0f by bit
    pattern there and non-zero inside; +-1 exactly passes (the inclusive range of tf.clip_by_value); the entries inside agree with
    central differences of the float64 restatement."""
    name = WITH_HEAD[0]
    state = _latents(name)[:4]
    acts = np.random.default_rng(4).uniform(-1.5, 1.5, (4, 5, 2)).astype(f32)
    acts[0, 0] = (1.0, -1.0)
    acts[1, 2] = (-1.0, 1.0)
    got = _gspec(name).returns_grad(state, horizon=5, mode=mode, seed=3, actions=acts)
    ga = got["grad_actions"]
    outside = np.abs(acts) > 1.0
    assert 0.2 < outside.mean() < 0.45
    assert not ga.view(np.uint32)[outside].any()
    assert np.all(ga[~outside] != 0.0) and np.all(ga[0, 0] != 0.0) and np.all(ga[1, 2] != 0.0)
    assert "eps" not in got
    rows = [0, 1]
    n_a, _, full = _fd_check(weights(name), _critic(), state[rows].astype(f64), acts[rows].astype(f64), got["normals"][rows], mode, LAMBDA, DISCOUNT,
                             got["scale"], (0, 2, 4), ())
    assert n_a >= 6
    assert not full["grad_actions"][outside[rows]].any()
    assert np.abs(ga[rows] - full["grad_actions"]).max() <= 1e-4 * np.abs(full["grad_actions"]).max()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", WITH_HEAD)
def test_closed_loop_is_open_loop_on_its_own_actions_and_the_forward_is_the_returns_specs(name, mode):
    """grad_actions and grad_state of the closed loop equal, byte for byte, those of the open loop on the actions the closed loop
    returned (the actor is not differentiated); every forward output is PolicyReturnsSpec.returns', bit for bit, with ids beyond
    2^32; actor_features is the start feature, then feature[t - 1]; eps is block 8's words 0-1."""
    state = _latents(name)[:5]
    ids = np.array([7, 8, (1 << 33) + 1, 9, 10], np.uint64)
    for pcont in (True, False):
        g = _gspec(name, pcont)
        closed = g.returns_grad(state, ids=ids, horizon=4, mode=mode, seed=12, lambda_=LAMBDA, discount=0.97)
        opened = g.returns_grad(state, ids=ids, horizon=4, mode=mode, seed=12, lambda_=LAMBDA, discount=0.97, actions=closed["action"])
        assert closed["grad_actions"].tobytes() == opened["grad_actions"].tobytes()
        assert closed["grad_state"].tobytes() == opened["grad_state"].tobytes()
        want = PolicyReturnsSpec(weights(name), _critic(pcont)).returns(state, ids=ids, horizon=4, mode=mode, seed=12, lambda_=LAMBDA, discount=0.97)
        assert set(want) <= set(closed)
        for k, v in want.items():
            assert closed[k].tobytes() == v.tobytes(), (pcont, k)
        assert np.array_equal(closed["actor_features"][:, 0], state[:, :230])
        assert np.array_equal(closed["actor_features"][:, 1:], closed["feature"][:, :-1])
        if mode == "sample":
            assert np.array_equal(closed["eps"], closed["normals"][:, :, 32:34]) and np.all(closed["eps"] != 0)
        else:
            assert "eps" not in closed


@pytest.mark.parametrize("name", WITH_HEAD)
def test_every_action_gradient_is_nonzero(name):
    """Non-vacuity: on the 64 posterior latents, H = 15, mode `sample`, with the synthetic critic of seed CRITIC_SEED, every (row, t)
    of the spec's grad_actions is non-zero - with and without the pcont head, at the recursion's two ends as well."""
    for pcont, lam in ((True, LAMBDA), (False, LAMBDA), (True, 0.0), (True, 1.0)):
        ga = _case(name, "sample", pcont, lam)[1]["grad_actions"]
        assert np.all(np.abs(ga).max(axis=2) > 0), (pcont, lam)
        assert np.all(ga != 0), (pcont, lam)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", WITH_HEAD)
def test_the_spec_is_as_close_to_float64_as_float32_can_be(name, mode):
    """64 posterior latents (item 17's spec in `sample`), H = 15: grad_actions, grad_state and returns of the spec against the
    float64 restatement within MARGIN x the error of the plain float32 restatement."""
    assert len(WITH_HEAD) == 2
    state, got = _case(name, mode)
    w, critic = weights(name), _critic()
    ref = restated(w, critic, state, got["action"], got["normals"], mode, LAMBDA, DISCOUNT, got["scale"], f64)
    own = restated(w, critic, state, got["action"], got["normals"], mode, LAMBDA, DISCOUNT, got["scale"], f32)
    missed = []
    for key in ("grad_actions", "grad_state", "returns"):
        assert own[key].dtype == f32
        spec_err = float(np.abs(got[key].astype(f64) - ref[key]).max())
        f32_err = float(np.abs(own[key].astype(f64) - ref[key]).max())
        print(f"{name} {mode} {key}: spec {spec_err:.3e} float32 {f32_err:.3e} ratio {spec_err / max(f32_err, 1e-300):.2f} "
              f"largest {float(np.abs(ref[key]).max()):.3e}")
        assert f32_err > 0
        if not spec_err <= MARGIN[key] * f32_err:
            missed.append((name, mode, key, spec_err, f32_err))
    assert not missed, missed


def _torch_actor_gradient(w, critic, state, eps_all, nrm_all, horizon, lambda_, discount, dtype):
    """The total derivative of actor_loss = -mean(stop_gradient(weight) returns) with respect to the actor's ten arrays, by torch
    autograd on the CPU at `dtype`: the closed-loop dream in mode `sample` under the plain tanh-normal actor, its input detached
    (dreamer/models.py:218-219), the draws held fixed.  Returns ({name: gradient}, the loss)."""
    import torch
    import torch.nn.functional as F
    T = lambda a: torch.tensor(np.asarray(a, f64), dtype=dtype)
    actor = {k: T(w[k]).requires_grad_(True) for k in ACTOR_KEYS}
    p = {k: T(w[k]) for k in (getattr(w, "files", None) or w.keys()) if k != "source" and np.asarray(w[k]).dtype.kind == "f"}
    p.update({k: T(v) for k, v in critic.items()})
    feat = T(state[:, :230])
    eps, nrm = T(eps_all), T(nrm_all)
    gb = p["gru_bias"].reshape(2, 600)

    def head(pre, x, n):
        for l in range(n):
            x = F.elu(x @ p[f"{pre}h{l}_w"] + p[f"{pre}h{l}_b"].reshape(-1))
        return (x @ p[pre + "hout_w"].reshape(400, 1))[:, 0] + p[pre + "hout_b"].reshape(-1)[0]

    r, v, pc = [], [], []
    for t in range(horizon):
        x = feat.detach()
        for l in range(4):
            x = F.elu(x @ actor[f"h{l}_w"] + actor[f"h{l}_b"])
        o = x @ actor["hout_w"] + actor["hout_b"]
        mu = 5.0 * torch.tanh(o[:, :2] / 5.0)
        sd = F.softplus(o[:, 2:] + float(np.log(np.exp(5.0) - 1.0))) + 1e-4
        act = torch.tanh(mu + sd * eps[:, t])
        stoch, deter = feat[:, :30], feat[:, 30:]
        x1 = F.elu(torch.cat([stoch, act], 1) @ p["img1_w"] + p["img1_b"].reshape(-1))
        mx, mh = x1 @ p["gru_kernel"] + gb[0], deter @ p["gru_recurrent"] + gb[1]
        z, rg = torch.sigmoid(mx[:, :200] + mh[:, :200]), torch.sigmoid(mx[:, 200:400] + mh[:, 200:400])
        c = torch.tanh(mx[:, 400:] + rg * mh[:, 400:])
        deter = z * deter + (1 - z) * c
        x2 = F.elu(deter @ p["img2_w"] + p["img2_b"].reshape(-1))
        o3 = x2 @ p["img3_w"] + p["img3_b"].reshape(-1)
        stoch = o3[:, :30] + (F.softplus(o3[:, 30:]) + 0.1) * nrm[:, t, :30]
        feat = torch.cat([stoch, deter], 1)
        r.append(head("reward_", feat, 2))
        v.append(head("value_", feat, 3))
        pc.append(torch.sigmoid(head("pcont_", feat, 3)) if "pcont_hout_w" in critic else torch.full_like(r[-1], float(f32(discount))))
    lam = float(f32(lambda_))
    R, rets = v[-1], []
    for t in range(horizon - 2, -1, -1):
        R = r[t] + pc[t] * ((1 - lam) * v[t + 1] + lam * R)
        rets.append(R)
    rets = torch.stack(rets[::-1], 1)
    wgt = torch.cumprod(torch.cat([torch.ones_like(pc[0])[:, None], torch.stack(pc[:horizon - 2], 1)], 1), 1).detach()
    loss = -(wgt * rets).mean()
    grads = torch.autograd.grad(loss, [actor[k] for k in ACTOR_KEYS])
    return {k: g.numpy() for k, g in zip(ACTOR_KEYS, grads)}, float(loss.detach())


def test_the_rows_through_the_actor_fit_spec_are_the_total_derivative_of_actor_loss():
    """End to end: the spec's rows (actor_features, eps, grad_actions under the default scale) through PolicyActorFitSpec in grad mode
    give the actor's ten gradient arrays; torch's float64 autograd of actor_loss, the actor's input detached, gives the reference.
    The spec chain is within ACTOR_MARGIN x the distance of torch's own float32 autograd from float64; the loss agrees too."""
    name, n, h = WITH_HEAD[0], 16, 6
    w, critic = weights(name), _critic()
    state = _latents(name)[:n]
    got = _gspec(name).returns_grad(state, horizon=h, mode="sample", seed=9, lambda_=LAMBDA, discount=DISCOUNT)
    assert got["scale"] == f32(-1.0 / (n * (h - 1)))
    step = PolicyActorFitSpec(w).step(got["actor_features"].reshape(-1, 230), grad_actions=got["grad_actions"].reshape(-1, 2),
                                      eps=got["eps"].reshape(-1, 2))
    ref, loss64 = _torch_actor_gradient(w, critic, state, got["eps"], got["normals"], h, LAMBDA, DISCOUNT, __import__("torch").float64)
    own, _ = _torch_actor_gradient(w, critic, state, got["eps"], got["normals"], h, LAMBDA, DISCOUNT, __import__("torch").float32)
    spec_loss = -float((got["weight"].astype(f64) * got["returns"].astype(f64)).mean())
    assert abs(spec_loss - loss64) <= 1e-5 * abs(loss64)
    spec_err = max(float(np.abs(step["grad"][k].astype(f64) - ref[k]).max()) for k in ACTOR_KEYS)
    f32_err = max(float(np.abs(own[k].astype(f64) - ref[k]).max()) for k in ACTOR_KEYS)
    big = max(float(np.abs(ref[k]).max()) for k in ACTOR_KEYS)
    print(f"actor gradient: spec chain {spec_err:.3e} torch float32 {f32_err:.3e} ratio {spec_err / f32_err:.2f} largest {big:.3e}")
    assert big > 0 and f32_err > 0
    assert spec_err <= ACTOR_MARGIN * f32_err
    assert spec_err <= 1e-4 * big


def test_edge_cases():
    """H = 2 (one step of the recursion: c_v[1] alone carries v, no c_v from the loop survives); lambda 0; lambda 1 (c_v is a zero
    before H - 1); discount 0 without a pcont head (the gradient flows through r_0 alone); scale 0 gives zeros."""
    name = WITH_HEAD[0]
    w = weights(name)
    state = _latents(name)[:6]
    # H = 2 against the float64 restatement
    for mode in MODES:
        got = _gspec(name).returns_grad(state, horizon=2, mode=mode, seed=2)
        ref = restated(w, _critic(), state, got["action"], got["normals"], mode, LAMBDA, DISCOUNT, got["scale"], f64)
        for k in ("grad_actions", "grad_state"):
            assert np.abs(got[k] - ref[k]).max() <= 1e-4 * np.abs(ref[k]).max(), (mode, k)
        assert np.all(got["grad_actions"] != 0)
    # the coefficients at the recursion's two ends
    got = _gspec(name).returns_grad(state, horizon=5, mode="sample", seed=2, lambda_=1.0)
    c_r, c_p, c_v = prg.coefficients(got["value"], got["pcont"], got["returns"], got["weight"], 1.0, got["scale"])
    assert not c_v[:, 1:4].any() and np.all(c_v[:, 4] != 0) and np.all(c_r != 0) and np.all(c_p != 0)
    got = _gspec(name).returns_grad(state, horizon=5, mode="sample", seed=2, lambda_=0.0)
    c_r, c_p, c_v = prg.coefficients(got["value"], got["pcont"], got["returns"], got["weight"], 0.0, got["scale"])
    assert np.array_equal(c_r, got["scale"] * got["weight"]) and np.all(c_v[:, 1:] != 0)
    ref = restated(w, _critic(), state, got["action"], got["normals"], "sample", 0.0, DISCOUNT, got["scale"], f64)
    assert np.abs(got["grad_actions"] - ref["grad_actions"]).max() <= 1e-4 * np.abs(ref["grad_actions"]).max()
    # discount 0, no pcont head: only r_0 is left of J
    for mode in MODES:
        zero = _gspec(name, False).returns_grad(state, horizon=4, mode=mode, seed=2, discount=0.0)
        assert not zero["grad_actions"][:, 1:].any() and np.all(zero["grad_actions"][:, 0] != 0.0)
        assert np.array_equal(zero["returns"][:, 0], zero["reward"][:, 0])
    # scale 0
    none = _gspec(name).returns_grad(state, horizon=4, mode="sample", seed=2, scale=0.0)
    assert not none["grad_actions"].any() and not none["grad_state"].any() and np.abs(none["returns"]).max() > 0


def test_abi_symbol_and_struct(hip_lib):
    """rc_policy_returns_grad is declared, exported and bound on a box without a GPU; the ctypes struct has the header's fields in
    order and its size; the paths that need no device refuse; rc_policy_returns_args and the ABI version are what they were."""
    import os
    from racing_dreamer_amd import _lib as L
    assert "rc_policy_returns_grad" in L.SYMBOLS and hasattr(hip_lib, "rc_policy_returns_grad")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "racecar_hip.h")).read()
    body = re.search(r"typedef struct rc_policy_returns_grad_args \{(.*?)\} rc_policy_returns_grad_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for n in re.findall(r"\w+", body) if n not in ("const", "float", "uint32_t", "int32_t", "uint64_t", "int64_t")]
    assert fields == [f[0] for f in L.RcPolicyReturnsGradArgs._fields_] and fields[0] == "struct_size"
    # 8 x 4 bytes, 4 x 8 bytes, 16 pointers
    assert C.sizeof(L.RcPolicyReturnsGradArgs) == 32 + 32 + 128
    assert set(L.RETURNS_GRAD_OUTPUTS) == set(L.RETURNS_OUTPUTS) | {"grad_actions", "actor_features", "eps", "grad_state"}
    assert hip_lib.rc_policy_returns_grad(None, None) == -1 and b"NULL" in hip_lib.rc_last_error()
    a = L.RcPolicyReturnsGradArgs(C.sizeof(L.RcPolicyReturnsGradArgs), 15, 1, 1, 0.95, 0.99, -1.0)
    assert hip_lib.rc_policy_returns_grad(None, C.byref(a)) == -1 and b"NULL" in hip_lib.rc_last_error()
    assert C.sizeof(L.RcPolicyReturnsArgs) == 24 + 24 + 96
    assert hip_lib.rc_abi_version() == 3
    from racing_dreamer_amd import build
    assert "racecar_returns_grad.hip" in build.SOURCES and "racecar_dream_grad.h" in build.HEADERS
    assert {"rc_policy_returns_grad_kernel", "rc_policy_returns_grad_sampled_kernel"} <= set(build.required_kernels("shipped"))
