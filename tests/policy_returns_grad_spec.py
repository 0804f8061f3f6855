"""PolicyReturnsGradSpec: the binary32 specification of the actor loss's gradient through the dream (DESIGN.md §2 item 26,
rc_policy_returns_grad; tests/policy_returns_grad_spec.c, which includes policy_returns_spec.c and through it the specs below), built
and loaded the way policy_returns_spec.py builds its library.  `returns_grad` takes what `PolicyReturnsSpec.returns` takes, plus
`scale`, and returns what it returns plus grad_actions, actor_features, eps and grad_state.  `restated` is the open-loop forward and
backward in plain NumPy at a dtype of the caller's choice (float64: the reference of the tests; float32: what a straightforward
implementation's own rounding amounts to)."""
import ctypes as C
import os

import numpy as np

import policy_imagine_spec as pis
import policy_returns_spec as prs
import policy_sample_spec as pss
import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_returns_grad_spec.c")
MODES = prs.MODES
FEAT = 230
f32 = np.float32
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = ps.build_and_load("policy_returns_grad_spec", [SRC, prs.SRC, pis.SRC, pss.SRC, ps.SRC])
    lib.prg_returns_grad.restype = None
    lib.prg_returns_grad.argtypes = ([C.POINTER(ps._Weights), C.POINTER(pis._Heads), C.POINTER(prs._Critic), C.c_int, C.c_uint32, C.c_uint32, C.c_int,
                                      C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_int]
                                     + [C.c_void_p] * 5)
    lib.prg_coefficients.restype = None
    lib.prg_coefficients.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_float, C.c_float] + [C.c_void_p] * 3
    _lib = lib
    return lib


def default_scale(rows, horizon):
    """float32(-1 / (rows (H - 1))): with it the sum of J over the rows is the reference's actor_loss."""
    return f32(-1.0 / (int(rows) * (int(horizon) - 1)))


def coefficients(value, pcont, returns, weight, lambda_, scale):
    """(c_r [n, H - 1], c_p [n, H - 1], c_v [n, H]; c_v[:, 0] = 0 is never used) of the forward's series, in the spec's order."""
    v, p, r, w = (np.ascontiguousarray(x, f32) for x in (value, pcont, returns, weight))
    n, h = v.shape
    c_r, c_p, c_v = np.zeros((n, h - 1), f32), np.zeros((n, h - 1), f32), np.zeros((n, h), f32)
    for i in range(n):
        load().prg_coefficients(h, v[i].ctypes.data, p[i].ctypes.data, r[i].ctypes.data, w[i].ctypes.data, float(lambda_), float(scale),
                                c_r[i].ctypes.data, c_p[i].ctypes.data, c_v[i].ctypes.data)
    return c_r, c_p, c_v


class PolicyReturnsGradSpec(prs.PolicyReturnsSpec):
    def __init__(self, weights, critic=None, threads=8):
        super().__init__(weights, critic, threads)
        self.glib = load()
        assert self.has_head and self.has_value, "the actor loss needs a reward head and a value head"

    def returns_grad(self, state, keys=None, ids=None, horizon=15, mode="sample", seed=0, lambda_=0.95, discount=0.99, scale=None, actions=None):
        """As PolicyReturnsSpec.returns (H >= 2); scale None: default_scale(n, H).  Returns its dict and grad_actions [n, H, 2],
        actor_features [n, H, 230], grad_state [n, 230] and - closed loop in `sample` - eps [n, H, 2]."""
        st = np.zeros((len(state), ps.STATE), f32)
        st[:, :np.shape(state)[1]] = state
        n, h = len(st), int(horizon)
        assert 2 <= h <= 64
        sc = default_scale(n, h) if scale is None else f32(scale)
        if keys is not None:
            keyed, ky = 0, np.ascontiguousarray(keys, np.uint32).reshape(n, 4)
        else:
            keyed, ky = 1, (np.arange(n, dtype=np.uint64) if ids is None else np.ascontiguousarray(ids, np.uint64).reshape(n))
        act_in = None if actions is None else np.ascontiguousarray(actions, f32).reshape(n, h, 2)
        out = dict(action=np.empty((n, h, 2), f32), feature=np.empty((n, h, FEAT), f32), normals=np.empty((n, h, prs.N_NORMALS), f32),
                   pcont=np.empty((n, h), f32), weight=np.empty((n, h - 1), f32), reward=np.empty((n, h), f32), value=np.empty((n, h), f32),
                   returns=np.empty((n, h - 1), f32), grad_actions=np.empty((n, h, 2), f32), actor_features=np.empty((n, h, FEAT), f32),
                   grad_state=np.empty((n, FEAT), f32))
        if mode == "sample" and act_in is None:
            out["eps"] = np.empty((n, h, 2), f32)
        start = np.zeros((3, n), f32)

        def ptr(a, lo):
            return None if a is None else a[lo:].ctypes.data

        def run(lo, hi):
            if hi > lo:
                self.glib.prg_returns_grad(C.byref(self.w), C.byref(self.hd), C.byref(self.cr), MODES[mode], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                                           hi - lo, h, float(lambda_), float(discount), float(sc), st[lo:].ctypes.data, keyed, ky[lo:].ctypes.data,
                                           ptr(act_in, lo), ptr(out["reward"], lo), ptr(out["value"], lo), ptr(out["pcont"], lo), ptr(out["returns"], lo),
                                           ptr(out["weight"], lo), ptr(out["action"], lo), ptr(out["feature"], lo), start[:, lo:].ctypes.data, n,
                                           ptr(out["normals"], lo), ptr(out["grad_actions"], lo), ptr(out["actor_features"], lo),
                                           ptr(out.get("eps"), lo), ptr(out["grad_state"], lo))

        if self.pool is None or n < 2 * self.threads:
            run(0, n)
        else:
            cuts = np.linspace(0, n, self.threads + 1).astype(int)
            list(self.pool.map(lambda k: run(int(cuts[k]), int(cuts[k + 1])), range(self.threads)))
        out["reward_start"], out["value_start"] = start[0].copy(), start[1].copy()
        if self.has_pcont:
            out["pcont_start"] = start[2].copy()
        out["scale"] = sc
        return out


def _elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _elu_grad(a):
    return np.where(a > 0, np.ones_like(a), a + 1)


def restated(w, critic, state, actions, normals, mode, lambda_, discount, scale, dtype, weight=None, backward=True):
    """RSSM.img_step under given actions, the three heads, the lambda-return, J = sum_t (scale weight[t]) returns[t] and its gradient,
    in NumPy at `dtype`: w the checkpoint (with the reward head), critic a mapping with value_* and optionally pcont_*; state
    [N, >= 230], actions [N, H, 2] raw (clamped here), normals [N, H, >= 30] (the step's draws, held fixed; `sample` only).  weight
    [N, H - 1]: the constant of the objective (None: the forward's own cumprod, as the reference's stop_gradient(cumprod)).  Returns a
    dict: reward, value, pcont [N, H], returns, weight [N, H - 1], J [N] and, if `backward`, grad_actions [N, H, 2], grad_state
    [N, 230]."""
    a = lambda key: np.asarray(w[key], dtype)
    b = lambda key: np.asarray(w[key], dtype).reshape(-1)
    ca = lambda key: np.asarray(critic[key], dtype)
    cb = lambda key: np.asarray(critic[key], dtype).reshape(-1)
    has_pcont = "pcont_hout_w" in critic
    N, H, _ = np.shape(actions)
    st = np.asarray(state, dtype)[:, :FEAT]
    stoch, deter = st[:, :30], st[:, 30:]
    raw_a = np.asarray(actions, dtype).reshape(N, H, 2)
    sample = mode == "sample"
    nrm = np.asarray(normals, dtype).reshape(N, H, -1)[:, :, :30] if sample else None
    gb = a("gru_bias").reshape(2, 600)
    img3_w, img3_b = a("img3_w"), b("img3_b")
    lam, disc, sc = dtype(f32(lambda_)), dtype(f32(discount)), dtype(f32(scale))

    def head3(pre, feat):
        a1 = _elu(feat @ ca(pre + "h0_w") + cb(pre + "h0_b"))
        a2 = _elu(a1 @ ca(pre + "h1_w") + cb(pre + "h1_b"))
        a3 = _elu(a2 @ ca(pre + "h2_w") + cb(pre + "h2_b"))
        return (a3 @ ca(pre + "hout_w").reshape(400, 1))[:, 0] + cb(pre + "hout_b")[0], (a1, a2, a3)

    def head3_back(pre, seed, acts):
        a1, a2, a3 = acts
        d = (seed[:, None] * ca(pre + "hout_w").reshape(1, 400)) * _elu_grad(a3)
        d = (d @ ca(pre + "h2_w").T) * _elu_grad(a2)
        d = (d @ ca(pre + "h1_w").T) * _elu_grad(a1)
        return d @ ca(pre + "h0_w").T

    kept, r, v, p = [], [], [], []
    for t in range(H):
        act = np.clip(raw_a[:, t], dtype(-1), dtype(1))
        x1 = _elu(np.concatenate([stoch, act], 1) @ a("img1_w") + b("img1_b"))
        mx, mh = x1 @ a("gru_kernel") + gb[0], deter @ a("gru_recurrent") + gb[1]
        z, rg, hh = _sigmoid(mx[:, :200] + mh[:, :200]), _sigmoid(mx[:, 200:400] + mh[:, 200:400]), mh[:, 400:]
        c = np.tanh(mx[:, 400:] + rg * hh)
        h = deter
        deter = z * h + (1 - z) * c
        x2 = _elu(deter @ a("img2_w") + b("img2_b"))
        o = x2 @ img3_w + img3_b
        raw = o[:, 30:]
        stoch = o[:, :30] + (_softplus(raw) + dtype(0.1)) * nrm[:, t] if sample else o[:, :30]
        feat = np.concatenate([stoch, deter], 1)
        ra1 = _elu(feat @ a("reward_h0_w") + b("reward_h0_b"))
        ra2 = _elu(ra1 @ a("reward_h1_w") + b("reward_h1_b"))
        r.append((ra2 @ a("reward_hout_w").reshape(400, 1))[:, 0] + b("reward_hout_b")[0])
        vt, va = head3("value_", feat)
        v.append(vt)
        if has_pcont:
            logit, pa = head3("pcont_", feat)
            p.append(_sigmoid(logit))
        else:
            pa = None
            p.append(np.full(N, disc, dtype))
        kept.append((x1, z, rg, c, hh, h, x2, raw, ra1, ra2, va, pa))
    r, v, p = np.stack(r, 1), np.stack(v, 1), np.stack(p, 1)
    R = np.empty((N, H), dtype)
    R[:, H - 1] = v[:, H - 1]
    for t in range(H - 2, -1, -1):
        R[:, t] = r[:, t] + p[:, t] * ((1 - lam) * v[:, t + 1] + lam * R[:, t + 1])
    own_w = np.concatenate([np.ones((N, 1), dtype), np.cumprod(p[:, :H - 2], axis=1)], 1)
    wgt = own_w if weight is None else np.asarray(weight, dtype)
    out = {"reward": r, "value": v, "pcont": p, "returns": R[:, :H - 1], "weight": own_w, "J": (sc * wgt * R[:, :H - 1]).sum(axis=1)}
    if not backward:
        return out
    A = np.empty((N, H - 1), dtype)
    for t in range(H - 1):
        A[:, t] = sc * wgt[:, t] + (A[:, t - 1] * p[:, t - 1] * lam if t else 0)
    c_r = A
    c_p = A * ((1 - lam) * v[:, 1:] + lam * R[:, 1:])
    c_v = np.zeros((N, H), dtype)
    c_v[:, 1:] = A * p[:, :H - 1] * (1 - lam)
    c_v[:, H - 1] += A[:, H - 2] * p[:, H - 2] * lam
    carry = np.zeros((N, FEAT), dtype)
    ga = np.zeros((N, H, 2), dtype)
    for t in range(H - 1, -1, -1):
        x1, z, rg, c, hh, h, x2, raw, ra1, ra2, va, pa = kept[t]
        g = carry
        if t < H - 1:
            d2 = (c_r[:, t, None] * a("reward_hout_w").reshape(1, 400)) * _elu_grad(ra2)
            d1 = (d2 @ a("reward_h1_w").T) * _elu_grad(ra1)
            g = d1 @ a("reward_h0_w").T + g
        if t >= 1:
            g = head3_back("value_", c_v[:, t], va) + g
        if has_pcont and t < H - 1:
            g = head3_back("pcont_", c_p[:, t] * (p[:, t] * (1 - p[:, t])), pa) + g
        gs = g[:, :30]
        if sample:
            dx2 = np.concatenate([gs, gs * nrm[:, t] * _sigmoid(raw)], 1) @ img3_w.T
        else:
            dx2 = gs @ img3_w[:, :30].T
        dx2 = dx2 * _elu_grad(x2)
        dd = dx2 @ a("img2_w").T + g[:, 30:]
        dz = dd * (h - c) * z * (1 - z)
        dc = dd * (1 - z) * (1 - c * c)
        dr = dc * hh * rg * (1 - rg)
        dx1 = (np.concatenate([dz, dr, dc], 1) @ a("gru_kernel").T) * _elu_grad(x1)
        rec = np.concatenate([dz, dr, dc * rg], 1) @ a("gru_recurrent").T
        din = dx1 @ a("img1_w").T
        carry = np.concatenate([din[:, :30], dd * z + rec], 1)
        inside = (raw_a[:, t] >= -1) & (raw_a[:, t] <= 1)
        ga[:, t] = np.where(inside, din[:, 30:], dtype(0))
    out["grad_actions"] = ga
    out["grad_state"] = carry
    return out
