"""PolicyDreamGradSpec: the binary32 specification of the dream's backward pass (rc_policy_dream_grad;
tests/policy_dream_grad_spec.c, which includes policy_dream_spec.c and through it the specs below), built and loaded the way
policy_dream_spec.py builds its library.  `dream_grad` takes what `PolicyDreamSpec.dream` takes and returns what the device call
returns.  `restated` is the same forward and backward in plain NumPy at a dtype of the caller's choice (float64: the reference
of the tests; float32: what a straightforward implementation's own rounding amounts to)."""
import ctypes as C
import os

import numpy as np

import policy_dream_spec as pds
import policy_imagine_spec as pis
import policy_sample_spec as pss
import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_dream_grad_spec.c")
MODES = pds.MODES
FEAT = 230
f32 = np.float32
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = ps.build_and_load("policy_dream_grad_spec", [SRC, pds.SRC, pis.SRC, pss.SRC, ps.SRC])
    lib.pdg_dream_grad.restype = None
    lib.pdg_dream_grad.argtypes = ([C.POINTER(ps._Weights), C.POINTER(pis._Heads), C.c_int, C.c_uint32, C.c_uint32] + [C.c_int] * 5 + [C.c_float]
                                   + [C.c_void_p] * 7)
    _lib = lib
    return lib


class PolicyDreamGradSpec(pds.PolicyDreamSpec):
    def __init__(self, weights, threads=8):
        super().__init__(weights, threads)
        self.glib = load()
        assert self.has_head, "the dream's backward pass needs a reward head"

    def dream_grad(self, state, actions, ids=None, mode="mean", seed=0, discount=1.0):
        """state [S, 232] (or [S, 230]), actions [S, K, H, 2] raw, ids uint64 [S] (default 0 .. S - 1).  Returns a dict: grad_actions
        [S, K, H, 2], grad_state [S, K, 230], return [S, K], reward [S, K, H]."""
        st = np.zeros((len(state), ps.STATE), f32)
        st[:, :np.shape(state)[1]] = state
        act = np.ascontiguousarray(actions, f32)
        s, k, h = act.shape[:3]
        assert act.shape == (s, k, h, 2) and s == len(st) and 1 <= h <= 64
        idv = np.arange(s, dtype=np.uint64) if ids is None else np.ascontiguousarray(ids, np.uint64).reshape(s)
        out = {"grad_actions": np.empty((s, k, h, 2), f32), "grad_state": np.empty((s, k, FEAT), f32), "return": np.empty((s, k), f32),
               "reward": np.empty((s, k, h), f32)}

        def run(lo, hi, k0, k1):
            if hi > lo and k1 > k0:
                self.glib.pdg_dream_grad(C.byref(self.w), C.byref(self.hd), MODES[mode], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, hi - lo, k, k0, k1,
                                         h, float(discount), st[lo:].ctypes.data, idv[lo:].ctypes.data, act[lo:].ctypes.data,
                                         out["return"][lo:].ctypes.data, out["reward"][lo:].ctypes.data, out["grad_actions"][lo:].ctypes.data,
                                         out["grad_state"][lo:].ctypes.data)

        if self.pool is None or s * k < 2 * self.threads:
            run(0, s, 0, k)
        elif s >= 2 * self.threads:
            cuts = np.linspace(0, s, self.threads + 1).astype(int)
            list(self.pool.map(lambda i: run(int(cuts[i]), int(cuts[i + 1]), 0, k), range(self.threads)))
        else:                                    # few starts, many candidates: split the candidates (each call writes its own rows)
            cuts = np.linspace(0, k, self.threads + 1).astype(int)
            list(self.pool.map(lambda i: run(0, s, int(cuts[i]), int(cuts[i + 1])), range(self.threads)))
        return out


def _elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _elu_grad(a):
    return np.where(a > 0, np.ones_like(a), a + 1)


def restated(w, state, actions, normals, mode, discount, dtype, backward=True):
    """RSSM.img_step under given actions, the reward head, the discounted return and its gradient, in NumPy at `dtype`: state
    [S, >= 230], actions [S, K, H, 2] raw, normals [S, K, H, >= 30] (the step's draws, held fixed; `sample` only).  Returns a dict as
    PolicyDreamGradSpec.dream_grad's (without the gradients if not `backward`)."""
    a = lambda key: np.asarray(w[key], dtype)
    b = lambda key: np.asarray(w[key], dtype).reshape(-1)
    S, K, H, _ = np.shape(actions)
    N = S * K
    st = np.repeat(np.asarray(state, dtype)[:, :FEAT], K, axis=0)
    stoch, deter = st[:, :30], st[:, 30:]
    raw_a = np.asarray(actions, dtype).reshape(N, H, 2)
    sample = mode == "sample"
    nrm = np.asarray(normals, dtype).reshape(N, H, -1)[:, :, :30] if sample else None
    gb = a("gru_bias").reshape(2, 600)
    img3_w, img3_b = a("img3_w"), b("img3_b")
    disc = dtype(f32(discount))
    ret, wgt, kept, rewards = np.zeros(N, dtype), dtype(1), [], []
    for t in range(H):
        act = np.clip(raw_a[:, t], dtype(-1), dtype(1))
        x1 = _elu(np.concatenate([stoch, act], 1) @ a("img1_w") + b("img1_b"))
        mx, mh = x1 @ a("gru_kernel") + gb[0], deter @ a("gru_recurrent") + gb[1]
        z, r, hh = _sigmoid(mx[:, :200] + mh[:, :200]), _sigmoid(mx[:, 200:400] + mh[:, 200:400]), mh[:, 400:]
        c = np.tanh(mx[:, 400:] + r * hh)
        h = deter
        deter = z * h + (1 - z) * c
        x2 = _elu(deter @ a("img2_w") + b("img2_b"))
        o = x2 @ img3_w + img3_b
        raw = o[:, 30:]
        stoch = o[:, :30] + (_softplus(raw) + dtype(0.1)) * nrm[:, t] if sample else o[:, :30]
        a1 = _elu(np.concatenate([stoch, deter], 1) @ a("reward_h0_w") + b("reward_h0_b"))
        a2 = _elu(a1 @ a("reward_h1_w") + b("reward_h1_b"))
        rew = (a2 @ a("reward_hout_w").reshape(400, 1))[:, 0] + b("reward_hout_b")[0]
        rewards.append(rew)
        ret = ret + wgt * rew
        kept.append((x1, z, r, c, hh, h, x2, raw, a1, a2, wgt))
        wgt = wgt * disc
    out = {"return": ret.reshape(S, K), "reward": np.stack(rewards, 1).reshape(S, K, H)}
    if not backward:
        return out
    carry = np.zeros((N, FEAT), dtype)
    ga = np.zeros((N, H, 2), dtype)
    for t in range(H - 1, -1, -1):
        x1, z, r, c, hh, h, x2, raw, a1, a2, wgt = kept[t]
        d2 = (wgt * a("reward_hout_w").reshape(1, 400)) * _elu_grad(a2)
        d1 = (d2 @ a("reward_h1_w").T) * _elu_grad(a1)
        g = d1 @ a("reward_h0_w").T + carry
        gs = g[:, :30]
        if sample:
            dx2 = np.concatenate([gs, gs * nrm[:, t] * _sigmoid(raw)], 1) @ img3_w.T
        else:
            dx2 = gs @ img3_w[:, :30].T
        dx2 = dx2 * _elu_grad(x2)
        dd = dx2 @ a("img2_w").T + g[:, 30:]
        dz = dd * (h - c) * z * (1 - z)
        dc = dd * (1 - z) * (1 - c * c)
        dr = dc * hh * r * (1 - r)
        dx1 = (np.concatenate([dz, dr, dc], 1) @ a("gru_kernel").T) * _elu_grad(x1)
        rec = np.concatenate([dz, dr, dc * r], 1) @ a("gru_recurrent").T
        din = dx1 @ a("img1_w").T
        carry = np.concatenate([din[:, :30], dd * z + rec], 1)
        inside = (raw_a[:, t] >= -1) & (raw_a[:, t] <= 1)
        ga[:, t] = np.where(inside, din[:, 30:], dtype(0))
    out["grad_actions"] = ga.reshape(S, K, H, 2)
    out["grad_state"] = carry.reshape(S, K, FEAT)
    return out
