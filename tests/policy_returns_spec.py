"""PolicyReturnsSpec: the binary32 specification of the critic and the lambda-return (rc_policy_returns;
tests/policy_returns_spec.c, which includes policy_imagine_spec.c and through it policy_sample_spec.c and policy_spec.c), built and
loaded the way policy_dream_spec.py builds its library.  `returns` takes the start latents [n, 232], the draws' keys - (global env,
episode, agent step, slot) per car for live latents, or 64-bit start ids for given states - and the critic's arrays, and returns
everything the device call returns, plus the normals it drew."""
import ctypes as C
import os

import numpy as np

import policy_imagine_spec as pis
import policy_sample_spec as pss
import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_returns_spec.c")
MODES = {"mean": 0, "sample": 1}
N_NORMALS = 36           # per row and step: the prior's 32 | block 8's 4
FEAT = 230
f32 = np.float32
_lib = None


class _Critic(C.Structure):
    _fields_ = [("vh_w", C.c_void_p * 3), ("vh_b", C.c_void_p * 3), ("vout_w", C.c_void_p), ("vout_b", C.c_void_p),
                ("ph_w", C.c_void_p * 3), ("ph_b", C.c_void_p * 3), ("pout_w", C.c_void_p), ("pout_b", C.c_void_p)]


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = ps.build_and_load("policy_returns_spec", [SRC, pis.SRC, pss.SRC, ps.SRC])
    lib.prs_returns.restype = None
    lib.prs_returns.argtypes = ([C.POINTER(ps._Weights), C.POINTER(pis._Heads), C.POINTER(_Critic), C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                 C.c_float, C.c_float, C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_int, C.c_void_p])
    lib.prs_lambda_return.restype = None
    lib.prs_lambda_return.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    lib.prs_normals.restype = None
    lib.prs_normals.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    _lib = lib
    return lib


def normals(start_id, t, first_block, n_blocks, seed):
    """The 4 n_blocks normals of blocks first_block .. of imagined step t of the start with the 64-bit id (tag 8)."""
    out = np.empty(4 * n_blocks, f32)
    load().prs_normals(int(start_id) & (2 ** 64 - 1), t, first_block, n_blocks, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, out.ctypes.data)
    return out


def lambda_return(r, v, p, lambda_):
    """(returns, weight) [n, H - 1] of r, v, p [n, H] in the spec's binary32 order."""
    r, v, p = (np.ascontiguousarray(x, f32) for x in (r, v, p))
    n, h = r.shape
    ret, wt = np.empty((n, h - 1), f32), np.empty((n, h - 1), f32)
    for i in range(n):
        load().prs_lambda_return(h, r[i].ctypes.data, v[i].ctypes.data, p[i].ctypes.data, float(lambda_), ret[i].ctypes.data, wt[i].ctypes.data)
    return ret, wt


class PolicyReturnsSpec(pis.PolicyImagineSpec):
    def __init__(self, weights, critic=None, threads=8):
        """weights: the checkpoint; critic: a mapping with the value_* arrays and, optionally, the pcont_* arrays (None: taken
        from `weights` if it holds them)."""
        super().__init__(weights, threads)
        self.rlib = load()
        src = critic if critic is not None else self.arrays
        self.critic = {k: np.ascontiguousarray(src[k], f32) for k in src.keys() if k.startswith(("value_", "pcont_"))}
        self.has_value = "value_hout_w" in self.critic
        self.has_pcont = "pcont_hout_w" in self.critic
        cr = _Critic()
        for name, pre, have in (("v", "value_", self.has_value), ("p", "pcont_", self.has_pcont)):
            if not have:
                continue
            for l in range(3):
                getattr(cr, name + "h_w")[l] = self.critic[f"{pre}h{l}_w"].ctypes.data
                getattr(cr, name + "h_b")[l] = self.critic[f"{pre}h{l}_b"].ctypes.data
            setattr(cr, name + "out_w", self.critic[pre + "hout_w"].ctypes.data)
            setattr(cr, name + "out_b", self.critic[pre + "hout_b"].ctypes.data)
        self.cr = cr

    def returns(self, state, keys=None, ids=None, horizon=15, mode="mean", seed=0, lambda_=0.95, discount=0.99, actions=None):
        """state [n, 232] (or [n, 230]) = stoch | deter | (unused); keys uint32 [n, 4] (live latents: PolicyImagineSpec's draws) or
        ids uint64 [n] (given states: tag 8; default 0 .. n - 1); actions [n, H, 2] or None.  Returns a dict: action [n, H, 2],
        feature [n, H, 230], normals [n, H, 36], pcont [n, H], weight [n, H - 1], with a reward head reward and reward_start, with a
        value head value and value_start (and, with both, returns [n, H - 1]), with a pcont head pcont_start."""
        st = np.zeros((len(state), ps.STATE), f32)
        st[:, :np.shape(state)[1]] = state
        n, h = len(st), int(horizon)
        if keys is not None:
            keyed, ky = 0, np.ascontiguousarray(keys, np.uint32).reshape(n, 4)
        else:
            keyed, ky = 1, (np.arange(n, dtype=np.uint64) if ids is None else np.ascontiguousarray(ids, np.uint64).reshape(n))
        act_in = None if actions is None else np.ascontiguousarray(actions, f32).reshape(n, h, 2)
        out = dict(action=np.empty((n, h, 2), f32), feature=np.empty((n, h, FEAT), f32), normals=np.empty((n, h, N_NORMALS), f32),
                   pcont=np.empty((n, h), f32))
        if h >= 2:
            out["weight"] = np.empty((n, h - 1), f32)
        if self.has_head:
            out["reward"] = np.empty((n, h), f32)
        if self.has_value:
            out["value"] = np.empty((n, h), f32)
        if self.has_head and self.has_value and h >= 2:
            out["returns"] = np.empty((n, h - 1), f32)
        start = np.zeros((3, n), f32)

        def ptr(a, lo):
            return None if a is None else a[lo:].ctypes.data

        def run(lo, hi):
            if hi > lo:
                self.rlib.prs_returns(C.byref(self.w), C.byref(self.hd), C.byref(self.cr), MODES[mode], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                                      hi - lo, h, float(lambda_), float(discount), st[lo:].ctypes.data, keyed, ky[lo:].ctypes.data, ptr(act_in, lo),
                                      ptr(out.get("reward"), lo), ptr(out.get("value"), lo), ptr(out["pcont"], lo), ptr(out.get("returns"), lo),
                                      ptr(out.get("weight"), lo), ptr(out["action"], lo), ptr(out["feature"], lo), start[:, lo:].ctypes.data, n,
                                      ptr(out["normals"], lo))

        if self.pool is None or n < 2 * self.threads:
            run(0, n)
        else:
            cuts = np.linspace(0, n, self.threads + 1).astype(int)
            list(self.pool.map(lambda k: run(int(cuts[k]), int(cuts[k + 1])), range(self.threads)))
        if self.has_head:
            out["reward_start"] = start[0].copy()
        if self.has_value:
            out["value_start"] = start[1].copy()
        if self.has_pcont:
            out["pcont_start"] = start[2].copy()
        return out
