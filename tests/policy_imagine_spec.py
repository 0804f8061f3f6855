"""PolicyImagineSpec: the binary32 specification of imagination (rc_policy_imagine; tests/policy_imagine_spec.c,
which includes policy_sample_spec.c and policy_spec.c), built and loaded the way policy_sample_spec.py builds its library.
`imagine` takes the packed latents [n, 232] and the draws' keys - (global env, episode, agent step, slot) per car - and returns
what the device call returns, plus the normals it drew."""
import ctypes as C
import os

import numpy as np

import policy_sample_spec as pss
import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_imagine_spec.c")
MODES = {"mean": 0, "sample": 1}
N_NORMALS = 36           # per car and step: the prior's 32 | block 8's 4
FEAT = 230
HEAD_KEYS = ("reward_h0_w", "reward_h0_b", "reward_h1_w", "reward_h1_b", "reward_hout_w", "reward_hout_b")
f32 = np.float32
_lib = None


class _Heads(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("img2_w", "img2_b", "img3_w", "img3_b", "rh0_w", "rh0_b", "rh1_w", "rh1_b", "rout_w", "rout_b")]


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = ps.build_and_load("policy_imagine_spec", [SRC, pss.SRC, ps.SRC])
    lib.pis_imagine.restype = None
    lib.pis_imagine.argtypes = [C.POINTER(ps._Weights), C.POINTER(_Heads), C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int] + [C.c_void_p] * 8
    lib.pis_normals.restype = None
    lib.pis_normals.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    _lib = lib
    return lib


def normals(key, t, first_block, n_blocks, seed):
    """The 4 n_blocks normals of blocks first_block .. of imagined step t of the car with key = (global env, episode, agent step, slot)."""
    k = np.asarray(key, np.uint32)
    out = np.empty(4 * n_blocks, f32)
    load().pis_normals(k.ctypes.data, t, first_block, n_blocks, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, out.ctypes.data)
    return out


class PolicyImagineSpec(ps.PolicySpec):
    def __init__(self, weights, threads=8):
        super().__init__(weights, threads)
        self.ilib = load()
        a = self.arrays
        self.has_head = all(k in a for k in HEAD_KEYS)
        hd = _Heads()
        for k in ("img2_w", "img2_b", "img3_w", "img3_b"):
            setattr(hd, k, a[k].ctypes.data)
        if self.has_head:
            for dst, src in zip(("rh0_w", "rh0_b", "rh1_w", "rh1_b", "rout_w", "rout_b"), HEAD_KEYS):
                setattr(hd, dst, a[src].ctypes.data)
        self.hd = hd

    def imagine(self, state, keys=None, horizon=15, mode="mean", seed=0, actions=None, reward=None, features=True, start_reward=None):
        """state [n, 232] (or [n, 230]) = stoch | deter | (unused), keys uint32 [n, 4], actions [n, H, 2] or None.  Returns a dict:
        action [n, H, 2], feature [n, H, 230], normals [n, H, 36], and with a head reward [n, H] and reward_start [n]."""
        st = np.zeros((len(state), ps.STATE), f32)
        st[:, :np.shape(state)[1]] = state
        n, h = len(st), int(horizon)
        ky = np.zeros((n, 4), np.uint32) if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(n, 4)
        assert mode == "mean" or keys is not None
        want_r = self.has_head if reward is None else reward
        want_s = self.has_head if start_reward is None else start_reward
        assert self.has_head or not (want_r or want_s)
        act_in = None if actions is None else np.ascontiguousarray(actions, f32).reshape(n, h, 2)
        out = dict(action=np.empty((n, h, 2), f32), normals=np.empty((n, h, N_NORMALS), f32))
        if features:
            out["feature"] = np.empty((n, h, FEAT), f32)
        if want_r:
            out["reward"] = np.empty((n, h), f32)
        if want_s:
            out["reward_start"] = np.empty(n, f32)

        def ptr(a, lo):
            return None if a is None else a[lo:].ctypes.data

        def run(lo, hi):
            if hi > lo:
                self.ilib.pis_imagine(C.byref(self.w), C.byref(self.hd), MODES[mode], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, hi - lo, h,
                                      st[lo:].ctypes.data, ky[lo:].ctypes.data, ptr(act_in, lo), ptr(out.get("reward"), lo), ptr(out["action"], lo),
                                      ptr(out.get("feature"), lo), ptr(out.get("reward_start"), lo), ptr(out["normals"], lo))

        if self.pool is None or n < 2 * self.threads:
            run(0, n)
        else:
            cuts = np.linspace(0, n, self.threads + 1).astype(int)
            list(self.pool.map(lambda k: run(int(cuts[k]), int(cuts[k + 1])), range(self.threads)))
        return out
