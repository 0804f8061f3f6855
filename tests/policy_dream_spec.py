"""PolicyDreamSpec: the binary32 specification of planning in the latent (rc_policy_dream_ahead;
tests/policy_dream_spec.c, which includes policy_imagine_spec.c and through it policy_sample_spec.c and policy_spec.c), built and
loaded the way policy_imagine_spec.py builds its library.  `dream` takes the start latents [S, 232], the starts' 64-bit ids and
the candidates' actions [S, K, H, 2] and returns what the device call returns, plus the normals it drew and the prior's mean and
std of every step."""
import ctypes as C
import os

import numpy as np

import policy_imagine_spec as pis
import policy_sample_spec as pss
import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_dream_spec.c")
MODES = {"mean": 0, "sample": 1}
N_NORMALS = 32           # per row and step: blocks 0-7 (30 used)
FEAT = 230
f32 = np.float32
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = ps.build_and_load("policy_dream_spec", [SRC, pis.SRC, pss.SRC, ps.SRC])
    lib.pds_dream.restype = None
    lib.pds_dream.argtypes = ([C.POINTER(ps._Weights), C.POINTER(pis._Heads), C.c_int, C.c_uint32, C.c_uint32] + [C.c_int] * 5 + [C.c_float]
                              + [C.c_void_p] * 9)
    lib.pds_return.restype = None
    lib.pds_return.argtypes = [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    lib.pds_normals.restype = None
    lib.pds_normals.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    _lib = lib
    return lib


def normals(start_id, candidate, t, first_block, n_blocks, seed):
    """The 4 n_blocks normals of blocks first_block .. of step t of candidate `candidate` of the start with the 64-bit id."""
    out = np.empty(4 * n_blocks, f32)
    load().pds_normals(int(start_id) & (2 ** 64 - 1), candidate, t, first_block, n_blocks, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, out.ctypes.data)
    return out


def discounted_return(reward, discount):
    """ret [...] of reward [..., H]: acc = 0, w = 1; per step acc = fmaf(w, r, acc), w = w * discount, in binary32."""
    r = np.ascontiguousarray(reward, f32)
    out = np.empty(r.shape[:-1], f32)
    load().pds_return(int(out.size), r.shape[-1], float(discount), r.ctypes.data, out.ctypes.data)
    return out


class PolicyDreamSpec(pis.PolicyImagineSpec):
    def __init__(self, weights, threads=8):
        super().__init__(weights, threads)
        self.dlib = load()

    def dream(self, state, actions, ids=None, mode="mean", seed=0, discount=1.0, head=None, candidates=None):
        """state [S, 232] (or [S, 230]) = stoch | deter | (unused), actions [S, K, H, 2], ids uint64 [S] (default 0 .. S - 1).
        Returns a dict: final_feature [S, K, 230], normals [S, K, H, 32], mean / std [S, K, H, 30], and with a head return [S, K]
        and reward [S, K, H].  candidates=(k0, k1): only those are computed (the other rows of the arrays are left as
        np.empty made them)."""
        st = np.zeros((len(state), ps.STATE), f32)
        st[:, :np.shape(state)[1]] = state
        act = np.ascontiguousarray(actions, f32)
        s, k, h = act.shape[:3]
        assert act.shape == (s, k, h, 2) and s == len(st)
        idv = np.arange(s, dtype=np.uint64) if ids is None else np.ascontiguousarray(ids, np.uint64).reshape(s)
        head = self.has_head if head is None else head
        assert self.has_head or not head
        k0, k1 = (0, k) if candidates is None else candidates
        out = dict(final_feature=np.empty((s, k, FEAT), f32), normals=np.empty((s, k, h, N_NORMALS), f32), mean=np.empty((s, k, h, 30), f32),
                   std=np.empty((s, k, h, 30), f32))
        if head:
            out["return"] = np.empty((s, k), f32)
            out["reward"] = np.empty((s, k, h), f32)

        def ptr(a, lo):
            return None if a is None else a[lo:].ctypes.data

        def run(lo, hi):
            if hi > lo:
                self.dlib.pds_dream(C.byref(self.w), C.byref(self.hd), MODES[mode], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, hi - lo, k, k0, k1, h,
                                    float(discount), st[lo:].ctypes.data, idv[lo:].ctypes.data, act[lo:].ctypes.data, ptr(out.get("return"), lo),
                                    ptr(out.get("reward"), lo), ptr(out["final_feature"], lo), ptr(out["normals"], lo), ptr(out["mean"], lo),
                                    ptr(out["std"], lo))

        if self.pool is None or s < 2 * self.threads:
            if self.pool is not None and s == 1 and k1 - k0 >= 2 * self.threads:
                # one start, many candidates: split the candidates (each call writes its own rows)
                cuts = np.linspace(k0, k1, self.threads + 1).astype(int)

                def part(i):
                    self.dlib.pds_dream(C.byref(self.w), C.byref(self.hd), MODES[mode], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, 1, k, int(cuts[i]),
                                        int(cuts[i + 1]), h, float(discount), st.ctypes.data, idv.ctypes.data, act.ctypes.data, ptr(out.get("return"), 0),
                                        ptr(out.get("reward"), 0), out["final_feature"].ctypes.data, out["normals"].ctypes.data,
                                        out["mean"].ctypes.data, out["std"].ctypes.data)
                list(self.pool.map(part, range(self.threads)))
            else:
                run(0, s)
        else:
            cuts = np.linspace(0, s, self.threads + 1).astype(int)
            list(self.pool.map(lambda i: run(int(cuts[i]), int(cuts[i + 1])), range(self.threads)))
        return out
