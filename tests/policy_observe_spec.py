"""PolicyObserveSpec: the binary32 specification of the world model over recorded sequences (rc_policy_observe;
tests/policy_observe_spec.c, which includes policy_imagine_spec.c and through it policy_sample_spec.c and policy_spec.c), built
and loaded the way policy_imagine_spec.py builds its library.  `observe` takes what the device call takes and returns every
output the device call can return, plus the normals it drew."""
import ctypes as C
import os

import numpy as np

import policy_imagine_spec as pis
import policy_sample_spec as pss
import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_observe_spec.c")
MODES = {"mean": 0, "sample": 1}
N_NORMALS = 32           # per row and step: blocks 0-7
f32 = np.float32
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = ps.build_and_load("policy_observe_spec", [SRC, pis.SRC, pss.SRC, ps.SRC])
    lib.pos_observe.restype = None
    lib.pos_observe.argtypes = ([C.POINTER(ps._Weights), C.POINTER(pis._Heads), C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int]
                                + [C.c_void_p] * 12)
    lib.pos_normals.restype = None
    lib.pos_normals.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.pos_kl.restype = None
    lib.pos_kl.argtypes = [C.c_int] + [C.c_void_p] * 5
    _lib = lib
    return lib


def kl(post_mean, post_std, prior_mean, prior_std):
    """The spec's KL(post || prior) of [n, 30] diagonal normals, summed over the 30 dimensions as `observe` sums it."""
    a = [np.ascontiguousarray(x, f32).reshape(-1, 30) for x in (post_mean, post_std, prior_mean, prior_std)]
    out = np.empty(len(a[0]), f32)
    load().pos_kl(len(out), *[x.ctypes.data for x in a], out.ctypes.data)
    return out


def normals(row_id, t, first_block, n_blocks, seed):
    """The 4 n_blocks normals of blocks first_block .. of step t of the row with id row_id."""
    out = np.empty(4 * n_blocks, f32)
    load().pos_normals(row_id, t, first_block, n_blocks, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, out.ctypes.data)
    return out


class PolicyObserveSpec(pis.PolicyImagineSpec):
    def __init__(self, weights, threads=8):
        super().__init__(weights, threads)
        self.olib = load()

    def observe(self, scan, action, context=None, mode="mean", seed=0, state=None, row_offset=0, reward=None):
        """scan [n, T, 1080] metres, action [n, T, 2] raw, state [n, 232] (or [n, 230]) or None.  Returns a dict: feature
        [n, T, 230], post_mean, post_std, prior_mean, prior_std [n, T, 30], kl [n, T], state [n, 232], normals [n, T, 32], and
        with a head reward [n, T]; post_* and kl hold NaN at t >= context."""
        scan = np.ascontiguousarray(scan, f32)
        n, T = scan.shape[:2]
        assert scan.shape == (n, T, 1080)
        act = np.ascontiguousarray(action, f32).reshape(n, T, 2)
        context = T if context is None else int(context)
        assert 1 <= context <= T
        st = None
        if state is not None:
            st = np.zeros((n, ps.STATE), f32)
            st[:, :np.shape(state)[1]] = state
        want_r = self.has_head if reward is None else reward
        assert self.has_head or not want_r
        out = dict(feature=np.empty((n, T, pis.FEAT), f32), prior_mean=np.empty((n, T, 30), f32), prior_std=np.empty((n, T, 30), f32),
                   post_mean=np.full((n, T, 30), np.nan, f32), post_std=np.full((n, T, 30), np.nan, f32), kl=np.full((n, T), np.nan, f32),
                   state=np.empty((n, ps.STATE), f32), normals=np.empty((n, T, N_NORMALS), f32))
        if want_r:
            out["reward"] = np.empty((n, T), f32)

        def ptr(a, lo):
            return None if a is None else a[lo:].ctypes.data

        def run(lo, hi):
            if hi > lo:
                self.olib.pos_observe(C.byref(self.w), C.byref(self.hd), MODES[mode], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                                      (int(row_offset) + lo) & (2 ** 64 - 1), hi - lo, T, context, ptr(scan, lo), ptr(act, lo), ptr(st, lo),
                                      ptr(out["feature"], lo), ptr(out["post_mean"], lo), ptr(out["post_std"], lo), ptr(out["prior_mean"], lo),
                                      ptr(out["prior_std"], lo), ptr(out["kl"], lo), ptr(out.get("reward"), lo), ptr(out["state"], lo),
                                      ptr(out["normals"], lo))

        if self.pool is None or n < 2 * self.threads:
            run(0, n)
        else:
            cuts = np.linspace(0, n, self.threads + 1).astype(int)
            list(self.pool.map(lambda k: run(int(cuts[k]), int(cuts[k + 1])), range(self.threads)))
        return out
