"""PolicyFitSpec: the binary32 specification of the critic's fit (rc_policy_fit_step; tests/policy_fit_spec.c,
which includes policy_returns_spec.c and through it the other specs), built and loaded the way policy_returns_spec.py builds its
library.  A PolicyFitSpec owns one head's eight arrays (copies, updated in place by `step`), its Adam moments and its step count."""
import ctypes as C
import os

import numpy as np

import policy_imagine_spec as pis
import policy_returns_spec as prs
import policy_sample_spec as pss
import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_fit_spec.c")
HEADS = {"value": 0, "pcont": 1}
LAYERS = ("h0_w", "h0_b", "h1_w", "h1_b", "h2_w", "h2_b", "hout_w", "hout_b")
SHAPES = ((230, 400), (400,), (400, 400), (400,), (400, 400), (400,), (400, 1), (1,))
DEFAULTS = dict(lr=8e-5, clip=1.0, beta1=0.9, beta2=0.999, epsilon=1e-7)
f32 = np.float32
_lib = None


class _Head(C.Structure):
    _fields_ = [("h_w", C.c_void_p * 3), ("h_b", C.c_void_p * 3), ("out_w", C.c_void_p), ("out_b", C.c_void_p)]


class _Opt(C.Structure):
    _fields_ = [("m", C.c_void_p), ("v", C.c_void_p), ("b1pow", C.c_double), ("b2pow", C.c_double), ("step", C.c_int32)]


class _Hyper(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("lr", "clip", "beta1", "beta2", "epsilon")]


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = ps.build_and_load("policy_fit_spec", [SRC, prs.SRC, pis.SRC, pss.SRC, ps.SRC])
    lib.pfs_grad_size.restype = C.c_int
    lib.pfs_tree.restype = C.c_double
    lib.pfs_tree.argtypes = [C.c_void_p, C.c_int64, C.c_int]
    lib.pfs_step.restype = None
    lib.pfs_step.argtypes = [C.POINTER(_Head), C.POINTER(_Opt), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_Hyper),
                             C.c_void_p, C.c_void_p]
    _lib = lib
    return lib


def tree_sum(x, square=False):
    """The spec's fixed tree over a float32 array, in binary64."""
    x = np.ascontiguousarray(x, f32).reshape(-1)
    return load().pfs_tree(x.ctypes.data, x.size, int(square))


def split(flat):
    """A flat [413 601] vector in the order of the gradient -> the eight arrays by layer name (copies)."""
    out, at = {}, 0
    for k, shape in zip(LAYERS, SHAPES):
        size = int(np.prod(shape))
        out[k] = np.array(flat[at:at + size]).reshape(shape)
        at += size
    assert at == len(flat)
    return out


class PolicyFitSpec:
    def __init__(self, critic, head="value"):
        """critic: a mapping with the head's `value_*` / `pcont_*` arrays (copied)."""
        self.lib, self.head = load(), head
        self.n_grad = self.lib.pfs_grad_size()
        self.arrays = {k: np.array(critic[f"{head}_{k}"], dtype=f32, order="C") for k in LAYERS}
        for k, shape in zip(LAYERS, SHAPES):
            assert self.arrays[k].shape == shape, (k, self.arrays[k].shape)
        hd = _Head()
        for l in range(3):
            hd.h_w[l] = self.arrays[f"h{l}_w"].ctypes.data
            hd.h_b[l] = self.arrays[f"h{l}_b"].ctypes.data
        hd.out_w, hd.out_b = self.arrays["hout_w"].ctypes.data, self.arrays["hout_b"].ctypes.data
        self.hd = hd
        self.m, self.v = np.zeros(self.n_grad, f32), np.zeros(self.n_grad, f32)
        self.opt = _Opt(self.m.ctypes.data, self.v.ctypes.data, 1.0, 1.0, 0)

    @property
    def step_count(self):
        return int(self.opt.step)

    def weights(self):
        """The head's arrays under the checkpoint's names (copies)."""
        return {f"{self.head}_{k}": a.copy() for k, a in self.arrays.items()}

    def step(self, features, target, weight=None, **hyper):
        """One update on features [N, 230], target [N], weight [N] or None.  Returns a dict: loss, grad_norm (float32), skipped,
        step (int), grad (the eight arrays of the gradient before the clip, by layer name)."""
        feat = np.ascontiguousarray(features, f32).reshape(-1, 230)
        n = len(feat)
        tgt = np.ascontiguousarray(target, f32).reshape(n)
        wgt = None if weight is None else np.ascontiguousarray(weight, f32).reshape(n)
        hp = _Hyper(**{**DEFAULTS, **hyper})
        grad, status = np.empty(self.n_grad, f32), np.empty(4, f32)
        self.lib.pfs_step(C.byref(self.hd), C.byref(self.opt), HEADS[self.head], n, feat.ctypes.data, tgt.ctypes.data,
                          None if wgt is None else wgt.ctypes.data, C.byref(hp), grad.ctypes.data, status.ctypes.data)
        return dict(loss=status[0], grad_norm=status[1], skipped=int(status[2]), step=int(status[3]), grad=split(grad), grad_flat=grad)
