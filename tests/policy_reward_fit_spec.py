"""PolicyRewardFitSpec: the binary32 specification of the reward head's fit (rc_policy_fit_step with
RC_POLICY_FIT_REWARD; tests/policy_reward_fit_spec.c, which includes policy_fit_spec.c and through it the other specs), built and
loaded the way policy_fit_spec.py builds its library.  A PolicyRewardFitSpec owns the head's six arrays (copies, updated in place by
`step`), its Adam moments and its step count."""
import ctypes as C
import os

import numpy as np

import policy_fit_spec as pfs
import policy_imagine_spec as pis
import policy_returns_spec as prs
import policy_sample_spec as pss
import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_reward_fit_spec.c")
LAYERS = ("h0_w", "h0_b", "h1_w", "h1_b", "hout_w", "hout_b")
KEYS = tuple("reward_" + k for k in LAYERS)
SHAPES = ((230, 400), (400,), (400, 400), (400,), (400, 1), (1,))
N_GRAD = 253201
DEFAULTS = dict(lr=6e-4, clip=1.0, beta1=0.9, beta2=0.999, epsilon=1e-7)      # the reference's model_lr, grad_clip; TF's Adam
f32 = np.float32
_lib = None


class _Head(C.Structure):
    _fields_ = [("h_w", C.c_void_p * 2), ("h_b", C.c_void_p * 2), ("out_w", C.c_void_p), ("out_b", C.c_void_p)]


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = ps.build_and_load("policy_reward_fit_spec", [SRC, pfs.SRC, prs.SRC, pis.SRC, pss.SRC, ps.SRC])
    lib.prfs_grad_size.restype = C.c_int
    lib.prfs_step.restype = None
    lib.prfs_step.argtypes = [C.POINTER(_Head), C.POINTER(pfs._Opt), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(pfs._Hyper),
                              C.c_void_p, C.c_void_p]
    _lib = lib
    return lib


def split(flat):
    """A flat [253 201] vector in the order of the gradient -> the six arrays by layer name (copies)."""
    out, at = {}, 0
    for k, shape in zip(LAYERS, SHAPES):
        size = int(np.prod(shape))
        out[k] = np.array(flat[at:at + size]).reshape(shape)
        at += size
    assert at == len(flat)
    return out


class PolicyRewardFitSpec:
    def __init__(self, heads):
        """heads: a mapping with the `reward_*` arrays (copied)."""
        self.lib = load()
        self.n_grad = self.lib.prfs_grad_size()
        self.arrays = {k: np.array(heads[f"reward_{k}"], dtype=f32, order="C") for k in LAYERS}
        for k, shape in zip(LAYERS, SHAPES):
            assert self.arrays[k].shape == shape, (k, self.arrays[k].shape)
        hd = _Head()
        for l in range(2):
            hd.h_w[l] = self.arrays[f"h{l}_w"].ctypes.data
            hd.h_b[l] = self.arrays[f"h{l}_b"].ctypes.data
        hd.out_w, hd.out_b = self.arrays["hout_w"].ctypes.data, self.arrays["hout_b"].ctypes.data
        self.hd = hd
        self.m, self.v = np.zeros(self.n_grad, f32), np.zeros(self.n_grad, f32)
        self.opt = pfs._Opt(self.m.ctypes.data, self.v.ctypes.data, 1.0, 1.0, 0)

    @property
    def step_count(self):
        return int(self.opt.step)

    def weights(self):
        """The head's arrays under the checkpoint's names (copies)."""
        return {f"reward_{k}": a.copy() for k, a in self.arrays.items()}

    def step(self, features, target, weight=None, **hyper):
        """One update on features [N, 230], target [N], weight [N] or None.  Returns a dict: loss, grad_norm (float32), skipped,
        step (int), grad (the six arrays of the gradient before the clip, by layer name), grad_flat."""
        feat = np.ascontiguousarray(features, f32).reshape(-1, 230)
        n = len(feat)
        tgt = np.ascontiguousarray(target, f32).reshape(n)
        wgt = None if weight is None else np.ascontiguousarray(weight, f32).reshape(n)
        hp = pfs._Hyper(**{**DEFAULTS, **hyper})
        grad, status = np.empty(self.n_grad, f32), np.empty(4, f32)
        self.lib.prfs_step(C.byref(self.hd), C.byref(self.opt), n, feat.ctypes.data, tgt.ctypes.data,
                           None if wgt is None else wgt.ctypes.data, C.byref(hp), grad.ctypes.data, status.ctypes.data)
        return dict(loss=status[0], grad_norm=status[1], skipped=int(status[2]), step=int(status[3]), grad=split(grad), grad_flat=grad)
