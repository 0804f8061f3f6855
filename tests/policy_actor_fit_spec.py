"""PolicyActorFitSpec: the binary32 specification of the actor's fit (rc_policy_actor_fit_step and
rc_policy_actor_forward; tests/policy_actor_fit_spec.c, which includes policy_fit_spec.c and through it the other specs), built and
loaded the way policy_fit_spec.py builds its library.  A PolicyActorFitSpec owns the actor's ten arrays (copies, updated in place by
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
SRC = os.path.join(HERE, "policy_actor_fit_spec.c")
KEYS = ("h0_w", "h0_b", "h1_w", "h1_b", "h2_w", "h2_b", "h3_w", "h3_b", "hout_w", "hout_b")      # the checkpoint's names
SHAPES = ((230, 400), (400,), (400, 400), (400,), (400, 400), (400,), (400, 400), (400,), (400, 4), (4,))
N_GRAD = 575204
DEFAULTS = dict(lr=8e-5, clip=1.0, beta1=0.9, beta2=0.999, epsilon=1e-7)      # the reference's actor_lr, grad_clip; TF's Adam
f32 = np.float32
_lib = None


class _Actor(C.Structure):
    _fields_ = [("h_w", C.c_void_p * 4), ("h_b", C.c_void_p * 4), ("out_w", C.c_void_p), ("out_b", C.c_void_p)]


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = ps.build_and_load("policy_actor_fit_spec", [SRC, pfs.SRC, prs.SRC, pis.SRC, pss.SRC, ps.SRC])
    lib.pafs_grad_size.restype = C.c_int
    lib.pafs_forward.restype = None
    lib.pafs_forward.argtypes = [C.POINTER(_Actor), C.c_int] + [C.c_void_p] * 5
    lib.pafs_step.restype = None
    lib.pafs_step.argtypes = [C.POINTER(_Actor), C.POINTER(pfs._Opt), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.POINTER(pfs._Hyper), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = lib
    return lib


def split(flat):
    """A flat [575 204] vector in the order of the gradient -> the ten arrays by name (copies)."""
    out, at = {}, 0
    for k, shape in zip(KEYS, SHAPES):
        size = int(np.prod(shape))
        out[k] = np.array(flat[at:at + size]).reshape(shape)
        at += size
    assert at == len(flat)
    return out


def _ptr(a):
    return None if a is None else a.ctypes.data


class PolicyActorFitSpec:
    def __init__(self, weights):
        """weights: a mapping with the actor's `h0_w` .. `hout_b` (copied)."""
        self.lib = load()
        self.n_grad = self.lib.pafs_grad_size()
        assert self.n_grad == N_GRAD
        self.arrays = {k: np.array(weights[k], dtype=f32, order="C") for k in KEYS}
        for k, shape in zip(KEYS, SHAPES):
            assert self.arrays[k].shape == shape, (k, self.arrays[k].shape)
        ac = _Actor()
        for l in range(4):
            ac.h_w[l] = self.arrays[f"h{l}_w"].ctypes.data
            ac.h_b[l] = self.arrays[f"h{l}_b"].ctypes.data
        ac.out_w, ac.out_b = self.arrays["hout_w"].ctypes.data, self.arrays["hout_b"].ctypes.data
        self.ac = ac
        self.m, self.v = np.zeros(self.n_grad, f32), np.zeros(self.n_grad, f32)
        self.opt = pfs._Opt(self.m.ctypes.data, self.v.ctypes.data, 1.0, 1.0, 0)

    @property
    def step_count(self):
        return int(self.opt.step)

    def weights(self):
        """The actor's arrays under the checkpoint's names (copies)."""
        return {k: a.copy() for k, a in self.arrays.items()}

    @staticmethod
    def _rows(features, pairs, weight):
        feat = np.ascontiguousarray(features, f32).reshape(-1, 230)
        n = len(feat)
        two = [None if p is None else np.ascontiguousarray(p, f32).reshape(n, 2) for p in pairs]
        return feat, n, two, None if weight is None else np.ascontiguousarray(weight, f32).reshape(n)

    def forward(self, features, eps=None):
        """action, mean, std [N, 2] of features [N, 230] under eps [N, 2] or None (the mode action)."""
        feat, n, (e,), _ = self._rows(features, (eps,), None)
        out = {k: np.empty((n, 2), f32) for k in ("action", "mean", "std")}
        self.lib.pafs_forward(C.byref(self.ac), n, feat.ctypes.data, _ptr(e), out["action"].ctypes.data, out["mean"].ctypes.data, out["std"].ctypes.data)
        return out

    def step(self, features, target=None, grad_actions=None, eps=None, weight=None, **hyper):
        """One update on features [N, 230] from exactly one of target [N, 2] and grad_actions [N, 2], under eps [N, 2] or None and
        weight [N] or None.  Returns a dict: loss, grad_norm (float32), skipped, step (int), grad (the ten arrays of the gradient
        before the clip, by name), grad_flat, grad_features [N, 230], out [N, 4] (the output layer before the step)."""
        assert (target is None) != (grad_actions is None)
        feat, n, (tgt, ga, e), wgt = self._rows(features, (target, grad_actions, eps), weight)
        hp = pfs._Hyper(**{**DEFAULTS, **hyper})
        grad, status, gfeat, out = np.empty(self.n_grad, f32), np.empty(4, f32), np.empty((n, 230), f32), np.empty((n, 4), f32)
        self.lib.pafs_step(C.byref(self.ac), C.byref(self.opt), n, feat.ctypes.data, _ptr(e), _ptr(wgt), _ptr(tgt), _ptr(ga), C.byref(hp),
                           grad.ctypes.data, gfeat.ctypes.data, out.ctypes.data, status.ctypes.data)
        return dict(loss=status[0], grad_norm=status[1], skipped=int(status[2]), step=int(status[3]), grad=split(grad), grad_flat=grad,
                    grad_features=gfeat, out=out)
