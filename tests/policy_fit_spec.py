"""The binary32 specification of the fit engine (tests/policy_fit_spec.c and, on top of it, tests/policy_actor_fit_spec.c, which
includes it and through it the other specs): one library, built and loaded the way policy_returns_spec.py builds its own, and FitSpec,
the base of PolicyFitSpec (the critic's heads, DESIGN.md §2 item 21, rc_policy_fit_step), PolicyRewardFitSpec (item 24) and
PolicyActorFitSpec (item 25).  A FitSpec owns one network's arrays (copies, updated in place by `step`), its Adam moments and its
step count."""
import ctypes as C
import os

import numpy as np

import policy_imagine_spec as pis
import policy_returns_spec as prs
import policy_sample_spec as pss
import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_fit_spec.c")
ACTOR_SRC = os.path.join(HERE, "policy_actor_fit_spec.c")           # the top of the include chain
HEADS = {"value": 0, "pcont": 1}
LAYERS = ("h0_w", "h0_b", "h1_w", "h1_b", "h2_w", "h2_b", "hout_w", "hout_b")
SHAPES = ((230, 400), (400,), (400, 400), (400,), (400, 400), (400,), (400, 1), (1,))
N_GRAD = 413601
DEFAULTS = dict(lr=8e-5, clip=1.0, beta1=0.9, beta2=0.999, epsilon=1e-7)
f32 = np.float32
_lib = None


class _Net(C.Structure):
    _fields_ = [("depth", C.c_int32), ("n_out", C.c_int32), ("h_w", C.c_void_p * 4), ("h_b", C.c_void_p * 4), ("out_w", C.c_void_p), ("out_b", C.c_void_p)]


class _Rows(C.Structure):
    _fields_ = [("kind", C.c_int32)] + [(k, C.c_void_p) for k in ("target", "weight", "eps", "grad")]


class _Opt(C.Structure):
    _fields_ = [("m", C.c_void_p), ("v", C.c_void_p), ("b1pow", C.c_double), ("b2pow", C.c_double), ("step", C.c_int32)]


class _Hyper(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("lr", "clip", "beta1", "beta2", "epsilon")]


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = ps.build_and_load("policy_fit_spec", [ACTOR_SRC, SRC, prs.SRC, pis.SRC, pss.SRC, ps.SRC])
    lib.pfs_grad_size.restype = C.c_int
    lib.pfs_grad_size.argtypes = [C.POINTER(_Net)]
    lib.pfs_tree.restype = C.c_double
    lib.pfs_tree.argtypes = [C.c_void_p, C.c_int64, C.c_int]
    for step in (lib.pfs_head_step, lib.pafs_step):
        step.restype = None
        step.argtypes = [C.POINTER(_Net), C.POINTER(_Opt), C.POINTER(_Rows), C.c_int, C.c_void_p, C.POINTER(_Hyper)] + [C.c_void_p] * 4
    lib.pafs_forward.restype = None
    lib.pafs_forward.argtypes = [C.POINTER(_Net), C.c_int] + [C.c_void_p] * 5
    _lib = lib
    return lib


def tree_sum(x, square=False):
    """The spec's fixed tree over a float32 array, in binary64."""
    x = np.ascontiguousarray(x, f32).reshape(-1)
    return load().pfs_tree(x.ctypes.data, x.size, int(square))


def split(flat, layers, shapes):
    """A flat vector in the order of the gradient -> the network's arrays by layer name (copies)."""
    out, at = {}, 0
    for k, shape in zip(layers, shapes):
        size = int(np.prod(shape))
        out[k] = np.array(flat[at:at + size]).reshape(shape)
        at += size
    assert at == len(flat)
    return out


def _ptr(a):
    return None if a is None else a.ctypes.data


def _as(a, *shape):
    return None if a is None else np.ascontiguousarray(a, f32).reshape(shape)


class FitSpec:
    """The engine over one network.  A subclass names LAYERS (the arrays in the order of the gradient), SHAPES, N_GRAD, DEFAULTS, the
    PREFIX of its arrays in the checkpoint, the KIND of its rule, the library's STEP and whether a step also returns grad_features and out."""
    LAYERS, SHAPES, N_GRAD, DEFAULTS, PREFIX, KIND, STEP, DOWN_TO_THE_FEATURES = LAYERS, SHAPES, N_GRAD, DEFAULTS, "", 0, "pfs_head_step", False

    def __init__(self, weights):
        """weights: a mapping with the network's arrays under PREFIX + the layer names (copied)."""
        self.lib = load()
        self.arrays = {k: np.array(weights[self.PREFIX + k], dtype=f32, order="C") for k in self.LAYERS}
        for k, shape in zip(self.LAYERS, self.SHAPES):
            assert self.arrays[k].shape == shape, (k, self.arrays[k].shape)
        net = _Net(len(self.LAYERS) // 2 - 1, self.SHAPES[-1][0])
        for l in range(net.depth):
            net.h_w[l] = self.arrays[f"h{l}_w"].ctypes.data
            net.h_b[l] = self.arrays[f"h{l}_b"].ctypes.data
        net.out_w, net.out_b = self.arrays["hout_w"].ctypes.data, self.arrays["hout_b"].ctypes.data
        self.net = net
        self.n_grad = self.lib.pfs_grad_size(C.byref(net))
        assert self.n_grad == self.N_GRAD
        self.m, self.v = np.zeros(self.n_grad, f32), np.zeros(self.n_grad, f32)
        self.opt = _Opt(self.m.ctypes.data, self.v.ctypes.data, 1.0, 1.0, 0)

    @property
    def step_count(self):
        return int(self.opt.step)

    def weights(self):
        """The network's arrays under the checkpoint's names (copies)."""
        return {self.PREFIX + k: a.copy() for k, a in self.arrays.items()}

    def _step(self, features, hyper, **given):
        """One update on features [N, 230] under the rule's rows `given`: weight [N], and target, eps, grad [N] at one output, [N, 2]
        at four; None where absent.  Returns a dict: loss, grad_norm (float32), skipped, step (int), grad (the arrays of the gradient
        before the clip, by layer name), grad_flat and, where DOWN_TO_THE_FEATURES, grad_features [N, 230] and out [N, n_out] (the
        output layer before the step)."""
        feat = _as(features, -1, 230)
        n = len(feat)
        given = {k: _as(a, *((n,) if k == "weight" or self.net.n_out == 1 else (n, 2))) for k, a in given.items()}
        rw = _Rows(self.KIND, **{k: _ptr(a) for k, a in given.items()})
        hp = _Hyper(**{**self.DEFAULTS, **hyper})
        grad, status = np.empty(self.n_grad, f32), np.empty(4, f32)
        gfeat, out = (np.empty((n, 230), f32), np.empty((n, self.net.n_out), f32)) if self.DOWN_TO_THE_FEATURES else (None, None)
        getattr(self.lib, self.STEP)(C.byref(self.net), C.byref(self.opt), C.byref(rw), n, feat.ctypes.data, C.byref(hp), grad.ctypes.data,
                                     _ptr(gfeat), _ptr(out), status.ctypes.data)
        got = dict(loss=status[0], grad_norm=status[1], skipped=int(status[2]), step=int(status[3]), grad=split(grad, self.LAYERS, self.SHAPES),
                   grad_flat=grad)
        if self.DOWN_TO_THE_FEATURES:
            got.update(grad_features=gfeat, out=out)
        return got


class HeadFitSpec(FitSpec):
    """A head with one output under Normal(o, 1) (KIND 0) or the Bernoulli likelihood (KIND 1)."""

    def step(self, features, target, weight=None, **hyper):
        """One update on features [N, 230], target [N], weight [N] or None: FitSpec._step's dict."""
        return self._step(features, hyper, target=target, weight=weight)


class PolicyFitSpec(HeadFitSpec):
    def __init__(self, critic, head="value"):
        """critic: a mapping with the head's `value_*` / `pcont_*` arrays (copied)."""
        self.head, self.PREFIX, self.KIND = head, head + "_", HEADS[head]
        super().__init__(critic)
