"""PolicyLidarDecodeSpec: the binary32 specification of the LiDAR distance decoder (rc_policy_decode_lidar;
tests/policy_lidar_decode_spec.c, which includes policy_sample_spec.c and through it policy_spec.c), built and loaded the way
policy_spec.py builds its library.  `decode` takes features [..., 230] = stoch | deter and, optionally, a scan [..., 1080] in
metres, and returns what the device call returns: mean, std float32 [..., 1080] and loglik float32 [...]."""
import ctypes as C
import os

import numpy as np

import policy_sample_spec as pss
import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_lidar_decode_spec.c")
FEAT, BEAMS = 230, 1080
KEYS = ("ldec_dense1_w", "ldec_dense1_b", "ldec_dense2_w", "ldec_dense2_b", "ldec_params_w", "ldec_params_b")
SHAPES = ((230, 256), (256,), (256, 512), (512,), (512, 2160), (2160,))
f32 = np.float32
_lib = None


class _Weights(C.Structure):
    _fields_ = [(k[5:], C.c_void_p) for k in KEYS]


def load():
    global _lib
    if _lib is None:
        _lib = ps.build_and_load("policy_lidar_decode_spec", [SRC, pss.SRC, ps.SRC])
        _lib.pls_decode.restype = None
        _lib.pls_decode.argtypes = [C.POINTER(_Weights), C.c_int] + [C.c_void_p] * 5
        _lib.pls_sum.restype = C.c_float
        _lib.pls_sum.argtypes = [C.c_void_p]
    return _lib


def ordered_sum(terms):
    """The spec's fixed-order binary32 sum of 1080 terms."""
    t = np.ascontiguousarray(terms, f32)
    assert t.shape == (BEAMS,)
    return f32(load().pls_sum(t.ctypes.data))


class PolicyLidarDecodeSpec:
    def __init__(self, weights, threads=8):
        self.lib = load()
        self.arrays = {k: np.ascontiguousarray(weights[k], f32) for k in KEYS}
        for k, shape in zip(KEYS, SHAPES):
            assert self.arrays[k].shape == shape, (k, self.arrays[k].shape)
        self.w = _Weights()
        for k in KEYS:
            setattr(self.w, k[5:], self.arrays[k].ctypes.data)
        self.threads = threads
        self.pool = ps.ThreadPoolExecutor(threads) if threads > 1 else None

    def decode(self, features, scan=None):
        """features [..., 230], scan [..., 1080] metres or None -> dict(mean, std [..., 1080]; loglik [...] when a scan is given)"""
        f = np.ascontiguousarray(features, f32)
        lead = f.shape[:-1]
        f = f.reshape(-1, FEAT)
        n = len(f)
        mean, std = np.empty((n, BEAMS), f32), np.empty((n, BEAMS), f32)
        y = ll = None
        if scan is not None:
            y = np.ascontiguousarray(scan, f32).reshape(n, BEAMS)
            ll = np.empty(n, f32)

        def run(lo, hi):
            if hi > lo:
                self.lib.pls_decode(C.byref(self.w), hi - lo, f[lo:].ctypes.data, None if y is None else y[lo:].ctypes.data,
                                    mean[lo:].ctypes.data, std[lo:].ctypes.data, None if ll is None else ll[lo:].ctypes.data)

        if self.pool is None or n < 2 * self.threads:
            run(0, n)
        else:
            cuts = np.linspace(0, n, self.threads + 1).astype(int)
            list(self.pool.map(lambda k: run(int(cuts[k]), int(cuts[k + 1])), range(self.threads)))
        out = dict(mean=mean.reshape(lead + (BEAMS,)), std=std.reshape(lead + (BEAMS,)))
        if ll is not None:
            out["loglik"] = ll.reshape(lead)
        return out
