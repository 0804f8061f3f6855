"""PolicyDecodeSpec: the binary32 specification of the observation decoder (rc_policy_decode;
tests/policy_decode_spec.c), built and loaded the way policy_spec.py builds its library.  `decode` takes features [n, 230] =
stoch | deter and returns what the device call returns: logits float32 [n, 64, 64] and image uint8 [n, 64, 64]."""
import ctypes as C
import os

import numpy as np

import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_decode_spec.c")
FEAT, IMG = 230, 64
DECODER_KEYS = ("dec_h1_w", "dec_h1_b", "dec_h2_k", "dec_h2_b", "dec_h3_k", "dec_h3_b", "dec_h4_k", "dec_h4_b", "dec_h5_k", "dec_h5_b")
DECODER_SHAPES = ((230, 64), (64,), (5, 5, 32, 64), (32,), (5, 5, 16, 32), (16,), (6, 6, 8, 16), (8,), (6, 6, 1, 8), (1,))
f32 = np.float32
_lib = None


class _Weights(C.Structure):
    _fields_ = [(k[4:], C.c_void_p) for k in DECODER_KEYS]


def load():
    global _lib
    if _lib is None:
        _lib = ps.build_and_load("policy_decode_spec", [SRC])
        _lib.pds_decode.restype = None
        _lib.pds_decode.argtypes = [C.POINTER(_Weights), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


class PolicyDecodeSpec:
    def __init__(self, weights, threads=8):
        self.lib = load()
        self.arrays = {k: np.ascontiguousarray(weights[k], f32) for k in DECODER_KEYS}
        for k, shape in zip(DECODER_KEYS, DECODER_SHAPES):
            assert self.arrays[k].shape == shape, (k, self.arrays[k].shape)
        self.w = _Weights()
        for k in DECODER_KEYS:
            setattr(self.w, k[4:], self.arrays[k].ctypes.data)
        self.threads = threads
        self.pool = ps.ThreadPoolExecutor(threads) if threads > 1 else None

    def decode(self, features):
        """features [..., 230] -> (logits float32 [..., 64, 64], image uint8 [..., 64, 64])"""
        f = np.ascontiguousarray(features, f32)
        lead = f.shape[:-1]
        f = f.reshape(-1, FEAT)
        n = len(f)
        logits, image = np.empty((n, IMG, IMG), f32), np.empty((n, IMG, IMG), np.uint8)

        def run(lo, hi):
            if hi > lo:
                self.lib.pds_decode(C.byref(self.w), hi - lo, f[lo:].ctypes.data, logits[lo:].ctypes.data, image[lo:].ctypes.data)

        if self.pool is None or n < 2 * self.threads:
            run(0, n)
        else:
            cuts = np.linspace(0, n, self.threads + 1).astype(int)
            list(self.pool.map(lambda k: run(int(cuts[k]), int(cuts[k + 1])), range(self.threads)))
        return logits.reshape(lead + (IMG, IMG)), image.reshape(lead + (IMG, IMG))
