"""The binary32 specification of the observation decoder's Bernoulli log-likelihood (rc_policy_decode_loglik;
tests/policy_decode_loglik_spec.c, which includes policy_sample_spec.c), built and loaded the way policy_spec.py builds its
library.  `loglik(logits, target)` takes the logits of PolicyDecodeSpec.decode and a uint8 target of the same shape."""
import ctypes as C
import os

import numpy as np

import policy_sample_spec as pss
import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_decode_loglik_spec.c")
IMG = 64
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = ps.build_and_load("policy_decode_loglik_spec", [SRC, pss.SRC, ps.SRC])
        _lib.pdl_loglik.restype = None
        _lib.pdl_loglik.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def loglik(logits, target):
    """logits float32 [..., 64, 64], target uint8 [..., 64, 64] -> float32 [...]"""
    lg = np.ascontiguousarray(logits, np.float32)
    tg = np.ascontiguousarray(target, np.uint8)
    assert lg.shape == tg.shape and lg.shape[-2:] == (IMG, IMG)
    lead = lg.shape[:-2]
    out = np.empty(int(np.prod(lead, dtype=np.int64)), np.float32)
    load().pdl_loglik(out.size, lg.ctypes.data, tg.ctypes.data, out.ctypes.data)
    return out.reshape(lead)
