"""PolicySpec: the binary32 specification of the deterministic Dreamer agent (tests/policy_spec.c), built at test
time with the system C compiler and loaded with ctypes.  It offers the interface of oracle.dreamer_policy_port.DreamerPolicy
(`initial`, `act(scan_m, state, reset=None)`), so every loop that drives the port drives the spec."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_spec.c")
BUILD_DIR = os.path.join(HERE, "_build")
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c11", "-fPIC", "-shared"]
f32 = np.float32
STATE = 232
_lib = None


class _Weights(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("gru_kernel", "gru_recurrent", "gru_bias", "img1_w", "img1_b", "obs1_w", "obs1_b", "obs2_w", "obs2_b")]
                + [("h_w", C.c_void_p * 4), ("h_b", C.c_void_p * 4), ("hout_w", C.c_void_p), ("hout_b", C.c_void_p)]
                + [(k, C.c_void_p) for k in ("hnorm_mean", "hnorm_var", "hnorm_gamma", "hnorm_beta")])


def _hardware_fma_flags(cc):
    """fmaf is correctly rounded with or without the instruction; with it the spec is some 50 times faster.  Use the flag only
    where the compiler takes it and this CPU has the instruction."""
    try:
        with open("/proc/cpuinfo") as f:
            flags = f.read()
    except OSError:
        return []
    if " fma " not in flags and " fma\n" not in flags:
        return []
    r = subprocess.run([cc, "-mfma", "-x", "c", "-fsyntax-only", "-"], input="int x;", capture_output=True, text=True)
    return ["-mfma"] if r.returncode == 0 else []


def build_and_load(name, sources):
    """Compile sources[0] - the others are the files it includes: they enter the hash only - into _build/<name>_<hash of the
    sources and flags>.so unless it is there, and load it."""
    cc = os.environ.get("CC", "cc")
    flags = CFLAGS + _hardware_fma_flags(cc)
    blobs = []
    for path in sources:
        with open(path, "rb") as f:
            blobs.append(f.read())
    # (the names the libraries have had: one source is hashed with the flags directly, several through a hash of their own)
    body = blobs[0] if len(blobs) == 1 else hashlib.sha256(b"".join(blobs)).digest()
    tag = hashlib.sha256(body + " ".join(flags).encode()).hexdigest()[:16]
    os.makedirs(BUILD_DIR, exist_ok=True)
    so = os.path.join(BUILD_DIR, f"{name}_{tag}.so")
    if not os.path.exists(so):
        fd, tmp = tempfile.mkstemp(suffix=".so", dir=BUILD_DIR)
        os.close(fd)
        subprocess.run([cc, *flags, sources[0], "-o", tmp, "-lm"], check=True)
        os.replace(tmp, so)
    return C.CDLL(so)


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = build_and_load("policy_spec", [SRC])
    lib.ps_act.restype = None
    lib.ps_act.argtypes = [C.POINTER(_Weights), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ps_map.restype = None
    lib.ps_map.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.ps_dense_rows.restype = None
    lib.ps_dense_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ps_postprocess.restype = C.c_float
    lib.ps_postprocess.argtypes = [C.c_float, C.c_float, C.c_float]
    _lib = lib
    return lib


def scalar_map(which, x):
    """The spec's exp / elu / sigmoid / tanh over a float32 array."""
    x = np.ascontiguousarray(x, f32)
    y = np.empty_like(x)
    load().ps_map({"exp": 0, "elu": 1, "sigmoid": 2, "tanh": 3}[which], x.size, x.ctypes.data, y.ctypes.data)
    return y


def dense(x, w, bias):
    """The spec's dense chain alone: x [rows, k] w [k, n] + bias [n], one fmaf chain per output, k ascending."""
    x, w, bias = (np.ascontiguousarray(a, f32) for a in (x, w, bias))
    out = np.empty((len(x), w.shape[1]), f32)
    load().ps_dense_rows(len(x), w.shape[0], w.shape[1], x.ctypes.data, w.ctypes.data, bias.ctypes.data, out.ctypes.data)
    return out


class PolicySpec:
    def __init__(self, weights, threads=8):
        self.lib = load()
        self.arrays = {k: np.ascontiguousarray(weights[k], f32) for k in getattr(weights, "files", None) or weights.keys()
                       if k != "source" and np.asarray(weights[k]).dtype.kind == "f"}
        a = self.arrays
        assert a["obs1_w"].shape == (1280, 200) and a["h0_w"].shape == (230, 400) and a["gru_bias"].shape == (2, 600)
        self.normalized = "hnorm_gamma" in a
        w = _Weights()
        for k in ("gru_kernel", "gru_recurrent", "gru_bias", "img1_w", "img1_b", "obs1_w", "obs1_b", "obs2_w", "obs2_b", "hout_w", "hout_b"):
            setattr(w, k, a[k].ctypes.data)
        for i in range(4):
            w.h_w[i] = a[f"h{i}_w"].ctypes.data
            w.h_b[i] = a[f"h{i}_b"].ctypes.data
        if self.normalized:
            for k in ("hnorm_mean", "hnorm_var", "hnorm_gamma", "hnorm_beta"):
                setattr(w, k, a[k].ctypes.data)
        self.w = w
        self.threads = max(1, int(threads))
        self.pool = ThreadPoolExecutor(self.threads) if self.threads > 1 else None

    def initial(self, n):
        return dict(stoch=np.zeros((n, 30), f32), deter=np.zeros((n, 200), f32), action=np.zeros((n, 2), f32))

    def act_packed(self, scan_m, state, fresh=None):
        """scan [n, 1080] metres, state [n, 232] = stoch | deter | raw previous action (not modified), fresh uint8 [n] or None.
        Returns (raw action [n, 2], new state [n, 232])."""
        scan = np.ascontiguousarray(scan_m, f32).reshape(-1, 1080)
        n = len(scan)
        st = np.array(state, f32, copy=True).reshape(n, STATE)
        fr = None if fresh is None else np.ascontiguousarray(np.asarray(fresh).reshape(n) != 0, np.uint8)
        act = np.empty((n, 2), f32)

        def run(lo, hi):
            if hi > lo:
                self.lib.ps_act(C.byref(self.w), hi - lo, scan[lo:hi].ctypes.data, st[lo:hi].ctypes.data,
                                None if fr is None else fr[lo:hi].ctypes.data, act[lo:hi].ctypes.data)

        if self.pool is None or n < 2 * self.threads:
            run(0, n)
        else:
            cuts = np.linspace(0, n, self.threads + 1).astype(int)
            list(self.pool.map(lambda k: run(int(cuts[k]), int(cuts[k + 1])), range(self.threads)))
        return act, st

    def act(self, scan_m, state, reset=None):
        packed = np.concatenate([state["stoch"], state["deter"], state["action"]], 1).astype(f32)
        action, st = self.act_packed(scan_m, packed, reset)
        return action, dict(stoch=st[:, :30].copy(), deter=st[:, 30:230].copy(), action=st[:, 230:].copy())

    def postprocess(self, action, low=(0.005, -1.0), high=(1.0, 1.0)):
        """postprocess_action's image of a raw action, in the spec's binary32 steps (what rc_policy_act writes when remap_actions is off)."""
        a = np.asarray(action, f32)
        out = np.empty_like(a)
        for j in range(2):
            out[:, j] = [self.lib.ps_postprocess(float(v), float(f32(low[j])), float(f32(high[j]))) for v in a[:, j]]
        return out
