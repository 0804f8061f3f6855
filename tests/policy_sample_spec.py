"""PolicySampleSpec: the binary32 specification of the Dreamer agent's sampled modes (tests/policy_sample_spec.c,
which includes policy_spec.c), built and loaded the way policy_spec.py builds PolicySpec.  `act_packed` takes the draw's keys -
(global env, episode, agent step, slot) per car - and can return the normals it drew, the winning candidate and the actor's
distribution; `EpisodeClock` keeps the two counters the device reads for an env that is driven with auto-reset."""
import ctypes as C
import os

import numpy as np

import policy_spec as ps

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_sample_spec.c")
MODES = {"mean": 0, "deploy": 1, "explore": 2}
EXPL_DEFAULT = {"mean": 0.0, "deploy": 0.0, "explore": 0.3}
N_NORMALS = 236          # per car: posterior 32 | block 8: 4 | candidates 200
f32 = np.float32
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = ps.build_and_load("policy_sample_spec", [SRC, ps.SRC])
    lib.pss_act.restype = None
    lib.pss_act.argtypes = [C.POINTER(ps._Weights), C.c_int, C.c_uint32, C.c_uint32, C.c_float, C.c_int] + [C.c_void_p] * 8
    lib.pss_map.restype = None
    lib.pss_map.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.pss_scores.restype = None
    lib.pss_scores.argtypes = [C.c_void_p] * 3
    lib.pss_normals.restype = None
    lib.pss_normals.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    _lib = lib
    return lib


def scalar_map(which, x):
    """The spec's log / softplus over a float32 array."""
    x = np.ascontiguousarray(x, f32)
    y = np.empty_like(x)
    load().pss_map({"log": 0, "softplus": 1}[which], x.size, x.ctypes.data, y.ctypes.data)
    return y


def normals(key, first_block, n_blocks, seed):
    """The 4 n_blocks normals of blocks first_block .. of the car with key = (global env, episode, agent step, slot)."""
    k = np.asarray(key, np.uint32)
    out = np.empty(4 * n_blocks, f32)
    load().pss_normals(k.ctypes.data, first_block, n_blocks, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, out.ctypes.data)
    return out


def scores(dist, cand):
    """The 100 candidates' scores as the spec computes them: dist = (mu 0, mu 1, sd 0, sd 1), cand [100, 2] normals."""
    d, c = np.ascontiguousarray(dist, f32), np.ascontiguousarray(cand, f32)
    out = np.empty(100, f32)
    load().pss_scores(d.ctypes.data, c.ctypes.data, out.ctypes.data)
    return out


class EpisodeClock:
    """The env's `episode` and `agent_steps` counters as the kernels keep them (auto-reset on): a reset of all envs starts
    episode + 1 at agent step 0; a step that respawns the env (its `fresh` flag) does the same, any other step adds one."""

    def __init__(self, num_envs, cars_per_env=1, first_env=0):
        self.cars = int(cars_per_env)
        self.first_env = int(first_env)
        self.episode = np.zeros(num_envs, np.uint32)
        self.agent_steps = np.zeros(num_envs, np.uint32)

    def reset(self):
        self.episode += 1
        self.agent_steps[:] = 0

    def step(self, fresh):
        fr = np.asarray(fresh).reshape(len(self.episode), self.cars)[:, 0] != 0
        self.episode += fr.astype(np.uint32)
        self.agent_steps = np.where(fr, 0, self.agent_steps + 1).astype(np.uint32)

    def keys(self):
        e = np.repeat(np.arange(len(self.episode)), self.cars)
        return np.stack([self.first_env + e, self.episode[e], self.agent_steps[e], np.tile(np.arange(self.cars), len(self.episode))], 1).astype(np.uint32)


class PolicySampleSpec(ps.PolicySpec):
    def __init__(self, weights, mode="deploy", seed=0, expl_amount=None, threads=8):
        super().__init__(weights, threads)
        self.slib = load()
        self.set_sampling(mode, seed, expl_amount)

    def set_sampling(self, mode="mean", seed=0, expl_amount=None):
        self.mode, self.seed = mode, int(seed)
        self.expl_amount = EXPL_DEFAULT[mode] if expl_amount is None else float(expl_amount)

    def act_packed(self, scan_m, state, fresh=None, keys=None, detail=False):
        """As PolicySpec.act_packed, with keys uint32 [n, 4] = (global env, episode, agent step, slot) per car.  detail: also
        returns dict(normals [n, 236], winner [n], dist [n, 4])."""
        scan = np.ascontiguousarray(scan_m, f32).reshape(-1, 1080)
        n = len(scan)
        st = np.array(state, f32, copy=True).reshape(n, ps.STATE)
        fr = None if fresh is None else np.ascontiguousarray(np.asarray(fresh).reshape(n) != 0, np.uint8)
        ky = np.zeros((n, 4), np.uint32) if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(n, 4)
        assert self.mode == "mean" or keys is not None
        act = np.empty((n, 2), f32)
        nrm, win, dist = np.zeros((n, N_NORMALS), f32), np.full(n, -1, np.int32), np.zeros((n, 4), f32)

        def run(lo, hi):
            if hi > lo:
                self.slib.pss_act(C.byref(self.w), MODES[self.mode], self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF, self.expl_amount,
                                  hi - lo, scan[lo:hi].ctypes.data, st[lo:hi].ctypes.data, None if fr is None else fr[lo:hi].ctypes.data,
                                  ky[lo:hi].ctypes.data, act[lo:hi].ctypes.data, nrm[lo:hi].ctypes.data, win[lo:hi].ctypes.data, dist[lo:hi].ctypes.data)

        if self.pool is None or n < 2 * self.threads:
            run(0, n)
        else:
            cuts = np.linspace(0, n, self.threads + 1).astype(int)
            list(self.pool.map(lambda k: run(int(cuts[k]), int(cuts[k + 1])), range(self.threads)))
        return (act, st, dict(normals=nrm, winner=win, dist=dist)) if detail else (act, st)

    def act(self, scan_m, state, reset=None, keys=None):
        packed = np.concatenate([state["stoch"], state["deter"], state["action"]], 1).astype(f32)
        action, st = self.act_packed(scan_m, packed, reset, keys)
        return action, dict(stoch=st[:, :30].copy(), deter=st[:, 30:230].copy(), action=st[:, 230:].copy())
