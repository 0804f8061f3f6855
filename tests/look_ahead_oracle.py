"""Test-side restatement of the look-ahead (include/racecar_hip.h, rc_look_ahead) on top of the CPU oracle,
which itself stays as it is.

Per candidate k: a `copy.deepcopy` of the oracle env (OracleRaceEnv, or the tests/dr_oracle.py / tests/track_set_oracle.py
variants: the copy carries their vehicle parameters and per-env tracks), auto-reset switched off on the copy, its `_observe`
replaced with a no-op (the actions are given: no scan is needed), stepped H times under actions[:, k, t].  An env that is
finished is frozen by the oracle's own step (reward +0.0, flags kept), so nothing is special-cased here.  The oracle that was
copied is not touched.
"""
import copy

import numpy as np

from oracle import racecar_oracle as ro

f32, i32 = np.float32, np.int32
OUTPUTS = ("reward", "flags", "return", "length", "final_state", "pose")
DONE, TRUNCATED, WALL, OPPONENT, WRONG_WAY = 1, 2, 4, 8, 16


def flags_of(env):
    """uint8 [n_cars]: bit 0 done, 1 truncated, 2 wall, 3 opponent, 4 wrong_way, as they stand now."""
    bit = lambda a: (np.asarray(a) != 0).astype(np.uint8)
    return bit(env.done) | bit(env.truncated) << 1 | bit(env.wall) << 2 | bit(env.opp) << 3 | bit(env.wrong_way) << 4


def branch(env):
    """A private copy of `env` that steps without resetting and without observing."""
    b = copy.deepcopy(env)
    b.cfg.auto_reset = False
    b._observe = lambda: None
    return b


def look_ahead(env, actions, repeat):
    """The six outputs (numpy, by name) for actions [E, K, H, A, 2] (or [E, K, H, 2] with one car per env)."""
    E, A = env.B, env.A
    actions = np.asarray(actions, f32)
    if actions.ndim == 4 and A == 1:
        actions = actions[:, :, :, None, :]
    assert actions.ndim == 5 and actions.shape[0] == E and actions.shape[3] == A and actions.shape[4] == 2, actions.shape
    K, H = actions.shape[1], actions.shape[2]
    out = {"reward": np.zeros((E, K, H, A), f32), "flags": np.zeros((E, K, H, A), np.uint8), "return": np.zeros((E, K, A), f32),
           "length": np.zeros((E, K), i32), "final_state": np.zeros((E, K, A, 8), f32), "pose": np.zeros((E, K, H, A, 3), f32)}
    for k in range(K):
        b = branch(env)
        finished = b.done.reshape(E, A).any(axis=1)
        for t in range(H):
            b.step(actions[:, k, t], repeat)
            out["length"][~finished, k] = t + 1                       # (the finishing step counted)
            finished = b.done.reshape(E, A).any(axis=1)
            out["reward"][:, k, t] = b.reward.reshape(E, A)
            out["flags"][:, k, t] = flags_of(b).reshape(E, A)
            out["return"][:, k] = out["return"][:, k] + b.reward.reshape(E, A)        # binary32, in step order from +0.0
            out["pose"][:, k, t] = np.stack([b.x, b.y, b.theta], 1).reshape(E, A, 3)
        time = np.repeat(b.steps.astype(f32) * ro.DT, A)
        fs = np.stack([b.x, b.y, b.theta, b.v, b.delta, b.omega, (b.lap - 1).astype(f32) + b.progress, time], 1)
        out["final_state"][:, k] = fs.astype(f32).reshape(E, A, 8)
    return out


def summary_from_rows(reward, flags, done0):
    """`return` and `length` as they follow from `reward` [E, K, H, A], `flags` [E, K, H, A] and done0 [E] (the env was finished
    before the call): the binary32 sum in step order from +0.0, and the steps until some slot's done bit stands."""
    E, K, H, A = reward.shape
    ret = np.zeros((E, K, A), f32)
    for t in range(H):
        ret = ret + reward[:, :, t]
    fin = (flags & DONE).any(axis=3)                                   # [E, K, H]
    first = np.where(fin.any(axis=2), fin.argmax(axis=2) + 1, H).astype(i32)
    return ret, np.where(np.asarray(done0, bool)[:, None], 0, first).astype(i32)


def oracle_state_bytes(env):
    """Every array the oracle holds, as bytes by attribute name (geometry dicts of a track set included): what "the restatement
    leaves the oracle it copied byte-identical" compares."""
    out = {}

    def walk(prefix, v):
        if isinstance(v, np.ndarray):
            out[prefix] = (v.dtype.str, v.shape, v.tobytes())
        elif isinstance(v, dict):
            for k, w in v.items():
                walk(f"{prefix}.{k}", w)
        elif isinstance(v, (list, tuple)):
            for i, w in enumerate(v):
                walk(f"{prefix}[{i}]", w)
        elif isinstance(v, (int, float, str, bool, np.generic, type(None))):
            out[prefix] = v
    for k, v in env.__dict__.items():
        if k != "cfg":
            walk(k, v)
    walk("cfg", dict(env.cfg.__dict__))
    return out
