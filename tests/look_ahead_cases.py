"""The cases of the look-ahead tests (tests/test_look_ahead_oracle.py on the CPU, tests/test_gpu_look_ahead.py on the device):
for each, how the oracle env and the device env are configured, how they are settled (the same seeded random actions on both)
and the candidate action sequences.  The settled oracle and its restatement (tests/look_ahead_oracle.py) are computed once per
case and process, shared by the tests that need them and never modified: tests work on copies.

The seeds and candidate amplitudes were chosen on the CPU with the oracle so that the cases the tests count on happen inside
the short horizons (a rollout that ends at a wall, one that ends at another car, one that does not end, a truncation): the
tests assert those counts from the restatement, so a case cannot pass empty."""
import copy
import functools

import numpy as np

from helpers import make_oracle
from oracle import racecar_oracle as ro

TRACK = "columbia"
SETTLE, REPEAT = 40, 4
N_STEP = ro.TASK_N_STEP_PROGRESS

# name -> (E, K, H, A, oracle config, device config, settle seed, candidate seed, steering amplitude)
CASES = {
    "a1": (5, 3, 4, 1, {}, {}, 3, 11, 1.0),
    "a2": (5, 3, 4, 2, {}, {}, 124, 135, 1.0),         # (the seed in 400 whose settling run leaves two cars about to touch)
    "a4": (5, 3, 4, 4, {}, {}, 11, 22, 1.0),
    "wide": (37, 7, 6, 1, {}, {}, 3, 11, 1.0),
    "one": (2, 1, 1, 1, {}, {}, 3, 11, 1.0),
    "long": (2, 2, 64, 1, {}, {}, 3, 11, 1.0),
    "remap": (5, 3, 4, 1, dict(remap_actions=True), dict(remap_actions=True), 3, 11, 1.0),
    "max_speed": (5, 3, 4, 1, dict(task=ro.TASK_MAX_SPEED), dict(task="max_speed"), 3, 11, 1.0),
    "nstep": (5, 3, 4, 4, dict(car_tasks=[-1, N_STEP, N_STEP, N_STEP], n_steps=10),
              dict(car_tasks=[None, "n_step_progress", "n_step_progress", "n_step_progress"], n_steps=10), 11, 22, 1.0),
    "time_limit": (5, 3, 4, 1, dict(time_limit_steps=SETTLE + 2), dict(time_limit_steps=SETTLE + 2), 3, 11, 1.0),
}


def settle_actions(seed, k, n_cars):
    """The settling run's actions of step k: seeded uniform, the motor command made positive so that the cars drive."""
    act = ro.random_actions(seed, k, n_cars)
    act[:, 0] = np.abs(act[:, 0])
    return act


def candidate_actions(seed, E, K, H, A, amplitude=1.0):
    """float32 [E, K, H, A, 2]: seeded uniform candidates, motor in [0, 1], steering in [-amplitude, amplitude]."""
    rng = np.random.default_rng(seed)
    act = rng.uniform(-1.0, 1.0, (E, K, H, A, 2)).astype(np.float32)
    act[..., 0] = np.abs(act[..., 0])
    act[..., 1] *= np.float32(amplitude)
    return act


def reset_mode(A):
    return ("random", ro.RESET_RANDOM) if A == 1 else ("random_ball", ro.RESET_RANDOM_BALL)


def no_scan(env):
    """The look-ahead tests never read a scan: the oracle skips it (the actions do not depend on observations)."""
    env._observe = lambda: None
    return env


def settle_oracle(ora, A, settle_seed, steps=SETTLE, repeat=REPEAT):
    ora.reset(mode=reset_mode(A)[1], seed=settle_seed)
    for k in range(steps):
        ora.step(settle_actions(settle_seed, k, ora.NC), repeat=repeat)
    return ora


def settle_device(env, settle_seed, steps=SETTLE, repeat=REPEAT):
    import torch
    env.reset(mode=reset_mode(env.cars_per_env)[0], seed=settle_seed)
    for k in range(steps):
        env.step(torch.from_numpy(settle_actions(settle_seed, k, env.n_cars)).to(env.device), repeat=repeat)
    return env


@functools.lru_cache(maxsize=None)
def _case(name):
    from look_ahead_oracle import look_ahead
    from racing_dreamer_amd.track_assets import load_track
    E, K, H, A, ocfg, _dcfg, settle_seed, cand_seed, amp = CASES[name]
    ora = no_scan(make_oracle(load_track(TRACK), num_envs=E, cars_per_env=A, auto_reset=True, **ocfg))
    settle_oracle(ora, A, settle_seed)
    actions = candidate_actions(cand_seed, E, K, H, A, amp)
    want = look_ahead(ora, actions, REPEAT)
    for v in (actions, *want.values()):
        v.setflags(write=False)
    return ora, actions, want


def case(name):
    """(a COPY of the settled oracle, the candidate actions, the restatement's outputs) - the last two read-only."""
    ora, actions, want = _case(name)
    return copy.deepcopy(ora), actions, want


def device_env(name, **extra):
    """The device env of a case, settled as its oracle was."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    E, _K, _H, A, _ocfg, dcfg, settle_seed, _cand_seed, _amp = CASES[name]
    return settle_device(BatchedRaceEnv(TRACK, E, A, auto_reset=True, **dcfg, **extra), settle_seed)


def endings(want, done0=None):
    """How the rollouts of a restatement end: counts of (finished by a wall contact, by an opponent contact, truncated, not
    finished), from the flags of each rollout's last step."""
    from look_ahead_oracle import DONE, OPPONENT, TRUNCATED, WALL
    last = want["flags"][:, :, -1]                       # [E, K, A]
    fin = (last & DONE).any(axis=2)
    inside = fin & (want["length"] > 0)
    wall = inside & ((last & WALL) != 0).any(axis=2)
    opp = inside & ((last & OPPONENT) != 0).any(axis=2)
    trunc = inside & ((last & TRUNCATED) != 0).any(axis=2)
    return dict(wall=int(wall.sum()), opponent=int(opp.sum()), truncated=int(trunc.sum()), unfinished=int((~fin).sum()))
