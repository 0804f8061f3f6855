"""Planning against the simulator's true dynamics (`BatchedRaceEnv.look_ahead`): a random-shooting
baseline beside the learned agents, and an expert that sees further than follow-the-gap.

    env.reset(mode="random", seed=0)
    for _ in range(steps):
        shooting_act(env, candidates=64, horizon=15)       # writes action_in
        env.step(None)

The candidates are generated in torch on the env's device; the look-ahead is one launch; the choice is a few torch operations
on [num_envs, candidates] - nothing here is a hot path of its own."""
from __future__ import annotations

from typing import Union

import torch


def shooting_candidates(env, candidates: int, horizon: int, hold: int = 5, seed: int = 0) -> torch.Tensor:
    """float32 [num_envs, candidates, horizon, cars_per_env, 2] on the env's device: piecewise-constant action sequences - a
    new U(-1, 1)^2 draw every `hold` agent steps, from a torch generator seeded with `seed` - in `step`'s convention.
    Candidate 0 repeats the env's current `action_in` ("keep doing what you do" is always among the choices)."""
    K, H, hold = int(candidates), int(horizon), int(hold)
    if K < 1 or H < 1 or hold < 1:
        raise ValueError(f"candidates, horizon and hold must be >= 1 (got {candidates}, {horizon}, {hold})")
    E, A = env.num_envs, env.cars_per_env
    device = torch.device(env.device)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    pieces = (H + hold - 1) // hold
    u = torch.rand((E, K, pieces, A, 2), generator=gen, dtype=torch.float32, device=device) * 2.0 - 1.0
    seq = u.repeat_interleave(hold, dim=2)[:, :, :H].contiguous()
    seq[:, 0] = env.views["action_in"].reshape(E, 1, A, 2).to(torch.float32)
    return seq


def first_best(score: torch.Tensor) -> torch.Tensor:
    """int64 [E]: per row of score [E, K] the LOWEST index among the entries equal to the row's maximum (a NaN never wins)."""
    s = torch.nan_to_num(score, nan=float("-inf"))
    k = torch.arange(s.shape[1], device=s.device).expand_as(s)
    return torch.where(s == s.max(dim=1, keepdim=True).values, k, s.shape[1]).min(dim=1).values


def shooting_act(env, candidates: Union[int, torch.Tensor] = 64, horizon: int = 15, hold: int = 5, seed: int = 0,
                 others: str = "hold", repeat=None) -> torch.Tensor:
    """Random shooting: look ahead under `candidates` sequences per env (`shooting_candidates`, or a tensor of explicit
    sequences [num_envs, K, H, cars_per_env, 2]) and take, per env, the one with the highest true return of car slot 0 - the
    lowest index among equals.  Writes that candidate's first action into `action_in` and returns `action_in`, so
    `env.step(None)` applies it.  With several cars per env, others="hold" keeps the other slots on their current `action_in`
    in every candidate (and so in what is written); others="free" leaves them what the candidates say.  `repeat`: as `look_ahead` (None: the env's default)."""
    if others not in ("hold", "free"):
        raise ValueError(f"others must be 'hold' or 'free', got {others!r}")
    E, A = env.num_envs, env.cars_per_env
    action_in = env.views["action_in"]
    seq = candidates if torch.is_tensor(candidates) else shooting_candidates(env, candidates, horizon, hold, seed)
    seq = seq.to(action_in.device, torch.float32).reshape(E, -1, seq.shape[2], A, 2)
    if A > 1 and others == "hold":
        seq = seq.clone()
        seq[:, :, :, 1:] = action_in.reshape(E, 1, 1, A, 2)[:, :, :, 1:]
    ret = env.look_ahead(seq, repeat=repeat, outputs=("return",))["return"]
    best = first_best(ret[:, :, 0])
    action_in.copy_(seq[torch.arange(E, device=seq.device), best, 0].reshape(action_in.shape))
    return action_in
