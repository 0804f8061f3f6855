"""evaluate(): the reference's evaluation protocol for a whole batch, on the device.

dreamer/evaluations/run_evaluation.py:43-64 is "for each track, run N episodes of the agent, log return / length / progress /
time of each" (dreamer/callbacks.py:56-100).  Here every env of a `BatchedRaceEnv` (also one built `with_track_set`) or a
`MixedTrackEnv` drives its first `episodes` episodes; the episode log (`enable_episode_log`, include/racecar_hip.h) keeps the
four numbers of each on the device, and the statistics per (track, car slot) are computed there from the log.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import torch

from . import _lib as L

STATS = ("ret", "length", "progress", "time")
CAUSES = (("wall", L.EP_WALL), ("opponent", L.EP_OPPONENT), ("truncated", L.EP_TRUNCATED), ("wrong_way", L.EP_WRONG_WAY),
          ("own_done", L.EP_OWN_DONE))


def _config(env):
    part = env.parts[0] if hasattr(env, "parts") else env
    return part._cfg, part.action_repeat


def n_tracks(env) -> int:
    if hasattr(env, "parts"):
        return len(env.parts)
    return len(getattr(env, "track_names", ())) or 1


def summarize(log: Dict[str, torch.Tensor], tracks: int, cars_per_env: int) -> Dict[str, torch.Tensor]:
    """Per (track, slot) statistics of an episode log (`env.episode_log()`), computed on the log's device in binary64: `episodes`
    int64 [T, A]; for each of ret, length, progress, time the tensors `<name>_mean`, `_std` (population), `_min`, `_max` [T, A]
    (NaN where a group has no episode); `share_<cause>` = fraction of the group's episodes that ended with that flag set
    (wall, opponent, truncated; wrong_way = seen during the episode; own_done = the car's own done ended it)."""
    G = tracks * cars_per_env
    g = log["track"].to(torch.int64) * cars_per_env + log["slot"].to(torch.int64)
    dev = g.device
    count = torch.bincount(g, minlength=G)
    cf = count.to(torch.float64)
    nan = torch.full((G,), float("nan"), dtype=torch.float64, device=dev)
    out = {"episodes": count.view(tracks, cars_per_env)}
    for name in STATS:
        x = log[name].to(torch.float64)
        mean = torch.zeros(G, dtype=torch.float64, device=dev).index_add_(0, g, x) / cf
        var = torch.zeros(G, dtype=torch.float64, device=dev).index_add_(0, g, (x - mean[g]) ** 2) / cf
        lo = torch.full((G,), float("inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, g, x, "amin")
        hi = torch.full((G,), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, g, x, "amax")
        for key, v in (("mean", mean), ("std", var.sqrt()), ("min", lo), ("max", hi)):
            out[f"{name}_{key}"] = torch.where(count > 0, v, nan).view(tracks, cars_per_env)
    flags = log["flags"].to(torch.int64)
    for cause, bit in CAUSES:
        hit = torch.zeros(G, dtype=torch.float64, device=dev).index_add_(0, g, ((flags & bit) != 0).to(torch.float64))
        out[f"share_{cause}"] = torch.where(count > 0, hit / cf, nan).view(tracks, cars_per_env)
    return out


def evaluate(env, act: Callable, episodes: int = 10, repeat: Optional[int] = None, max_calls: Optional[int] = None,
             reset_mode: str = "grid", seed: Optional[int] = None, poll_every: int = 32) -> Dict[str, object]:
    """Run every env of `env` (auto_reset=True) for its first `episodes` episodes under `act` and return the statistics per
    (track, car slot) - run_evaluation.py's protocol, all envs at once.

    act: callable taking the env.  It either fills `action_in` itself and returns None (`lambda e: e.policy_act()`,
    `lambda e: e.follow_the_gap_reference()`) or returns the actions as a tensor [num_envs, cars_per_env, 2].
    episodes / repeat: the reference's defaults are 10 episodes per track and, for the Dreamer agents, an action repeat of 8
    (run_evaluation.py:76,108); repeat=None keeps the env's `action_repeat`.
    max_calls: the step budget (default: `episodes` episodes of the longest possible length by the env's time limits).

    Only each env's FIRST `episodes` episodes count (the log's per-env quota): a fixed step budget that counts "whatever finished"
    over-weights short episodes - an env that crashes early recycles fast and would contribute many more episodes than one that
    drives full laps.  The loop polls one device counter (`envs_at_quota`) every `poll_every` calls, not every call, and stops
    when every env has reached the quota or at `max_calls`; `unfinished_envs` then says how many had not.

    Returns summarize()'s tensors plus `calls`, `unfinished_envs`, `counters` (the log's) and `tracks`.  The log stays enabled:
    `env.episode_log()` has the rows the statistics were computed from."""
    cfg, own_repeat = _config(env)
    if not cfg.auto_reset:
        raise ValueError("evaluate() needs an env built with auto_reset=True (a finished env must start its next episode itself)")
    if episodes < 1:
        raise ValueError(f"episodes must be >= 1, got {episodes}")
    rep = own_repeat if repeat is None else int(repeat)
    if max_calls is None:
        per_episode = math.ceil(cfg.time_limit / (0.01 * rep)) + 1
        if cfg.time_limit_steps > 0:
            per_episode = min(per_episode, cfg.time_limit_steps)
        max_calls = episodes * per_episode
    env.enable_episode_log(env.n_cars * int(episodes), max_episodes=int(episodes))
    env.reset(mode=reset_mode, seed=seed)
    calls, at_quota = 0, 0
    while calls < max_calls:
        a = act(env)
        env.step(a if isinstance(a, torch.Tensor) else None, rep)
        calls += 1
        if calls % poll_every == 0 or calls == max_calls:
            at_quota = env.episode_counters["envs_at_quota"]
            if at_quota >= env.num_envs:
                break
    counters = env.episode_counters
    out = summarize(env.episode_log(), n_tracks(env), env.cars_per_env)
    out.update(calls=calls, unfinished_envs=env.num_envs - counters["envs_at_quota"], counters=counters, tracks=n_tracks(env))
    return out
