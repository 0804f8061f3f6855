"""Cost of the look-ahead (include/racecar_hip.h, rc_look_ahead) against the same sub-steps done by brute force.

Workload: austria, 1 car per env, 4 096 envs x 64 candidates x 15 agent steps at repeat 4 (262 144 rollouts, 15.7 M sub-steps), from
the state after `--settle` agent steps of follow_the_gap_reference; candidates from planning.shooting_candidates; outputs `return`
+ `length`, and once more with all six.  Timed by the launch's own timestamps (rc_look_ahead_time).
Yardstick, measured in the same run on code the look-ahead does not touch: the dynamics kernel's time per call at repeat 4 on a
handle of 262 144 envs settled the same way (kernel_times()), x 15.  The two are measured alternately for `--rounds` rounds; the
median and the spread of each are reported.  Condition (set before anything was measured): look-ahead <= 1.05 x yardstick.
`--closed-loop`: as a record without a threshold, planning.shooting_act against follow_the_gap_reference in closed loop on austria
and columbia, 1 024 envs, 500 agent steps: mean progress per episode and wall contacts from the episode log.  Prints ONE JSON line.

    python tools/look_ahead_cost.py [--rounds 5] [--launches 20] [--closed-loop] [--out profiles/look_ahead_cost.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TARGET = 1.05
REPEAT = 4
ALL = ("reward", "flags", "return", "length", "final_state", "pose")


def settle(env, steps):
    env.reset(mode="random", seed=0)
    for _ in range(steps):
        env.follow_the_gap_reference(dt=0.01 * REPEAT)
        env.step(None, repeat=REPEAT)
    env.sync()


def time_look_ahead(env, actions, outputs, out, launches):
    env.reset_kernel_times()
    env.set_profiling(True, kernels=[31])             # no RC_K_* timer on: only the look-ahead's own launch is timed
    for _ in range(launches):
        env.look_ahead(actions, repeat=REPEAT, outputs=outputs, out=out)
    env.sync()
    env.set_profiling(False)
    ms, n = env.look_ahead_time()
    return ms / n


def time_dynamics(env, launches):
    from racing_dreamer_amd import _lib as L
    env.reset_kernel_times()
    env.set_profiling(True, kernels=[L.K_DYNAMICS])
    for _ in range(launches):
        env.follow_the_gap_reference(dt=0.01 * REPEAT)
        env.step(None, repeat=REPEAT)
    env.sync()
    env.set_profiling(False)
    return env.kernel_times()["rc_dynamics_kernel"]["avg_ms"]


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5),
            "spread": round((max(xs) - min(xs)) / statistics.median(xs), 4)}


def closed_loop(track, agent, envs, steps):
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.planning import shooting_act
    env = BatchedRaceEnv(track, envs, 1, auto_reset=True, action_repeat=REPEAT, time_limit_steps=250)      # (every env ends two episodes)
    env.enable_episode_log(envs * 64)
    env.reset(mode="random", seed=0)
    for k in range(steps):
        if agent == "shooting":
            shooting_act(env, candidates=64, horizon=15, hold=5, seed=k)
        else:
            env.follow_the_gap_reference()
        env.step(None)
    log = env.episode_log()
    n = int(log["progress"].numel())
    row = {"track": track, "agent": agent, "episodes": n,
           "mean_progress_per_episode": round(float(log["progress"].mean()), 5) if n else None,
           "mean_length": round(float(log["length"].float().mean()), 2) if n else None,
           "wall_contacts": int(((log["flags"] & L.EP_WALL) != 0).sum()) if n else 0}
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=15)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--closed-loop", action="store_true")
    ap.add_argument("--closed-loop-steps", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.planning import shooting_candidates
    E, K, H = args.envs, args.candidates, args.horizon
    env = BatchedRaceEnv("austria", E, 1, auto_reset=True)
    brute = BatchedRaceEnv("austria", E * K, 1, auto_reset=True)
    settle(env, args.settle)
    settle(brute, args.settle)
    actions = shooting_candidates(env, K, H, hold=5, seed=0)
    shapes = {n: (getattr(torch, L.LOOK_AHEAD_OUTPUTS[n][1]), L.LOOK_AHEAD_OUTPUTS[n][2](E, K, H, 1)) for n in ALL}
    out = {n: torch.empty(s, dtype=d, device=env.device) for n, (d, s) in shapes.items()}
    two, six, dyn = [], [], []
    time_look_ahead(env, actions, ("return", "length"), out, 3)          # warm-up
    time_dynamics(brute, 3)
    for _ in range(args.rounds):
        two.append(time_look_ahead(env, actions, ("return", "length"), out, args.launches))
        dyn.append(time_dynamics(brute, args.launches))
        six.append(time_look_ahead(env, actions, ALL, out, args.launches))
    length = out["length"]
    res = {"tool": "tools/look_ahead_cost.py", "device": torch.cuda.get_device_name(0), "track": "austria", "cars_per_env": 1, "envs": E,
           "candidates": K, "horizon": H, "repeat": REPEAT, "rollouts": E * K, "settle_agent_steps": args.settle, "rounds": args.rounds,
           "launches_per_round": args.launches, "rollouts_finished_inside_horizon": int((length < H).sum()),
           "look_ahead_return_length": spread(two), "look_ahead_all_six_outputs": spread(six),
           "dynamics_kernel_per_call_at_rollouts_envs": spread(dyn)}
    yard = H * statistics.median(dyn)
    res["yardstick_ms"] = round(yard, 5)
    res["ratio"] = round(statistics.median(two) / yard, 4)
    res["ratio_all_six_outputs"] = round(statistics.median(six) / yard, 4)
    res["target"] = f"look-ahead (return + length) <= {TARGET} x {H} dynamics calls at {E * K} envs"
    res["target_met"] = res["ratio"] <= TARGET
    res["verdict"] = "met" if res["target_met"] else "missed"
    env.close()
    brute.close()
    if args.closed_loop:
        res["closed_loop"] = {"envs": 1024, "agent_steps": args.closed_loop_steps, "time_limit_steps": 250, "threshold": None,
                              "rows": [closed_loop(t, a, 1024, args.closed_loop_steps) for t in ("austria", "columbia") for a in ("shooting", "follow_the_gap_reference")]}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
