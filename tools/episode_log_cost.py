"""Cost of the episode log (include/racecar_hip.h, rc_episode_log_*): ms per step of N envs x 1 car on austria, obs `lidar`,
auto-reset, random-action rollout, with the log OFF and ON - two envs of the same process, same seeds - plus the time of the
log's own launches (count + update) between two stream events around them (rc_episode_log_time), at 65 536 envs and at 4 096
(the latency regime, where two more launches show most).  track_set_cost.py's loop: `--settle` untimed steps after the reset, the
warm-up, then `--steps` steps between two stream events; the log's launches then timed in a pass of their own.  Off and on run
interleaved for `--rounds` rounds (the median is reported).  Prints ONE JSON line.

    python tools/episode_log_cost.py [--envs 65536,4096] [--steps 200] [--warmup 20] [--settle 150] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TARGET = 1.05            # on / off at 65 536 envs (set before anything was measured: < 2 % of the step's bytes, two short launches)


def time_one(env, args, k0, log_on):
    import torch
    env.reset(mode="random", seed=0)
    if log_on:
        env.clear_episode_log()
    torch.cuda.set_stream(env.stream)
    for k in range(args.settle):
        env.step_random(seed=2, step=k)
    for k in range(args.warmup):
        env.step_random(seed=1, step=k0 + k)
    env.sync()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(env.stream)
    for k in range(args.steps):
        env.step_random(seed=1, step=k0 + args.warmup + k)
    ev1.record(env.stream)
    env.sync()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.steps * 1e3
    gpu = ev0.elapsed_time(ev1) / args.steps
    own = None
    if log_on:
        n, k = min(args.steps, 100), k0 + args.warmup + args.steps
        env.reset_kernel_times()
        env.set_profiling(True, kernels=[31])          # no RC_K_* timer on: only the log's own event pair is recorded
        env.sync()
        for j in range(n):
            env.step_random(seed=1, step=k + j)
        env.sync()
        env.set_profiling(False)
        ms, launches = env.episode_log_time()
        own = ms / max(launches, 1)
    torch.cuda.set_stream(torch.cuda.default_stream())
    return gpu, wall, own


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--envs", default="65536,4096")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--settle", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    out = {"tool": "tools/episode_log_cost.py", "track": "austria", "obs": "lidar", "cars_per_env": 1, "action_repeat": 1, "steps": args.steps,
           "warmup": args.warmup, "settle_steps": args.settle, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "envs": {}}
    for n in (int(v) for v in args.envs.split(",")):
        envs = {"off": BatchedRaceEnv("austria", n, 1, auto_reset=True), "on": BatchedRaceEnv("austria", n, 1, auto_reset=True)}
        envs["on"].enable_episode_log(n * 32)
        runs = {"off": [], "on": []}
        for r in range(args.rounds):
            for name in ("off", "on"):
                runs[name].append(time_one(envs[name], args, 1000 * (r + 1), name == "on"))
        res = {}
        for name in ("off", "on"):
            gpu = statistics.median(x[0] for x in runs[name])
            wall = statistics.median(x[1] for x in runs[name])
            res[name] = {"gpu_ms_per_step": round(gpu, 4), "ms_per_step": round(wall, 4), "env_steps_per_s": round(n / (wall * 1e-3))}
        res["on"]["log_launches_ms"] = round(statistics.median(x[2] for x in runs["on"]), 5)
        res["on"]["counters_last_round"] = envs["on"].episode_counters
        res["on_over_off"] = round(res["on"]["gpu_ms_per_step"] / res["off"]["gpu_ms_per_step"], 4)
        if n == 65536:
            res["target"] = f"<= {TARGET} x the step with the log off"
            res["target_met"] = res["on_over_off"] <= TARGET
        out["envs"][str(n)] = res
        for e in envs.values():
            e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
