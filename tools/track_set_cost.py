"""Cost of the track set (include/racecar_hip.h, rc_set_track_set): ms per step and per-kernel times of 65 536 envs x 1 car on
BASELINE configs[4]'s three tracks (columbia / austria / barcelona), auto-reset, random-action rollout, for obs `lidar` and
`lidar_occupancy`: MixedTrackEnv (a fixed equal split, one group launch per kernel) against a track set in order `sequential` and
`random` (every env switches track at every reset).  dr_cost.py's loop: `--settle` untimed steps after the reset, the warm-up,
then `--steps` steps between two stream events; each kernel then timed in a pass of its own.  The configurations run interleaved
for `--rounds` rounds (the median is reported).  Prints ONE JSON line.

    python tools/track_set_cost.py [--envs 65536] [--steps 200] [--warmup 20] [--settle 150] [--rounds 3]
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

TRACKS = ("columbia", "austria", "barcelona")
CONFIGS = ("mixed", "sequential", "random")
TARGETS = {"lidar": 1.10, "lidar_occupancy": 1.15}


def make_env(name, obs, args):
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    if name == "mixed":
        n = len(TRACKS)
        return MixedTrackEnv(list(TRACKS), [args.envs // n + (1 if k < args.envs % n else 0) for k in range(n)], obs_type=obs,
                             auto_reset=True)
    return BatchedRaceEnv.with_track_set(list(TRACKS), args.envs, 1, order=name, seed=1, obs_type=obs, auto_reset=True)


def _timed_handles(env):
    """(handle whose timers the group launches / the set's kernels use, handles whose renders are timed)"""
    parts = getattr(env, "parts", None)
    return (parts[0], parts) if parts else (env, [env])


def time_one(env, obs, args, k0):
    import torch
    from racing_dreamer_amd import _lib as L
    env.reset(mode="random", seed=0)
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
    lead, renders = _timed_handles(env)
    kids = (L.K_DYNAMICS, L.K_RAYCAST) + ((L.K_PATCH,) if obs == "lidar_occupancy" else ())
    kt, k = {}, k0 + args.warmup + args.steps
    n = min(args.steps, 100)
    for kid in kids:
        handles = renders if kid == L.K_PATCH else [lead]
        for h in handles:
            h.reset_kernel_times()
            h.set_profiling(True, kernels=[kid])
        env.sync()
        for j in range(n):
            env.step_random(seed=1, step=k + j)
        k += n
        env.sync()
        total = 0.0
        for h in handles:
            h.set_profiling(False)
            v = h.kernel_times()[L.KERNEL_NAMES[kid]]
            total += v["total_ms"] / n
        kt[L.KERNEL_NAMES[kid]] = total
    torch.cuda.set_stream(torch.cuda.default_stream())
    return gpu, wall, kt


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--settle", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--obs", default="lidar,lidar_occupancy")
    args = ap.parse_args()
    import torch
    out = {"tool": "tools/track_set_cost.py", "envs": args.envs, "cars_per_env": 1, "tracks": list(TRACKS), "action_repeat": 1,
           "steps": args.steps, "warmup": args.warmup, "settle_steps": args.settle, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "obs": {}}
    for obs in args.obs.split(","):
        envs = {name: make_env(name, obs, args) for name in CONFIGS}
        runs = {name: [] for name in CONFIGS}
        for r in range(args.rounds):
            for name in CONFIGS:
                runs[name].append(time_one(envs[name], obs, args, 1000 * (r + 1)))
        res = {}
        for name in CONFIGS:
            gpu = statistics.median(x[0] for x in runs[name])
            wall = statistics.median(x[1] for x in runs[name])
            kt = {k: round(statistics.median(x[2][k] for x in runs[name]), 4) for k in runs[name][0][2]}
            res[name] = {"gpu_ms_per_step": round(gpu, 4), "ms_per_step": round(wall, 4), "env_steps_per_s": round(args.envs / (wall * 1e-3)),
                         "kernels_ms": kt}
            if name != "mixed":
                res[name]["scan_kernel"] = envs[name].scan_kernel_name()
        for name in CONFIGS[1:]:
            res[name]["step_over_mixed"] = round(res[name]["gpu_ms_per_step"] / res["mixed"]["gpu_ms_per_step"], 3)
            res[name]["target"] = f"<= {TARGETS[obs]} x MixedTrackEnv's step"
            res[name]["target_met"] = res[name]["step_over_mixed"] <= TARGETS[obs]
        out["obs"][obs] = res
        for e in envs.values():
            e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
