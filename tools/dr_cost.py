"""Cost of per-episode domain randomization (include/racecar_hip.h, rc_set_vehicle_randomization / rc_set_lidar_noise): ms per
step and per-kernel times of the headline workload (65 536 envs x 1 car, austria, 1080-beam lidar, random-action rollout) with
the features off, vehicle randomization on (spec.DR_DEPLOYMENT_LOCK + wide longitudinal bands), LiDAR noise on (sigma 0.3 m,
p_drop 0.05) and both - the headline's loop: `--settle` untimed steps after the reset, the warm-up, then `--steps` steps
between two stream events; each kernel then timed in a pass of its own (launch-attached events on that kernel only), as bench.py
does.  The four configurations run interleaved for `--rounds` rounds (the median is reported), so that a drift of the clocks
does not land on one of them.  Prints ONE JSON line.

    python tools/dr_cost.py [--envs 65536] [--track austria] [--steps 200] [--warmup 20] [--settle 150] [--rounds 3]
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

CONFIGS = ("off", "vehicle", "noise", "both")
WIDE_LO = (0.168, 2.0, 0.4, 3.0, 0.02)
WIDE_HI = (0.294, 8.0, 1.6, 8.0, 0.05)


def make_env(name, args):
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv(args.track, args.envs, 1, auto_reset=True)
    if name in ("vehicle", "both"):
        env.set_vehicle_randomization(WIDE_LO, WIDE_HI, seed=1)
    if name in ("noise", "both"):
        env.set_lidar_noise(0.3, 0.05, seed=2)
    return env


def time_one(env, args, k0):
    """(ms per step between two stream events, wall ms per step, per-kernel ms) after settle + warm-up."""
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
    kt, k = {}, k0 + args.warmup + args.steps
    for kid in (L.K_RAYCAST, L.K_DYNAMICS):
        env.reset_kernel_times()
        env.set_profiling(True, kernels=[kid])
        env.sync()
        for j in range(min(args.steps, 100)):
            env.step_random(seed=1, step=k + j)
        k += min(args.steps, 100)
        env.sync()
        env.set_profiling(False)
        v = env.kernel_times()[L.KERNEL_NAMES[kid]]
        kt[L.KERNEL_NAMES[kid]] = v["avg_ms"]
    torch.cuda.set_stream(torch.cuda.default_stream())
    return gpu, wall, kt


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--track", default="austria")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--settle", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    envs = {name: make_env(name, args) for name in CONFIGS}
    names = {name: envs[name].scan_kernel_name() for name in CONFIGS}
    runs = {name: [] for name in CONFIGS}
    for r in range(args.rounds):
        for name in CONFIGS:
            runs[name].append(time_one(envs[name], args, 1000 * (r + 1)))
    out = {"tool": "tools/dr_cost.py", "envs": args.envs, "cars_per_env": 1, "track": args.track, "obs_type": "lidar",
           "action_repeat": 1, "steps": args.steps, "warmup": args.warmup, "settle_steps": args.settle, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "vehicle_bands": {"lo": WIDE_LO, "hi": WIDE_HI},
           "noise": {"sigma": 0.3, "p_drop": 0.05}, "configs": {}}
    for name in CONFIGS:
        gpu = statistics.median(x[0] for x in runs[name])
        wall = statistics.median(x[1] for x in runs[name])
        kt = {k: round(statistics.median(x[2][k] for x in runs[name]), 4) for k in runs[name][0][2]}
        out["configs"][name] = {"gpu_ms_per_step": round(gpu, 4), "ms_per_step": round(wall, 4),
                                "env_steps_per_s": round(args.envs / (wall * 1e-3)), "kernels_ms": kt, "scan_kernel": names[name]}
    off = out["configs"]["off"]
    for name in CONFIGS[1:]:
        c = out["configs"][name]
        c["step_over_off"] = round(c["gpu_ms_per_step"] / off["gpu_ms_per_step"], 3)
        c["scan_over_off"] = round(c["kernels_ms"]["rc_raycast_kernel"] / off["kernels_ms"]["rc_raycast_kernel"], 3)
        c["dynamics_over_off"] = round(c["kernels_ms"]["rc_dynamics_kernel"] / off["kernels_ms"]["rc_dynamics_kernel"], 3)
    out["noise_scan_target"] = "noisy scan <= 1.25 x the clean scan"
    out["noise_scan_target_met"] = out["configs"]["noise"]["scan_over_off"] <= 1.25
    for e in envs.values():
        e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
