"""Cost of the trained Dreamer agent on the device (rc_policy_act): device time per call against a plain fp32 torch baseline of the
same layers on the same device, and the closed loop policy_act + step(repeat) beside step_random.

    python tools/policy_cost.py [--envs 65536] [--track austria] [--out profiles/policy_cost.json]

    python tools/policy_cost.py --modes [--out profiles/policy_sample_cost.json]

`--modes`: the sampled modes instead (rc_policy_set_sampling) - per-call time of `mean`, `deploy` and `explore` and their closed
loops at repeat 4, all in this one process, with the target deploy <= 1.15 x mean reported as met or missed.

One process.  Device times are RC_K_POLICY events (the dispatch's own start / stop timestamps) after a warm-up, the median over
windows; the torch baseline is timed with stream events around a window of calls (its dozen launches per call included - that is
what it costs).  The baseline is a RATE baseline: torch.addmm sums in another order than the spec."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MACS_PER_CAR = 32 * 200 + 2 * 200 * 600 + 1280 * 200 + 200 * 30 + 230 * 400 + 3 * 400 * 400 + 400 * 2       # 1 081 200
PEAK_TF = 155.0          # measured f32-input MFMA peak of the MI355X


class TorchAgent:
    """The same layers in plain fp32 torch: weights and scans resident, no host copies (torch.addmm / F.elu / a hand-written GRU)."""

    def __init__(self, weights, device):
        import torch
        self.w = {k: torch.from_numpy(np.ascontiguousarray(weights[k], np.float32)).to(device) for k in weights.files if k != "source"}
        w = self.w
        self.obs2_w, self.obs2_b = w["obs2_w"][:, :30].contiguous(), w["obs2_b"][:30].contiguous()
        self.hout_w, self.hout_b = w["hout_w"][:, :2].contiguous(), w["hout_b"][:2].contiguous()

    def act(self, scan, state, fresh):
        import torch
        import torch.nn.functional as F
        w = self.w
        state = state * (fresh == 0).unsqueeze(1).to(torch.float32)
        stoch, deter, prev = state[:, :30], state[:, 30:230], state[:, 230:]
        embed = torch.clamp(scan, 0.0, 15.0) / 15.0 - 0.5
        x = F.elu(torch.addmm(w["img1_b"], torch.cat([stoch, prev], 1), w["img1_w"]))
        mx, mh = torch.addmm(w["gru_bias"][0], x, w["gru_kernel"]), torch.addmm(w["gru_bias"][1], deter, w["gru_recurrent"])
        z, r = torch.sigmoid(mx[:, :200] + mh[:, :200]), torch.sigmoid(mx[:, 200:400] + mh[:, 200:400])
        deter = z * deter + (1.0 - z) * torch.tanh(mx[:, 400:] + r * mh[:, 400:])
        x = F.elu(torch.addmm(w["obs1_b"], torch.cat([deter, embed], 1), w["obs1_w"]))
        stoch = torch.addmm(self.obs2_b, x, self.obs2_w)
        h = torch.cat([stoch, deter], 1)
        for i in range(4):
            h = F.elu(torch.addmm(w[f"h{i}_b"], h, w[f"h{i}_w"]))
        action = torch.tanh(5.0 * torch.tanh(torch.addmm(self.hout_b, h, self.hout_w) / 5.0))
        return action, torch.cat([stoch, deter, action], 1)


def measure(n, args):
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, n, 1, auto_reset=True, remap_actions=True)
    env.load_policy(weights)
    res = {"cars": n}
    with torch.cuda.stream(env.stream):
        out = env.reset(mode="random", seed=1)
        for k in range(args.settle):                       # the agent drives: scans and latents of a run, not of a start
            env.policy_act()
            out = env.step(None, repeat=4)
        env.sync()
        # ---- policy_act alone: RC_K_POLICY events
        windows = []
        for r in range(args.rounds):
            env.reset_kernel_times()
            env.set_profiling(True, kernels=[L.K_POLICY])
            for k in range(args.calls):
                env.policy_act()
            env.sync()
            env.set_profiling(False)
            windows.append(env.kernel_times()["rc_policy_kernel"]["avg_ms"])
        ms = statistics.median(windows)
        res["policy_act_ms"] = round(ms, 4)
        res["policy_act_windows_ms"] = [round(v, 4) for v in windows]
        res["tflops"] = round(2 * MACS_PER_CAR * n / (ms * 1e-3) / 1e12, 2)
        res["fraction_of_155_tf"] = round(res["tflops"] / PEAK_TF, 3)
        # ---- the torch baseline on the same scans
        agent = TorchAgent(weights, env.device)
        scan, fresh = out["lidar"].view(n, 1080), out["fresh"].view(n)
        state = env.policy_state.clone()
        for k in range(5):
            agent.act(scan, state, fresh)
        windows = []
        for r in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(args.calls):
                agent.act(scan, state, fresh)
            b.record()
            b.synchronize()
            windows.append(a.elapsed_time(b) / args.calls)
        res["torch_fp32_ms"] = round(statistics.median(windows), 4)
        res["torch_fp32_windows_ms"] = [round(v, 4) for v in windows]
        res["hip_over_torch"] = round(ms / res["torch_fp32_ms"], 3)
        # ---- closed loop: policy_act + step(None, repeat 4), and step_random at the same repeat
        for name in ("policy", "random"):
            for k in range(10):
                env.policy_act() if name == "policy" else None
                env.step(None, repeat=4) if name == "policy" else env.step_random(seed=3, step=k, repeat=4)
            env.sync()
            t0 = time.perf_counter()
            for k in range(args.loop_steps):
                if name == "policy":
                    env.policy_act()
                    env.step(None, repeat=4)
                else:
                    env.step_random(seed=3, step=100 + k, repeat=4)
            env.sync()
            dt = (time.perf_counter() - t0) / args.loop_steps
            res[f"loop_{name}_ms_per_agent_step"] = round(dt * 1e3, 4)
            res[f"loop_{name}_env_steps_per_s"] = round(n * 4 / dt)
        res["agent_share_of_agent_step"] = round(1.0 - res["loop_random_ms_per_agent_step"] / res["loop_policy_ms_per_agent_step"], 3)
    env.close()
    return res


def measure_modes(n, args):
    """Per-call device time (RC_K_POLICY, both kernels are timed under it) and closed-loop rate of the three modes on one env."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, n, 1, auto_reset=True, remap_actions=True)
    env.load_policy(weights)
    res = {"cars": n}
    with torch.cuda.stream(env.stream):
        env.reset(mode="random", seed=1)
        for k in range(args.settle):
            env.policy_act()
            env.step(None, repeat=4)
        env.sync()
        for mode in ("mean", "deploy", "explore"):
            env.set_policy_sampling(mode, seed=1)
            for k in range(5):
                env.policy_act()
            windows = []
            for r in range(args.rounds):
                env.reset_kernel_times()
                env.set_profiling(True, kernels=[L.K_POLICY])
                for k in range(args.calls):
                    env.policy_act()
                env.sync()
                env.set_profiling(False)
                windows.append(env.kernel_times()["rc_policy_kernel"]["avg_ms"])
            res[f"{mode}_ms"] = round(statistics.median(windows), 4)
            res[f"{mode}_windows_ms"] = [round(v, 4) for v in windows]
        for mode in ("mean", "deploy", "explore"):
            env.set_policy_sampling(mode, seed=1)
            for k in range(10):
                env.policy_act()
                env.step(None, repeat=4)
            env.sync()
            t0 = time.perf_counter()
            for k in range(args.loop_steps):
                env.policy_act()
                env.step(None, repeat=4)
            env.sync()
            dt = (time.perf_counter() - t0) / args.loop_steps
            res[f"loop_{mode}_ms_per_agent_step"] = round(dt * 1e3, 4)
            res[f"loop_{mode}_env_steps_per_s"] = round(n * 4 / dt)
        res["deploy_over_mean"] = round(res["deploy_ms"] / res["mean_ms"], 4)
        res["explore_over_mean"] = round(res["explore_ms"] / res["mean_ms"], 4)
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--track", default="austria")
    ap.add_argument("--checkpoint", default="austria")
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop-steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--modes", action="store_true", help="measure the sampled modes (profiles/policy_sample_cost.json)")
    args = ap.parse_args()
    import torch
    if args.modes:
        out = {"tool": "tools/policy_cost.py --modes", "track": args.track, "checkpoint": args.checkpoint, "device": torch.cuda.get_device_name(0),
               "calls_per_window": args.calls, "windows": args.rounds, "settle_agent_steps": args.settle, "loop_repeat": 4,
               "sizes": [measure_modes(n, args) for n in args.envs]}
        last = out["sizes"][-1]
        out["target_deploy_over_mean"] = 1.15
        out["target_met_at_largest_size"] = bool(last["deploy_over_mean"] <= 1.15)
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
    out = {"tool": "tools/policy_cost.py", "track": args.track, "checkpoint": args.checkpoint, "device": torch.cuda.get_device_name(0),
           "macs_per_car": MACS_PER_CAR, "calls_per_window": args.calls, "windows": args.rounds, "settle_agent_steps": args.settle,
           "sizes": [measure(n, args) for n in args.envs]}
    last = out["sizes"][-1]
    out["condition_hip_no_slower_than_torch_at_largest_size"] = bool(last["policy_act_ms"] <= last["torch_fp32_ms"])
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
