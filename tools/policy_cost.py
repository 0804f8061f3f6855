"""Cost of the trained Dreamer agent on the device (rc_policy_act): device time per call against a plain fp32 torch baseline of the
same layers on the same device, and the closed loop policy_act + step(repeat) beside step_random.

    python tools/policy_cost.py [--envs 65536] [--track austria] [--out profiles/policy_cost.json]

    python tools/policy_cost.py --modes [--out profiles/policy_sample_cost.json]

`--modes`: the sampled modes instead (rc_policy_set_sampling) - per-call time of `mean`, `deploy` and `explore` and their closed
loops at repeat 4, all in this one process, with the target deploy <= 1.15 x mean reported as met or missed.

    python tools/policy_cost.py --imagine [--out profiles/policy_imagine_cost.json]

`--imagine`: imagination (rc_policy_imagine) at H = 15 - `mean`, `sample` and open loop, with the reward only and with all outputs -
beside `policy_act` (`mean`) of the same run, with the target: time per imagined step <= (padded MACs of an imagined step / padded
MACs of an agent step) x the agent's call + 5 %, reported as met or missed.

    python tools/policy_cost.py --decode [--out profiles/policy_decode_cost.json]
    python tools/policy_cost.py --decode-lidar [--out profiles/policy_decode_lidar_cost.json]

`--decode`: the observation decoder (rc_policy_decode) on the live latents of 65 536 cars on treitlstrasse_v2 under obs_type
lidar_occupancy - `image` only, `logits` only, `image` + `mismatch` - beside torch.nn.functional.conv_transpose2d in fp32 on the same
four layers plus the dense layer at the same row count, with the condition `logits` time <= torch's reported as met or missed, and
the fp32 issue floor of the decoder's 1 423 872 fma per image.

    python tools/policy_cost.py --observe [--out profiles/policy_observe_cost.json]

`--observe`: recorded sequences (rc_policy_observe) at 65 536 rows x T = 15, context = T - `mean` with the features only, with the
reward head on top, `sample`, and `mean` with every output - beside `policy_act` (`mean`) of the same run on the same number of cars,
with the condition: time per observed step <= 1.0 x that call (an observed step performs 0.52 of its multiply-adds), and beside the
same 15 steps (posterior, prior and KL) in plain fp32 torch, each reported as met or missed.

    python tools/policy_cost.py --returns [--out profiles/policy_returns_cost.json]

`--returns`: the critic and the lambda-return (rc_policy_returns) at 65 536 starts x H = 15, `mean`, outputs returns + weight, both
heads of a synthetic critic - beside rc_policy_imagine with the reward output on the same cars in the same run, with the condition:
time per step <= 1.734 x that call's (the ratio of the nominal multiply-adds) x 1.05, reported as met or missed; also the value head
alone (1.367), `sample`, policy_value on 65 536 x 230 features, and - a record, not a condition - the three heads and a Python
lambda-return in plain fp32 torch on features already in memory.

    python tools/policy_cost.py --returns-grad [--out profiles/policy_returns_grad_cost.json]

`--returns-grad`: the actor loss's gradient through the dream (rc_policy_returns_grad) at 2 450 starts (the reference's batch of 50 x 50
with a pcont head) and at 65 536 starts, H = 15, `sample`, outputs grad_actions + actor_features + eps, both heads of a synthetic
critic - alternated, window by window, with policy_returns(outputs = returns, weight) on the same cars in the same run, with the
condition: time per call <= that call's x 1.706 (forward + backward multiply-adds over forward multiply-adds: the actor runs forward
only, the prior and the three heads both ways) x 1.05 + the stash's bytes (4 648 floats per row and step, written once and read once)
at the bandwidth of a device-to-device copy measured in that run, reported as met or missed at each size.  Records without a
threshold: world_model.behaviour_learning_step's wall time per step on a 50 x 50 batch, and the call with every forward output.

    python tools/policy_cost.py --fit [--out profiles/policy_fit_cost.json]

`--fit`: one step of the critic's fit (rc_policy_fit_step: forward, backward, clip, Adam on the value head) at 14 336 rows (tools/fit_critic.py's
1 024 envs x 14) and 35 000 rows (the reference's 2 500 starts x 14), beside the same iteration done the way tools/fit_critic.py --fit
torch does it - torch autograd, clip_grad_norm_, Adam.step and the load_critic upload with the synchronisation it forces - with the
condition: device step <= 1.0 x that, reported as met or missed; and, a record without a threshold, the same torch step without the
upload.  All three are wall-clock times per iteration over a window of iterations that ends with a synchronisation.  Then the reward
head's step (reward_fit, the same engine at two hidden layers, 665 200 multiply-adds per row against 1 145 200) beside critic_fit of
the same run, and - a record - the torch step on the reward head's layers (profiles/reward_fit_cost.json).  Then the actor's step
(actor_fit, the engine at four hidden layers: 1 630 404 multiply-adds per row against the value step's 1 146 401, both with the bias
rows) beside critic_fit of the same run under the condition actor_fit <= 1.422 x critic_fit x 1.05, and - records - the step with
grad_features, the forward alone (policy_action) and a plain fp32 torch step on the actor's layers
(profiles/actor_fit_cost.json).  `--device-only` leaves
the torch steps out and `--root DIR` imports the package from another checkout: the two halves of an A/B against a parent build.

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


def _packed_ld():
    """The leading dimensions the weight packer pads to (RC_POLICY_LD* of racing_dreamer_amd/csrc/racecar_policy.h): the columns a
    layer's MFMA tiles cover, so the MACs the kernels issue follow the packing and not a copy of it."""
    import re
    with open(os.path.join(ROOT, "racing_dreamer_amd", "csrc", "racecar_policy.h")) as f:
        ld = {k: int(v) for k, v in re.findall(r"#define RC_POLICY_(LD\w+) (\d+)\b", f.read())}
    assert set(ld) >= {"LD200", "LD400", "LDSMALL", "LDPAIR"}, ld
    return ld


# MACs as the kernels issue them: a layer of K rows costs K x (the packed width its tiles cover)
_LD = _packed_ld()
PADDED_ACTOR = 230 * _LD["LD400"] + 3 * 400 * _LD["LD400"] + 400 * _LD["LDSMALL"]
PADDED_GRU = 32 * _LD["LD200"] + 2 * 200 * 3 * _LD["LD200"]
PADDED_AGENT_STEP = PADDED_GRU + 1280 * _LD["LD200"] + 200 * _LD["LDSMALL"] + PADDED_ACTOR
PADDED_HEAD = 230 * _LD["LD400"] + 400 * _LD["LD400"] + 400 * _LD["LDSMALL"]
# mode mean, closed loop, reward: img3 is packed at LDPAIR (mean | std) and mode mean issues its mean tile only
PADDED_IMAGINED_STEP = PADDED_ACTOR + PADDED_GRU + 200 * _LD["LD200"] + 200 * (_LD["LDPAIR"] // 2) + PADDED_HEAD
# mode sample also issues the std tiles of img3 and of the actor's hout (not in the target's ratio, which is for `mean`)
PADDED_IMAGINED_STEP_SAMPLE = PADDED_IMAGINED_STEP + 200 * (_LD["LDPAIR"] // 2) + 400 * (_LD["LDPAIR"] - _LD["LDSMALL"])
MACS_IMAGINED_STEP = 230 * 400 + 3 * 400 * 400 + 400 * 2 + 32 * 200 + 2 * 200 * 600 + 200 * 200 + 200 * 30 + 230 * 400 + 400 * 400 + 400


class TorchImagine(TorchAgent):
    """H imagined steps (mode mean, closed loop, reward) in plain fp32 torch."""

    def imagine(self, state, horizon):
        import torch
        import torch.nn.functional as F
        w = self.w
        stoch, deter = state[:, :30], state[:, 30:230]
        rewards = []
        for t in range(horizon):
            h = torch.cat([stoch, deter], 1)
            for i in range(4):
                h = F.elu(torch.addmm(w[f"h{i}_b"], h, w[f"h{i}_w"]))
            action = torch.tanh(5.0 * torch.tanh(torch.addmm(self.hout_b, h, self.hout_w) / 5.0))
            x = F.elu(torch.addmm(w["img1_b"], torch.cat([stoch, action], 1), w["img1_w"]))
            mx, mh = torch.addmm(w["gru_bias"][0], x, w["gru_kernel"]), torch.addmm(w["gru_bias"][1], deter, w["gru_recurrent"])
            z, r = torch.sigmoid(mx[:, :200] + mh[:, :200]), torch.sigmoid(mx[:, 200:400] + mh[:, 200:400])
            deter = z * deter + (1.0 - z) * torch.tanh(mx[:, 400:] + r * mh[:, 400:])
            x = F.elu(torch.addmm(w["img2_b"], deter, w["img2_w"]))
            stoch = torch.addmm(w["img3_b"][:30], x, w["img3_w"][:, :30])
            h = torch.cat([stoch, deter], 1)
            for i in range(2):
                h = F.elu(torch.addmm(w[f"reward_h{i}_b"], h, w[f"reward_h{i}_w"]))
            rewards.append(torch.addmm(w["reward_hout_b"], h, w["reward_hout_w"]))
        return torch.cat(rewards, 1)


def measure_imagine(n, args):
    """Per-call device time (RC_K_POLICY) of policy_act (`mean`) and of rc_policy_imagine at H = args.horizon in six variants."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, n, 1, auto_reset=True, remap_actions=True)
    env.load_policy(weights)
    h = args.horizon
    res = {"cars": n, "horizon": h}

    def timed(call):
        for k in range(3):
            call()
        windows = []
        for r in range(args.rounds):
            env.reset_kernel_times()
            env.set_profiling(True, kernels=[L.K_POLICY])
            for k in range(args.calls):
                call()
            env.sync()
            env.set_profiling(False)
            windows.append(env.kernel_times()["rc_policy_kernel"]["avg_ms"])
        return statistics.median(windows), [round(v, 4) for v in windows]

    with torch.cuda.stream(env.stream):
        env.reset(mode="random", seed=1)
        for k in range(args.settle):
            env.policy_act()
            env.step(None, repeat=4)
        env.sync()
        act_ms, act_windows = timed(env.policy_act)
        res["policy_act_mean_ms"], res["policy_act_mean_windows_ms"] = round(act_ms, 4), act_windows
        bufs = dict(reward=torch.empty((n, h), device=env.device), actions=torch.empty((n, h, 2), device=env.device),
                    features=torch.empty((n, h, 230), device=env.device), reward_start=torch.empty(n, device=env.device))
        given = (torch.rand((n, h, 2), device=env.device) * 2.0 - 1.0).contiguous()
        limit = PADDED_IMAGINED_STEP / PADDED_AGENT_STEP * act_ms * 1.05
        res["target_ms_per_imagined_step"] = round(limit, 4)
        for variant, mode, open_loop in (("mean", "mean", False), ("sample", "sample", False), ("open_loop", "mean", True)):
            for outputs in ("reward", "all"):
                tensors = dict(actions_in=given if open_loop else None, reward=bufs["reward"], actions=None, features=None, reward_start=None)
                if outputs == "all":
                    tensors.update(actions=bufs["actions"], features=bufs["features"], reward_start=bufs["reward_start"])
                a = dict(horizon=h, mode=L.IMAGINE_MODES[mode], seed=1, mask=1)
                ms, windows = timed(lambda: L.check(env._imagine(a, tensors, 0, n)))
                macs = MACS_IMAGINED_STEP - (230 * 400 + 3 * 400 * 400 + 400 * 2 if open_loop else 0)
                res[f"{variant}_{outputs}"] = {"ms_per_call": round(ms, 4), "windows_ms": windows, "ms_per_imagined_step": round(ms / h, 4),
                                               "tflops": round(2 * macs * n * h / (ms * 1e-3) / 1e12, 2),
                                               "step_over_policy_act": round(ms / h / act_ms, 4)}
        res["target_met"] = bool(res["mean_reward"]["ms_per_imagined_step"] <= limit)
        res["mean_step_over_target"] = round(res["mean_reward"]["ms_per_imagined_step"] / limit, 4)
        # ---- the torch baseline of the same layers (mode mean, closed loop, reward)
        agent = TorchImagine(weights, env.device)
        state = env.policy_state.clone()
        for k in range(2):
            agent.imagine(state, h)
        windows = []
        for r in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(max(1, args.calls // 4)):
                agent.imagine(state, h)
            e1.record()
            e1.synchronize()
            windows.append(e0.elapsed_time(e1) / max(1, args.calls // 4))
        res["torch_fp32_ms_per_call"] = round(statistics.median(windows), 4)
        res["hip_over_torch"] = round(res["mean_reward"]["ms_per_call"] / res["torch_fp32_ms_per_call"], 3)
    env.close()
    return res


# ---- the critic and the lambda-return: nominal multiply-adds per imagined step
MACS_RETURNS_BASE = MACS_IMAGINED_STEP + 200 * 30                  # actor + prior (img3's 60 columns) + reward head: 1 123 600
MACS_CRITIC_HEAD = 230 * 400 + 2 * 400 * 400 + 400                 # DenseDecoder((), 3, 400): 412 400


class TorchReturns(TorchImagine):
    """The three heads on given features [n, H, 230] in plain fp32 torch, and the lambda-return as a Python loop over the horizon."""

    def __init__(self, weights, critic, device):
        import torch
        super().__init__(weights, device)
        self.c = {k: torch.from_numpy(v).to(device) for k, v in critic.items()}

    def head(self, w, prefix, layers, h):
        import torch
        import torch.nn.functional as F
        for i in range(layers):
            h = F.elu(torch.addmm(w[f"{prefix}_h{i}_b"], h, w[f"{prefix}_h{i}_w"]))
        return torch.addmm(w[f"{prefix}_hout_b"], h, w[f"{prefix}_hout_w"])

    def returns(self, features, lambda_):
        import torch
        n, h, _ = features.shape
        flat = features.reshape(n * h, 230)
        r = self.head(self.w, "reward", 2, flat).reshape(n, h)
        v = self.head(self.c, "value", 3, flat).reshape(n, h)
        p = torch.sigmoid(self.head(self.c, "pcont", 3, flat)).reshape(n, h)
        agg, out = v[:, -1], []
        for t in range(h - 2, -1, -1):
            agg = r[:, t] + p[:, t] * v[:, t + 1] * (1.0 - lambda_) + p[:, t] * lambda_ * agg
            out.append(agg)
        weight = torch.cumprod(torch.cat([torch.ones_like(p[:, :1]), p[:, :-2]], 1), 1)
        return torch.stack(out[::-1], 1), weight


def measure_returns(n, args):
    """Per-call device time (RC_K_POLICY) of rc_policy_returns at H = args.horizon beside rc_policy_imagine with the reward output on
    the same cars in the same run; the value head alone, mode sample, policy_value on n x 230 features; the torch restatement."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.critic import init_critic
    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, n, 1, auto_reset=True, remap_actions=True)
    env.load_policy(weights)
    critic = init_critic(0)
    env.load_critic(critic)
    h = args.horizon
    res = {"cars": n, "horizon": h}

    def timed(call):
        for k in range(3):
            call()
        windows = []
        for r in range(args.rounds):
            env.reset_kernel_times()
            env.set_profiling(True, kernels=[L.K_POLICY])
            for k in range(args.calls):
                call()
            env.sync()
            env.set_profiling(False)
            windows.append(env.kernel_times()["rc_policy_kernel"]["avg_ms"])
        return statistics.median(windows), [round(v, 4) for v in windows]

    def entry(ms, windows, macs, steps):
        return {"ms_per_call": round(ms, 4), "windows_ms": windows, "ms_per_step": round(ms / steps, 4),
                "tflops": round(2 * macs * n * steps / (ms * 1e-3) / 1e12, 2)}

    with torch.cuda.stream(env.stream):
        env.reset(mode="random", seed=1)
        for k in range(args.settle):
            env.policy_act()
            env.step(None, repeat=4)
        env.sync()
        reward = torch.empty((n, h), device=env.device)
        a = dict(horizon=h, mode=L.IMAGINE_MODES["mean"], seed=1, mask=1)
        tensors = dict(actions_in=None, reward=reward, actions=None, features=None, reward_start=None)
        ms, windows = timed(lambda: L.check(env._imagine(a, tensors, 0, n)))
        res["imagine_mean_reward"] = entry(ms, windows, MACS_RETURNS_BASE, h)
        base = ms / h
        out = {k: torch.empty((n, h - 1), device=env.device) for k in ("returns", "weight")}
        out["value"] = torch.empty((n, h), device=env.device)
        for name, mode, pcont, names, macs in (("mean_returns_weight", "mean", True, ("returns", "weight"), MACS_RETURNS_BASE + 2 * MACS_CRITIC_HEAD),
                                               ("sample_returns_weight", "sample", True, ("returns", "weight"), MACS_RETURNS_BASE + 2 * MACS_CRITIC_HEAD),
                                               ("mean_returns_value_head_alone", "mean", False, ("returns",), MACS_RETURNS_BASE + MACS_CRITIC_HEAD)):
            env.load_critic(critic if pcont else {k: v for k, v in critic.items() if k.startswith("value_")})
            ms, windows = timed(lambda: env.policy_returns(h, mode, seed=1, outputs=names, out=out))
            res[name] = entry(ms, windows, macs, h)
            res[name]["step_over_imagine_step"] = round(ms / h / base, 4)
        env.load_critic(critic)
        for name, ratio in (("mean_returns_weight", (MACS_RETURNS_BASE + 2 * MACS_CRITIC_HEAD) / MACS_RETURNS_BASE),
                            ("mean_returns_value_head_alone", (MACS_RETURNS_BASE + MACS_CRITIC_HEAD) / MACS_RETURNS_BASE)):
            limit = ratio * base * 1.05
            res[name].update(macs_ratio=round(ratio, 3), target_ms_per_step=round(limit, 4), met=bool(res[name]["ms_per_step"] <= limit),
                             step_over_target=round(res[name]["ms_per_step"] / limit, 4))
        feats = env.policy_imagine(1, features=True)["feature"].reshape(n, 230).contiguous()
        ms, windows = timed(lambda: env.policy_value(feats))
        res["policy_value_features"] = entry(ms, windows, MACS_CRITIC_HEAD, 1)
        # ---- a record, not a condition: the three heads and the recursion in plain fp32 torch on features already in memory
        features = env.policy_imagine(h, features=True)["feature"]
        agent = TorchReturns(weights, critic, env.device)
        for k in range(2):
            agent.returns(features, 0.95)
        windows = []
        for r in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(max(1, args.calls // 4)):
                agent.returns(features, 0.95)
            e1.record()
            e1.synchronize()
            windows.append(e0.elapsed_time(e1) / max(1, args.calls // 4))
        res["torch_fp32_heads_and_recursion_ms_per_call"] = round(statistics.median(windows), 4)
    env.close()
    return res


# rc_policy_returns_grad beside rc_policy_returns, per row and step, mode sample, both heads: the forward as it is counted above (with
# the actor's two std columns), the backward = the transposed products of the prior and of the three heads; the actor has none
MACS_RGRAD_FORWARD = MACS_RETURNS_BASE + 400 * 2 + 2 * MACS_CRITIC_HEAD                        # 1 949 200
MACS_RGRAD_BACKWARD = ((400 * 400 + 400 * 230 + 400) + 2 * MACS_CRITIC_HEAD                   # reward; value, pcont
                       + 60 * 200 + 200 * 200 + 2 * 600 * 200 + 200 * 32)                     # img3, img2, gru_k, gru_r, img1: 1 375 600
RGRAD_STASH_FLOATS = 4648


def measure_returns_grad(n, args):
    """Per-call device time (RC_K_POLICY) of rc_policy_returns_grad at H = args.horizon, mode sample, alternated window by window with
    rc_policy_returns(returns, weight) on the same cars; the copy bandwidth of the same run; behaviour_learning_step's wall time."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.critic import init_critic
    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, n, 1, auto_reset=True, remap_actions=True)
    env.load_policy(weights)
    env.load_critic(init_critic(0))
    h = args.horizon
    res = {"starts": n, "horizon": h}

    def window(call):
        env.reset_kernel_times()
        env.set_profiling(True, kernels=[L.K_POLICY])
        for k in range(args.calls):
            call()
        env.sync()
        env.set_profiling(False)
        return env.kernel_times()["rc_policy_kernel"]["avg_ms"]

    with torch.cuda.stream(env.stream):
        env.reset(mode="random", seed=1)
        for k in range(args.settle):
            env.policy_act()
            env.step(None, repeat=4)
        env.sync()
        fwd = {k: torch.empty((n, h - 1), device=env.device) for k in ("returns", "weight")}
        bwd = dict(grad_actions=torch.empty((n, h, 2), device=env.device), actor_features=torch.empty((n, h, 230), device=env.device),
                   eps=torch.empty((n, h, 2), device=env.device))
        calls = {"returns": lambda: env.policy_returns(h, "sample", seed=1, outputs=tuple(fwd), out=fwd),
                 "returns_grad": lambda: env.policy_returns_grad(h, "sample", seed=1, outputs=tuple(bwd), out=bwd)}
        for call in calls.values():
            for k in range(3):
                call()
        windows = {k: [] for k in calls}
        for r in range(args.rounds):                     # alternated: a drift of the clocks falls on both
            for k, call in calls.items():
                windows[k].append(window(call))
        # the bandwidth of a device-to-device copy of about the stash's size (at most 1 GiB), bytes copied per second
        stash_bytes = n * h * RGRAD_STASH_FLOATS * 4
        src = torch.empty(min(stash_bytes, 1 << 30) // 4, device=env.device)
        dst = torch.empty_like(src)
        copies = []
        for r in range(args.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            copies.append(src.numel() * 4 / (e0.elapsed_time(e1) * 1e-3))
        copy_bw = statistics.median(copies[1:])
        del src, dst
        base, ms = statistics.median(windows["returns"]), statistics.median(windows["returns_grad"])
        ratio = (MACS_RGRAD_FORWARD + MACS_RGRAD_BACKWARD) / MACS_RGRAD_FORWARD
        stash_ms = stash_bytes / copy_bw * 1e3
        limit = base * ratio * 1.05 + stash_ms
        res["policy_returns_sample_returns_weight"] = {"ms_per_call": round(base, 4), "windows_ms": [round(v, 4) for v in windows["returns"]]}
        res["policy_returns_grad"] = {"ms_per_call": round(ms, 4), "windows_ms": [round(v, 4) for v in windows["returns_grad"]],
                                      "over_policy_returns": round(ms / base, 4), "macs_ratio": round(ratio, 4),
                                      "tflops": round(2 * (MACS_RGRAD_FORWARD + MACS_RGRAD_BACKWARD) * n * h / (ms * 1e-3) / 1e12, 2),
                                      "stash_bytes": stash_bytes, "copy_bytes_per_s": round(copy_bw), "stash_allowance_ms": round(stash_ms, 4),
                                      "target_ms_per_call": round(limit, 4), "met": bool(ms <= limit), "over_target": round(ms / limit, 4)}
        every = tuple(L.RETURNS_GRAD_OUTPUTS)
        env.policy_returns_grad(h, "sample", seed=1, outputs=every)
        res["policy_returns_grad_every_output_ms_per_call"] = round(window(lambda: env.policy_returns_grad(h, "sample", seed=1, outputs=every)), 4)
        # ---- a record: the reference's pair of updates from one dream, wall clock per step over a window that ends with a synchronisation
        if n <= 4096:
            rng = np.random.default_rng(0)
            batch = dict(lidar=torch.from_numpy(rng.uniform(0.2, 12.0, (50, 50, 1080)).astype(np.float32)).to(env.device),
                         action=torch.from_numpy(rng.uniform(-1, 1, (50, 50, 2)).astype(np.float32)).to(env.device))
            from racing_dreamer_amd.world_model import behaviour_learning_step
            env.actor_fit_begin()
            env.critic_fit_begin("value")
            for k in range(2):
                behaviour_learning_step(env, batch, horizon=h, seed=k)
            env.sync()
            steps = max(2, args.calls // 4)
            t0 = time.perf_counter()
            for k in range(steps):
                behaviour_learning_step(env, batch, horizon=h, seed=2 + k)
            env.sync()
            res["behaviour_learning_step_50x50_wall_ms_per_step"] = round((time.perf_counter() - t0) / steps * 1e3, 3)
    env.close()
    return res


MACS_FIT_ROW = (230 * 400 + 2 * 400 * 400 + 400) * 2 + 2 * 400 * 400 + 400      # forward + weight gradients + backward data: 1 145 200
MACS_REWARD_FIT_ROW = (230 * 400 + 400 * 400 + 400) * 2 + 400 * 400 + 400       # the same at two hidden layers: 665 200 (x 0.58)
# the actor's step beside the value head's, counted with the bias rows: forward + backward data + weight gradient
MACS_VALUE_STEP_ROW = 412400 + 320400 + 413601
MACS_ACTOR_STEP_ROW = 573600 + 481600 + 575204                                  # x 1.422
MACS_ACTOR_GRAD_FEATURES_ROW = 230 * 400                                        # delta1 W0^T: + 92 000
ACTOR_SPREAD_ALLOWANCE = 1.05                                                   # policy_returns' condition used the same margin


def measure_fit(rows, args):
    """Wall-clock time per iteration of critic_fit beside tools/fit_critic.py's torch step with and without its load_critic upload;
    then reward_fit (where the package has it) beside critic_fit and - a record - beside the torch step on the reward head's layers.
    `--device-only` leaves the torch steps out: the figures an A/B of two builds needs."""
    import math
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.critic import init_critic
    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, 64, 1, auto_reset=True, remap_actions=True)
    env.load_policy(weights)
    start = init_critic(0, pcont=False)
    env.load_critic(start)
    gen = torch.Generator(device="cpu").manual_seed(0)
    feat = torch.randn((rows, 230), generator=gen).to(env.device)
    target = torch.randn((rows,), generator=gen).to(env.device)
    weight = torch.rand((rows,), generator=gen).to(env.device)
    params = {k: torch.from_numpy(v).to(env.device).requires_grad_(True) for k, v in start.items()}
    opt = torch.optim.Adam(list(params.values()), lr=8e-5)

    def torch_step(upload):
        x = feat
        for i in range(3):
            x = torch.nn.functional.elu(torch.addmm(params[f"value_h{i}_b"], x, params[f"value_h{i}_w"]))
        value = torch.addmm(params["value_hout_b"], x, params["value_hout_w"])[:, 0]
        loss = -(weight * (-0.5 * (value - target) ** 2 - 0.5 * math.log(2.0 * math.pi))).mean()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(params.values()), 100.0)
        opt.step()
        if upload:
            env.load_critic({k: v.detach().cpu().numpy() for k, v in params.items()})

    def wall(call, iters):
        for k in range(3):
            call()
        env.sync()
        torch.cuda.synchronize()
        windows = []
        for r in range(args.rounds):
            t0 = time.perf_counter()
            for k in range(iters):
                call()
            env.sync()
            torch.cuda.synchronize()
            windows.append((time.perf_counter() - t0) * 1e3 / iters)
        return statistics.median(windows), [round(v, 4) for v in windows]

    def device(step, macs):
        """{wall clock per iteration, its windows, TFLOP/s, the five launches' RC_K_POLICY time} of one fit step"""
        ms, windows = wall(step, args.calls)
        entry = {"ms_per_iteration": round(ms, 4), "windows_ms": windows, "tflops": round(2 * macs * rows / (ms * 1e-3) / 1e12, 2)}
        env.reset_kernel_times()
        env.set_profiling(True, kernels=[L.K_POLICY])
        for k in range(args.calls):
            step()
        env.sync()
        env.set_profiling(False)
        entry["device_ms_five_launches"] = round(env.kernel_times()["rc_policy_kernel"]["avg_ms"], 4)
        return entry

    res = {"rows": rows}
    with torch.cuda.stream(env.stream):
        if not args.device_only:
            ms, windows = wall(lambda: torch_step(True), args.calls)
            res["torch_step_with_load_critic_upload"] = {"ms_per_iteration": round(ms, 4), "windows_ms": windows}
            ms, windows = wall(lambda: torch_step(False), args.calls)
            res["torch_step_without_upload"] = {"ms_per_iteration": round(ms, 4), "windows_ms": windows}
        env.load_critic(start)
        env.critic_fit_begin("value")
        res["critic_fit"] = device(lambda: env.critic_fit(feat, target, weight), MACS_FIT_ROW)
        env.critic_fit_end("value")
        if hasattr(env, "reward_fit"):
            env.reward_fit_begin()
            res["reward_fit"] = device(lambda: env.reward_fit(feat, target, weight), MACS_REWARD_FIT_ROW)
            env.reward_fit_end()
            res["reward_fit"].update(macs_over_critic_fit=round(MACS_REWARD_FIT_ROW / MACS_FIT_ROW, 4),
                                     over_critic_fit=round(res["reward_fit"]["ms_per_iteration"] / res["critic_fit"]["ms_per_iteration"], 4))
            if not args.device_only:
                head = {k: torch.from_numpy(np.array(weights[k])).to(env.device).requires_grad_(True) for k in L.HEAD_KEYS}
                head_opt = torch.optim.Adam(list(head.values()), lr=6e-4)

                def torch_reward_step():
                    x = feat
                    for i in range(2):
                        x = torch.nn.functional.elu(torch.addmm(head[f"reward_h{i}_b"], x, head[f"reward_h{i}_w"]))
                    reward = torch.addmm(head["reward_hout_b"], x, head["reward_hout_w"])[:, 0]
                    loss = -(weight * (-0.5 * (reward - target) ** 2 - 0.5 * math.log(2.0 * math.pi))).mean()
                    head_opt.zero_grad()
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_(list(head.values()), 1.0)
                    head_opt.step()
                ms, windows = wall(torch_reward_step, args.calls)
                res["torch_reward_step_without_upload"] = {"ms_per_iteration": round(ms, 4), "windows_ms": windows}
                res["reward_fit"]["over_torch_without_upload"] = round(res["reward_fit"]["ms_per_iteration"] / ms, 4)
        if hasattr(env, "actor_fit"):
            # the actor's step (the engine at four hidden layers) beside critic_fit of the same run: target mode, no grad_features;
            # then - records - the step with grad_features, the forward alone and a plain fp32 torch step on the same layers
            actions = (torch.rand((rows, 2), generator=gen) * 2.0 - 1.0).to(env.device)
            env.actor_fit_begin()
            res["actor_fit"] = device(lambda: env.actor_fit(feat, target=actions), MACS_ACTOR_STEP_ROW)
            res["actor_fit_grad_features"] = device(lambda: env.actor_fit(feat, target=actions, grad_features=True),
                                                    MACS_ACTOR_STEP_ROW + MACS_ACTOR_GRAD_FEATURES_ROW)
            env.actor_fit_end()
            res["actor_forward"] = device(lambda: env.policy_action(feat), 573600)
            ratio = MACS_ACTOR_STEP_ROW / MACS_VALUE_STEP_ROW
            ms, base = res["actor_fit"]["ms_per_iteration"], res["critic_fit"]["ms_per_iteration"]
            res["actor_fit"].update(macs_over_critic_fit=round(ratio, 4), over_critic_fit=round(ms / base, 4),
                                    bound_ms=round(ratio * base * ACTOR_SPREAD_ALLOWANCE, 4), met=bool(ms <= ratio * base * ACTOR_SPREAD_ALLOWANCE))
            if not args.device_only:
                actor = {k: torch.from_numpy(np.array(weights[k])).to(env.device).requires_grad_(True) for k in L.ACTOR_KEYS}
                actor_opt = torch.optim.Adam(list(actor.values()), lr=8e-5)

                def torch_actor_step():
                    x = feat
                    for i in range(4):
                        x = torch.nn.functional.elu(torch.addmm(actor[f"h{i}_b"], x, actor[f"h{i}_w"]))
                    out = torch.addmm(actor["hout_b"], x, actor["hout_w"])
                    loss = (0.5 * ((torch.tanh(5.0 * torch.tanh(out[:, :2] / 5.0)) - actions) ** 2).sum(1)).mean()
                    actor_opt.zero_grad()
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_(list(actor.values()), 1.0)
                    actor_opt.step()
                ms_t, windows = wall(torch_actor_step, args.calls)
                res["torch_actor_step_without_upload"] = {"ms_per_iteration": round(ms_t, 4), "windows_ms": windows}
                res["actor_fit"]["over_torch_without_upload"] = round(ms / ms_t, 4)
    if not args.device_only:
        ms, base = res["critic_fit"]["ms_per_iteration"], res["torch_step_with_load_critic_upload"]["ms_per_iteration"]
        res["critic_fit"].update(over_torch_with_upload=round(ms / base, 4), met=bool(ms <= base),
                                 over_torch_without_upload=round(ms / res["torch_step_without_upload"]["ms_per_iteration"], 4))
    env.close()
    return res


FMA_PER_IMAGE = 230 * 64 + 64 * 800 + 320000 + 778752 + 259200          # h1 .. h5 (issue #16's table): 1 423 872
FMA_PER_S_PEAK = 256 * 4 * 32 * 2.4e9      # 256 CUs x 4 SIMDs x 32 fp32 fma per clock (v_pk_fma_f32: 64 FLOP / clk / SIMD) x 2.4 GHz


def torch_decode(w, feat):
    """The decoder's layers in plain fp32 torch: addmm, then four conv_transpose2d (stride 2) + relu; logits [n, 64, 64]."""
    import torch
    import torch.nn.functional as F
    x = torch.addmm(w["dec_h1_b"], feat, w["dec_h1_w"]).view(-1, 64, 1, 1)
    for name in ("dec_h2", "dec_h3", "dec_h4", "dec_h5"):
        x = F.relu(F.conv_transpose2d(x, w[name + "_k"], w[name + "_b"], stride=2))
    return x[:, 0]


def measure_decode(n, args):
    """Per-call device time (RC_K_POLICY) of rc_policy_decode on the live latents in three output sets, and the torch baseline."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, n, 1, obs_type="lidar_occupancy", auto_reset=True, remap_actions=True)
    env.load_policy(weights)
    res = {"cars": n}

    def timed(call):
        for k in range(3):
            call()
        windows = []
        for r in range(args.rounds):
            env.reset_kernel_times()
            env.set_profiling(True, kernels=[L.K_POLICY])
            for k in range(args.calls):
                call()
            env.sync()
            env.set_profiling(False)
            windows.append(env.kernel_times()["rc_policy_kernel"]["avg_ms"])
        return statistics.median(windows), [round(v, 4) for v in windows]

    with torch.cuda.stream(env.stream):
        env.reset(mode="random", seed=1)
        for k in range(args.settle):
            env.policy_act()
            env.step(None, repeat=4)
        env.sync()
        bufs = dict(logits=torch.empty((n, 64, 64), device=env.device), image=torch.empty((n, 64, 64), dtype=torch.uint8, device=env.device),
                    mismatch=torch.empty(n, dtype=torch.int32, device=env.device))
        for variant, names in (("image", ("image",)), ("logits", ("logits",)), ("image_mismatch", ("image", "mismatch"))):
            tensors = {k: (bufs[k] if k in names else None) for k in bufs}
            ms, windows = timed(lambda: L.check(env._decode(None, 1, tensors, 0, n)))
            res[variant] = {"ms_per_call": round(ms, 4), "windows_ms": windows, "us_per_image": round(ms * 1e3 / n, 4),
                            "fp32_issue_floor_ms": round(FMA_PER_IMAGE * n / FMA_PER_S_PEAK * 1e3, 4),
                            "fraction_of_issue_floor": round(FMA_PER_IMAGE * n / FMA_PER_S_PEAK * 1e3 / ms, 3)}
        env.sync()
        res["mean_mismatch_pixels"] = round(float(bufs["mismatch"].float().mean()), 1)
        # ---- the torch baseline of the same layers on the same features (its own layouts: NCHW, kernels [in, out, kh, kw])
        w = {k: torch.from_numpy(np.ascontiguousarray(weights[k], np.float32)).to(env.device) for k in weights.files if k.startswith("dec_")}
        for k in ("dec_h2_k", "dec_h3_k", "dec_h4_k", "dec_h5_k"):
            w[k] = w[k].permute(3, 2, 0, 1).contiguous()
        feat = env.policy_state[:, :230].contiguous()
        for k in range(3):
            ref = torch_decode(w, feat)
        L.check(env._decode(None, 1, dict(logits=bufs["logits"], image=None, mismatch=None), 0, n))
        env.sync()
        res["max_abs_difference_from_torch"] = float((ref - bufs["logits"]).abs().max())
        del ref
        windows = []
        for r in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(max(1, args.calls // 4)):
                torch_decode(w, feat)
            e1.record()
            e1.synchronize()
            windows.append(e0.elapsed_time(e1) / max(1, args.calls // 4))
        res["torch_fp32_ms_per_call"] = round(statistics.median(windows), 4)
        res["torch_fp32_windows_ms"] = [round(v, 4) for v in windows]
        res["hip_over_torch"] = round(res["logits"]["ms_per_call"] / res["torch_fp32_ms_per_call"], 3)
        res["met"] = bool(res["logits"]["ms_per_call"] <= res["torch_fp32_ms_per_call"])
    env.close()
    return res


MACS_LIDAR_DECODER = 230 * 256 + 256 * 512 + 512 * 2160           # dense1, dense2, params: 1 295 872


def torch_lidar_loglik(w, feat, scan):
    """LidarDistanceDecoder and Normal.log_prob in plain fp32 torch: three addmm, relu, leaky_relu, softplus; loglik [n]."""
    import torch
    import torch.nn.functional as F
    x = torch.addmm(w["ldec_dense1_b"], feat, w["ldec_dense1_w"])
    x = F.relu(torch.addmm(w["ldec_dense2_b"], x, w["ldec_dense2_w"]))
    x = F.leaky_relu(torch.addmm(w["ldec_params_b"], x, w["ldec_params_w"]), 0.2)
    y = torch.clamp(scan, 0.0, 15.0) / 15.0 - 0.5
    return torch.distributions.Normal(x[:, :1080], F.softplus(x[:, 1080:])).log_prob(y).sum(1)


def measure_decode_lidar(n, args):
    """Per-call device time (RC_K_POLICY) of rc_policy_decode_lidar on the live latents of n cars in three output sets, beside the
    `mean` agent call of the same run scaled by the ratio of multiply-adds and beside the same layers in plain fp32 torch; then
    the occupancy decoder's loglik launch beside policy_decode(logits=True) plus the torch sum."""
    import torch
    import torch.nn.functional as F
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.decoder import init_lidar_decoder
    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    ldec = init_lidar_decoder(0, -3.0)
    res = {"cars": n}

    def timed(env, call, calls):
        for k in range(3):
            call()
        windows = []
        for r in range(args.rounds):
            env.reset_kernel_times()
            env.set_profiling(True, kernels=[L.K_POLICY])
            for k in range(calls):
                call()
            env.sync()
            env.set_profiling(False)
            windows.append(env.kernel_times()["rc_policy_kernel"]["avg_ms"])
        return statistics.median(windows), [round(v, 4) for v in windows]

    def torch_timed(call, calls):
        for k in range(3):
            call()
        windows = []
        for r in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(calls):
                call()
            e1.record()
            e1.synchronize()
            windows.append(e0.elapsed_time(e1) / calls)
        return statistics.median(windows), [round(v, 4) for v in windows]

    env = BatchedRaceEnv(args.track, n, 1, auto_reset=True, remap_actions=True)
    env.load_policy(weights)
    env.load_lidar_decoder(ldec)
    with torch.cuda.stream(env.stream):
        env.reset(mode="random", seed=1)
        for k in range(args.settle):
            env.policy_act()
            env.step(None, repeat=4)
        env.sync()
        act_ms, act_windows = timed(env, env.policy_act, args.calls)
        res["policy_act_mean_ms"], res["policy_act_windows_ms"] = round(act_ms, 4), act_windows
        bufs = dict(mean=torch.empty((n, 1080), device=env.device), std=torch.empty((n, 1080), device=env.device),
                    loglik=torch.empty(n, device=env.device))
        for variant, names in (("loglik", ("loglik",)), ("mean", ("mean",)), ("all", ("mean", "std", "loglik"))):
            tensors = {k: (bufs[k] if k in names else None) for k in bufs}
            ms, windows = timed(env, lambda: L.check(env._decode_lidar(None, 1, None, tensors, 0, n)), args.calls)
            res[variant] = {"ms_per_call": round(ms, 4), "windows_ms": windows, "us_per_row": round(ms * 1e3 / n, 4),
                            "tflops": round(2 * MACS_LIDAR_DECODER * n / (ms * 1e-3) / 1e12, 2)}
        ratio = MACS_LIDAR_DECODER / MACS_PER_CAR
        res["loglik"]["target_ms"] = round(act_ms * ratio * 1.05, 4)
        res["loglik"]["over_scaled_agent_call"] = round(res["loglik"]["ms_per_call"] / (act_ms * ratio), 3)
        res["loglik"]["met"] = bool(res["loglik"]["ms_per_call"] <= act_ms * ratio * 1.05)
        w = {k: torch.from_numpy(v).to(env.device) for k, v in ldec.items()}
        feat, scan = env.policy_state[:, :230].contiguous(), env.views["lidar"].view(n, 1080)
        ref = torch_lidar_loglik(w, feat, scan)
        env.sync()
        res["max_relative_difference_from_torch"] = float(((ref - bufs["loglik"]).abs() / ref.abs()).max())
        del ref
        t_ms, t_windows = torch_timed(lambda: torch_lidar_loglik(w, feat, scan), max(1, args.calls // 4))
        res["torch_fp32_ms_per_call"], res["torch_fp32_windows_ms"] = round(t_ms, 4), t_windows
        res["hip_over_torch"] = round(res["loglik"]["ms_per_call"] / t_ms, 3)
        res["no_slower_than_torch"] = bool(res["loglik"]["ms_per_call"] <= t_ms)
    env.close()
    del bufs
    torch.cuda.empty_cache()
    # ---- the occupancy decoder: loglik in the launch, beside logits out and the sum in torch
    occ_w = np.load(os.path.join(ROOT, "tests", "golden", "dreamer_policy_treitlstrasse_occupancy.npz"))
    env = BatchedRaceEnv("treitlstrasse_v2", n, 1, obs_type="lidar_occupancy", auto_reset=True, remap_actions=True)
    env.load_policy(occ_w)
    with torch.cuda.stream(env.stream):
        env.reset(mode="random", seed=1)
        for k in range(args.settle):
            env.policy_act()
            env.step(None, repeat=4)
        env.sync()
        loglik, logits = torch.empty(n, device=env.device), torch.empty((n, 64, 64), device=env.device)
        seen = env.views["lidar_occupancy"].view(n, 64, 64)
        ms, windows = timed(env, lambda: L.check(env._decode_loglik(None, 1, None, dict(loglik=loglik, logits=None, image=None), 0, n)), max(1, args.calls // 4))
        occ = {"loglik_launch_ms": round(ms, 4), "loglik_launch_windows_ms": windows}
        ms, windows = timed(env, lambda: L.check(env._decode(None, 1, dict(logits=logits, image=None, mismatch=None), 0, n)), max(1, args.calls // 4))
        occ["decode_logits_ms"], occ["decode_logits_windows_ms"] = round(ms, 4), windows
        t_ms, t_windows = torch_timed(lambda: (seen.float() * logits - F.softplus(logits)).flatten(1).sum(1), max(1, args.calls // 4))
        occ["torch_sum_ms"], occ["torch_sum_windows_ms"] = round(t_ms, 4), t_windows
        occ["loglik_launch_over_logits_plus_torch_sum"] = round(occ["loglik_launch_ms"] / (occ["decode_logits_ms"] + t_ms), 3)
        res["occupancy"] = occ
    env.close()
    return res


MACS_OBSERVED_STEP = 32 * 200 + 2 * 200 * 600 + 200 * 200 + 200 * 60 + 1280 * 200 + 200 * 60       # 566 400: prior and posterior, both halves


class TorchObserve(TorchAgent):
    """T observed steps (mode mean: posterior and prior statistics, the KL, the features) in plain fp32 torch."""

    def observe(self, scan, action):
        import torch
        import torch.nn.functional as F
        w = self.w
        n, T = scan.shape[:2]
        stoch, deter = scan.new_zeros((n, 30)), scan.new_zeros((n, 200))
        feats, kls = [], []
        for t in range(T):
            embed = torch.clamp(scan[:, t], 0.0, 15.0) / 15.0 - 0.5
            x = F.elu(torch.addmm(w["img1_b"], torch.cat([stoch, torch.clamp(action[:, t], -1.0, 1.0)], 1), w["img1_w"]))
            mx, mh = torch.addmm(w["gru_bias"][0], x, w["gru_kernel"]), torch.addmm(w["gru_bias"][1], deter, w["gru_recurrent"])
            z, r = torch.sigmoid(mx[:, :200] + mh[:, :200]), torch.sigmoid(mx[:, 200:400] + mh[:, 200:400])
            deter = z * deter + (1.0 - z) * torch.tanh(mx[:, 400:] + r * mh[:, 400:])
            x = torch.addmm(w["img3_b"], F.elu(torch.addmm(w["img2_b"], deter, w["img2_w"])), w["img3_w"])
            qm, qs = x[:, :30], F.softplus(x[:, 30:]) + 0.1
            x = torch.addmm(w["obs2_b"], F.elu(torch.addmm(w["obs1_b"], torch.cat([deter, embed], 1), w["obs1_w"])), w["obs2_w"])
            stoch, sp = x[:, :30], F.softplus(x[:, 30:]) + 0.1
            kls.append((torch.log(qs) - torch.log(sp) + (sp ** 2 + (stoch - qm) ** 2) / (2.0 * qs ** 2) - 0.5).sum(1))
            feats.append(torch.cat([stoch, deter], 1))
        return torch.stack(feats, 1), torch.stack(kls, 1)


def measure_observe(n, args):
    """Per-call device time (RC_K_POLICY) of policy_act (`mean`) on n cars and of rc_policy_observe on n rows x T = args.horizon."""
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, n, 1, auto_reset=True, remap_actions=True)
    env.load_policy(weights)
    T = args.horizon
    res = {"rows": n, "length": T, "context": T}

    def timed(call):
        for k in range(3):
            call()
        windows = []
        for r in range(args.rounds):
            env.reset_kernel_times()
            env.set_profiling(True, kernels=[L.K_POLICY])
            for k in range(args.calls):
                call()
            env.sync()
            env.set_profiling(False)
            windows.append(env.kernel_times()["rc_policy_kernel"]["avg_ms"])
        return statistics.median(windows), [round(v, 4) for v in windows]

    with torch.cuda.stream(env.stream):
        out = env.reset(mode="random", seed=1)
        for k in range(args.settle):
            env.policy_act()
            out = env.step(None, repeat=4)
        scans, acts = [], []
        for k in range(T):                                  # the recording: T agent steps of the same run
            fresh = out["fresh"].view(n, 1) != 0
            scans.append(out["lidar"].view(n, 1080).clone())
            acts.append(torch.where(fresh, torch.zeros_like(env.policy_state[:, 230:]), env.policy_state[:, 230:]))
            env.policy_act()
            out = env.step(None, repeat=4)
        scan, action = torch.stack(scans, 1).contiguous(), torch.stack(acts, 1).contiguous()
        del scans, acts
        env.sync()
        act_ms, act_windows = timed(env.policy_act)
        res["policy_act_mean_ms"], res["policy_act_mean_windows_ms"] = round(act_ms, 4), act_windows
        every = ("feature", "post_mean", "post_std", "prior_mean", "prior_std", "kl", "state")
        bufs = {k: torch.empty((n, 232) if k == "state" else (n, T) + L.OBSERVE_OUTPUTS[k][1], device=env.device) for k in every + ("reward",)}
        for variant, mode, names in (("mean_features", "mean", ("feature",)), ("mean_features_reward", "mean", ("feature", "reward")),
                                     ("sample_features", "sample", ("feature",)), ("mean_all", "mean", every)):
            ms, windows = timed(lambda: env.policy_observe(scan, action, mode=mode, seed=1, outputs=names, out=bufs))
            res[variant] = {"ms_per_call": round(ms, 4), "windows_ms": windows, "ms_per_observed_step": round(ms / T, 4),
                            "step_over_policy_act": round(ms / T / act_ms, 4)}
        res["condition_met"] = bool(res["mean_features"]["ms_per_observed_step"] <= act_ms)
        # ---- the torch baseline of the same layers (mode mean: features, prior and posterior statistics, KL)
        agent = TorchObserve(weights, env.device)
        for k in range(2):
            agent.observe(scan, action)
        windows = []
        for r in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(max(1, args.calls // 4)):
                agent.observe(scan, action)
            e1.record()
            e1.synchronize()
            windows.append(e0.elapsed_time(e1) / max(1, args.calls // 4))
        res["torch_fp32_ms_per_call"] = round(statistics.median(windows), 4)
        res["torch_fp32_windows_ms"] = [round(v, 4) for v in windows]
        res["hip_over_torch"] = round(res["mean_all"]["ms_per_call"] / res["torch_fp32_ms_per_call"], 3)
        res["no_slower_than_torch"] = bool(res["mean_all"]["ms_per_call"] <= res["torch_fp32_ms_per_call"])
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
    ap.add_argument("--imagine", action="store_true", help="measure imagination (profiles/policy_imagine_cost.json)")
    ap.add_argument("--decode", action="store_true", help="measure the observation decoder (profiles/policy_decode_cost.json)")
    ap.add_argument("--decode-lidar", action="store_true", help="measure the LiDAR distance decoder (profiles/policy_decode_lidar_cost.json)")
    ap.add_argument("--observe", action="store_true", help="measure recorded sequences (profiles/policy_observe_cost.json)")
    ap.add_argument("--returns", action="store_true", help="measure the critic and the lambda-return (profiles/policy_returns_cost.json)")
    ap.add_argument("--returns-grad", action="store_true", help="measure the actor loss's gradient through the dream (profiles/policy_returns_grad_cost.json)")
    ap.add_argument("--fit", action="store_true", help="measure the critic's fit (profiles/policy_fit_cost.json)")
    ap.add_argument("--device-only", action="store_true", help="--fit: the device steps alone, no torch baseline (an A/B of two builds)")
    ap.add_argument("--root", default=None, help="import racing_dreamer_amd from this checkout instead (--fit --device-only: the other build of an A/B)")
    ap.add_argument("--horizon", type=int, default=15)
    args = ap.parse_args()
    if args.root:
        sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if args.fit:
        sizes = args.envs if args.envs != [4096, 65536] else [14336, 35000]
        out = {"tool": "tools/policy_cost.py --fit" + (" --device-only" if args.device_only else ""), "checkpoint": args.checkpoint,
               "critic": "critic.init_critic(0, pcont=False)", "reward_head": "the checkpoint's",
               "device": torch.cuda.get_device_name(0), "iterations_per_window": args.calls, "windows": args.rounds,
               "macs_per_row_forward_backward": MACS_FIT_ROW, "macs_per_row_forward_backward_reward": MACS_REWARD_FIT_ROW,
               "clock": "wall clock per iteration over a window that ends with a synchronisation",
               "condition": "critic_fit ms_per_iteration <= 1.0 x torch_step_with_load_critic_upload ms_per_iteration of the same run, at every size",
               "sizes": [measure_fit(n, args) for n in sizes]}
        out["condition_met"] = None if args.device_only else all(s["critic_fit"]["met"] for s in out["sizes"])
        if all("actor_fit" in s for s in out["sizes"]):
            out["macs_per_row_value_step"], out["macs_per_row_actor_step"] = MACS_VALUE_STEP_ROW, MACS_ACTOR_STEP_ROW
            out["actor_condition"] = ("actor_fit ms_per_iteration <= (macs_per_row_actor_step / macs_per_row_value_step = 1.422) x critic_fit "
                                      f"ms_per_iteration of the same run x {ACTOR_SPREAD_ALLOWANCE}, at every size")
            out["actor_condition_met"] = all(s["actor_fit"]["met"] for s in out["sizes"])
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
    if args.returns_grad:
        sizes = args.envs if args.envs != [4096, 65536] else [2450, 65536]
        out = {"tool": "tools/policy_cost.py --returns-grad", "track": args.track, "checkpoint": args.checkpoint, "critic": "critic.init_critic(0)",
               "device": torch.cuda.get_device_name(0), "calls_per_window": args.calls, "windows": args.rounds, "settle_agent_steps": args.settle,
               "mode": "sample", "macs_per_step_forward": MACS_RGRAD_FORWARD, "macs_per_step_backward": MACS_RGRAD_BACKWARD,
               "stash_floats_per_row_and_step": RGRAD_STASH_FLOATS, "spread_allowance": 1.05,
               "condition": "policy_returns_grad ms_per_call <= policy_returns(returns, weight) ms_per_call of the same run x macs_ratio x 1.05 "
                            "+ stash_bytes / copy_bytes_per_s of the same run, at every size",
               "sizes": [measure_returns_grad(n, args) for n in sizes]}
        out["condition_met"] = all(s["policy_returns_grad"]["met"] for s in out["sizes"])
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
    if args.returns:
        sizes = args.envs if args.envs != [4096, 65536] else [65536]
        out = {"tool": "tools/policy_cost.py --returns", "track": args.track, "checkpoint": args.checkpoint, "critic": "critic.init_critic(0)",
               "device": torch.cuda.get_device_name(0), "calls_per_window": args.calls, "windows": args.rounds, "settle_agent_steps": args.settle,
               "macs_per_step_actor_prior_reward": MACS_RETURNS_BASE, "macs_per_critic_head": MACS_CRITIC_HEAD,
               "macs_per_step_with_both_heads": MACS_RETURNS_BASE + 2 * MACS_CRITIC_HEAD, "spread_allowance": 1.05,
               "condition": "mean_returns_weight ms_per_step <= macs_ratio x imagine_mean_reward ms_per_step of the same run x 1.05, at the largest size",
               "sizes": [measure_returns(n, args) for n in sizes]}
        out["condition_met"] = out["sizes"][-1]["mean_returns_weight"]["met"]
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
    if args.observe:
        sizes = args.envs if args.envs != [4096, 65536] else [65536]
        out = {"tool": "tools/policy_cost.py --observe", "track": args.track, "checkpoint": args.checkpoint, "device": torch.cuda.get_device_name(0),
               "calls_per_window": args.calls, "windows": args.rounds, "settle_agent_steps": args.settle,
               "macs_per_observed_step": MACS_OBSERVED_STEP, "macs_per_agent_step": MACS_PER_CAR, "macs_ratio": round(MACS_OBSERVED_STEP / MACS_PER_CAR, 3),
               "condition": "mean_features ms_per_observed_step <= 1.0 x policy_act_mean_ms of the same run on as many cars, at the largest size",
               "second_line": "mean_all ms_per_call beside the same steps in plain fp32 torch (torch_fp32_ms_per_call)",
               "sizes": [measure_observe(n, args) for n in sizes]}
        out["condition_met"] = out["sizes"][-1]["condition_met"]
        out["no_slower_than_torch"] = out["sizes"][-1]["no_slower_than_torch"]
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
    if args.decode_lidar:
        sizes = args.envs if args.envs != [4096, 65536] else [65536]
        out = {"tool": "tools/policy_cost.py --decode-lidar", "track": args.track, "checkpoint": args.checkpoint,
               "decoder": "decoder.init_lidar_decoder(0, -3.0)", "device": torch.cuda.get_device_name(0), "calls_per_window": args.calls,
               "windows": args.rounds, "settle_agent_steps": args.settle, "macs_per_row": MACS_LIDAR_DECODER, "macs_per_agent_step": MACS_PER_CAR,
               "macs_ratio": round(MACS_LIDAR_DECODER / MACS_PER_CAR, 4), "spread_allowance": 1.05,
               "condition": "loglik ms_per_call <= macs_ratio x policy_act_mean_ms of the same run x 1.05, at the largest size",
               "second_condition": "loglik ms_per_call <= torch_fp32_ms_per_call (three addmm and Normal.log_prob) of the same run",
               "sizes": [measure_decode_lidar(n, args) for n in sizes]}
        out["condition_met"] = out["sizes"][-1]["loglik"]["met"]
        out["no_slower_than_torch"] = out["sizes"][-1]["no_slower_than_torch"]
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
    if args.decode:
        if args.checkpoint == "austria":                       # (the default checkpoint has no decoder)
            args.checkpoint, args.track = "treitlstrasse_occupancy", "treitlstrasse_v2"
        sizes = args.envs if args.envs != [4096, 65536] else [65536]
        out = {"tool": "tools/policy_cost.py --decode", "track": args.track, "checkpoint": args.checkpoint, "device": torch.cuda.get_device_name(0),
               "calls_per_window": args.calls, "windows": args.rounds, "settle_agent_steps": args.settle, "fma_per_image": FMA_PER_IMAGE,
               "fp32_peak_fma_per_s": FMA_PER_S_PEAK, "condition": "logits ms_per_call <= torch_fp32_ms_per_call at the largest size",
               "sizes": [measure_decode(n, args) for n in sizes]}
        out["met"] = out["sizes"][-1]["met"]
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
    if args.imagine:
        out = {"tool": "tools/policy_cost.py --imagine", "track": args.track, "checkpoint": args.checkpoint, "device": torch.cuda.get_device_name(0),
               "calls_per_window": args.calls, "windows": args.rounds, "settle_agent_steps": args.settle,
               "macs_per_imagined_step": MACS_IMAGINED_STEP, "macs_per_agent_step": MACS_PER_CAR,
               "padded_macs_per_imagined_step": PADDED_IMAGINED_STEP, "padded_macs_per_agent_step": PADDED_AGENT_STEP,
               "padded_ratio": round(PADDED_IMAGINED_STEP / PADDED_AGENT_STEP, 4), "spread_allowance": 1.05,
               "padded_macs_per_imagined_step_sample": PADDED_IMAGINED_STEP_SAMPLE,
               "note": "padded MACs follow RC_POLICY_LD* of racecar_policy.h; the ratio and the target are for mode mean, closed loop, "
                       "reward only - mode sample's extra std tiles (img3, hout) are in padded_macs_per_imagined_step_sample only",
               "sizes": [measure_imagine(n, args) for n in args.envs]}
        out["target_met_at_largest_size"] = out["sizes"][-1]["target_met"]
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
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
