"""Cost of planning in the dream (include/racecar_hip.h, rc_policy_dream_ahead) against the only way to score the same candidates
before it, and how the dream's ranking of candidates agrees with the simulator's.

Cost.  Workload: 4 096 starts x 64 candidates x H = 15 (262 144 rows), checkpoint austria, from the live latents after `--settle`
closed-loop agent steps; candidates from planning.shooting_candidates; output `return` only, mode `mean`.  Yardstick, measured in
the same run: the open-loop rc_policy_imagine (actions given, reward only, no features) on a second env of 262 144 cars whose
latents are copies of the 4 096, K each - the same layer work on the same rows.  The two are measured alternately for `--rounds`
rounds of `--calls` launches, by the launches' own timestamps (RC_K_POLICY); the median and the spread of each are reported.
Condition (set before anything was measured): dream_ahead <= 1.05 x yardstick.  Beside it, as a record: mode `sample`, and all
three outputs.  Before timing, the two calls' rewards are compared byte for byte.

`--agreement`: world_model.dream_vs_truth on austria and columbia (checkpoint austria: the repository has none trained on
columbia), `--agreement-envs` single-car envs after the same settling, 64 candidates x H = 15 at repeat 4: Spearman rank correlation
of imagined and true returns per env, whether the two first-best candidates agree, and the regret of the dream's choice - means
and quartiles over envs.  A record without a threshold.  Prints ONE JSON line per mode.

    python tools/dream_ahead_cost.py [--rounds 5] [--calls 10] [--out profiles/dream_ahead_cost.json]
    python tools/dream_ahead_cost.py --agreement [--out profiles/dream_ahead_agreement.json]

`--grad`: the cost of the dream's backward pass (rc_policy_dream_grad) at the same shape, mode `mean`, outputs
`grad_actions` + `return`, against dream_ahead with `return` alternately in the same run.  Condition (set before anything was
measured): dream_ahead_grad <= (multiply-adds of forward + backward / multiply-adds of forward, counted from the layer shapes below)
x 1.05 x dream_ahead + the stash's bytes written and read / the bandwidth of a plain device-to-device copy measured in the same
run (a copy of one chunk's stash: it reads and writes as many bytes as the chunk's stash is written and read).  Beside it: mode
`sample`, and the chunk_rows the scratch's limit produced.  With `--grad --agreement`: shooting-64, CEM and gradient-refined
shooting-8 on austria and columbia - the imagined return of each planner's choice, its true return (look_ahead), the regret
against the best of the 64 shooting candidates in truth, and the launches per decision.  A record without a threshold.

    python tools/dream_ahead_cost.py --grad [--out profiles/dream_grad_cost.json]
    python tools/dream_ahead_cost.py --grad --agreement [--out profiles/dream_grad_agreement.json]
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
ALL = ("return", "reward", "final_feature")


def checkpoint(name):
    return os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{name}.npz")


def settle(env, steps, seed=1):
    env.reset(mode="random", seed=seed)
    for _ in range(steps):
        env.policy_act()
        env.step(None, repeat=REPEAT)
    env.policy_act()                                        # the latent takes in the last scan: the dream starts where the env stands
    env.sync()


def timed(env, call, calls):
    from racing_dreamer_amd import _lib as L
    env.reset_kernel_times()
    env.set_profiling(True, kernels=[L.K_POLICY])
    for _ in range(calls):
        call()
    env.sync()
    env.set_profiling(False)
    return env.kernel_times()["rc_policy_kernel"]["avg_ms"]


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5),
            "spread": round((max(xs) - min(xs)) / statistics.median(xs), 4)}


def cost(args):
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.planning import shooting_candidates, to_dream_actions
    S, K, H = args.starts, args.candidates, args.horizon
    env = BatchedRaceEnv("austria", S, 1, auto_reset=True, remap_actions=True)
    env.load_policy(checkpoint(args.checkpoint))
    settle(env, args.settle)
    brute = BatchedRaceEnv("austria", S * K, 1, auto_reset=True, remap_actions=True)
    brute.load_policy(checkpoint(args.checkpoint))
    brute.reset(mode="random", seed=1)
    brute.policy_state.copy_(env.policy_state.repeat_interleave(K, dim=0))
    acts = to_dream_actions(shooting_candidates(env, K, H, hold=5, seed=0))          # [S, K, H, 2]
    out = {"return": torch.empty((S, K), device=env.device), "reward": torch.empty((S, K, H), device=env.device),
           "final_feature": torch.empty((S, K, L.POLICY_FEATURE), device=env.device)}
    tensors = dict(actions_in=acts.reshape(S * K, H, 2), reward=torch.empty((S * K, H), device=env.device), actions=None, features=None,
                   reward_start=None)
    a = dict(horizon=H, mode=L.IMAGINE_MODES["mean"], seed=1, mask=1)

    def dream(mode, outputs):
        return lambda: env.dream_ahead(acts, mode, seed=1, outputs=outputs, out=out)

    def imagine():
        brute._enter()
        L.check(brute._imagine(a, tensors, 0, S * K))
        brute._exit()

    # the two compute the same rewards (and this warms both up)
    dream("mean", ALL)()
    imagine()
    torch.cuda.synchronize()
    same = out["reward"].reshape(S * K, H).cpu().numpy().tobytes() == tensors["reward"].cpu().numpy().tobytes()
    variants = {"dream_ahead_mean_return": dream("mean", ("return",)), "dream_ahead_sample_return": dream("sample", ("return",)),
                "dream_ahead_mean_all_outputs": dream("mean", ALL), "dream_ahead_sample_all_outputs": dream("sample", ALL)}
    for call in variants.values():
        timed(env, call, 2)
    timed(brute, imagine, 2)
    times = {k: [] for k in variants}
    yard = []
    for _ in range(args.rounds):
        for k, call in variants.items():
            times[k].append(timed(env, call, args.calls))
            if k == "dream_ahead_mean_return":
                yard.append(timed(brute, imagine, args.calls))
    res = {"tool": "tools/dream_ahead_cost.py", "device": torch.cuda.get_device_name(0), "checkpoint": args.checkpoint, "starts": S, "candidates": K,
           "horizon": H, "rows": S * K, "settle_agent_steps": args.settle, "rounds": args.rounds, "calls_per_round": args.calls,
           "rewards_byte_identical_to_policy_imagine": bool(same)}
    for k, v in times.items():
        res[k] = spread(v)
    res["policy_imagine_open_loop_reward_at_rows_cars"] = spread(yard)
    y = statistics.median(yard)
    res["ratio"] = round(statistics.median(times["dream_ahead_mean_return"]) / y, 4)
    for k in list(variants)[1:]:
        res["ratio_" + k[len("dream_ahead_"):]] = round(statistics.median(times[k]) / y, 4)
    res["target"] = f"dream_ahead (mean, return) <= {TARGET} x open-loop policy_imagine (reward) on {S * K} cars, same run"
    res["target_met"] = bool(res["ratio"] <= TARGET)
    res["verdict"] = "met" if res["target_met"] else "missed"
    env.close()
    brute.close()
    return res


# multiply-adds per (row, step) from the layer shapes, mode `mean` (img3: the 30 mean columns; `sample`: 60)
FORWARD_MACS = {"img1": 32 * 200, "gru_kernel": 200 * 600, "gru_recurrent": 200 * 600, "img2": 200 * 200, "img3": 200 * 30, "rh0": 230 * 400,
                "rh1": 400 * 400, "rout": 400}
BACKWARD_MACS = {"rout^T": 400, "rh1^T": 400 * 400, "rh0^T": 400 * 230, "img3^T": 30 * 200, "img2^T": 200 * 200, "gru_kernel^T": 600 * 200,
                 "gru_recurrent^T": 600 * 200, "img1^T": 200 * 32}
STASH_FLOATS = 2240                                         # a (row, step)'s place in the stash
STASH_USED = {"mean": 2200, "sample": 2230}                 # floats written, and read back, per (row, step)
STASH_LIMIT = 1 << 30


def grad_cost(args):
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.planning import shooting_candidates, to_dream_actions
    S, K, H = args.starts, args.candidates, args.horizon
    env = BatchedRaceEnv("austria", S, 1, auto_reset=True, remap_actions=True)
    env.load_policy(checkpoint(args.checkpoint))
    settle(env, args.settle)
    acts = to_dream_actions(shooting_candidates(env, K, H, hold=5, seed=0))          # [S, K, H, 2]
    fwd_out = {"return": torch.empty((S, K), device=env.device)}
    out = {"return": torch.empty((S, K), device=env.device), "grad_actions": torch.empty((S, K, H, 2), device=env.device)}
    chunk_rows = min(STASH_LIMIT // (H * STASH_FLOATS * 4) // 32 * 32, (S * K + 31) // 32 * 32)
    chunk_bytes = chunk_rows * H * STASH_FLOATS * 4
    src = torch.empty(chunk_bytes // 4, device=env.device).normal_()
    dst = torch.empty_like(src)

    def forward():
        env.dream_ahead(acts, "mean", seed=1, outputs=("return",), out=fwd_out)

    def grad(mode):
        return lambda: env.dream_ahead_grad(acts, mode, seed=1, outputs=("grad_actions", "return"), out=out)

    def copy_ms(n=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    forward()
    grad("mean")()
    torch.cuda.synchronize()
    same = fwd_out["return"].cpu().numpy().tobytes() == out["return"].cpu().numpy().tobytes()
    ret_only = {"return": torch.empty((S, K), device=env.device)}
    variants = {"dream_ahead_grad_mean": grad("mean"), "dream_ahead_grad_sample": grad("sample"),
                # `return` alone: the kernel's forward with the stash written and no backward - where the time goes
                "dream_ahead_grad_mean_forward_and_stash_only": lambda: env.dream_ahead_grad(acts, "mean", seed=1, outputs=("return",), out=ret_only)}
    for call in variants.values():
        timed(env, call, 1)
    timed(env, forward, 2)
    copy_ms(2)
    times, yard, copies = {k: [] for k in variants}, [], []
    for _ in range(args.rounds):
        for k, call in variants.items():
            times[k].append(timed(env, call, args.calls))
            if k == "dream_ahead_grad_mean":
                yard.append(timed(env, forward, args.calls))
                copies.append(copy_ms())
    fwd, bwd = sum(FORWARD_MACS.values()), sum(BACKWARD_MACS.values())
    factor = (fwd + bwd) / fwd
    y, c = statistics.median(yard), statistics.median(copies)
    stash_bytes = S * K * H * STASH_USED["mean"] * 4          # written once and read once: the traffic of a copy of as many bytes
    allowance = stash_bytes / chunk_bytes * c
    bound = factor * TARGET * y + allowance
    g = statistics.median(times["dream_ahead_grad_mean"])
    res = {"tool": "tools/dream_ahead_cost.py --grad", "device": torch.cuda.get_device_name(0), "checkpoint": args.checkpoint, "starts": S,
           "candidates": K, "horizon": H, "rows": S * K, "settle_agent_steps": args.settle, "rounds": args.rounds, "calls_per_round": args.calls,
           "return_byte_identical_to_dream_ahead": bool(same), "chunk_rows": chunk_rows, "launches_per_call": -(-S * K // chunk_rows),
           "chunk_rows_source": "derived here as dream_grad_run derives it (racecar_dream_grad.hip: the 1 GiB limit / (H x 2 240 floats), rounded down "
                                "to a multiple of 32), not read back from the library",
           "stash_bytes_per_chunk": chunk_bytes, "forward_macs_per_row_step": fwd, "backward_macs_per_row_step": bwd, "mac_factor": round(factor, 4)}
    for k, v in times.items():
        res[k] = spread(v)
    res["dream_ahead_mean_return"] = spread(yard)
    res["device_copy_of_one_chunks_stash"] = dict(spread(copies), bytes=chunk_bytes,
                                                  copied_gb_per_s=round(chunk_bytes / c / 1e6, 1))
    res["stash_bytes_written_and_read"] = 2 * stash_bytes
    res["stash_allowance_ms"] = round(allowance, 3)
    res["bound_ms"] = round(bound, 3)
    res["ratio_to_dream_ahead"] = round(g / y, 4)
    res["ratio_sample_to_dream_ahead"] = round(statistics.median(times["dream_ahead_grad_sample"]) / y, 4)
    res["target"] = (f"dream_ahead_grad (mean, grad_actions + return) <= {factor:.3f} x {TARGET} x dream_ahead (mean, return) + the stash's bytes "
                     f"written and read / the device copy's bandwidth, same run")
    res["target_met"] = bool(g <= bound)
    res["verdict"] = "met" if res["target_met"] else "missed"
    env.close()
    return res


def grad_agreement(args):
    import numpy as np
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.planning import dream_cem_act, dream_gradient_act, dream_shooting_act, shooting_candidates, to_dream_actions
    from racing_dreamer_amd.world_model import dream_vs_truth

    def stats(x):
        x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float64)
        x = x[np.isfinite(x)]
        return {"mean": round(float(x.mean()), 5), "median": round(float(np.median(x)), 5), "envs": int(x.size)}

    E, H, discount = args.agreement_envs, args.horizon, 0.99
    rows = []
    for track in args.tracks:
        env = BatchedRaceEnv(track, E, 1, auto_reset=True, remap_actions=True)
        env.load_policy(checkpoint(args.checkpoint))
        settle(env, args.settle)
        start = env.views["action_in"].clone()
        wide = shooting_candidates(env, 64, H, hold=5, seed=0)                          # [E, 64, H, 1, 2]
        base = dream_vs_truth(env, wide, repeat=REPEAT)                                 # imagined (discount 1) and true returns of the 64
        best_true = base["true"].max(dim=1).values
        idx = torch.arange(E, device=wide.device)

        def score(seq, launches):
            """seq [E, H, 2]: the planner's chosen sequence, scored by the dream and by the simulator through dream_vs_truth"""
            d = dream_vs_truth(env, seq.reshape(E, 1, H, 1, 2), repeat=REPEAT)
            return {"imagined_return": stats(d["imagined"][:, 0]), "true_return": stats(d["true"][:, 0]),
                    "regret_to_best_of_64_in_truth": stats(best_true - d["true"][:, 0]), "launches_per_decision": launches}

        row = {"track": track, "true_return_best_minus_worst_of_64": stats(best_true - base["true"].min(dim=1).values)}
        # shooting-64: the candidate the dream ranks first (one dream_ahead launch)
        acts64 = to_dream_actions(wide)
        pick = env.dream_ahead(acts64, outputs=("return",))["return"].argmax(dim=1)
        row["shooting_64"] = score(acts64[idx, pick], 1)
        # CEM: dream_cem_act's loop, its final mean recovered from what it writes - only the first action is; so rerun its loop here
        gen = torch.Generator(device=wide.device)
        gen.manual_seed(0)
        mean = torch.zeros((E, 1, H, 2), device=wide.device)
        std = torch.ones((E, 1, H, 2), device=wide.device)
        for _ in range(3):
            draws = (mean + std * torch.randn((E, 64, H, 2), generator=gen, device=wide.device)).clamp_(-1.0, 1.0)
            ret = torch.nan_to_num(env.dream_ahead(draws, outputs=("return",))["return"], nan=float("-inf"))
            elite = draws[idx.unsqueeze(1), ret.topk(8, dim=1).indices]
            mean, std = elite.mean(dim=1, keepdim=True), elite.std(dim=1, unbiased=False, keepdim=True)
        env.views["action_in"].copy_(start)
        dream_cem_act(env, candidates=64, horizon=H, iterations=3, elites=8, seed=0)
        assert torch.equal(env.views["action_in"].reshape(E, 2), mean[:, 0, 0])          # the loop above is dream_cem_act's
        row["cem_64x3"] = score(mean[:, 0], 3)
        # gradient-refined shooting-8 (10 dream_ahead_grad launches and one dream_ahead)
        env.views["action_in"].copy_(start)
        info = {}
        dream_gradient_act(env, candidates=8, horizon=H, iterations=10, step=0.2, hold=5, seed=0, discount=discount, info=info)
        row["gradient_8x10"] = score(info["actions"], 11)
        row["gradient_8x10"]["imagined_gain_over_its_8_candidates_discount_0.99"] = stats(info["return"] - info["initial_return"].max(dim=1).values)
        # shooting-8 on the same eight candidates, for scale
        env.views["action_in"].copy_(start)
        acts8 = to_dream_actions(shooting_candidates(env, 8, H, hold=5, seed=0))
        row["shooting_8"] = score(acts8[idx, info["initial_return"].argmax(dim=1)], 1)
        env.views["action_in"].copy_(start)
        rows.append(row)
        env.close()
    return {"tool": "tools/dream_ahead_cost.py --grad --agreement", "device": torch.cuda.get_device_name(0), "checkpoint": args.checkpoint, "envs": E,
            "horizon": H, "repeat": REPEAT, "settle_agent_steps": args.settle, "mode": "mean",
            "note": "imagined_return and true_return are dream_vs_truth's of each planner's chosen sequence (undiscounted); threshold none",
            "threshold": None, "rows": rows}


def agreement(args):
    import numpy as np
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.planning import shooting_candidates
    from racing_dreamer_amd.world_model import dream_vs_truth

    def stats(x):
        x = np.asarray(x, np.float64)
        x = x[np.isfinite(x)]
        q = np.percentile(x, [25, 50, 75])
        return {"mean": round(float(x.mean()), 5), "q25": round(float(q[0]), 5), "median": round(float(q[1]), 5), "q75": round(float(q[2]), 5),
                "envs": int(x.size)}

    rows = []
    for track in args.tracks:
        env = BatchedRaceEnv(track, args.agreement_envs, 1, auto_reset=True, remap_actions=True)
        env.load_policy(checkpoint(args.checkpoint))
        settle(env, args.settle)
        cand = shooting_candidates(env, args.candidates, args.horizon, hold=5, seed=0)
        d = dream_vs_truth(env, cand, repeat=REPEAT)
        torch.cuda.synchronize()
        rows.append({"track": track, "rank_correlation": stats(d["rank_correlation"].cpu().numpy()),
                     "argmax_agreement": round(float(d["argmax_agree"].float().mean()), 5), "regret": stats(d["regret"].cpu().numpy()),
                     "true_return_best_minus_worst": stats((d["true"].max(dim=1).values - d["true"].min(dim=1).values).cpu().numpy()),
                     "imagined_return": stats(d["imagined"].mean(dim=1).cpu().numpy()), "true_return": stats(d["true"].mean(dim=1).cpu().numpy())})
        env.close()
    return {"tool": "tools/dream_ahead_cost.py --agreement", "device": torch.cuda.get_device_name(0), "checkpoint": args.checkpoint,
            "envs": args.agreement_envs, "candidates": args.candidates, "horizon": args.horizon, "repeat": REPEAT, "settle_agent_steps": args.settle,
            "mode": "mean", "chance_argmax_agreement": round(1.0 / args.candidates, 5), "threshold": None, "rows": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--starts", type=int, default=4096)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=15)
    ap.add_argument("--checkpoint", default="austria")
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--agreement", action="store_true")
    ap.add_argument("--grad", action="store_true")
    ap.add_argument("--agreement-envs", type=int, default=1024)
    ap.add_argument("--tracks", nargs="+", default=["austria", "columbia"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.grad:
        res = grad_agreement(args) if args.agreement else grad_cost(args)
    else:
        res = agreement(args) if args.agreement else cost(args)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
