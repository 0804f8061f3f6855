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
    ap.add_argument("--agreement-envs", type=int, default=1024)
    ap.add_argument("--tracks", nargs="+", default=["austria", "columbia"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = agreement(args) if args.agreement else cost(args)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
