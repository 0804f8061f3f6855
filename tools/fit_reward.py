#!/usr/bin/env python3
"""Fit a shipped checkpoint's reward head to THIS simulator's rewards on the device, world model and actor frozen, and see how much
of the gap between the dream and the simulator the head explains.  (Needs a GPU.)

    python tools/fit_reward.py [--checkpoint austria] [--track austria] [--envs 1024] [--iterations 400] [--out profiles/fit_reward_austria.json]
    python tools/fit_reward.py --track columbia --out profiles/fit_reward_columbia.json

The shipped reward heads were trained in the reference's simulator; against this one the dream's reward correlates 0.767 on austria
and 0.033 on columbia (profiles/imagine_open_loop.json).  Here: `--envs` envs run `--collect` agent steps under the device agent
in `explore` mode with a TrajectoryRing recording them; then `--iterations` times one batch of 50 windows x 50 steps is drawn from
the ring and `world_model.reward_learning_step` moves the head (`policy_observe(mode="sample")`, then `reward_fit`: the reference's
model_lr 6e-4 and grad_clip 1.0, TF's Adam) - the step makes no host copy; the draw reads its count of failed windows.  Only the head's six arrays move: the
reference trains this term inside its model loss, where the gradient also reaches the RSSM and the encoder.

The record, before and after the fit, all on HELD-OUT data - a second run of the same envs from another reset seed under another
sampling seed, recorded into the cleared ring:
  reward_loglik     `world_model.model_terms` on windows drawn from the held-out ring
  open_loop         `world_model.imagined_vs_simulated`: the correlation of imagined against simulated reward under the actor's own
                    actions, H = 15, the pairs of steps whose env was still running (profiles/imagine_open_loop.json's figure)
  planning          `world_model.dream_vs_truth` on 64 shooting candidates: rank correlation, first-choice agreement and regret
                    (profiles/dream_ahead_agreement.json's figures)
Both heads are scored on the same latents and the same env state (`load_reward_head` resets neither).  The fitted weights are
not kept; their sha256 is.  A record without a threshold: if the head does not carry the gap, it says so."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 4               # sub-steps per agent step: what the checkpoints were trained with


def stats(x):
    import torch
    x = x.to(torch.float64).flatten()
    x = x[~torch.isnan(x)]                                   # (a constant row has no rank correlation)
    q = torch.quantile(x, torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64, device=x.device))
    return {"mean": round(float(x.mean()), 5), "q25": round(float(q[0]), 5), "median": round(float(q[1]), 5), "q75": round(float(q[2]), 5), "envs": int(x.numel())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--checkpoint", default="austria")
    ap.add_argument("--track", default="austria")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--collect", type=int, default=150, help="agent steps recorded before the fit (the ring's capacity)")
    ap.add_argument("--iterations", type=int, default=400)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--length", type=int, default=50)
    ap.add_argument("--horizon", type=int, default=15)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--held-out-batches", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--held-out-seed", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=6e-4)
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.planning import shooting_candidates
    from racing_dreamer_amd.replay import TrajectoryRing
    from racing_dreamer_amd.world_model import dream_vs_truth, imagined_vs_simulated, model_terms, reward_learning_step

    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, args.envs, 1, auto_reset=True, remap_actions=True)
    env.load_policy(weights)
    if not env.policy_has_reward_head:
        raise SystemExit(f"checkpoint {args.checkpoint} has no reward head")
    fields = ("lidar", "action", "reward")
    ring = TrajectoryRing(env, args.collect + 1)

    def collect(seed):
        """a run of every env from reset seed `seed` under the exploring agent, recorded from its first record on"""
        ring.clear()
        env.set_policy_sampling("explore", seed=seed)
        ring.reset(mode="random", seed=seed + 1)
        for k in range(args.collect):
            env.policy_act()
            ring.step(None, repeat=REPEAT)

    def score(held):
        """the held-out figures of the head that is loaded, on the window batches `held` and the env as it stands"""
        loglik = torch.stack([model_terms(env, batch)["reward_loglik"].double() for batch in held]).mean()
        pair = imagined_vs_simulated(env, args.horizon, "mean", repeat=REPEAT)
        p, s = pair["predicted"][pair["alive"]].double(), pair["simulated"][pair["alive"]].double()
        cand = shooting_candidates(env, args.candidates, args.horizon, hold=5, seed=args.held_out_seed + 2)
        plan = dream_vs_truth(env, cand, repeat=REPEAT)
        return {"reward_loglik": round(float(loglik), 6),
                "open_loop": {"pairs": int(p.numel()), "correlation": round(float(torch.corrcoef(torch.stack([p, s]))[0, 1]), 5),
                              "predicted_mean": round(float(p.mean()), 5), "simulated_mean": round(float(s.mean()), 5)},
                "planning": {"rank_correlation": stats(plan["rank_correlation"]),
                             "argmax_agreement": round(float(plan["argmax_agree"].double().mean()), 5), "regret": stats(plan["regret"])}}

    curve = []
    with torch.cuda.stream(env.stream):
        shipped = env.reward_head_weights()
        collect(args.seed)
        env.reward_fit_begin()
        gen = torch.Generator(device="cpu").manual_seed(args.seed)
        for it in range(args.iterations):
            batch = ring.sample(args.batch, args.length, fields=fields, generator=gen)      # (check: a window that found no start raises)
            status = reward_learning_step(env, batch, seed=args.seed + it, lr=args.lr, clip=args.clip)
            if it % 10 == 0 or it == args.iterations - 1:        # (the record reads three scalars back: outside the fit itself)
                curve.append({"iteration": it, "reward_loss": round(float(status["reward_loss"]), 6), "grad_norm": round(float(status["grad_norm"]), 6),
                              "skipped": int(status["skipped"])})
        fitted = env.reward_head_weights()
        env.reward_fit_end()
        digest = hashlib.sha256(b"".join(fitted[k].tobytes() for k in L.HEAD_KEYS)).hexdigest()
        # ---- held out: another run of the same envs; both heads on the same latents, the same env state, the same windows
        collect(args.held_out_seed)
        gen = torch.Generator(device="cpu").manual_seed(args.held_out_seed)
        held = [ring.sample(args.batch, args.length, fields=fields, generator=gen) for k in range(args.held_out_batches)]
        env.load_reward_head(shipped)
        before = score(held)
        env.load_reward_head(fitted)
        after = score(held)
        env.sync()
    ring.detach()
    out = {"tool": "tools/fit_reward.py", "device": torch.cuda.get_device_name(0), "checkpoint": args.checkpoint, "track": args.track,
           "envs": args.envs, "collected_agent_steps": args.collect, "agent_mode": "explore", "repeat": REPEAT, "iterations": args.iterations,
           "batch": [args.batch, args.length], "optimizer": f"reward_fit (TF Adam) lr {args.lr:g}, grad clip {args.clip:g}",
           "seed": args.seed, "held_out_seed": args.held_out_seed, "held_out_batches": args.held_out_batches, "horizon": args.horizon,
           "candidates": args.candidates, "chance_argmax_agreement": round(1.0 / args.candidates, 5), "threshold": None,
           "loss_curve": curve, "final_reward_head_sha256": digest, "held_out": {"before": before, "after": after}}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    env.close()


if __name__ == "__main__":
    main()
