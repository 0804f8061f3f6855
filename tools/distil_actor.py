#!/usr/bin/env python3
"""Distil a planner that sees the true dynamics into a shipped checkpoint's actor, on the device, and see what the actor gains.
(Needs a GPU.)

    python tools/distil_actor.py [--checkpoint austria] [--track austria] [--envs 256] [--iterations 300] [--out profiles/distil_actor_austria.json]
    python tools/distil_actor.py --track columbia --out profiles/distil_actor_columbia.json

The expert is `planning.shooting_act` (`--candidates` piecewise-constant sequences over `--horizon` agent steps, scored by the
simulator's own look-ahead).  `planning.distil_actor` is the DAgger loop: the ACTOR drives (`policy_act` in `--act` mode, then the
step), every visited latent is labelled with the expert's action and `actor_fit(target=...)` takes one step (the reference's actor_lr
8e-5 and grad_clip 1.0 unless `--lr` / `--clip` say otherwise, TF's Adam).  World model, heads and critic are frozen: the actor's ten
arrays move and nothing else.  No step of the loop makes a host copy; the losses are read once, at the end.

The record: `evaluate.evaluate` (the reference's protocol: each env's first `--episodes` episodes) of the actor in mode `mean` on a
HELD-OUT reset seed, before and after the distillation and - for scale - of the expert itself on the same seed; the loss curve; the
sha256 of the fitted actor (the weights are not kept).  A record without a threshold: if the actor does not gain, it says so."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 4               # sub-steps per agent step: what the checkpoints were trained with


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--checkpoint", default="austria")
    ap.add_argument("--track", default="austria")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--act", default="explore", choices=["explore", "mean"])
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=15)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--max-calls", type=int, default=600, help="evaluate()'s step budget per evaluation")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--held-out-seed", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=8e-5)
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.evaluate import evaluate
    from racing_dreamer_amd.planning import distil_actor, shooting_act

    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, args.envs, 1, auto_reset=True, remap_actions=True, action_repeat=REPEAT)
    env.load_policy(weights)
    calls = [0]

    def expert(e):
        calls[0] += 1
        return shooting_act(e, candidates=args.candidates, horizon=args.horizon, seed=args.seed + calls[0])

    def score(act):
        got = evaluate(env, act, episodes=args.episodes, max_calls=args.max_calls, reset_mode="random", seed=args.held_out_seed)
        row = {k: round(float(got[k][0, 0]), 5) for k in ("ret_mean", "length_mean", "progress_mean", "time_mean", "share_wall")}
        row.update(episodes=int(got["episodes"][0, 0]), calls=int(got["calls"]), unfinished_envs=int(got["unfinished_envs"]))
        env.disable_episode_log()
        return row

    def actor(e):
        e.policy_act()

    out = {"tool": "tools/distil_actor.py", "checkpoint": args.checkpoint, "track": args.track, "envs": args.envs, "device": torch.cuda.get_device_name(0),
           "expert": f"planning.shooting_act, {args.candidates} candidates, horizon {args.horizon}, on the simulator's true dynamics",
           "iterations": args.iterations, "act": args.act, "lr": args.lr, "clip": args.clip, "rows_per_step": env.n_cars,
           "evaluation": f"evaluate.evaluate, each env's first {args.episodes} episodes, random starts from seed {args.held_out_seed}, at most "
                         f"{args.max_calls} agent steps, action repeat {REPEAT}; the actor in mode mean"}
    with torch.cuda.stream(env.stream):
        env.set_policy_sampling("mean")
        out["before"] = score(actor)
        out["expert_itself"] = score(expert)
        env.reset(mode="random", seed=args.seed)
        env.actor_fit_begin()
        env.sync()
        t0 = time.perf_counter()
        losses = distil_actor(env, expert, args.iterations, act=args.act, seed=args.seed, lr=args.lr, clip=args.clip)
        env.sync()
        torch.cuda.synchronize()
        out["distil_seconds"] = round(time.perf_counter() - t0, 3)
        env.actor_fit_end()
        curve = losses.cpu().numpy().astype(np.float64)
        tenth = max(1, len(curve) // 10)
        out["loss_first_tenth"], out["loss_last_tenth"] = round(float(curve[:tenth].mean()), 6), round(float(curve[-tenth:].mean()), 6)
        out["loss_curve_every_tenth"] = [round(float(curve[i:i + tenth].mean()), 6) for i in range(0, len(curve), tenth)]
        out["after"] = score(actor)
    fitted = env.actor_weights()
    out["fitted_actor_sha256"] = hashlib.sha256(b"".join(fitted[k].tobytes() for k in L.ACTOR_KEYS)).hexdigest()
    out["progress_mean_after_minus_before"] = round(out["after"]["progress_mean"] - out["before"]["progress_mean"], 5)
    out["ret_mean_after_minus_before"] = round(out["after"]["ret_mean"] - out["before"]["ret_mean"], 5)
    env.close()
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
