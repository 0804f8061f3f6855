#!/usr/bin/env python3
"""Train a shipped checkpoint's actor and a value head the way the reference does - both updates from one dream per replay batch - on
the device, the world model frozen, and record what happens to the driver.  (Needs a GPU.)

    python tools/train_behaviour.py [--checkpoint austria] [--track austria] [--steps 100] [--out profiles/train_behaviour_austria.json]
    python tools/train_behaviour.py --critic critic.npz          (a value head fitted by tools/fit_critic.py --fit device, saved with critic.save_critic)

An exploring agent (`policy_act` in mode "explore") fills a device-resident `TrajectoryRing`; every step then draws a batch of
`--windows` x `--length` records from it and calls `world_model.behaviour_learning_step`: `policy_observe` in `sample`, ONE
`policy_returns_grad` from the posterior features under the actor, `actor_fit` on the rows it returns and `critic_fit` on the imagined
features, returns and weights of the same launch (dreamer/models.py:113-137; actor_lr and value_lr 8e-5, grad_clip 1.0 of
dream.py:86-88 unless the options say otherwise).  The reward head, the RSSM and the pcont head (none is loaded: pcont is the
constant discount) do not move; the critic starts from `critic.init_critic(--critic-seed, pcont=False)` or from `--critic`.  No step
of the loop makes a host copy; the losses are read once, at the end.

The record: actor_loss and value_loss along the run, and `evaluate.evaluate` (the reference's protocol) of the actor in mode `mean` on
a held-out reset seed before and after; the sha256 of the fitted actor (the weights are not kept).  A record WITHOUT a threshold:
nobody has measured whether a frozen world model improves the driver here, and if it does not, the record says so."""
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
    ap.add_argument("--collect", type=int, default=150, help="agent steps of the exploring agent recorded into the ring")
    ap.add_argument("--steps", type=int, default=100, help="behaviour learning steps")
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--length", type=int, default=50)
    ap.add_argument("--horizon", type=int, default=15)
    ap.add_argument("--discount", type=float, default=0.99)
    ap.add_argument("--lambda", dest="lambda_", type=float, default=0.95)
    ap.add_argument("--critic", default=None, help="an .npz of critic.save_critic; default: the synthetic critic.init_critic(--critic-seed, pcont=False)")
    ap.add_argument("--critic-seed", type=int, default=0)
    ap.add_argument("--actor-lr", type=float, default=8e-5)
    ap.add_argument("--value-lr", type=float, default=8e-5)
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--max-calls", type=int, default=600, help="evaluate()'s step budget per evaluation")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--held-out-seed", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.critic import init_critic, load_critic_file
    from racing_dreamer_amd.evaluate import evaluate
    from racing_dreamer_amd.replay import TrajectoryRing
    from racing_dreamer_amd.world_model import behaviour_learning_step

    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, args.envs, 1, auto_reset=True, remap_actions=True, action_repeat=REPEAT)
    env.load_policy(weights)
    if not env.policy_has_reward_head:
        raise SystemExit(f"checkpoint {args.checkpoint} has no reward head: there is no return to learn from")
    env.load_critic(load_critic_file(args.critic) if args.critic else init_critic(args.critic_seed, pcont=False))

    def score():
        env.set_policy_sampling("mean")
        got = evaluate(env, lambda e: e.policy_act(), episodes=args.episodes, max_calls=args.max_calls, reset_mode="random", seed=args.held_out_seed)
        row = {k: round(float(got[k][0, 0]), 5) for k in ("ret_mean", "length_mean", "progress_mean", "time_mean", "share_wall")}
        row.update(episodes=int(got["episodes"][0, 0]), calls=int(got["calls"]), unfinished_envs=int(got["unfinished_envs"]))
        env.disable_episode_log()
        return row

    out = {"tool": "tools/train_behaviour.py", "checkpoint": args.checkpoint, "track": args.track, "envs": args.envs,
           "device": torch.cuda.get_device_name(0), "critic": args.critic or f"critic.init_critic({args.critic_seed}, pcont=False)",
           "collector": f"policy_act in mode explore, {args.collect} agent steps of {args.envs} envs, action repeat {REPEAT}",
           "steps": args.steps, "batch": [args.windows, args.length], "horizon": args.horizon, "lambda": args.lambda_, "discount": args.discount,
           "actor_lr": args.actor_lr, "value_lr": args.value_lr, "clip": args.clip,
           "evaluation": f"evaluate.evaluate, each env's first {args.episodes} episodes, random starts from seed {args.held_out_seed}, at most "
                         f"{args.max_calls} agent steps; the actor in mode mean",
           "threshold": None}
    with torch.cuda.stream(env.stream):
        out["before"] = score()
        ring = TrajectoryRing(env, args.collect + 2)
        env.set_policy_sampling("explore", seed=args.seed)
        ring.reset(mode="random", seed=args.seed)
        for k in range(args.collect):
            env.policy_act()
            ring.step(None)
        ring.detach()
        env.actor_fit_begin()
        env.critic_fit_begin("value")
        gen = torch.Generator()
        gen.manual_seed(args.seed)
        env.sync()
        t0 = time.perf_counter()
        curve = []
        for i in range(args.steps):
            batch = ring.sample(args.windows, args.length, fields=("lidar", "action"), generator=gen, check=False)
            got = behaviour_learning_step(env, batch, horizon=args.horizon, lambda_=args.lambda_, discount=args.discount, seed=args.seed + i,
                                          actor_fit=dict(lr=args.actor_lr, clip=args.clip), value_fit=dict(lr=args.value_lr, clip=args.clip))
            curve.append(torch.stack([got["actor_loss"].float(), got["value_loss"].float().reshape(()), got["actor"]["grad_norm"].reshape(()),
                                      got["value"]["grad_norm"].reshape(()), got["actor"]["skipped"].float().reshape(())]))
        env.sync()
        torch.cuda.synchronize()
        out["train_seconds"] = round(time.perf_counter() - t0, 3)
        out["ms_per_step"] = round(out["train_seconds"] / max(args.steps, 1) * 1e3, 3)
        env.actor_fit_end()
        env.critic_fit_end("value")
        curve = torch.stack(curve).cpu().numpy().astype(np.float64)
        tenth = max(1, len(curve) // 10)
        for j, name in enumerate(("actor_loss", "value_loss", "actor_grad_norm", "value_grad_norm")):
            out[name + "_every_tenth"] = [round(float(curve[i:i + tenth, j].mean()), 6) for i in range(0, len(curve), tenth)]
        out["skipped_actor_steps"] = int(curve[:, 4].sum())
        out["after"] = score()
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
