"""Imagination against the simulator, open loop: after a settling run the agent's world model imagines H = 15 steps ahead under its
own actor (`env.policy_imagine`), then the real env is driven with exactly those actions from the same states, and the head's
predicted reward is set beside the simulated reward of each step.

    python tools/imagine_open_loop.py [--tracks austria columbia] [--envs 1024] [--out profiles/imagine_open_loop.json] [--pure]

`--pure` takes the pairs from `world_model.imagined_vs_simulated` instead - the same dream, the simulated side from
`env.look_ahead`, which leaves the env where it stands (the finishing step of an env is not counted there either).

A record for users, with no pass or fail threshold: the reward scale of the simulator the checkpoints were trained on against this
one's is not pinned."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(track, args):
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv(track, args.envs, args.cars, auto_reset=True, remap_actions=True)
    env.load_policy(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env.reset(mode="random", seed=args.seed)
    for k in range(args.settle):
        env.policy_act()
        env.step(None, repeat=4)
    env.policy_act()                                        # the latent takes in the last scan: the dream starts where the env stands
    n, h = env.n_cars, args.horizon
    if args.pure:
        from racing_dreamer_amd.world_model import imagined_vs_simulated
        pairs = imagined_vs_simulated(env, h, "mean", repeat=4)
        real, ok, pred = (pairs[k].cpu().numpy() for k in ("simulated", "alive", "predicted"))
        real, pred = real.astype(np.float64), pred.astype(np.float64)
    else:
        dream = env.policy_imagine(h, "mean")
        real, alive = [], torch.ones(n, dtype=torch.bool, device=env.device)
        ok = []
        for t in range(h):
            out = env.step(dream["action"][:, t].reshape(env.num_envs, env.cars_per_env, 2), repeat=4)
            real.append(out["reward"].reshape(n).clone())
            alive &= out["fresh"].reshape(n) == 0               # (an env that was reset on the way has left the imagined episode)
            ok.append(alive.clone())
        real, ok, pred = torch.stack(real, 1).cpu().numpy().astype(np.float64), torch.stack(ok, 1).cpu().numpy(), dream["reward"].cpu().numpy().astype(np.float64)
    env.close()
    rows = []
    for slot in range(args.cars):
        sel = np.zeros(n, bool)
        sel[slot::args.cars] = True
        m = ok & sel[:, None]
        p, r = pred[m], real[m]
        per_step = [{"t": t, "cars": int(m[:, t].sum()), "predicted_mean": float(pred[m[:, t], t].mean()), "simulated_mean": float(real[m[:, t], t].mean())}
                    for t in range(h) if m[:, t].any()]
        rows.append({"track": track, "slot": slot, "pairs": int(m.sum()), "correlation": float(np.corrcoef(p, r)[0, 1]) if m.sum() > 2 and p.std() > 0 and r.std() > 0 else None,
                     "mean_error_predicted_minus_simulated": float((p - r).mean()), "predicted_mean": float(p.mean()), "simulated_mean": float(r.mean()),
                     "per_step": per_step})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", nargs="+", default=["austria", "columbia"])
    ap.add_argument("--checkpoint", default="austria")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--cars", type=int, default=1)
    ap.add_argument("--horizon", type=int, default=15)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pure", action="store_true", help="simulated rewards from env.look_ahead (world_model.imagined_vs_simulated): the env is not driven")
    args = ap.parse_args()
    out = {"tool": "tools/imagine_open_loop.py", "checkpoint": args.checkpoint, "envs": args.envs, "cars_per_env": args.cars, "horizon": args.horizon,
           "settle_agent_steps": args.settle, "repeat": 4, "mode": "mean", **({"pure": True} if args.pure else {}), "threshold": None, "rows": [r for tr in args.tracks for r in measure(tr, args)]}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
