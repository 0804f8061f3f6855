#!/usr/bin/env python3
"""Fit a value head for a shipped checkpoint by the reference's own rule, world model and actor frozen, and see whether planning
with its bootstrap agrees better with the simulator.  (Needs a GPU.)

    python tools/fit_critic.py [--checkpoint austria] [--envs 1024] [--iterations 400] [--out profiles/fit_critic_austria.json]
    python tools/fit_critic.py --fit device --out profiles/fit_critic_device_austria.json

No shipped checkpoint holds a value head; the reference trains one beside the actor (dreamer/models.py:113-137, value_lr 8e-5 of
dream.py:86 and grad_clip 1.0 of dream.py:88).  Each iteration here: one agent step of a running env under `policy_act`; one
`policy_returns(mode="sample", outputs=("features", "returns", "weight"))` from the live latents with the critic as it stands - the
targets; one Adam step on value_loss = -mean(weight * Normal(value(features[:, :-1]), 1).log_prob(returns)) for a
230-400-400-400-1 ELU MLP.  `--fit torch` (the default, what produced profiles/fit_critic_austria.json): torch autograd and
torch.optim.Adam, then `load_critic` with the new weights - a copy to the host and back in every iteration; its `--clip` defaults
to the 100 that profile was recorded with.  `--fit device`: `critic_fit` (rc_policy_fit_step: the reference's clip 1.0 and TF's
Adam), nothing leaves the GPU inside the loop.  No pcont head is fitted: pcont is the constant discount 0.99.

The record: the loss curve, the sha256 of the final weights (which are not kept: they are not reference data), and - next to
profiles/dream_ahead_agreement.json's numbers - how well 64 candidates' scores in the dream at H = 15 agree with the simulator's true
return over the same 15 steps and over 30 (the horizon the bootstrap is meant to see), without and with `bootstrap=True`
(score = discounted return + discount^H value(final feature)).  A record without a threshold: if the fit does not help, it says so."""
import argparse
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 4               # sub-steps per agent step: what the checkpoints were trained with, and dream_ahead_agreement.json's


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
    ap.add_argument("--iterations", type=int, default=400)
    ap.add_argument("--horizon", type=int, default=15)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--discount", type=float, default=0.99)
    ap.add_argument("--lambda", dest="lambda_", type=float, default=0.95)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fit", choices=("torch", "device"), default="torch", help="torch: autograd, torch.optim.Adam and load_critic "
                    "(what profiles/fit_critic_austria.json was recorded with); device: critic_fit, no host copy inside the loop")
    ap.add_argument("--clip", type=float, default=None, help="global-norm clip; default 100 with --fit torch, so that "
                    "profiles/fit_critic_austria.json stays what produced it, and the reference's 1.0 (dream.py:88) with --fit device")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    clip = args.clip if args.clip is not None else (100.0 if args.fit == "torch" else 1.0)
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.critic import init_critic
    from racing_dreamer_amd.planning import _dream_score, first_best, shooting_candidates, to_dream_actions
    from racing_dreamer_amd.world_model import rank_correlation

    weights = np.load(os.path.join(ROOT, "tests", "golden", f"dreamer_policy_{args.checkpoint}.npz"))
    env = BatchedRaceEnv(args.track, args.envs, 1, auto_reset=True, remap_actions=True)
    env.load_policy(weights)
    if not env.policy_has_reward_head:
        raise SystemExit(f"checkpoint {args.checkpoint} has no reward head")
    h, n = args.horizon, args.envs
    torch.manual_seed(args.seed)
    start = init_critic(args.seed, pcont=False)
    params = {k: torch.from_numpy(v).to(env.device).requires_grad_(True) for k, v in start.items()}
    opt = torch.optim.Adam(list(params.values()), lr=8e-5)

    def value_of(feat):
        x = feat
        for i in range(3):
            x = torch.nn.functional.elu(torch.addmm(params[f"value_h{i}_b"], x, params[f"value_h{i}_w"]))
        return torch.addmm(params["value_hout_b"], x, params["value_hout_w"])[:, 0]

    def upload():
        env.load_critic({k: v.detach().cpu().numpy() for k, v in params.items()})

    upload()
    if args.fit == "device":
        env.critic_fit_begin("value")
    curve = []
    with torch.cuda.stream(env.stream):
        env.reset(mode="random", seed=1)
        for k in range(args.settle):
            env.policy_act()
            env.step(None, repeat=REPEAT)
        for it in range(args.iterations):
            env.policy_act()
            env.step(None, repeat=REPEAT)
            got = env.policy_returns(h, "sample", seed=args.seed + it, lambda_=args.lambda_, discount=args.discount,
                                     outputs=("features", "returns", "weight"))
            feat = got["features"][:, :-1].reshape(-1, L.POLICY_FEATURE)
            target, weight = got["returns"].reshape(-1), got["weight"].reshape(-1)
            if args.fit == "device":
                loss = env.critic_fit(feat, target, weight, head="value", lr=8e-5, clip=clip)["loss"]
            else:
                loss = -(weight * (-0.5 * (value_of(feat) - target) ** 2 - 0.5 * math.log(2.0 * math.pi))).mean()
                opt.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(list(params.values()), clip)
                opt.step()
                upload()
            if it % 10 == 0 or it == args.iterations - 1:        # (the record reads two scalars back: outside the fit itself)
                curve.append({"iteration": it, "value_loss": round(float(loss.detach()), 6), "mean_return": round(float(target.mean()), 5)})
        if args.fit == "device":
            fitted = env.critic_weights()
            env.critic_fit_end("value")
        else:
            fitted = {k: params[k].detach().cpu().numpy() for k in L.VALUE_KEYS}
        digest = hashlib.sha256(b"".join(fitted[k].tobytes() for k in L.VALUE_KEYS)).hexdigest()

        # ---- the agreement of the dream's scores with the simulator, without and with the bootstrap
        long_h = 2 * h
        cand = shooting_candidates(env, args.candidates, long_h, hold=5, seed=args.seed + 1)      # [E, K, 2H, 1, 2]
        acts = to_dream_actions(cand[:, :, :h].contiguous())
        true = {f"true_return_{steps}_steps": env.look_ahead(cand[:, :, :steps].contiguous(), repeat=REPEAT, outputs=("return",))["return"][:, :, 0] for steps in (h, long_h)}
        scores = {"plain_return": _dream_score(env, acts, False, args.discount),
                  "bootstrap": _dream_score(env, acts, True, args.discount)}
        rows = torch.arange(n, device=env.device)
        agreement = {}
        for sname, score in scores.items():
            for tname, tr in true.items():
                pick, best = first_best(score), first_best(tr)
                agreement[f"{sname}_vs_{tname}"] = {"rank_correlation": stats(rank_correlation(score, tr)),
                                                    "argmax_agreement": round(float((pick == best).double().mean()), 5),
                                                    "regret": stats(tr[rows, best] - tr[rows, pick])}
        env.sync()
    out = {"tool": "tools/fit_critic.py", "device": torch.cuda.get_device_name(0), "checkpoint": args.checkpoint, "track": args.track, "envs": n,
           "iterations": args.iterations, "horizon": h, "lambda": args.lambda_, "discount": args.discount, "fit": args.fit,
           "optimizer": f"{'torch.optim.Adam' if args.fit == 'torch' else 'critic_fit (TF Adam)'} lr 8e-5, grad clip {clip:g}",
           "initial_critic": f"critic.init_critic({args.seed}, pcont=False)", "pcont": "constant discount (no pcont head fitted)",
           "loss_curve": curve, "final_value_weights_sha256": digest, "candidates": args.candidates, "long_horizon": long_h, "repeat": REPEAT,
           "chance_argmax_agreement": round(1.0 / args.candidates, 5), "threshold": None, "agreement": agreement}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    env.close()


if __name__ == "__main__":
    main()
