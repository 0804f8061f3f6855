"""Planning against the simulator's true dynamics (`BatchedRaceEnv.look_ahead`): a random-shooting
baseline beside the learned agents, and an expert that sees further than follow-the-gap - and the same planners against the
world model's dream (`BatchedRaceEnv.dream_ahead`, item 19: PlaNet-style random shooting and the cross-entropy method on the
imagined return of a checkpoint with a reward head; `dream_gradient_act` refines a few shooting candidates along the gradient
of that return, `BatchedRaceEnv.dream_ahead_grad`, item 23).

    env.reset(mode="random", seed=0)
    for _ in range(steps):
        shooting_act(env, candidates=64, horizon=15)       # writes action_in
        env.step(None)

`dream_shooting_act`, `dream_cem_act` and `dream_gradient_act` take `shooting_act`'s place in that loop after `policy_act` has carried the latents to
the current observation (on an env built with `remap_actions=True`: the dream's actions are raw, in [-1, 1], and what is written
into `action_in` is raw too).

The candidates are generated in torch on the env's device; the look-ahead is one launch; the choice is a few torch operations
on [num_envs, candidates] - nothing here is a hot path of its own."""
from __future__ import annotations

from typing import Optional, Union

import torch


def shooting_candidates(env, candidates: int, horizon: int, hold: int = 5, seed: int = 0) -> torch.Tensor:
    """float32 [num_envs, candidates, horizon, cars_per_env, 2] on the env's device: piecewise-constant action sequences - a
    new U(-1, 1)^2 draw every `hold` agent steps, from a torch generator seeded with `seed` - in `step`'s convention.
    Candidate 0 repeats the env's current `action_in` ("keep doing what you do" is always among the choices)."""
    K, H, hold = int(candidates), int(horizon), int(hold)
    if K < 1 or H < 1 or hold < 1:
        raise ValueError(f"candidates, horizon and hold must be >= 1 (got {candidates}, {horizon}, {hold})")
    E, A = env.num_envs, env.cars_per_env
    device = torch.device(env.device)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    pieces = (H + hold - 1) // hold
    u = torch.rand((E, K, pieces, A, 2), generator=gen, dtype=torch.float32, device=device) * 2.0 - 1.0
    seq = u.repeat_interleave(hold, dim=2)[:, :, :H].contiguous()
    seq[:, 0] = env.views["action_in"].reshape(E, 1, A, 2).to(torch.float32)
    return seq


def first_best(score: torch.Tensor) -> torch.Tensor:
    """int64 [E]: per row of score [E, K] the LOWEST index among the entries equal to the row's maximum (a NaN never wins)."""
    s = torch.nan_to_num(score, nan=float("-inf"))
    k = torch.arange(s.shape[1], device=s.device).expand_as(s)
    return torch.where(s == s.max(dim=1, keepdim=True).values, k, s.shape[1]).min(dim=1).values


def shooting_act(env, candidates: Union[int, torch.Tensor] = 64, horizon: int = 15, hold: int = 5, seed: int = 0,
                 others: str = "hold", repeat=None) -> torch.Tensor:
    """Random shooting: look ahead under `candidates` sequences per env (`shooting_candidates`, or a tensor of explicit
    sequences [num_envs, K, H, cars_per_env, 2]) and take, per env, the one with the highest true return of car slot 0 - the
    lowest index among equals.  Writes that candidate's first action into `action_in` and returns `action_in`, so
    `env.step(None)` applies it.  With several cars per env, others="hold" keeps the other slots on their current `action_in`
    in every candidate (and so in what is written); others="free" leaves them what the candidates say.  `repeat`: as `look_ahead` (None: the env's default)."""
    if others not in ("hold", "free"):
        raise ValueError(f"others must be 'hold' or 'free', got {others!r}")
    E, A = env.num_envs, env.cars_per_env
    action_in = env.views["action_in"]
    seq = candidates if torch.is_tensor(candidates) else shooting_candidates(env, candidates, horizon, hold, seed)
    seq = seq.to(action_in.device, torch.float32).reshape(E, -1, seq.shape[2], A, 2)
    if A > 1 and others == "hold":
        seq = seq.clone()
        seq[:, :, :, 1:] = action_in.reshape(E, 1, 1, A, 2)[:, :, :, 1:]
    ret = env.look_ahead(seq, repeat=repeat, outputs=("return",))["return"]
    best = first_best(ret[:, :, 0])
    action_in.copy_(seq[torch.arange(E, device=seq.device), best, 0].reshape(action_in.shape))
    return action_in


def to_dream_actions(seq: torch.Tensor) -> torch.Tensor:
    """`look_ahead`'s candidates [E, K, H, A, 2] as `dream_ahead`'s [E * A, K, H, 2]: one start per car, car = env * A + slot."""
    E, K, H, A, _ = seq.shape
    return seq.permute(0, 3, 1, 2, 4).reshape(E * A, K, H, 2).contiguous()


def _needs_head(env, who: str) -> None:
    if not env.policy_has_reward_head:
        raise RuntimeError(f"{who} needs a checkpoint with a reward head (reward_* arrays)")


def _dream_score(env, acts: torch.Tensor, bootstrap: bool, discount: float, **where) -> torch.Tensor:
    """[starts, K]: the imagined return of every candidate - `dream_ahead`'s call of the planners as it always was - or, with
    `bootstrap`, the discounted return plus discount^H times the value head on the feature the candidate ends in
    (`policy_value`): a plan that sees beyond its horizon.  `where`: the caller's `slots`, passed on as it always passed them."""
    if not bootstrap:
        return env.dream_ahead(acts, **where, outputs=("return",))["return"]
    if not env.policy_has_value_head:
        raise RuntimeError("bootstrap=True needs a value head (load_critic, or a checkpoint with value_* arrays)")
    got = env.dream_ahead(acts, **where, discount=discount, outputs=("return", "final_feature"))
    value = env.policy_value(got["final_feature"])["value"]
    return got["return"] + float(discount) ** int(acts.shape[2]) * value


def dream_shooting_act(env, candidates: Union[int, torch.Tensor] = 64, horizon: int = 15, hold: int = 5, seed: int = 0, slots=None,
                       bootstrap: bool = False, discount: float = 0.99) -> torch.Tensor:
    """Random shooting in the dream: the candidates of `shooting_candidates` (or a tensor of explicit sequences
    [num_envs, K, H, cars_per_env, 2]), each car's own sequences scored by the imagined return from its live latent
    (`dream_ahead`, mode "mean"), the highest taken - the lowest index among equals.  Writes that candidate's first action into
    `action_in` for the cars in `slots` (None: every car; the others keep theirs) and returns `action_in`.  `bootstrap=True`
    (needs a value head): the score is the return discounted by `discount` plus discount^H times the value of the final
    feature; `discount` is not read otherwise."""
    _needs_head(env, "dream_shooting_act")
    E, A = env.num_envs, env.cars_per_env
    action_in = env.views["action_in"]
    seq = candidates if torch.is_tensor(candidates) else shooting_candidates(env, candidates, horizon, hold, seed)
    seq = seq.to(action_in.device, torch.float32).reshape(E, -1, seq.shape[2], A, 2)
    acts = to_dream_actions(seq)                                                           # [E A, K, H, 2]
    ret = _dream_score(env, acts, bootstrap, discount, slots=slots)                            # [E A, K]
    best = first_best(ret)
    first = acts[torch.arange(E * A, device=acts.device), best, 0].reshape(E, A, 2)
    flat = action_in.reshape(E, A, 2)
    for a in (range(A) if slots is None else sorted({int(b) for b in slots})):
        flat[:, a] = first[:, a]
    return action_in


def dream_cem_act(env, candidates: int = 64, horizon: int = 15, iterations: int = 3, elites: int = 8, seed: int = 0,
                  bootstrap: bool = False, discount: float = 0.99) -> torch.Tensor:
    """The cross-entropy method in the dream (PlaNet's planner): per car a Gaussian over the sequence [H, 2], mean 0 and
    standard deviation 1 at first; `iterations` times, `candidates` sequences are drawn from it (clipped to [-1, 1]), scored by
    the imagined return from the car's live latent, and the Gaussian is refit to the `elites` best (mean, and the biased
    standard deviation).  All draws come from one torch generator seeded with `seed`.  Writes the first action of the final
    mean into `action_in` and returns `action_in`.  `bootstrap`, `discount`: as `dream_shooting_act`."""
    _needs_head(env, "dream_cem_act")
    K, H, n_it, top = int(candidates), int(horizon), int(iterations), int(elites)
    if K < 1 or H < 1 or n_it < 1 or not 1 <= top <= K:
        raise ValueError(f"candidates, horizon and iterations must be >= 1 and elites in [1, candidates] (got {candidates}, {horizon}, {iterations}, {elites})")
    n = env.num_envs * env.cars_per_env
    action_in = env.views["action_in"]
    device = action_in.device
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    mean = torch.zeros((n, 1, H, 2), dtype=torch.float32, device=device)
    std = torch.ones((n, 1, H, 2), dtype=torch.float32, device=device)
    rows = torch.arange(n, device=device).unsqueeze(1)
    for _ in range(n_it):
        noise = torch.randn((n, K, H, 2), generator=gen, dtype=torch.float32, device=device)
        acts = (mean + std * noise).clamp_(-1.0, 1.0)
        ret = torch.nan_to_num(_dream_score(env, acts, bootstrap, discount), nan=float("-inf"))
        elite = acts[rows, ret.topk(top, dim=1).indices]                                   # [n, top, H, 2]
        mean = elite.mean(dim=1, keepdim=True)
        std = elite.std(dim=1, unbiased=False, keepdim=True)
    action_in.copy_(mean[:, 0, 0].reshape(action_in.shape))
    return action_in


def dream_gradient_act(env, candidates: Union[int, torch.Tensor] = 8, horizon: int = 15, iterations: int = 10, step: float = 0.2, hold: int = 5,
                       seed: int = 0, slots=None, discount: float = 0.99, info: Optional[dict] = None) -> torch.Tensor:
    """Gradient-based planning in the dream: start from the candidates of `shooting_candidates` (or a tensor of explicit sequences
    [num_envs, K, H, cars_per_env, 2]); `iterations` times, one `dream_ahead_grad` call (mode "mean") scores every sequence and
    gives d return / d actions, and every sequence moves by `step` along its gradient normalised by its largest entry,
    a <- clamp(a + step g / max|g|, -1, 1); one `dream_ahead` call scores the last iterate.  Per (car, candidate) the
    best-scoring iterate seen is kept, so the result never scores below `dream_shooting_act` on the same candidates under the
    same `discount`.  Writes the first action of the best iterate of the best candidate - the lowest index among equals - into
    `action_in` for the cars in `slots` (None: every car) and returns `action_in`.  `info`, a dict, receives `return` [cars] of
    what was chosen, `initial_return` [cars, K] of the candidates as given and `actions` [cars, H, 2], the chosen sequence."""
    _needs_head(env, "dream_gradient_act")
    n_it, step = int(iterations), float(step)
    if n_it < 0 or not step > 0.0:
        raise ValueError(f"iterations must be >= 0 and step > 0 (got {iterations}, {step})")
    E, A = env.num_envs, env.cars_per_env
    action_in = env.views["action_in"]
    seq = candidates if torch.is_tensor(candidates) else shooting_candidates(env, candidates, horizon, hold, seed)
    seq = seq.to(action_in.device, torch.float32).reshape(E, -1, seq.shape[2], A, 2)
    acts = to_dream_actions(seq)                                                           # [E A, K, H, 2]
    best_ret = best_acts = first_ret = None
    for it in range(n_it + 1):
        if it < n_it:
            got = env.dream_ahead_grad(acts, slots=slots, discount=discount, outputs=("grad_actions", "return"))
        else:
            got = env.dream_ahead(acts, slots=slots, discount=discount, outputs=("return",))
        ret = torch.nan_to_num(got["return"], nan=float("-inf"))
        if best_ret is None:
            first_ret, best_ret, best_acts = ret, ret.clone(), acts.clone()
        else:
            better = ret > best_ret
            best_ret = torch.where(better, ret, best_ret)
            best_acts = torch.where(better[:, :, None, None], acts, best_acts)
        if it < n_it:
            g = torch.nan_to_num(got["grad_actions"], nan=0.0, posinf=0.0, neginf=0.0)
            scale = g.abs().amax(dim=(2, 3), keepdim=True).clamp_min(1e-30)
            acts = (acts + step * (g / scale)).clamp_(-1.0, 1.0)
    best = first_best(best_ret)
    rows = torch.arange(E * A, device=acts.device)
    chosen = best_acts[rows, best]                                                         # [E A, H, 2]
    first = chosen[:, 0].reshape(E, A, 2)
    flat = action_in.reshape(E, A, 2)
    for a in (range(A) if slots is None else sorted({int(b) for b in slots})):
        flat[:, a] = first[:, a]
    if info is not None:
        info.update({"return": best_ret[rows, best], "initial_return": first_ret, "actions": chosen})
    return action_in


def distil_step(env, expert, slots=None, **fit) -> dict:
    """One step of distilling a planner into the actor, on an env built with `remap_actions=True` whose
    actor optimizer is open (`actor_fit_begin`): read every car's live feature from `policy_state` (as `policy_act` last left
    it), ask `expert(env)` - one of the planners above, e.g. `lambda e: shooting_act(e, 64)`, or any callable that returns raw
    actions shaped like `action_in` - for its action at the present state, put `action_in` back as it was, and take one
    `actor_fit(features, target=the expert's actions)` step; `fit` is passed on to it (lr, clip, eps, ...).  `slots`: the car
    slots whose rows are fitted (None: all).  Returns `actor_fit`'s status with `target` [rows, 2] and `features` [rows, 230]."""
    E, A = env.num_envs, env.cars_per_env
    action_in = env.views["action_in"]
    kept = action_in.clone()
    label = expert(env)
    label = (action_in if label is None else label).to(action_in.device, torch.float32).reshape(E, A, 2).clone()
    action_in.copy_(kept)
    feat = env.policy_state[:, :230].reshape(E, A, 230)
    if slots is not None:
        pick = sorted({int(a) for a in slots})
        feat, label = feat[:, pick], label[:, pick]
    feat, label = feat.reshape(-1, 230).contiguous(), label.reshape(-1, 2).clamp(-1.0, 1.0).contiguous()
    out = dict(env.actor_fit(feat, target=label, **fit))
    out["target"], out["features"] = label, feat
    return out


def distil_actor(env, expert, iterations: int, act: str = "explore", seed: int = 0, expl_amount: Optional[float] = None,
                 slots=None, **fit) -> torch.Tensor:
    """DAgger on the device: `iterations` times the ACTOR drives - `policy_act` in mode `act` ("explore": its own draw plus
    exploration noise, so that the visited latents spread; or "mean"), then `step` - and `distil_step` fits it to `expert`'s
    action on every visited latent, before the step is taken.  The actor's optimizer must be open (`actor_fit_begin`); the
    sampling mode is restored at the end.  Returns the per-iteration `loss` as a device tensor [iterations]."""
    if act not in ("explore", "mean"):
        raise ValueError(f"act must be 'explore' or 'mean', got {act!r}")
    before = env.policy_sampling
    env.set_policy_sampling(act, seed=seed, expl_amount=expl_amount)
    losses = []
    try:
        for _ in range(int(iterations)):
            env.policy_act(slots)
            losses.append(distil_step(env, expert, slots=slots, **fit)["loss"])
            env.step(None)
    finally:
        env.set_policy_sampling(before["mode"], seed=before["seed"], expl_amount=before["expl_amount"])
    return torch.stack(losses) if losses else torch.zeros(0, device=env.views["action_in"].device)
