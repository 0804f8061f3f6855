"""What the reference does with a replay batch before the gradient, on device-resident batches (`BatchedRaceEnv.policy_observe`,
DESIGN.md §2 item 17): the open-loop summary of dreamer/models.py:243-277 `_image_summaries` (and
dreamer/evaluations/produce_reconstruction.py:36-57) and the two scalars dreamer/models.py:84-110 `_train` logs from the world
model.  A batch is a dict of device tensors as `TrajectoryRing.sample` returns it: `lidar` [B, T, 1080] in metres, `action`
[B, T, 2] RAW in [-1, 1] (what a ring records when the env was built with `remap_actions=True`), and where needed
`lidar_occupancy` [B, T, 64, 64(, 1)] and `reward` [B, T]."""
from __future__ import annotations

import math
from typing import Dict

import torch


def open_loop_summary(env, batch: Dict[str, torch.Tensor], context: int = 5) -> Dict[str, torch.Tensor]:
    """The reference's "observe `context` steps, imagine the rest" for a `lidar_occupancy` checkpoint: `policy_observe` with
    `context`, then `policy_decode` on the features [B, T, 230].  Returns float32 [B, T, 64, 64] tensors `truth` (the recorded
    occupancy), `model` (the decoder's image: the reconstruction for t < context, the open-loop prediction after it) and
    `error` = (model - truth + 1) / 2 in {0, 1/2, 1}, and `mismatch` int64 [B, T]: the pixels in which the two differ."""
    feat = env.policy_observe(batch["lidar"], batch["action"], context=context)["feature"]
    model = env.policy_decode(features=feat)["image"].to(torch.float32)
    truth = batch["lidar_occupancy"].to(model.device).reshape(model.shape).to(torch.float32)
    return dict(truth=truth, model=model, error=(model - truth + 1) / 2, mismatch=(model != truth).flatten(-2).sum(-1))


def model_terms(env, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """`div` = mean over the batch of KL(post || prior) and, when the checkpoint has a reward head, `reward_loglik` = the mean of
    Normal(predicted reward, 1).log_prob(batch["reward"]): the two world-model scalars of `_train`, computed in torch from
    `policy_observe`'s outputs (context = T: `RSSM.observe`)."""
    head = env.policy_has_reward_head
    out = env.policy_observe(batch["lidar"], batch["action"], outputs=("kl", "reward") if head else ("kl",))
    terms = {"div": out["kl"].mean()}
    if head:
        r = batch["reward"].to(out["reward"].device, torch.float32).reshape(out["reward"].shape)
        terms["reward_loglik"] = (-0.5 * (r - out["reward"]) ** 2 - 0.5 * math.log(2.0 * math.pi)).mean()
    return terms


def _lidar_decoder_needed(env, what: str) -> None:
    if not getattr(env, "policy_has_lidar_decoder", False):
        raise RuntimeError(f"{what} needs a LidarDistanceDecoder (load_lidar_decoder, or ldec_* arrays in the checkpoint)")


def _image_term(env, batch, feat, what: str) -> torch.Tensor:
    """The mean over the features' leading dimensions of the loaded decoder's log-probability of the recorded observation: the
    LidarDistanceDecoder's of `lidar` when one is loaded, else the LidarOccupancyDecoder's of `lidar_occupancy`; float64."""
    if getattr(env, "policy_has_lidar_decoder", False):
        scan = batch["lidar"].reshape(feat.shape[:-1] + (1080,))
        return env.policy_decode_lidar(features=feat, target=scan, outputs=("loglik",))["loglik"].double().mean()
    if getattr(env, "policy_has_decoder", False):
        return env.policy_decode_loglik(target=batch["lidar_occupancy"], features=feat, outputs=("loglik",))["loglik"].double().mean()
    raise RuntimeError(f"{what} needs an observation decoder: a LidarDistanceDecoder (load_lidar_decoder, or ldec_* arrays in the "
                       f"checkpoint) or a LidarOccupancyDecoder (dec_* arrays)")


def image_loglik(env, batch: Dict[str, torch.Tensor], mode: str = "sample", seed: int = 0) -> torch.Tensor:
    """`likes.image` of dreamer/models.py:99: the mean over [B, T] of the decoder's log-probability of the recorded observation on
    the posterior features (`policy_observe`, context = T), a float64 scalar on the device.  It uses whichever decoder is loaded:
    `policy_decode_lidar` against `batch["lidar"]`, else `policy_decode_loglik` against `batch["lidar_occupancy"]`."""
    feat = env.policy_observe(batch["lidar"], batch["action"], mode=mode, seed=seed, outputs=("feature",))["feature"]
    return _image_term(env, batch, feat, "image_loglik")


def model_loss(env, batch: Dict[str, torch.Tensor], kl_scale: float = 1.0, free_nats: float = 3.0, pcont_scale: float = 10.0,
               discount: float = 0.99, seed: int = 0) -> Dict[str, torch.Tensor]:
    """The world-model loss of dreamer/models.py:99-110 on a replay batch, forward only, every term from the device: one
    `policy_observe(mode="sample", seed)` - the posterior is sampled, as training does - gives the features, the KL and the
    reward head's prediction; the loaded decoder the image term (as `image_loglik`); `policy_value` the pcont head's probability (when a pcont
    head is loaded; its soft target is `discount * batch["discount"]`).  Returns float64 device scalars: `div` (the mean KL, before
    the free nats), `image_loglik`, `reward_loglik`, `pcont_loglik` (already times `pcont_scale`, as the reference's
    `likes.pcont`) and `model_loss = kl_scale * max(div, free_nats) - (image_loglik + reward_loglik + pcont_loglik)`.  The
    defaults are dream.py:73-76.  Needs a reward head and a decoder."""
    if not (getattr(env, "policy_has_lidar_decoder", False) or getattr(env, "policy_has_decoder", False)):
        raise RuntimeError("model_loss needs an observation decoder (a LidarDistanceDecoder or a LidarOccupancyDecoder)")
    if not env.policy_has_reward_head:
        raise RuntimeError("model_loss needs a checkpoint with a reward head (reward_* arrays)")
    obs = env.policy_observe(batch["lidar"], batch["action"], mode="sample", seed=seed, outputs=("feature", "kl", "reward"))
    feat, lead = obs["feature"], obs["feature"].shape[:-1]
    out = {"div": obs["kl"].double().mean()}
    out["image_loglik"] = _image_term(env, batch, feat, "model_loss")
    r = batch["reward"].to(feat.device, torch.float64).reshape(lead)
    out["reward_loglik"] = (-0.5 * (r - obs["reward"].double()) ** 2 - 0.5 * math.log(2.0 * math.pi)).mean()
    likes = out["image_loglik"] + out["reward_loglik"]
    if env.policy_has_pcont_head:
        p = env.policy_value(features=feat, outputs=("pcont",))["pcont"].double()
        t = discount * batch["discount"].to(feat.device, torch.float64).reshape(lead)
        out["pcont_loglik"] = pcont_scale * (t * torch.log(p) + (1.0 - t) * torch.log1p(-p)).mean()
        likes = likes + out["pcont_loglik"]
    out["model_loss"] = kl_scale * torch.clamp(out["div"], min=free_nats) - likes
    return out


def lidar_open_loop_summary(env, batch: Dict[str, torch.Tensor], context: int = 5) -> Dict[str, torch.Tensor]:
    """The `lidar` branch of dreamer/models.py:246-258 `_image_summaries` without the rasteriser: `policy_observe` with `context`,
    then `policy_decode_lidar` on the features.  Returns float32 [B, T, 1080] tensors in metres: `truth` (the recorded scan),
    `model` = (mean + 0.5) * 15 (the reconstruction for t < context, the open-loop prediction after it) and `error` = model - truth."""
    _lidar_decoder_needed(env, "lidar_open_loop_summary")
    feat = env.policy_observe(batch["lidar"], batch["action"], context=context)["feature"]
    model = (env.policy_decode_lidar(features=feat, outputs=("mean",))["mean"] + 0.5) * 15.0
    truth = batch["lidar"].to(model.device, torch.float32).reshape(model.shape)
    return dict(truth=truth, model=model, error=model - truth)


def behaviour_terms(env, batch: Dict[str, torch.Tensor], horizon: int = 15, lambda_: float = 0.95, seed: int = 0,
                    discount: float = 0.99) -> Dict[str, torch.Tensor]:
    """The forward half of the reference's behaviour learning on a replay batch (dreamer/models.py:113-133),
    two launches: `policy_observe(mode="sample")` gives the posterior features [B, T, 230]; when a pcont head is loaded each
    window's last step is dropped (`_imagine_ahead`, models.py:214-215); every remaining feature is a start of one
    `policy_returns(mode="sample")` under the actor.  Returns `returns`, `weight` [S, H - 1] and `value` [S, H] (S = B x T or
    B x (T - 1), window-major) and the two scalars of the reference, summed in float64: `actor_loss` = -mean(weight * returns),
    `value_loss` = -mean(weight * Normal(value[:, :-1], 1).log_prob(returns)).  Forward only: no gradient flows anywhere."""
    feat = env.policy_observe(batch["lidar"], batch["action"], mode="sample", seed=seed, outputs=("feature",))["feature"]
    if env.policy_has_pcont_head:
        feat = feat[..., :-1, :]
    state = torch.nn.functional.pad(feat.reshape(-1, feat.shape[-1]), (0, 2))
    out = env.policy_returns(horizon, "sample", seed=seed, lambda_=lambda_, discount=discount, state=state, outputs=("returns", "weight", "value"))
    w, ret, val = out["weight"].double(), out["returns"].double(), out["value"][:, :-1].double()
    out["actor_loss"] = -(w * ret).mean()
    out["value_loss"] = -(w * (-0.5 * (val - ret) ** 2 - 0.5 * math.log(2.0 * math.pi))).mean()
    return out


def value_learning_step(env, batch: Dict[str, torch.Tensor], horizon: int = 15, lambda_: float = 0.95, discount: float = 0.99,
                        seed: int = 0, **fit) -> Dict[str, torch.Tensor]:
    """The reference's value update on a replay batch (dreamer/models.py:113-137), three launches and no host
    copy: `behaviour_terms`' two - `policy_observe(mode="sample")`, each window's last step dropped when a pcont head is loaded,
    `policy_returns(mode="sample", outputs=("features", "returns", "weight"))` - then `critic_fit(features[:, :-1], returns,
    weight)` on the value head, whose optimizer must be open (`critic_fit_begin`).  `fit` goes to `critic_fit` (lr, clip, ...).
    Returns the fit's status (`loss`, `grad_norm`, `skipped`, `step`) and `value_loss` = `loss`: what `behaviour_terms` calls
    value_loss, on the weights before the update."""
    feat = env.policy_observe(batch["lidar"], batch["action"], mode="sample", seed=seed, outputs=("feature",))["feature"]
    if env.policy_has_pcont_head:
        feat = feat[..., :-1, :]
    state = torch.nn.functional.pad(feat.reshape(-1, feat.shape[-1]), (0, 2))
    out = env.policy_returns(horizon, "sample", seed=seed, lambda_=lambda_, discount=discount, state=state,
                             outputs=("features", "returns", "weight"))
    status = env.critic_fit(out["features"][:, :-1], out["returns"], out["weight"], head="value", **fit)
    status["value_loss"] = status["loss"]
    return status


def _dream_with_gradient(env, batch, horizon, lambda_, discount, seed, extra=()):
    """`value_learning_step`'s starts - `policy_observe(mode="sample")`, each window's last step dropped when a pcont head is loaded -
    and ONE `policy_returns_grad(mode="sample")` from them under the actor: the rows `actor_fit` takes, `returns` and `weight`, and
    `extra`.  `actor_loss` = -mean(weight * returns) of the same launch, summed in float64."""
    feat = env.policy_observe(batch["lidar"], batch["action"], mode="sample", seed=seed, outputs=("feature",))["feature"]
    if env.policy_has_pcont_head:
        feat = feat[..., :-1, :]
    state = torch.nn.functional.pad(feat.reshape(-1, feat.shape[-1]), (0, 2))
    out = env.policy_returns_grad(horizon, "sample", seed=seed, lambda_=lambda_, discount=discount, state=state,
                                  outputs=("grad_actions", "actor_features", "eps", "returns", "weight") + tuple(extra))
    out["actor_loss"] = -(out["weight"].double() * out["returns"].double()).mean()
    return out


def _actor_step(env, out, fit):
    return env.actor_fit(out["actor_features"].reshape(-1, out["actor_features"].shape[-1]), grad_actions=out["grad_actions"].reshape(-1, 2),
                         eps=out["eps"].reshape(-1, 2), **fit)


def actor_learning_step(env, batch: Dict[str, torch.Tensor], horizon: int = 15, lambda_: float = 0.95, discount: float = 0.99,
                        seed: int = 0, **fit) -> Dict[str, torch.Tensor]:
    """The reference's actor update on a replay batch (dreamer/models.py:113-128 under actor_opt), no host
    copy: `policy_observe(mode="sample")`, each window's last step dropped when a pcont head is loaded, as `value_learning_step`;
    one `policy_returns_grad` (scale -1 / (rows (H - 1)): the gradient of actor_loss = -mean(weight * returns) with respect to
    every imagined action, weight held constant and the actor's input detached, as the reference's tape has them); then
    `actor_fit(actor_features, grad_actions=..., eps=...)` on the actor's optimizer, which must be open (`actor_fit_begin`) - the
    actor's own backward pass, the global-norm clip and Adam.  `fit` goes to `actor_fit` (lr, clip, ...).  Returns the fit's status
    (`loss` = 0 in grad mode, `grad_norm`, `skipped`, `step`) and `actor_loss`, on the weights before the update."""
    out = _dream_with_gradient(env, batch, horizon, lambda_, discount, seed)
    status = _actor_step(env, out, fit)
    status["actor_loss"] = out["actor_loss"]
    return status


def behaviour_learning_step(env, batch: Dict[str, torch.Tensor], horizon: int = 15, lambda_: float = 0.95, discount: float = 0.99,
                            seed: int = 0, actor_fit=None, value_fit=None) -> Dict[str, torch.Tensor]:
    """The reference's pair of behaviour updates from ONE dream (dreamer/models.py:113-137): `actor_learning_step`'s rollout also
    returns the imagined features; the actor's step is taken from its rows and the value head's from `critic_fit(features[:, :-1],
    returns, weight)`.  Both gradients are of the weights before either update, as the reference's two tapes are: the rollout's
    outputs are on the device before `actor_fit` runs, and the value step reads nothing the actor's step writes.  Both optimizers
    must be open (`actor_fit_begin`, `critic_fit_begin("value")`); `actor_fit` and `value_fit` are dicts of their hyper-parameters.
    Returns `actor` and `value` (the two status dicts), `actor_loss` and `value_loss` (= value["loss"])."""
    out = _dream_with_gradient(env, batch, horizon, lambda_, discount, seed, extra=("features",))
    actor = _actor_step(env, out, dict(actor_fit or {}))
    value = env.critic_fit(out["features"][:, :-1], out["returns"], out["weight"], head="value", **dict(value_fit or {}))
    return dict(actor=actor, value=value, actor_loss=out["actor_loss"], value_loss=value["loss"])


def pcont_learning_step(env, batch: Dict[str, torch.Tensor], discount: float = 0.99, seed: int = 0, **fit) -> Dict[str, torch.Tensor]:
    """One step of the pcont head ALONE on a replay batch, the world model frozen: the head on the posterior features
    (`policy_observe(mode="sample")`) against the soft targets `discount * batch["discount"]` [B, T] (dreamer/models.py:101-105),
    through `critic_fit(head="pcont")`, whose optimizer must be open.  This is NOT the reference's rule: there the pcont likelihood
    is a term of the model loss and its gradient also reaches the RSSM and the encoder; here nothing but the head's eight arrays
    moves.  The reference multiplies the term by `pcont_scale` = 10 inside the loss: a caller who wants that passes `weight=10`
    (a tensor of the targets' shape, or a number).  Returns the fit's status."""
    weight = fit.pop("weight", None)
    feat = env.policy_observe(batch["lidar"], batch["action"], mode="sample", seed=seed, outputs=("feature",))["feature"]
    target = discount * batch["discount"].to(feat.device, torch.float32).reshape(feat.shape[:-1])
    if weight is not None and not torch.is_tensor(weight):
        weight = torch.full_like(target, float(weight))
    return env.critic_fit(feat, target, weight, head="pcont", **fit)


def reward_learning_step(env, batch: Dict[str, torch.Tensor], seed: int = 0, **fit) -> Dict[str, torch.Tensor]:
    """One step of the reward head ALONE on a replay batch, the world model frozen, `policy_observe`'s launch plus the
    fit's five and no host copy: the head on the posterior features (`policy_observe(mode="sample", seed)` on `batch["lidar"]` and
    `batch["action"]`) against `batch["reward"]` [B, T] under Normal(., 1) (dreamer/models.py:97-100), through `reward_fit`,
    whose optimizer must be open (`reward_fit_begin`).  `fit` goes to `reward_fit` (weight, lr, clip, ...).  This is NOT the
    reference's rule: there the reward likelihood is a term of the model loss under model_opt and its gradient also reaches the
    RSSM and the encoder; here nothing but the head's six arrays moves.  Returns the fit's status (`loss`, `grad_norm`, `skipped`,
    `step`) and `reward_loss` = `loss` = -`model_terms`' reward_loglik on these features, on the weights before the update."""
    feat = env.policy_observe(batch["lidar"], batch["action"], mode="sample", seed=seed, outputs=("feature",))["feature"]
    target = batch["reward"].to(feat.device, torch.float32).reshape(feat.shape[:-1])
    status = env.reward_fit(feat, target, **fit)
    status["reward_loss"] = status["loss"]
    return status


def imagined_vs_simulated(env, horizon: int = 15, mode: str = "mean", seed: int = 0, repeat=None) -> Dict[str, torch.Tensor]:
    """The world model's dream beside what the simulator would really do, without spending the run:
    `policy_imagine` from every car's latent under the actor's own actions, then `look_ahead` with one candidate per env - those
    actions - from the env's live state.  Returns `predicted` and `simulated` float32 [n_cars, horizon] (the reward head's
    reward and the true one of each step), `alive` bool [n_cars, horizon] (the steps after which the car's env was not yet
    finished: later pairs compare a dream with a frozen env) and `action` [n_cars, horizon, 2].  Both calls are pure - no state,
    no `action_in`, no latent changes - so this can run at every step of a live run.  `repeat`: the action repeat of the simulated
    steps (None: the env's default, as `step`).  Needs a checkpoint with a reward head."""
    if not env.policy_has_reward_head:
        raise RuntimeError("imagined_vs_simulated needs a checkpoint with a reward head (reward_* arrays)")
    E, A, h = env.num_envs, env.cars_per_env, int(horizon)
    dream = env.policy_imagine(h, mode, seed)
    actions = dream["action"].reshape(E, A, h, 2).permute(0, 2, 1, 3).reshape(E, 1, h, A, 2)
    real = env.look_ahead(actions, repeat=repeat, outputs=("reward", "flags"))
    simulated = real["reward"].reshape(E, h, A).permute(0, 2, 1).reshape(E * A, h)
    finished = ((real["flags"].reshape(E, h, A) & 1) != 0).any(dim=2)                       # [E, h]: some slot's done bit after step t
    alive = (~finished).unsqueeze(1).expand(E, A, h).reshape(E * A, h)
    return dict(predicted=dream["reward"], simulated=simulated, alive=alive, action=dream["action"])


def rank_correlation(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Spearman's rank correlation of the rows of a and b [E, K], float64 [E]: Pearson's correlation of the ranks, equal values
    sharing the mean of their ranks; NaN for a row that is constant in a or in b."""
    def ranks(x):
        x = x.to(torch.float64)
        less = (x.unsqueeze(2) > x.unsqueeze(1)).sum(dim=2)                  # entries below x[e, i]
        equal = (x.unsqueeze(2) == x.unsqueeze(1)).sum(dim=2)                # entries equal to it, itself counted
        return less.to(torch.float64) + (equal.to(torch.float64) - 1.0) / 2.0
    ra, rb = ranks(a), ranks(b)
    da, db = ra - ra.mean(dim=1, keepdim=True), rb - rb.mean(dim=1, keepdim=True)
    return (da * db).sum(dim=1) / torch.sqrt((da * da).sum(dim=1) * (db * db).sum(dim=1))


def dream_vs_truth(env, candidates: torch.Tensor, repeat=None) -> Dict[str, torch.Tensor]:
    """The same K candidate sequences scored in the dream and in the simulator, for an env with one car
    per env: `candidates` float32 [num_envs, K, H, 1, 2] (or [num_envs, K, H, 2]), raw in [-1, 1] - the env must have been
    built with `remap_actions=True`, so that `look_ahead` reads them as the dream does.  Returns per env `imagined` and `true`
    float32 [E, K] (`dream_ahead`'s return from the live latent, `look_ahead`'s from the live state), `rank_correlation`
    float64 [E] (Spearman), `argmax_agree` bool [E] (the first best of both is the same candidate), `regret` float32 [E] = the
    best true return minus the true return of the dream's choice (>= 0).  Both calls are pure, so this can run at any step of a
    live run.  `repeat`: as `look_ahead`.  Needs a checkpoint with a reward head."""
    from .planning import first_best, to_dream_actions
    if not env.policy_has_reward_head:
        raise RuntimeError("dream_vs_truth needs a checkpoint with a reward head (reward_* arrays)")
    if env.cars_per_env != 1:
        raise ValueError(f"dream_vs_truth compares per env: it needs one car per env, got {env.cars_per_env}")
    E = env.num_envs
    seq = candidates.to(env.device, torch.float32)
    seq = seq.reshape(E, seq.shape[1], seq.shape[2], 1, 2)
    imagined = env.dream_ahead(to_dream_actions(seq), outputs=("return",))["return"]
    true = env.look_ahead(seq, repeat=repeat, outputs=("return",))["return"][:, :, 0]
    pick, best = first_best(imagined), first_best(true)
    rows = torch.arange(E, device=true.device)
    return dict(imagined=imagined, true=true, rank_correlation=rank_correlation(imagined, true), argmax_agree=pick == best,
                regret=true[rows, best] - true[rows, pick])
