"""The float64 / float32 yardstick of the fit specs' tests (test_policy_fit_spec.py, test_policy_reward_fit_spec.py,
test_policy_actor_fit_spec.py): the optimizer half of the reference's update (dreamer/tools.py:421-455) in NumPy, over a dict of arrays
and any head's gradient function, and the two helpers the three files share."""
import numpy as np


def _elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def _err(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


class Restatement:
    """The update in dtype dt: clip_by_global_norm, then Adam - TF's ResourceApplyAdam, or (torch=True) torch.optim.Adam's
    placement of epsilon.  weights: {name: array} in the order of the gradient; gradient(W, *rows) -> (loss, {name: array}) or
    (loss, {name: array}, grad_features)."""

    def __init__(self, weights, defaults, gradient, dt, torch=False):
        self.W = {k: np.asarray(a).astype(dt) for k, a in weights.items()}
        self.defaults, self.gradient, self.dt, self.torch, self.t = defaults, gradient, dt, torch, 0
        self.m = {k: np.zeros_like(a) for k, a in self.W.items()}
        self.v = {k: np.zeros_like(a) for k, a in self.W.items()}

    def step(self, *rows, **hyper):
        dt = self.dt
        hp = {k: dt(np.float32(v)) for k, v in {**self.defaults, **hyper}.items()}
        loss, g, *gfeat = self.gradient(self.W, *rows)
        norm = np.sqrt(sum((a.astype(dt) ** 2).sum(dtype=dt) for a in g.values()))
        out = dict(loss=loss, grad_norm=norm, grad=g, skipped=int(not np.isfinite(norm)), **({"grad_features": gfeat[0]} if gfeat else {}))
        if out["skipped"]:
            return out
        scale = hp["clip"] / max(norm, hp["clip"]) if hp["clip"] > 0 else dt(1)
        self.t += 1
        c1, c2 = 1 - hp["beta1"] ** self.t, 1 - hp["beta2"] ** self.t
        for k in self.W:
            gk = g[k] * scale
            self.m[k] = hp["beta1"] * self.m[k] + (1 - hp["beta1"]) * gk
            self.v[k] = hp["beta2"] * self.v[k] + (1 - hp["beta2"]) * gk * gk
            if self.torch:
                self.W[k] = self.W[k] - hp["lr"] / c1 * self.m[k] / (np.sqrt(self.v[k]) / np.sqrt(c2) + hp["epsilon"])
            else:
                self.W[k] = self.W[k] - hp["lr"] * np.sqrt(c2) / c1 * self.m[k] / (np.sqrt(self.v[k]) + hp["epsilon"])
        return out
