"""PolicyActorFitSpec: the binary32 specification of the actor's fit (rc_policy_actor_fit_step and
rc_policy_actor_forward): the fit engine of tests/policy_fit_spec.c at four hidden layers and four outputs under the tanh-normal rule
of tests/policy_actor_fit_spec.c.  A PolicyActorFitSpec owns the actor's ten arrays (copies, updated in place by `step`), its Adam
moments and its step count."""
import ctypes as C

import numpy as np

from policy_fit_spec import FitSpec, _as, _ptr, f32

KEYS = ("h0_w", "h0_b", "h1_w", "h1_b", "h2_w", "h2_b", "h3_w", "h3_b", "hout_w", "hout_b")      # the checkpoint's names
SHAPES = ((230, 400), (400,), (400, 400), (400,), (400, 400), (400,), (400, 400), (400,), (400, 4), (4,))
N_GRAD = 575204
DEFAULTS = dict(lr=8e-5, clip=1.0, beta1=0.9, beta2=0.999, epsilon=1e-7)      # the reference's actor_lr, grad_clip; TF's Adam


class PolicyActorFitSpec(FitSpec):
    """weights: a mapping with the actor's `h0_w` .. `hout_b` (copied)."""
    LAYERS, SHAPES, N_GRAD, DEFAULTS, STEP, DOWN_TO_THE_FEATURES = KEYS, SHAPES, N_GRAD, DEFAULTS, "pafs_step", True

    def forward(self, features, eps=None):
        """action, mean, std [N, 2] of features [N, 230] under eps [N, 2] or None (the mode action)."""
        feat = _as(features, -1, 230)
        n = len(feat)
        e = _as(eps, n, 2)
        out = {k: np.empty((n, 2), f32) for k in ("action", "mean", "std")}
        self.lib.pafs_forward(C.byref(self.net), n, feat.ctypes.data, _ptr(e), out["action"].ctypes.data, out["mean"].ctypes.data, out["std"].ctypes.data)
        return out

    def step(self, features, target=None, grad_actions=None, eps=None, weight=None, **hyper):
        """One update on features [N, 230] from exactly one of target [N, 2] and grad_actions [N, 2], under eps [N, 2] or None and
        weight [N] or None.  Returns a dict: loss, grad_norm (float32), skipped, step (int), grad (the ten arrays of the gradient
        before the clip, by name), grad_flat, grad_features [N, 230], out [N, 4] (the output layer before the step)."""
        assert (target is None) != (grad_actions is None)
        return self._step(features, hyper, target=target, grad=grad_actions, eps=eps, weight=weight)
