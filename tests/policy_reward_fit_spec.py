"""PolicyRewardFitSpec: the binary32 specification of the reward head's fit (rc_policy_fit_step with
RC_POLICY_FIT_REWARD): the fit engine of tests/policy_fit_spec.c at two hidden layers, under the value head's Normal(o, 1).  A
PolicyRewardFitSpec owns the head's six arrays (copies, updated in place by `step`), its Adam moments and its step count."""
from policy_fit_spec import HeadFitSpec

LAYERS = ("h0_w", "h0_b", "h1_w", "h1_b", "hout_w", "hout_b")
KEYS = tuple("reward_" + k for k in LAYERS)
SHAPES = ((230, 400), (400,), (400, 400), (400,), (400, 1), (1,))
N_GRAD = 253201
DEFAULTS = dict(lr=6e-4, clip=1.0, beta1=0.9, beta2=0.999, epsilon=1e-7)      # the reference's model_lr, grad_clip; TF's Adam


class PolicyRewardFitSpec(HeadFitSpec):
    """heads: a mapping with the `reward_*` arrays (copied)."""
    LAYERS, SHAPES, N_GRAD, DEFAULTS, PREFIX = LAYERS, SHAPES, N_GRAD, DEFAULTS, "reward_"
