"""ctypes binding of libracecar_hip.so (include/racecar_hip.h).

There is no CPU fallback: if the library has not been built, importing the binding raises with
the build command.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``python -m racing_dreamer_amd.build``.
"""
from __future__ import annotations

import ctypes as C
import os

LIB_DIR = os.path.join(os.path.dirname(__file__), "lib")
LIB_PATH = os.path.join(LIB_DIR, "libracecar_hip.so")

RC_ABI_VERSION = 3          # include/racecar_hip.h
RC_N_BEAMS = 1080
RC_PATCH = 64
RC_MAX_CARS = 4

# rc_field
(F_LIDAR, F_POSE, F_VELOCITY, F_SPEED, F_ACTION, F_REWARD, F_DISCOUNT, F_PROGRESS_TOTAL, F_TIME, F_OCCUPANCY,
 F_PROGRESS, F_LAP, F_CHECKPOINT, F_DONE, F_TRUNCATED, F_WALL_COLLISION, F_OPPONENT_COLLISION, F_WRONG_WAY,
 F_FRESH, F_ACCELERATION, F_STEERING_ANGLE, F_ACTION_IN, F_COUNT) = range(23)

GATHER_FULL, GATHER_FULL_U16, GATHER_SUMMARY = range(3)
GATHER_MODES = {"full": GATHER_FULL, "full-u16": GATHER_FULL_U16, "summary": GATHER_SUMMARY}

# rc_debug_set knobs (experiments / validation only; all 0 in production)
DBG_RAY_THREADS, DBG_RAY_SPLIT, DBG_RAY_WG_PER_CU, DBG_BAND_LOG2, DBG_PATCH_VARIANT, DBG_SCAN_BOUNDED, DBG_SCAN_ORDER, DBG_EXACT_CHUNK = range(8)
DEBUG_KNOBS = {"ray_threads": DBG_RAY_THREADS, "ray_split": DBG_RAY_SPLIT, "ray_wg_per_cu": DBG_RAY_WG_PER_CU,
               "band_log2": DBG_BAND_LOG2, "patch_variant": DBG_PATCH_VARIANT, "scan_bounded": DBG_SCAN_BOUNDED,
               "scan_order": DBG_SCAN_ORDER, "exact_chunk": DBG_EXACT_CHUNK}
P2P_EXPORT_BYTES = 256

K_DYNAMICS, K_RAYCAST, K_PATCH, K_RESET, K_ACTIONS, K_FTG, K_POLICY, K_COUNT = range(8)
KERNEL_NAMES = {K_DYNAMICS: "rc_dynamics_kernel", K_RAYCAST: "rc_raycast_kernel", K_PATCH: "rc_patch_kernel",
                K_RESET: "rc_reset_kernel", K_ACTIONS: "rc_random_actions_kernel", K_FTG: "rc_ftg_kernel", K_POLICY: "rc_policy_kernel"}


class RcConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32), ("num_envs", C.c_int32), ("cars_per_env", C.c_int32),
        ("first_env", C.c_int64), ("obs_type", C.c_int32), ("task", C.c_int32), ("laps", C.c_int32),
        ("time_limit", C.c_float), ("terminate_on_collision", C.c_int32), ("collision_reward", C.c_float),
        ("remap_actions", C.c_int32), ("action_low", C.c_float * 2), ("action_high", C.c_float * 2),
        ("time_limit_steps", C.c_int32), ("auto_reset", C.c_int32), ("lidar_transform", C.c_int32),
        ("external_arena", C.c_void_p),
        ("external_arena_bytes", C.c_size_t), ("stream", C.c_void_p),
        ("car_task", C.c_int32 * 4), ("n_steps", C.c_int32),
        ("arena_total_cars", C.c_int32), ("arena_first_car", C.c_int32),
    ]


class RcEpisodeRow(C.Structure):
    """rc_episode_row (include/racecar_hip.h): one car's episode, 48 bytes."""
    _fields_ = [("env", C.c_int32), ("slot", C.c_int32), ("track", C.c_int32), ("episode", C.c_uint32), ("call", C.c_uint32),
                ("length", C.c_int32), ("ret", C.c_float), ("progress", C.c_float), ("time", C.c_float), ("laps", C.c_int32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


EPISODE_COUNTERS = ("written", "dropped", "skipped", "abandoned", "envs_at_quota", "calls")      # uint64 each, in this order
EP_WALL, EP_OPPONENT, EP_TRUNCATED, EP_WRONG_WAY, EP_OWN_DONE = 1, 2, 4, 8, 16                  # rc_episode_row.flags


class RcPolicyArray(C.Structure):
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32)]


# rc_policy_weights: the checkpoint's arrays in order (oracle-independent: the names are the fixture's keys)
POLICY_KEYS = ("gru_kernel", "gru_recurrent", "gru_bias", "img1_w", "img1_b", "img2_w", "img2_b", "img3_w", "img3_b",
               "obs1_w", "obs1_b", "obs2_w", "obs2_b", "h0_w", "h0_b", "h1_w", "h1_b", "h2_w", "h2_b", "h3_w", "h3_b",
               "hout_w", "hout_b", "hnorm_mean", "hnorm_var", "hnorm_gamma", "hnorm_beta")
POLICY_OPTIONAL = ("img2_w", "img2_b", "img3_w", "img3_b", "hnorm_mean", "hnorm_var", "hnorm_gamma", "hnorm_beta")
POLICY_STATE = 232          # stoch 30 | deter 200 | raw previous action 2


class RcPolicyWeights(C.Structure):
    _fields_ = [("struct_size", C.c_uint32)] + [(k, RcPolicyArray) for k in POLICY_KEYS]


class RcPolicySampling(C.Structure):
    """rc_policy_sampling (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("seed", C.c_uint64), ("expl_amount", C.c_float)]


POLICY_MODES = {"mean": 0, "deploy": 1, "explore": 2}          # RC_POLICY_MODE_*
POLICY_MODE_SAMPLES = 100
POLICY_EXPL_DEFAULT = {"mean": 0.0, "deploy": 0.0, "explore": 0.3}      # eval_noise off; dream.py:96-99 expl_amount


HEAD_KEYS = ("reward_h0_w", "reward_h0_b", "reward_h1_w", "reward_h1_b", "reward_hout_w", "reward_hout_b")
POLICY_FEATURE = 230        # stoch 30 | deter 200
IMAGINE_MODES = {"mean": 0, "sample": 1}                       # RC_POLICY_IMAGINE_*
IMAGINE_MAX_HORIZON = 64


class RcPolicyHeads(C.Structure):
    """rc_policy_heads (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32)] + [(k, RcPolicyArray) for k in HEAD_KEYS]


class RcPolicyImagineArgs(C.Structure):
    """rc_policy_imagine_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("horizon", C.c_int32), ("mode", C.c_int32), ("slot_mask", C.c_uint32), ("seed", C.c_uint64),
                ("actions_in", C.c_void_p), ("reward", C.c_void_p), ("actions", C.c_void_p), ("features", C.c_void_p), ("reward_start", C.c_void_p)]


# dream_ahead's output names -> (rc_policy_dream_ahead_args field, trailing shape after [starts, K] as a function of H)
DREAM_AHEAD_OUTPUTS = {"return": ("ret", lambda H: ()), "reward": ("reward", lambda H: (H,)),
                       "final_feature": ("final_feature", lambda H: (POLICY_FEATURE,))}


class RcPolicyDreamAheadArgs(C.Structure):
    """rc_policy_dream_ahead_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("horizon", C.c_int32), ("mode", C.c_int32), ("candidates", C.c_int32), ("slot_mask", C.c_uint32),
                ("discount", C.c_float), ("seed", C.c_uint64), ("starts", C.c_int64), ("row_offset", C.c_uint64), ("state_in", C.c_void_p),
                ("actions_in", C.c_void_p), ("ret", C.c_void_p), ("reward", C.c_void_p), ("final_feature", C.c_void_p)]


# dream_ahead_grad's output names -> (rc_policy_dream_grad_args field, trailing shape after [starts, K] as a function of H)
DREAM_GRAD_OUTPUTS = {"grad_actions": ("grad_actions", lambda H: (H, 2)), "grad_state": ("grad_state", lambda H: (POLICY_FEATURE,)),
                      "return": ("ret", lambda H: ()), "reward": ("reward", lambda H: (H,))}


class RcPolicyDreamGradArgs(C.Structure):
    """rc_policy_dream_grad_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("horizon", C.c_int32), ("mode", C.c_int32), ("candidates", C.c_int32), ("slot_mask", C.c_uint32),
                ("discount", C.c_float), ("seed", C.c_uint64), ("starts", C.c_int64), ("row_offset", C.c_uint64), ("chunk_rows", C.c_int64),
                ("state_in", C.c_void_p), ("actions_in", C.c_void_p), ("grad_actions", C.c_void_p), ("grad_state", C.c_void_p),
                ("ret", C.c_void_p), ("reward", C.c_void_p)]


_CRITIC_LAYERS = ("h0_w", "h0_b", "h1_w", "h1_b", "h2_w", "h2_b", "hout_w", "hout_b")
VALUE_KEYS = tuple("value_" + k for k in _CRITIC_LAYERS)
PCONT_KEYS = tuple("pcont_" + k for k in _CRITIC_LAYERS)
CRITIC_KEYS = VALUE_KEYS + PCONT_KEYS


class RcPolicyCritic(C.Structure):
    """rc_policy_critic (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32)] + [(k, RcPolicyArray) for k in CRITIC_KEYS]


# policy_returns' output names -> (rc_policy_returns_args field, trailing shape after [rows] as a function of H)
RETURNS_OUTPUTS = {"reward": ("reward", lambda H: (H,)), "value": ("value", lambda H: (H,)), "pcont": ("pcont", lambda H: (H,)),
                   "returns": ("returns", lambda H: (H - 1,)), "weight": ("weight", lambda H: (H - 1,)),
                   "actions": ("actions", lambda H: (H, 2)), "features": ("features", lambda H: (H, POLICY_FEATURE)),
                   "reward_start": ("reward_start", lambda H: ()), "value_start": ("value_start", lambda H: ()),
                   "pcont_start": ("pcont_start", lambda H: ())}


class RcPolicyReturnsArgs(C.Structure):
    """rc_policy_returns_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("horizon", C.c_int32), ("mode", C.c_int32), ("slot_mask", C.c_uint32), ("lambda_", C.c_float),
                ("discount", C.c_float), ("seed", C.c_uint64), ("starts", C.c_int64), ("row_offset", C.c_uint64), ("state_in", C.c_void_p),
                ("actions_in", C.c_void_p), ("reward", C.c_void_p), ("value", C.c_void_p), ("pcont", C.c_void_p), ("returns", C.c_void_p),
                ("weight", C.c_void_p), ("actions", C.c_void_p), ("features", C.c_void_p), ("reward_start", C.c_void_p),
                ("value_start", C.c_void_p), ("pcont_start", C.c_void_p)]


# policy_returns_grad's output names: policy_returns' and the four of the backward pass
RETURNS_GRAD_OUTPUTS = dict(RETURNS_OUTPUTS, grad_actions=("grad_actions", lambda H: (H, 2)),
                            actor_features=("actor_features", lambda H: (H, POLICY_FEATURE)), eps=("eps", lambda H: (H, 2)),
                            grad_state=("grad_state", lambda H: (POLICY_FEATURE,)))


class RcPolicyReturnsGradArgs(C.Structure):
    """rc_policy_returns_grad_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("horizon", C.c_int32), ("mode", C.c_int32), ("slot_mask", C.c_uint32), ("lambda_", C.c_float),
                ("discount", C.c_float), ("scale", C.c_float), ("reserved", C.c_uint32), ("seed", C.c_uint64), ("starts", C.c_int64),
                ("row_offset", C.c_uint64), ("chunk_rows", C.c_int64), ("state_in", C.c_void_p), ("actions_in", C.c_void_p),
                ("reward", C.c_void_p), ("value", C.c_void_p), ("pcont", C.c_void_p), ("returns", C.c_void_p), ("weight", C.c_void_p),
                ("actions", C.c_void_p), ("features", C.c_void_p), ("reward_start", C.c_void_p), ("value_start", C.c_void_p),
                ("pcont_start", C.c_void_p), ("grad_actions", C.c_void_p), ("actor_features", C.c_void_p), ("eps", C.c_void_p),
                ("grad_state", C.c_void_p)]


FIT_HEADS = {"value": 0, "pcont": 1}                            # RC_POLICY_FIT_*: the critic's (critic_fit)
FIT_REWARD = 2                                                  # RC_POLICY_FIT_REWARD: the reward head's own (reward_fit)
HEAD_SHAPES = ((230, 400), (400,), (400, 400), (400,), (400, 1), (1,))      # of HEAD_KEYS
CRITIC_SHAPES = ((230, 400), (400,), (400, 400), (400,), (400, 400), (400,), (400, 1), (1,))      # of VALUE_KEYS / PCONT_KEYS


class RcPolicyFitConfig(C.Structure):
    """rc_policy_fit_config (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("head", C.c_int32)]


class RcPolicyFitArgs(C.Structure):
    """rc_policy_fit_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("head", C.c_int32), ("rows", C.c_int64), ("features", C.c_void_p), ("target", C.c_void_p),
                ("weight", C.c_void_p), ("lr", C.c_float), ("clip", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("epsilon", C.c_float), ("status", C.c_void_p)]


FIT_ACTOR = 3                                                   # RC_POLICY_FIT_ACTOR: the actor's own (actor_fit)
ACTOR_KEYS = ("h0_w", "h0_b", "h1_w", "h1_b", "h2_w", "h2_b", "h3_w", "h3_b", "hout_w", "hout_b")      # rc_policy_actor, of POLICY_KEYS
ACTOR_SHAPES = ((230, 400), (400,), (400, 400), (400,), (400, 400), (400,), (400, 400), (400,), (400, 4), (4,))
ACTOR_OUTPUTS = ("action", "mean", "std")                       # policy_action's


class RcPolicyActorFitArgs(C.Structure):
    """rc_policy_actor_fit_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("rows", C.c_int64), ("features", C.c_void_p), ("eps", C.c_void_p), ("weight", C.c_void_p),
                ("target", C.c_void_p), ("grad", C.c_void_p), ("grad_features", C.c_void_p), ("lr", C.c_float), ("clip", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float), ("status", C.c_void_p)]


class RcPolicyActorForwardArgs(C.Structure):
    """rc_policy_actor_forward_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("rows", C.c_int64), ("features", C.c_void_p), ("eps", C.c_void_p), ("action", C.c_void_p),
                ("mean", C.c_void_p), ("std", C.c_void_p)]


class RcPolicyActor(C.Structure):
    """rc_policy_actor (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32)] + [(k, RcPolicyArray) for k in ACTOR_KEYS]


LOOK_AHEAD_MAX_HORIZON = 64
LA_DONE, LA_TRUNCATED, LA_WALL, LA_OPPONENT, LA_WRONG_WAY = 1, 2, 4, 8, 16      # rc_look_ahead's flags
# look_ahead's output names -> (rc_look_ahead_args field, torch dtype name, shape as a function of (E, K, H, A))
LOOK_AHEAD_OUTPUTS = {"reward": ("reward", "float32", lambda E, K, H, A: (E, K, H, A)),
                      "flags": ("flags", "uint8", lambda E, K, H, A: (E, K, H, A)),
                      "return": ("ret", "float32", lambda E, K, H, A: (E, K, A)),
                      "length": ("length", "int32", lambda E, K, H, A: (E, K)),
                      "final_state": ("final_state", "float32", lambda E, K, H, A: (E, K, A, 8)),
                      "pose": ("pose", "float32", lambda E, K, H, A: (E, K, H, A, 3))}


class RcLookAheadArgs(C.Structure):
    """rc_look_ahead_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("candidates", C.c_int32), ("horizon", C.c_int32), ("repeat", C.c_int32),
                ("actions", C.c_void_p), ("reward", C.c_void_p), ("flags", C.c_void_p), ("ret", C.c_void_p), ("length", C.c_void_p),
                ("final_state", C.c_void_p), ("pose", C.c_void_p)]


OBSERVE_MODES = {"mean": 0, "sample": 1}                       # RC_POLICY_OBSERVE_*
OBSERVE_MAX_LENGTH = 64
# policy_observe's output names -> (rc_policy_observe_args field, trailing shape after [rows, T]; None: [rows, 232])
OBSERVE_OUTPUTS = {"feature": ("features", (POLICY_FEATURE,)), "post_mean": ("post_mean", (30,)), "post_std": ("post_std", (30,)),
                   "prior_mean": ("prior_mean", (30,)), "prior_std": ("prior_std", (30,)), "kl": ("kl", ()), "reward": ("reward", ()),
                   "state": ("state_out", None)}


class RcPolicyObserveArgs(C.Structure):
    """rc_policy_observe_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("length", C.c_int32), ("context", C.c_int32), ("mode", C.c_int32), ("rows", C.c_int64),
                ("seed", C.c_uint64), ("row_offset", C.c_uint64), ("scan", C.c_void_p), ("actions", C.c_void_p), ("state_in", C.c_void_p),
                ("features", C.c_void_p), ("post_mean", C.c_void_p), ("post_std", C.c_void_p), ("prior_mean", C.c_void_p),
                ("prior_std", C.c_void_p), ("kl", C.c_void_p), ("reward", C.c_void_p), ("state_out", C.c_void_p)]


DECODER_KEYS = ("dec_h1_w", "dec_h1_b", "dec_h2_k", "dec_h2_b", "dec_h3_k", "dec_h3_b", "dec_h4_k", "dec_h4_b", "dec_h5_k", "dec_h5_b")
DECODE_IMAGE = 64           # the decoded lidar_occupancy image is 64 x 64


class RcPolicyDecoder(C.Structure):
    """rc_policy_decoder (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32)] + [(k, RcPolicyArray) for k in DECODER_KEYS]


class RcPolicyDecodeArgs(C.Structure):
    """rc_policy_decode_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("features", C.c_void_p), ("rows", C.c_int64), ("slot_mask", C.c_uint32),
                ("logits", C.c_void_p), ("image", C.c_void_p), ("mismatch", C.c_void_p)]


class RcPolicyDecodeLoglikArgs(C.Structure):
    """rc_policy_decode_loglik_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("features", C.c_void_p), ("rows", C.c_int64), ("slot_mask", C.c_uint32),
                ("target", C.c_void_p), ("loglik", C.c_void_p), ("logits", C.c_void_p), ("image", C.c_void_p)]


LIDAR_DECODER_KEYS = ("ldec_dense1_w", "ldec_dense1_b", "ldec_dense2_w", "ldec_dense2_b", "ldec_params_w", "ldec_params_b")
LIDAR_DECODER_SHAPES = ((230, 256), (256,), (256, 512), (512,), (512, 2160), (2160,))
# policy_decode_lidar's output names -> trailing shape after the leading dimensions
DECODE_LIDAR_OUTPUTS = {"mean": (RC_N_BEAMS,), "std": (RC_N_BEAMS,), "loglik": ()}


class RcPolicyLidarDecoder(C.Structure):
    """rc_policy_lidar_decoder (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32)] + [(k, RcPolicyArray) for k in LIDAR_DECODER_KEYS]


class RcPolicyDecodeLidarArgs(C.Structure):
    """rc_policy_decode_lidar_args (include/racecar_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("features", C.c_void_p), ("rows", C.c_int64), ("slot_mask", C.c_uint32),
                ("target", C.c_void_p), ("mean", C.c_void_p), ("std", C.c_void_p), ("loglik", C.c_void_p)]


def _fill_arrays(struct, weights, names, optional=()):
    import numpy as np
    keys = set(weights.files) if hasattr(weights, "files") else set(weights.keys())
    keep = []
    for k in names:
        if k not in keys:
            if k in optional:
                continue
            raise KeyError(f"policy weights lack {k!r}")
        a = np.ascontiguousarray(weights[k], np.float32)
        if a.ndim == 4:                                     # a transposed convolution's [kh, kw, out, in] as [kh kw out, in]
            a = a.reshape(-1, a.shape[3])
        if a.ndim not in (1, 2):
            raise ValueError(f"policy weights: {k} has {a.ndim} dimensions")
        keep.append(a)
        arr = getattr(struct, k)
        arr.data = a.ctypes.data
        arr.rows, arr.cols = (1, a.shape[0]) if a.ndim == 1 else a.shape
    return keep


def policy_heads(weights):
    """rc_policy_heads over a mapping that holds the reward_* arrays (or an .npz path), as policy_weights; None if it holds none."""
    import numpy as np
    if isinstance(weights, (str, os.PathLike)):
        weights = np.load(weights)
    keys = set(weights.files) if hasattr(weights, "files") else set(weights.keys())
    if not any(k.startswith("reward_") for k in keys):
        return None
    h = RcPolicyHeads()
    h.struct_size = C.sizeof(RcPolicyHeads)
    return h, _fill_arrays(h, weights, HEAD_KEYS)


def policy_critic(weights):
    """rc_policy_critic over a mapping that holds the value_* arrays and, optionally, the pcont_* arrays (or an .npz path), as
    policy_heads; None if it holds no value_* array."""
    import numpy as np
    if isinstance(weights, (str, os.PathLike)):
        weights = np.load(weights)
    keys = set(weights.files) if hasattr(weights, "files") else set(weights.keys())
    if not any(k.startswith("value_") for k in keys):
        return None
    h = RcPolicyCritic()
    h.struct_size = C.sizeof(RcPolicyCritic)
    pcont = PCONT_KEYS if any(k.startswith("pcont_") for k in keys) else ()
    return h, _fill_arrays(h, weights, VALUE_KEYS + pcont)


def policy_actor(weights):
    """rc_policy_actor over a mapping that holds the actor's ten arrays `h0_w` .. `hout_b` (or an .npz path), as policy_heads."""
    import numpy as np
    if isinstance(weights, (str, os.PathLike)):
        weights = np.load(weights)
    a = RcPolicyActor()
    a.struct_size = C.sizeof(RcPolicyActor)
    return a, _fill_arrays(a, weights, ACTOR_KEYS)


def policy_decoder(weights):
    """rc_policy_decoder over a mapping that holds the dec_* arrays of a LidarOccupancyDecoder (or an .npz path), as policy_heads;
    None if it holds none."""
    import numpy as np
    if isinstance(weights, (str, os.PathLike)):
        weights = np.load(weights)
    keys = set(weights.files) if hasattr(weights, "files") else set(weights.keys())
    if not any(k.startswith("dec_") for k in keys):
        return None
    d = RcPolicyDecoder()
    d.struct_size = C.sizeof(RcPolicyDecoder)
    return d, _fill_arrays(d, weights, DECODER_KEYS)


def policy_lidar_decoder(weights):
    """rc_policy_lidar_decoder over a mapping that holds the ldec_* arrays of a LidarDistanceDecoder (or an .npz path), as
    policy_heads; None if it holds none."""
    import numpy as np
    if isinstance(weights, (str, os.PathLike)):
        weights = np.load(weights)
    keys = set(weights.files) if hasattr(weights, "files") else set(weights.keys())
    if not any(k.startswith("ldec_") for k in keys):
        return None
    d = RcPolicyLidarDecoder()
    d.struct_size = C.sizeof(RcPolicyLidarDecoder)
    return d, _fill_arrays(d, weights, LIDAR_DECODER_KEYS)


def policy_weights(weights):
    """rc_policy_weights over a mapping of float32 arrays (or an .npz path).  Returns (struct, the arrays it points into -
    keep them alive until rc_policy_load has returned)."""
    import numpy as np
    if isinstance(weights, (str, os.PathLike)):
        weights = np.load(weights)
    w = RcPolicyWeights()
    w.struct_size = C.sizeof(RcPolicyWeights)
    return w, _fill_arrays(w, weights, POLICY_KEYS, POLICY_OPTIONAL)


# every symbol include/racecar_hip.h declares: name -> (restype, argtypes)
_P = C.POINTER
SYMBOLS = {
    "rc_default_config": (None, [_P(RcConfig)]),
    "rc_arena_bytes": (C.c_size_t, [_P(RcConfig)]),
    "rc_field_layout": (C.c_int, [_P(RcConfig), C.c_int32, _P(C.c_size_t), _P(C.c_size_t)]),
    "rc_create": (C.c_int, [_P(RcConfig), _P(C.c_void_p)]),
    "rc_destroy": (None, [C.c_void_p]),
    "rc_load_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int32]),
    "rc_set_source_frame": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double]),
    "rc_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64]),
    "rc_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "rc_step_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "rc_set_pose": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rc_set_vehicle_randomization": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "rc_set_vehicle_params": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rc_vehicle_params": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_size_t)]),
    "rc_set_lidar_noise": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_uint64]),
    "rc_set_track_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64]),
    "rc_set_next_track": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rc_track_ids": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_size_t)]),
    "rc_follow_the_gap": (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    "rc_follow_the_gap_reference": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p]),
    "rc_policy_load": (C.c_int, [C.c_void_p, _P(RcPolicyWeights)]),
    "rc_policy_unload": (C.c_int, [C.c_void_p]),
    "rc_policy_act": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rc_policy_state": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_size_t)]),
    "rc_policy_set_sampling": (C.c_int, [C.c_void_p, _P(RcPolicySampling)]),
    "rc_policy_get_sampling": (C.c_int, [C.c_void_p, _P(RcPolicySampling)]),
    "rc_policy_load_heads": (C.c_int, [C.c_void_p, _P(RcPolicyHeads)]),
    "rc_policy_imagine": (C.c_int, [C.c_void_p, _P(RcPolicyImagineArgs)]),
    "rc_policy_dream_ahead": (C.c_int, [C.c_void_p, _P(RcPolicyDreamAheadArgs)]),
    "rc_policy_dream_grad": (C.c_int, [C.c_void_p, _P(RcPolicyDreamGradArgs)]),
    "rc_policy_load_critic": (C.c_int, [C.c_void_p, _P(RcPolicyCritic)]),
    "rc_policy_returns": (C.c_int, [C.c_void_p, _P(RcPolicyReturnsArgs)]),
    "rc_policy_returns_grad": (C.c_int, [C.c_void_p, _P(RcPolicyReturnsGradArgs)]),
    "rc_policy_fit_begin": (C.c_int, [C.c_void_p, _P(RcPolicyFitConfig)]),
    "rc_policy_fit_step": (C.c_int, [C.c_void_p, _P(RcPolicyFitArgs)]),
    "rc_policy_fit_end": (C.c_int, [C.c_void_p, C.c_int32]),
    "rc_policy_read_critic": (C.c_int, [C.c_void_p, _P(RcPolicyCritic)]),
    "rc_policy_read_heads": (C.c_int, [C.c_void_p, _P(RcPolicyHeads)]),
    "rc_policy_actor_fit_step": (C.c_int, [C.c_void_p, _P(RcPolicyActorFitArgs)]),
    "rc_policy_actor_forward": (C.c_int, [C.c_void_p, _P(RcPolicyActorForwardArgs)]),
    "rc_policy_read_actor": (C.c_int, [C.c_void_p, _P(RcPolicyActor)]),
    "rc_policy_load_actor": (C.c_int, [C.c_void_p, _P(RcPolicyActor)]),
    "rc_policy_observe": (C.c_int, [C.c_void_p, _P(RcPolicyObserveArgs)]),
    "rc_policy_load_decoder": (C.c_int, [C.c_void_p, _P(RcPolicyDecoder)]),
    "rc_policy_decode": (C.c_int, [C.c_void_p, _P(RcPolicyDecodeArgs)]),
    "rc_policy_decode_loglik": (C.c_int, [C.c_void_p, _P(RcPolicyDecodeLoglikArgs)]),
    "rc_policy_load_lidar_decoder": (C.c_int, [C.c_void_p, _P(RcPolicyLidarDecoder)]),
    "rc_policy_decode_lidar": (C.c_int, [C.c_void_p, _P(RcPolicyDecodeLidarArgs)]),
    "rc_episode_log_enable": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32]),
    "rc_episode_log_disable": (C.c_int, [C.c_void_p]),
    "rc_episode_log": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_size_t), _P(C.c_void_p), _P(C.c_size_t)]),
    "rc_episode_log_clear": (C.c_int, [C.c_void_p]),
    "rc_episode_log_time": (C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_uint64)]),
    "rc_look_ahead": (C.c_int, [C.c_void_p, _P(RcLookAheadArgs)]),
    "rc_look_ahead_time": (C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_uint64)]),
    "rc_fill_random_actions": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32]),
    "rc_step_random": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32]),
    "rc_step_group": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "rc_step_random_group": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, C.c_int32]),
    "rc_get": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p), _P(C.c_size_t)]),
    "rc_copy_out": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "rc_trajectory_slab": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_size_t)]),
    "rc_gather_rows_bytes": (C.c_size_t, [C.c_void_p, C.c_uint32, C.c_int32]),
    "rc_gather_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_size_t]),
    "rc_sample_windows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64,
                                    C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rc_sample_batch_bytes": (C.c_size_t, [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, _P(C.c_size_t), _P(C.c_size_t)]),
    "rc_sample_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64,
                                  C.c_uint32, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_size_t]),
    "rc_sync": (C.c_int, [C.c_void_p]),
    "rc_stream": (C.c_void_p, [C.c_void_p]),
    "rc_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "rc_kernel_time": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_double), _P(C.c_uint64)]),
    "rc_reset_kernel_times": (C.c_int, [C.c_void_p]),
    "rc_set_raycast_variant": (C.c_int, [C.c_void_p, C.c_int32]),
    "rc_debug_set": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "rc_debug_scan_stamps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "rc_scan_overruns": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "rc_scan_kernel_name": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "rc_comm_count": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "rc_p2p_setup": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]),
    "rc_p2p_connect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rc_gather_trajectory_p2p": (C.c_int, [C.c_void_p]),
    "rc_gather_p2p_wait": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p), _P(C.c_size_t)]),
    "rc_p2p_slot": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p), _P(C.c_size_t)]),
    "rc_p2p_disconnect": (C.c_int, [C.c_void_p]),
    "rc_p2p_teardown": (C.c_int, [C.c_void_p]),
    "rc_device_alloc": (C.c_int, [C.c_void_p, C.c_size_t, _P(C.c_void_p)]),
    "rc_device_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rc_copy_from_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rc_compact_bytes": (C.c_size_t, [_P(RcConfig)]),
    "rc_set_compact_slab": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rc_compact_layout": (C.c_int, [C.c_void_p, _P(C.c_size_t), _P(C.c_size_t), _P(C.c_size_t)]),
    "rc_comm_library": (C.c_int, [C.c_char_p]),
    "rc_comm_unique_id": (C.c_int, [C.c_void_p, C.c_size_t]),
    "rc_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32]),
    "rc_gather_bytes": (C.c_size_t, [C.c_void_p, C.c_int32]),
    "rc_gather_trajectory": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "rc_gather_wait": (C.c_int, [C.c_void_p, C.c_int32]),
    "rc_spec_tables": (None, [C.c_void_p, C.c_void_p]),
    "rc_set_arena": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rc_selftest_reciprocal": (C.c_int, [C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rc_selftest_sqrt": (C.c_int, [C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rc_selftest_div6": (C.c_int, [C.c_int32, _P(C.c_uint64), _P(C.c_uint64)]),
    "rc_selftest_exact_estimate": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "rc_last_error": (C.c_char_p, []),
    "rc_abi_version": (C.c_int, []),
    "rc_build_id": (C.c_char_p, []),
}


class RacecarHipError(RuntimeError):
    pass


_lib = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """dlopen the HIP library and bind every declared symbol.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RacecarHipError(
            f"{path} not found: the HIP extension is not built. Run `python -m racing_dreamer_amd.build` "
            "(needs hipcc; cross-compiles for gfx950 without a GPU). There is no CPU fallback.")
    if path == LIB_PATH and not os.environ.get("RC_ALLOW_STALE_LIBRARY"):
        # A library that does not belong to the sources beside it would let every test pass on yesterday's kernels: refuse it.
        # (The identity is a hash of flags and file CONTENTS compiled into the library, racing_dreamer_amd/build.py; the A/B
        # scripts under tools/, which put variant builds in the library's place, set RC_ALLOW_STALE_LIBRARY=1.)
        from . import build as _build
        if os.path.isdir(_build.CSRC) and _build.needs_build(path):
            raise RacecarHipError(
                f"{path} was built from other sources than the ones in {_build.CSRC} (its build id {_build.library_build_id(path)}, "
                f"theirs {_build.source_hash()}): run `python -m racing_dreamer_amd.build` (or __graft_entry__.build()) first.")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)     # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.rc_abi_version() != RC_ABI_VERSION:
        raise RacecarHipError(f"ABI version mismatch: {path} reports {lib.rc_abi_version()}, this binding expects "
                              f"{RC_ABI_VERSION} - rebuild with `python -m racing_dreamer_amd.build --force`")
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load_library().rc_last_error()
        raise RacecarHipError(f"libracecar_hip error {rc}: {msg.decode() if msg else '?'}")
