"""BatchedRaceEnv: the Python host of the MI355X batched racing environment.

Thin layer over the C-ABI (include/racecar_hip.h): torch allocates the output arena and the
stream, the HIP library does all the work, and every output is a zero-copy torch view of the
arena.  The surface mirrors what the reference's callers consume from racecar_gym
(SURVEY.md §8b): ``reset(mode=...)`` / ``step(actions)`` returning ``lidar``, ``pose``,
``velocity``, ``speed``, ``lidar_occupancy``, ``reward``, ``done`` and the info keys
``progress``, ``lap``, ``time``, ``wrong_way``, ``wall_collision``
(dreamer/wrappers.py:62-77,210-226; baselines/.../sb_experiment.py:82-88), batched over
``num_envs x cars_per_env``.

The returned tensors are views of buffers that the next step()/reset() overwrites; clone what
must be kept.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Union

import numpy as np
import torch
import torch.utils.dlpack

from . import _lib as L
from . import spec
from .track_assets import Track, load_track

_FIELD_VIEWS = {
    # name: (field id, torch dtype, trailing shape)
    "lidar": (L.F_LIDAR, torch.float32, (L.RC_N_BEAMS,)),
    "pose": (L.F_POSE, torch.float32, (6,)),
    "velocity": (L.F_VELOCITY, torch.float32, (6,)),
    "speed": (L.F_SPEED, torch.float32, ()),
    "action": (L.F_ACTION, torch.float32, (2,)),
    "reward": (L.F_REWARD, torch.float32, ()),
    "discount": (L.F_DISCOUNT, torch.float32, ()),
    "progress_total": (L.F_PROGRESS_TOTAL, torch.float32, ()),
    "time": (L.F_TIME, torch.float32, ()),
    "lidar_occupancy": (L.F_OCCUPANCY, torch.uint8, (L.RC_PATCH, L.RC_PATCH, 1)),
    "progress": (L.F_PROGRESS, torch.float32, ()),
    "lap": (L.F_LAP, torch.int32, ()),
    "checkpoint": (L.F_CHECKPOINT, torch.int32, ()),
    "done": (L.F_DONE, torch.uint8, ()),
    "truncated": (L.F_TRUNCATED, torch.uint8, ()),
    "wall_collision": (L.F_WALL_COLLISION, torch.uint8, ()),
    "opponent_collision": (L.F_OPPONENT_COLLISION, torch.uint8, ()),
    "wrong_way": (L.F_WRONG_WAY, torch.uint8, ()),
    "fresh": (L.F_FRESH, torch.uint8, ()),
    "acceleration": (L.F_ACCELERATION, torch.float32, ()),
    "steering_angle": (L.F_STEERING_ANGLE, torch.float32, ()),
    "action_in": (L.F_ACTION_IN, torch.float32, (2,)),
}

# lidar_occupancy_reference: the 64 x 64 patch computed EXACTLY as the reference's OccupancyMapObs.step does (dreamer/wrappers.py:
# 396-406; spline rotation + antialiased bicubic resize restated to the binary64 operation) instead of by the one-tap sampler
OBS_TYPES = {"lidar": 0, "lidar_occupancy": 1, "lidar_occupancy_reference": 2}
# scaling fused into the scan's store: metres | dreamer (x/15 - 0.5, tools.py:274) | unit (x/15, single_agent.py:92-99)
LIDAR_TRANSFORMS = {"metres": 0, "dreamer": 1, "unit": 2}
TRACK_ORDERS = {"sequential": 0, "random": 1, "manual": 2}         # include/racecar_hip.h, RC_TRACK_ORDER_*
TASKS = {"maximize_progress": spec.TASK_MAX_PROGRESS, "max_progress": spec.TASK_MAX_PROGRESS,
         "max_speed": spec.TASK_MAX_SPEED, "n_step_progress": spec.TASK_N_STEP_PROGRESS}


class _DLDevice(C.Structure):
    _fields_ = [("device_type", C.c_int32), ("device_id", C.c_int32)]


class _DLDataType(C.Structure):
    _fields_ = [("code", C.c_uint8), ("bits", C.c_uint8), ("lanes", C.c_uint16)]


class _DLTensor(C.Structure):
    _fields_ = [("data", C.c_void_p), ("device", _DLDevice), ("ndim", C.c_int32), ("dtype", _DLDataType),
                ("shape", C.POINTER(C.c_int64)), ("strides", C.POINTER(C.c_int64)), ("byte_offset", C.c_uint64)]


class _DLManagedTensor(C.Structure):
    _fields_ = [("dl_tensor", _DLTensor), ("manager_ctx", C.c_void_p), ("deleter", C.c_void_p)]


class _BorrowedDeviceArray:
    """A float32 array in device memory that the library owns, handed to torch through DLPack without a copy (no deleter: the
    memory stays the library's).  Valid while the handle lives."""

    def __init__(self, ptr: int, shape, device: torch.device, kind: int = 10, code: int = 2):   # 10 = kDLROCM (1 = kDLCPU); code 2 = float, 0 = int
        self._shape = (C.c_int64 * len(shape))(*shape)
        self._managed = _DLManagedTensor()
        t = self._managed.dl_tensor
        t.data, t.device, t.ndim = ptr, _DLDevice(kind, device.index or 0), len(shape)
        t.dtype, t.shape, t.strides, t.byte_offset = _DLDataType(code, 32, 1), self._shape, None, 0     # 32-bit, row-major
        self._kind, self._index = kind, device.index or 0

    def __dlpack_device__(self):
        return (self._kind, self._index)

    def __dlpack__(self, stream=None, **_kw):
        new = C.pythonapi.PyCapsule_New
        new.restype, new.argtypes = C.py_object, [C.c_void_p, C.c_char_p, C.c_void_p]
        return new(C.addressof(self._managed), b"dltensor", None)


def _ensure_lab() -> None:
    """Build the lab library (scan variants 0-6, the stamps build) if the one on disk does not belong to the sources - the
    request that `libracecar_lab.so` exists for.  libracecar_hip.so loads it itself, on the first launch of a lab kernel."""
    from . import build
    if build.lab_needs_build():
        build.build_lab(verbose=False)


def _imagine_setup(env, horizon, mode, seed, actions, slots, features, start_reward, out):
    """policy_imagine's arguments and tensors (shared by BatchedRaceEnv and MixedTrackEnv): (scalar args, the tensors by
    rc_policy_imagine_args field - one row per car -, the dict to return)."""
    if mode not in L.IMAGINE_MODES:
        raise ValueError(f"imagination mode must be one of {sorted(L.IMAGINE_MODES)}, got {mode!r}")
    h, n = int(horizon), env.n_cars
    if not 1 <= h <= L.IMAGINE_MAX_HORIZON:
        raise ValueError(f"horizon must be in [1, {L.IMAGINE_MAX_HORIZON}], got {horizon}")
    if start_reward and not env.policy_has_reward_head:
        raise L.RacecarHipError("start_reward needs a checkpoint with a reward head (reward_* arrays)")
    shapes = {"action": (n, h, 2)}
    if env.policy_has_reward_head:
        shapes["reward"] = (n, h)
    if features:
        shapes["feature"] = (n, h, L.POLICY_FEATURE)
    if start_reward:
        shapes["reward_start"] = (n,)
    result = {}
    for name, shape in shapes.items():
        t = None if out is None else out.get(name)
        if t is None:
            t = (torch.empty if slots is None else torch.zeros)(shape, dtype=torch.float32, device=env.device)
        elif t.shape != shape or t.dtype != torch.float32 or t.device != torch.device(env.device) or not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be a contiguous float32 tensor of shape {shape} on {env.device}")
        result[name] = t
    if actions is not None:
        actions = actions.to(env.device, torch.float32).reshape(n, h, 2).contiguous()
    args = dict(horizon=h, mode=L.IMAGINE_MODES[mode], seed=int(seed) & (2 ** 64 - 1),
                mask=(1 << env.cars_per_env) - 1 if slots is None else sum({1 << int(a) for a in slots}))
    tensors = dict(actions_in=actions, reward=result.get("reward"), actions=result["action"], features=result.get("feature"),
                   reward_start=result.get("reward_start"))
    return args, tensors, result


def _dream_setup(env, actions, mode, seed, state, row_offset, slots, discount, outputs, out, table=None, who="dream_ahead"):
    """dream_ahead's arguments and tensors (shared by BatchedRaceEnv and MixedTrackEnv): (scalar args, the tensors by
    rc_policy_dream_ahead_args field - one row per start -, the dict to return).  What only the library can tell (no policy, no
    head, slots with a state, the size of starts x K) is left to it, which names it.  `table`, `who`: dream_ahead_grad's outputs
    (L.DREAM_GRAD_OUTPUTS) and name - the two calls share everything else."""
    table = L.DREAM_AHEAD_OUTPUTS if table is None else table
    if mode not in L.IMAGINE_MODES:
        raise ValueError(f"{who} mode must be one of {sorted(L.IMAGINE_MODES)}, got {mode!r}")
    S = env.n_cars
    if state is not None:
        if state.dim() < 1 or state.shape[-1] != L.POLICY_FEATURE + 2 or state.numel() == 0:
            raise ValueError(f"state must be [starts >= 1, {L.POLICY_FEATURE + 2}] = stoch | deter | (2 unused), got {tuple(state.shape)}")
        S = state.numel() // (L.POLICY_FEATURE + 2)
    a = actions.to(env.device, torch.float32)
    if a.dim() != 4 or a.shape[0] != S or a.shape[3] != 2:
        raise ValueError(f"actions must be [starts={S}, candidates, horizon, 2], got shape {tuple(actions.shape)}")
    a = a.contiguous()
    K, H = int(a.shape[1]), int(a.shape[2])
    if K < 1:
        raise ValueError(f"{who} needs at least one candidate")
    if not 1 <= H <= L.IMAGINE_MAX_HORIZON:
        raise ValueError(f"horizon must be in [1, {L.IMAGINE_MAX_HORIZON}], got {H}")
    discount = float(discount)
    if not 0.0 <= discount <= 1.0:
        raise ValueError(f"discount must be in [0, 1], got {discount}")
    names = tuple(outputs)
    unknown = [n for n in names if n not in table]
    if unknown:
        raise ValueError(f"{who} outputs must be among {sorted(table)}, got {unknown}")
    tensors, result = {"actions_in": a}, {}
    tensors.update({field: None for field, _ in table.values()})
    if state is not None:
        tensors["state_in"] = state.to(env.device, torch.float32).reshape(S, L.POLICY_FEATURE + 2).contiguous()
        mask = 0 if slots is None else sum({1 << int(b) for b in slots})        # (slots with a state: the library refuses and says why)
    else:
        mask = (1 << env.cars_per_env) - 1 if slots is None else sum({1 << int(b) for b in slots})
    for name in names:
        field, tail = table[name]
        shape = (S, K) + tail(H)
        t = None if out is None else out.get(name)
        if t is None:
            t = (torch.empty if slots is None else torch.zeros)(shape, dtype=torch.float32, device=env.device)
        elif t.shape != shape or t.dtype != torch.float32 or t.device != torch.device(env.device) or not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be a contiguous float32 tensor of shape {shape} on {env.device}")
        tensors[field] = result[name] = t
    args = dict(horizon=H, mode=L.IMAGINE_MODES[mode], candidates=K, mask=mask, discount=discount, seed=int(seed) & (2 ** 64 - 1),
                starts=S, row_offset=int(row_offset) & (2 ** 64 - 1), live=state is None)
    return args, tensors, result


def _chunk_rows(chunk_rows) -> int:
    n = int(chunk_rows)
    if n < 0:
        raise ValueError(f"chunk_rows must be >= 0, got {chunk_rows}")
    return n


def _returns_setup(env, horizon, mode, seed, lambda_, discount, actions, state, row_offset, slots, outputs, out, table=None, what="policy_returns"):
    """policy_returns' arguments and tensors (shared by BatchedRaceEnv and MixedTrackEnv, and by policy_returns_grad with its own
    `table` of outputs): (scalar args, the tensors by rc_policy_returns_args field - one row per start -, the dict to return).  What
    only the library can tell (no policy, a missing head, slots with a state, a horizon too short for the outputs) is left to it,
    which names it."""
    table = L.RETURNS_OUTPUTS if table is None else table
    if mode not in L.IMAGINE_MODES:
        raise ValueError(f"{what} mode must be one of {sorted(L.IMAGINE_MODES)}, got {mode!r}")
    H, S = int(horizon), env.n_cars
    if not 0 <= H <= L.IMAGINE_MAX_HORIZON:
        raise ValueError(f"horizon must be in [0, {L.IMAGINE_MAX_HORIZON}], got {horizon}")
    if state is not None:
        if state.dim() < 1 or state.shape[-1] != L.POLICY_FEATURE + 2 or state.numel() == 0:
            raise ValueError(f"state must be [starts >= 1, {L.POLICY_FEATURE + 2}] = stoch | deter | (2 unused), got {tuple(state.shape)}")
        S = state.numel() // (L.POLICY_FEATURE + 2)
    lambda_, discount = float(lambda_), float(discount)
    if not 0.0 <= lambda_ <= 1.0 or not 0.0 <= discount <= 1.0:
        raise ValueError(f"lambda_ and discount must be in [0, 1], got {lambda_} and {discount}")
    names = tuple(outputs)
    unknown = [n for n in names if n not in table]
    if unknown:
        raise ValueError(f"{what} outputs must be among {sorted(table)}, got {unknown}")
    tensors, result = {"state_in": None, "actions_in": None}, {}
    tensors.update({field: None for field, _ in table.values()})
    if actions is not None and H > 0:
        tensors["actions_in"] = actions.to(env.device, torch.float32).reshape(S, H, 2).contiguous()
    if state is not None:
        tensors["state_in"] = state.to(env.device, torch.float32).reshape(S, L.POLICY_FEATURE + 2).contiguous()
        mask = 0 if slots is None else sum({1 << int(b) for b in slots})        # (slots with a state: the library refuses and says why)
    else:
        mask = (1 << env.cars_per_env) - 1 if slots is None else sum({1 << int(b) for b in slots})
    for name in names:
        field, tail = table[name]
        shape = (S,) + tuple(max(d, 0) for d in tail(H))
        t = None if out is None else out.get(name)
        if t is None:
            t = (torch.empty if slots is None else torch.zeros)(shape, dtype=torch.float32, device=env.device)
        elif t.shape != shape or t.dtype != torch.float32 or t.device != torch.device(env.device) or not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be a contiguous float32 tensor of shape {shape} on {env.device}")
        tensors[field] = result[name] = t
    args = dict(horizon=H, mode=L.IMAGINE_MODES[mode], mask=mask, lambda_=lambda_, discount=discount, seed=int(seed) & (2 ** 64 - 1),
                starts=S, row_offset=int(row_offset) & (2 ** 64 - 1), live=state is None)
    return args, tensors, result


def _returns_grad_setup(env, horizon, mode, seed, lambda_, discount, scale, actions, state, row_offset, slots, outputs, out, chunk_rows):
    """policy_returns_grad's arguments and tensors, as `_returns_setup`'s, with the scale (None: float32(-1 / (rows (H - 1))), rows
    = the starts of the call: `state`'s rows, or the cars of `slots`) and the chunk."""
    args, tensors, result = _returns_setup(env, horizon, mode, seed, lambda_, discount, actions, state, row_offset, slots, outputs, out,
                                           L.RETURNS_GRAD_OUTPUTS, "policy_returns_grad")
    if args["horizon"] < 2:
        raise ValueError(f"horizon must be in [2, {L.IMAGINE_MAX_HORIZON}], got {horizon}")
    rows = args["starts"] if state is not None else env.num_envs * bin(args["mask"]).count("1")
    args["scale"] = float(np.float32(-1.0 / (max(rows, 1) * (args["horizon"] - 1)))) if scale is None else float(np.float32(scale))
    args["chunk_rows"] = _chunk_rows(chunk_rows)
    return args, tensors, result


def _value_setup(env, features, slots, outputs):
    """policy_value as an H = 0 policy_returns: (the state [rows, 232] or None, the leading shape, the *_start output names)."""
    names = tuple(outputs)
    unknown = [n for n in names if n not in ("reward", "value", "pcont")]
    if unknown:
        raise ValueError(f"policy_value outputs must be among ['pcont', 'reward', 'value'], got {unknown}")
    if features is None:
        return None, (env.n_cars,), tuple(n + "_start" for n in names)
    if features.shape[-1] != L.POLICY_FEATURE or features.numel() == 0:
        raise ValueError(f"features must be [..., {L.POLICY_FEATURE}] with at least one row, got {tuple(features.shape)}")
    lead = tuple(features.shape[:-1])
    flat = features.to(env.device, torch.float32).reshape(-1, L.POLICY_FEATURE)
    return torch.nn.functional.pad(flat, (0, 2)), lead, tuple(n + "_start" for n in names)


def _fit_setup(env, features, target, weight, head):
    """critic_fit's and reward_fit's (head None) tensors (shared by BatchedRaceEnv and MixedTrackEnv): contiguous float32 [N, 230], [N], [N] or None on the
    env's device, and the status block."""
    if head is not None and head not in L.FIT_HEADS:
        raise ValueError(f"head must be one of {sorted(L.FIT_HEADS)}, got {head!r}")
    if features.shape[-1] != L.POLICY_FEATURE or features.numel() == 0:
        raise ValueError(f"features must be [..., {L.POLICY_FEATURE}] with at least one row, got {tuple(features.shape)}")
    feat = features.to(env.device, torch.float32).reshape(-1, L.POLICY_FEATURE).contiguous()
    n = feat.shape[0]
    tgt = target.to(env.device, torch.float32).reshape(-1).contiguous()
    wgt = None if weight is None else weight.to(env.device, torch.float32).reshape(-1).contiguous()
    if tgt.numel() != n or (wgt is not None and wgt.numel() != n):
        raise ValueError(f"features have {n} rows, target {tgt.numel()}" + ("" if wgt is None else f", weight {wgt.numel()}"))
    return feat, tgt, wgt, torch.empty(4, dtype=torch.float32, device=env.device)


def _fit_status(status):
    return {"loss": status[0], "grad_norm": status[1], "skipped": status[2], "step": status[3]}


def _actor_rows(env, features, pairs, rows):
    """actor_fit's and policy_action's tensors (shared by BatchedRaceEnv and MixedTrackEnv): `features` as contiguous float32
    [N, 230] on the env's device with its leading shape, each of `pairs` (name -> tensor or None) as [N, 2], each of `rows` as [N]."""
    if features.shape[-1] != L.POLICY_FEATURE or features.numel() == 0:
        raise ValueError(f"features must be [..., {L.POLICY_FEATURE}] with at least one row, got {tuple(features.shape)}")
    lead = tuple(features.shape[:-1])
    feat = features.to(env.device, torch.float32).reshape(-1, L.POLICY_FEATURE).contiguous()
    n = feat.shape[0]
    out = {}
    for name, t in list(pairs.items()) + list(rows.items()):
        width = 2 if name in pairs else 1
        if t is None:
            out[name] = None
            continue
        t = torch.as_tensor(t).to(env.device, torch.float32).reshape(-1).contiguous()
        if t.numel() != n * width:
            raise ValueError(f"features have {n} rows, {name} {t.numel()} elements, not {n * width}")
        out[name] = t
    return feat, lead, out


def _actor_fit_setup(env, features, target, grad_actions, eps, weight, grad_features):
    """actor_fit's tensors: (features [N, 230], the [N, 2] / [N] inputs by name, grad_features [N, 230] or None, its shape, status)."""
    if (target is None) == (grad_actions is None):
        raise ValueError("actor_fit takes exactly one of target and grad_actions")
    feat, lead, t = _actor_rows(env, features, dict(target=target, grad=grad_actions, eps=eps), dict(weight=weight))
    gfeat = torch.empty(feat.shape, dtype=torch.float32, device=env.device) if grad_features else None
    return feat, t, gfeat, lead + (L.POLICY_FEATURE,), torch.empty(4, dtype=torch.float32, device=env.device)


def _look_ahead_setup(env, actions, repeat, outputs, out):
    """look_ahead's arguments and tensors (shared by BatchedRaceEnv and MixedTrackEnv): (scalar args, the tensors by
    rc_look_ahead_args field - env-major, one row per env -, the dict to return)."""
    E, A = env.num_envs, env.cars_per_env
    a = actions.to(env.device, torch.float32)
    if a.dim() == 4 and A == 1:
        a = a.unsqueeze(3)
    if a.dim() != 5 or a.shape[0] != E or a.shape[3] != A or a.shape[4] != 2:
        raise ValueError(f"actions must be [num_envs={E}, candidates, horizon, cars_per_env={A}, 2]"
                         f"{' or [num_envs, candidates, horizon, 2]' if A == 1 else ''}, got shape {tuple(actions.shape)}")
    a = a.contiguous()
    K, H = int(a.shape[1]), int(a.shape[2])
    if K < 1:
        raise ValueError("look_ahead needs at least one candidate")
    names = tuple(outputs)
    unknown = [n for n in names if n not in L.LOOK_AHEAD_OUTPUTS]
    if unknown:
        raise ValueError(f"look_ahead outputs must be among {sorted(L.LOOK_AHEAD_OUTPUTS)}, got {unknown}")
    tensors, result = {"actions": a}, {}
    for name in names:
        field, dtype, shape_of = L.LOOK_AHEAD_OUTPUTS[name]
        shape, dtype = shape_of(E, K, H, A), getattr(torch, dtype)
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=env.device)
        elif t.shape != shape or t.dtype != dtype or t.device != torch.device(env.device) or not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {shape} on {env.device}")
        tensors[field] = result[name] = t
    return dict(candidates=K, horizon=H, repeat=int(repeat)), tensors, result


def _observe_setup(env, lidar, action, context, mode, seed, state, row_offset, outputs, out):
    """policy_observe's arguments and tensors (shared by BatchedRaceEnv and MixedTrackEnv): (the filled rc_policy_observe_args, the
    tensors it points into - keep them until the call has been made -, the dict to return)."""
    if mode not in L.OBSERVE_MODES:
        raise ValueError(f"observe mode must be one of {sorted(L.OBSERVE_MODES)}, got {mode!r}")
    if lidar.dim() < 2 or lidar.shape[-1] != 1080 or action.shape[-1] != 2 or tuple(action.shape[:-1]) != tuple(lidar.shape[:-1]):
        raise ValueError(f"lidar must be [..., T, 1080] and action [..., T, 2], got {tuple(lidar.shape)} and {tuple(action.shape)}")
    lead, t_len = tuple(lidar.shape[:-2]), int(lidar.shape[-2])
    rows = 1
    for d in lead:
        rows *= int(d)
    if not 1 <= t_len <= L.OBSERVE_MAX_LENGTH:
        raise ValueError(f"the sequence length must be in [1, {L.OBSERVE_MAX_LENGTH}], got {t_len}")
    context = t_len if context is None else int(context)
    if not 1 <= context <= t_len:
        raise ValueError(f"context must be in [1, {t_len}], got {context}")
    outputs = tuple(outputs)
    unknown = [k for k in outputs if k not in L.OBSERVE_OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}: choose from {sorted(L.OBSERVE_OUTPUTS)}")
    keep = [lidar.to(env.device, torch.float32).reshape(rows, t_len, 1080).contiguous(),
            action.to(env.device, torch.float32).reshape(rows, t_len, 2).contiguous()]
    a = L.RcPolicyObserveArgs(C.sizeof(L.RcPolicyObserveArgs), t_len, context, L.OBSERVE_MODES[mode], rows, int(seed) & (2 ** 64 - 1),
                              int(row_offset) & (2 ** 64 - 1), keep[0].data_ptr(), keep[1].data_ptr())
    if state is not None:
        if tuple(state.shape) != lead + (L.POLICY_FEATURE + 2,):
            raise ValueError(f"state must be {lead + (L.POLICY_FEATURE + 2,)} = stoch | deter | (2 unused), got {tuple(state.shape)}")
        keep.append(state.to(env.device, torch.float32).reshape(rows, L.POLICY_FEATURE + 2).contiguous())
        a.state_in = keep[-1].data_ptr()
    result = {}
    for name in outputs:
        field, tail = L.OBSERVE_OUTPUTS[name]
        shape = lead + ((L.POLICY_FEATURE + 2,) if tail is None else (t_len,) + tail)
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=torch.float32, device=env.device)
        elif t.shape != shape or t.dtype != torch.float32 or t.device != torch.device(env.device) or not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be a contiguous float32 tensor of shape {shape} on {env.device}")
        result[name] = t
        setattr(a, field, t.data_ptr())
    return a, keep, result


def _decode_setup(env, features, slots, logits, image, mismatch, out):
    """policy_decode's arguments and tensors (shared by BatchedRaceEnv and MixedTrackEnv): (features as [rows, 230] or None, the
    slot mask, the tensors by rc_policy_decode_args field with their leading dimensions flattened, the dict to return).  What
    the call refuses (no policy, no decoder, no output, slots or mismatch with features) is left to the library, which names it."""
    mask = (1 << env.cars_per_env) - 1 if slots is None else sum({1 << int(a) for a in slots})
    if features is not None:
        if features.shape[-1] != L.POLICY_FEATURE:
            raise ValueError(f"features must be [..., {L.POLICY_FEATURE}], got {tuple(features.shape)}")
        lead = tuple(features.shape[:-1])
        features = features.to(env.device, torch.float32).reshape(-1, L.POLICY_FEATURE).contiguous()
        mask = 0 if slots is None else mask                  # (slots with features: the library refuses and says why)
    else:
        lead = (env.n_cars,)
    side = L.DECODE_IMAGE
    shapes = {}
    if logits:
        shapes["logits"] = (lead + (side, side), torch.float32)
    if image:
        shapes["image"] = (lead + (side, side), torch.uint8)
    if mismatch:
        shapes["mismatch"] = ((env.n_cars,), torch.int32)
    result = {}
    for name, (shape, dtype) in shapes.items():
        t = None if out is None else out.get(name)
        if t is None:
            t = (torch.empty if slots is None else torch.zeros)(shape, dtype=dtype, device=env.device)
        elif t.shape != shape or t.dtype != dtype or t.device != torch.device(env.device) or not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {shape} on {env.device}")
        result[name] = t
    flat = {k: (v if k == "mismatch" else v.view(-1, side, side)) for k, v in result.items()}
    return features, mask, dict(logits=flat.get("logits"), image=flat.get("image"), mismatch=flat.get("mismatch")), result


def _decode_loglik_setup(env, target, features, slots, outputs, out):
    """policy_decode_loglik's arguments and tensors (shared by BatchedRaceEnv and MixedTrackEnv): (features as [rows, 230] or None, the
    slot mask, the target as uint8 [rows, 64, 64] or None, the output tensors by rc_policy_decode_loglik_args field with their
    leading dimensions flattened, the dict to return).  The refusals are the library's."""
    mask = (1 << env.cars_per_env) - 1 if slots is None else sum({1 << int(a) for a in slots})
    side = L.DECODE_IMAGE
    kinds = {"loglik": ((), torch.float32), "logits": ((side, side), torch.float32), "image": ((side, side), torch.uint8)}
    outputs = tuple(outputs)
    unknown = [k for k in outputs if k not in kinds]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}: choose from {sorted(kinds)}")
    if features is not None:
        if features.shape[-1] != L.POLICY_FEATURE:
            raise ValueError(f"features must be [..., {L.POLICY_FEATURE}], got {tuple(features.shape)}")
        lead = tuple(features.shape[:-1])
        features = features.to(env.device, torch.float32).reshape(-1, L.POLICY_FEATURE).contiguous()
        mask = 0 if slots is None else mask                  # (slots with features: the library refuses and says why)
    else:
        lead = (env.n_cars,)
    if target is not None:
        n = 1
        for d in lead:
            n *= int(d)
        if target.numel() != n * side * side:
            raise ValueError(f"target must be {lead + (side, side)} (or with a trailing 1), got {tuple(target.shape)}")
        target = target.to(env.device, torch.uint8).reshape(-1, side, side).contiguous()
    result, flat = {}, {}
    for name in outputs:
        tail, dtype = kinds[name]
        shape = lead + tail
        t = None if out is None else out.get(name)
        if t is None:
            t = (torch.empty if slots is None else torch.zeros)(shape, dtype=dtype, device=env.device)
        elif t.shape != shape or t.dtype != dtype or t.device != torch.device(env.device) or not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {shape} on {env.device}")
        result[name] = t
        flat[name] = t.view((-1,) + tail)
    return features, mask, target, dict(loglik=flat.get("loglik"), logits=flat.get("logits"), image=flat.get("image")), result


def _decode_lidar_setup(env, features, slots, target, outputs, out):
    """policy_decode_lidar's arguments and tensors (shared by BatchedRaceEnv and MixedTrackEnv): (features as [rows, 230] or None, the
    slot mask, the target as [rows, 1080] or None, the output tensors by rc_policy_decode_lidar_args field with their leading
    dimensions flattened, the dict to return).  What the call refuses (no policy, no decoder, no output, slots with features,
    loglik without a target, a target with live latents) is left to the library, which names it."""
    mask = (1 << env.cars_per_env) - 1 if slots is None else sum({1 << int(a) for a in slots})
    outputs = tuple(outputs)
    unknown = [k for k in outputs if k not in L.DECODE_LIDAR_OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}: choose from {sorted(L.DECODE_LIDAR_OUTPUTS)}")
    if features is not None:
        if features.shape[-1] != L.POLICY_FEATURE:
            raise ValueError(f"features must be [..., {L.POLICY_FEATURE}], got {tuple(features.shape)}")
        lead = tuple(features.shape[:-1])
        features = features.to(env.device, torch.float32).reshape(-1, L.POLICY_FEATURE).contiguous()
        mask = 0 if slots is None else mask                  # (slots with features: the library refuses and says why)
    else:
        lead = (env.n_cars,)
    if target is not None:
        if tuple(target.shape) != lead + (L.RC_N_BEAMS,):
            raise ValueError(f"target must be {lead + (L.RC_N_BEAMS,)} in metres, got {tuple(target.shape)}")
        target = target.to(env.device, torch.float32).reshape(-1, L.RC_N_BEAMS).contiguous()
    result, flat = {}, {}
    for name in outputs:
        tail = L.DECODE_LIDAR_OUTPUTS[name]
        shape = lead + tail
        t = None if out is None else out.get(name)
        if t is None:
            t = (torch.empty if slots is None else torch.zeros)(shape, dtype=torch.float32, device=env.device)
        elif t.shape != shape or t.dtype != torch.float32 or t.device != torch.device(env.device) or not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be a contiguous float32 tensor of shape {shape} on {env.device}")
        result[name] = t
        flat[name] = t.view((-1,) + tail)
    return features, mask, target, dict(mean=flat.get("mean"), std=flat.get("std"), loglik=flat.get("loglik")), result


class BatchedRaceEnv:
    def __init__(self, track: Union[str, Track], num_envs: int, cars_per_env: int = 1, obs_type: str = "lidar",
                 action_repeat: int = 1, seed: int = 0, device: int = 0, first_env: int = 0,
                 task: str = "maximize_progress", laps: int = 10, time_limit: float = 180.0,
                 terminate_on_collision: bool = True, collision_reward: float = -1.0,
                 remap_actions: bool = False, action_low=spec.ACTION_LOW, action_high=spec.ACTION_HIGH,
                 time_limit_steps: int = 0, auto_reset: bool = False, profiling: bool = False,
                 lidar_transform: str = "metres", car_tasks=None, n_steps: int = 10,
                 shared_arena: Optional[torch.Tensor] = None, arena_total_cars: int = 0, arena_first_car: int = 0,
                 stream: Optional[torch.cuda.Stream] = None, vehicle_randomization=None, lidar_noise=None):
        """car_tasks: optional task name per car slot (agents A, B, ... of a scenario yml; None entries = `task`), e.g.
        ["maximize_progress", "n_step_progress", ...] for baselines/scenarios/max_progress/columbia.yml; n_steps: the
        window of `n_step_progress` in sub-steps.  shared_arena / arena_total_cars / arena_first_car / stream: this env
        fills cars [arena_first_car, ...) of an arena laid out for arena_total_cars cars and runs on the given stream -
        how `MixedTrackEnv` puts one handle per track behind one set of output tensors.  vehicle_randomization = (lo, hi, seed)
        and lidar_noise = (sigma, p_drop, seed): the same as calling `set_vehicle_randomization` / `set_lidar_noise` right
        after construction."""
        if obs_type not in OBS_TYPES:
            raise ValueError(f"obs_type must be one of {sorted(OBS_TYPES)}, got {obs_type!r}")
        if task not in TASKS:
            raise ValueError(f"task must be one of {sorted(TASKS)}, got {task!r}")
        self._lib = L.load_library()                     # raises if the HIP extension is missing
        if not torch.cuda.is_available():
            raise L.RacecarHipError("no HIP device visible to torch; BatchedRaceEnv has no CPU fallback")
        self.track = load_track(track) if isinstance(track, str) else track
        self.num_envs, self.cars_per_env = int(num_envs), int(cars_per_env)
        self.n_cars = self.num_envs * self.cars_per_env
        self.obs_type, self.action_repeat, self.seed = obs_type, int(action_repeat), int(seed)
        if self.track.open and task != "max_speed":
            import warnings
            warnings.warn(f"track {self.track.name!r} is not a loop (tracks/index.json: open): progress never comes round, so no lap is ever "
                          f"completed and `lap > laps` never ends an episode there", stacklevel=2)
        self.device = torch.device("cuda", device)
        self.first_env = int(first_env)

        cfg = L.RcConfig()
        self._lib.rc_default_config(C.byref(cfg))
        cfg.device, cfg.num_envs, cfg.cars_per_env, cfg.first_env = device, self.num_envs, self.cars_per_env, first_env
        cfg.obs_type, cfg.task, cfg.laps, cfg.time_limit = OBS_TYPES[obs_type], TASKS[task], laps, time_limit
        cfg.terminate_on_collision, cfg.collision_reward = int(terminate_on_collision), collision_reward
        cfg.remap_actions = int(remap_actions)
        cfg.action_low[:] = [float(v) for v in action_low]
        cfg.action_high[:] = [float(v) for v in action_high]
        cfg.time_limit_steps, cfg.auto_reset = int(time_limit_steps), int(auto_reset)
        for a, name in enumerate(car_tasks or ()):
            if name is not None:
                if name not in TASKS:
                    raise ValueError(f"car_tasks[{a}] must be one of {sorted(TASKS)}, got {name!r}")
                cfg.car_task[a] = TASKS[name]
        cfg.n_steps = int(n_steps)
        if lidar_transform not in LIDAR_TRANSFORMS:
            raise ValueError(f"lidar_transform must be one of {sorted(LIDAR_TRANSFORMS)}, got {lidar_transform!r}")
        cfg.lidar_transform = LIDAR_TRANSFORMS[lidar_transform]
        cfg.arena_total_cars, cfg.arena_first_car = int(arena_total_cars), int(arena_first_car)
        nbytes = self._lib.rc_arena_bytes(C.byref(cfg))
        if shared_arena is not None:
            if shared_arena.dtype != torch.uint8 or shared_arena.numel() < nbytes or shared_arena.data_ptr() % 64:
                raise ValueError(f"shared_arena must be a 64-byte aligned uint8 tensor of at least {nbytes} bytes")
            self.arena, self._arena_view = shared_arena, shared_arena[:nbytes]
            self.stream = stream if stream is not None else torch.cuda.Stream(device=self.device)
        else:
            with torch.cuda.device(self.device):
                self.arena = torch.zeros(nbytes + 64, dtype=torch.uint8, device=self.device)
                self.stream = stream if stream is not None else torch.cuda.Stream(device=self.device)
            pad = (-self.arena.data_ptr()) % 64
            self._arena_view = self.arena[pad:pad + nbytes]
        cfg.external_arena = self._arena_view.data_ptr()
        cfg.external_arena_bytes = nbytes
        cfg.stream = self.stream.cuda_stream
        self._cfg = cfg
        self._h = C.c_void_p()
        L.check(self._lib.rc_create(C.byref(cfg), C.byref(self._h)))
        self._load_track(self.track)
        self.views: Dict[str, torch.Tensor] = {}
        self._host_layout = {}
        base = self._arena_view.data_ptr()
        for name, (fid, dtype, tail) in _FIELD_VIEWS.items():
            if fid == L.F_OCCUPANCY and obs_type == "lidar":
                continue
            ptr, nb = C.c_void_p(), C.c_size_t()
            L.check(self._lib.rc_get(self._h, fid, C.byref(ptr), C.byref(nb)))
            off = ptr.value - base
            t = self._arena_view[off:off + nb.value].view(dtype)
            self.views[name] = t.view(self.num_envs, self.cars_per_env, *tail)
            self._host_layout[name] = (off, nb.value, str(dtype).replace("torch.", ""), tail)
        self.slab = self.summary_slab = None
        if not (arena_total_cars and arena_total_cars != self.n_cars):     # (a slice of a shared arena has no slab of its own)
            ptr, nb = C.c_void_p(), C.c_size_t()
            L.check(self._lib.rc_trajectory_slab(self._h, C.byref(ptr), C.byref(nb)))
            self.slab = self._arena_view[ptr.value - base:ptr.value - base + nb.value]
            # the record without the bulky observations: pose .. time (76 B per car), contiguous in the arena
            p0, n0, p1, n1 = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
            L.check(self._lib.rc_get(self._h, L.F_POSE, C.byref(p0), C.byref(n0)))
            L.check(self._lib.rc_get(self._h, L.F_TIME, C.byref(p1), C.byref(n1)))
            self.summary_slab = self._arena_view[p0.value - base:p1.value - base + n1.value]
        self._own_views = self.views
        ptr, nb = C.c_void_p(), C.c_size_t()
        L.check(self._lib.rc_vehicle_params(self._h, C.byref(ptr), C.byref(nb)))
        self._vp_array = _BorrowedDeviceArray(ptr.value, (self.n_cars, len(spec.VEHICLE_PARAMS)), self.device)
        self._vehicle_params = torch.utils.dlpack.from_dlpack(self._vp_array)
        if vehicle_randomization is not None:
            self.set_vehicle_randomization(*vehicle_randomization)
        if lidar_noise is not None:
            self.set_lidar_noise(*lidar_noise)
        if profiling:
            self.set_profiling(True)

    # ------------------------------------------------------------------ plumbing
    def _load_track(self, t: Track) -> None:
        occ = np.ascontiguousarray(t.occ_words, np.uint32)
        drv = np.ascontiguousarray(t.drv_words, np.uint32)
        prog = np.ascontiguousarray(t.progress, np.float32)
        cl = np.ascontiguousarray(t.centerline, np.float32)
        L.check(self._lib.rc_load_track(
            self._h, occ.ctypes.data, drv.ctypes.data, prog.ctypes.data, t.height, t.width, t.pitch,
            np.float32(t.resolution), np.float32(t.origin[0]), np.float32(t.origin[1]), cl.ctypes.data, len(cl)))
        if self.obs_type == "lidar_occupancy_reference":
            # where the grid lies in the source image the reference's GridMap.to_pixel indexes (compat/racecar_gym/core/gridmaps.py)
            r0, c0, fh, _fw = t.crop
            res = float(t.resolution)
            L.check(self._lib.rc_set_source_frame(self._h, int(fh), int(r0 + t.height - 1), int(c0), C.c_double(float(t.origin[0]) - c0 * res),
                                                  C.c_double(float(t.origin[1]) - (fh - (r0 + t.height)) * res), C.c_double(res)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.rc_destroy(self._h)
            self._h = C.c_void_p()
        for src in getattr(self, "_ts_sources", ()):       # (a track set's source handles outlive the owner)
            src.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self) -> None:
        L.check(self._lib.rc_sync(self._h))

    def _enter(self) -> None:
        # order the env's stream after whatever produced the actions on torch's current stream; nothing to do
        # when the caller already works on the env's stream (`with torch.cuda.stream(env.stream): ...`), which
        # saves two cross-stream event waits per call (a few microseconds each on the device queue)
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream != self.stream.cuda_stream:
            self.stream.wait_stream(cur)

    def _exit(self) -> None:
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream != self.stream.cuda_stream:
            cur.wait_stream(self.stream)

    # ------------------------------------------------------------------ env API
    def reset(self, mask: Optional[Union[np.ndarray, torch.Tensor]] = None, mode: str = "grid",
              seed: Optional[int] = None) -> Dict[str, torch.Tensor]:
        if mode not in spec.RESET_MODES:
            raise ValueError(f"reset mode must be one of {sorted(spec.RESET_MODES)}, got {mode!r}")
        if seed is not None:
            self.seed = int(seed)
        mptr = None
        if mask is not None:
            m = np.ascontiguousarray(torch.as_tensor(mask).cpu().numpy().astype(np.uint8).reshape(self.num_envs))
            mptr = m.ctypes.data
        self._enter()
        L.check(self._lib.rc_reset(self._h, mptr, spec.RESET_MODES[mode], C.c_uint64(self.seed)))
        self._exit()
        return self.views

    def step(self, actions: Optional[torch.Tensor] = None, repeat: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """One agent step.  ``actions``: float32 [num_envs, cars_per_env, 2] = (motor, steering) on the
        env's device, or None to use the device-side ``action_in`` buffer."""
        repeat = self.action_repeat if repeat is None else int(repeat)
        ptr = None
        if actions is not None:
            if actions.device != self.device:
                actions = actions.to(self.device, non_blocking=True)
            actions = actions.to(torch.float32).contiguous()
            if actions.numel() != self.n_cars * 2:
                raise ValueError(f"actions must hold {self.n_cars} x 2 values, got shape {tuple(actions.shape)}")
            ptr = actions.data_ptr()
        self._enter()
        L.check(self._lib.rc_step(self._h, ptr, repeat))
        self._exit()
        return self.views

    def step_random(self, seed: int, step: int, repeat: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """``fill_random_actions(seed, step)`` + ``step(None, repeat)`` in one pass of the dynamics kernel (identical
        results): the step of a synthetic random-action rollout (the reference's default prefill policy,
        dreamer/dream.py:207-210)."""
        repeat = self.action_repeat if repeat is None else int(repeat)
        self._enter()
        L.check(self._lib.rc_step_random(self._h, C.c_uint64(seed), C.c_uint32(step), repeat))
        self._exit()
        return self.views

    def set_pose(self, xyyaw) -> Dict[str, torch.Tensor]:
        """Teleport every car: float32 [num_envs, cars_per_env, 3] = x, y, yaw; recomputes the observation."""
        a = np.ascontiguousarray(np.asarray(xyyaw, np.float32).reshape(self.n_cars, 3))
        self._enter()
        L.check(self._lib.rc_set_pose(self._h, a.ctypes.data))
        self._exit()
        return self.views

    # ------------------------------------------------------------------ domain randomization (include/racecar_hip.h)
    def set_vehicle_randomization(self, lo=None, hi=None, seed: int = 0) -> None:
        """Random mode of the five per-car vehicle parameters (`spec.VEHICLE_PARAMS`: wheel_max, accel_max, drag, max_vel,
        steer_step): at every reset of an env, rc_reset or auto-reset, each car draws value = lo + u (hi - lo) from Philox keyed
        by `seed` and (global env id, episode, call, 2).  Takes effect at each env's next reset.  lo = hi = None: off (the
        spec's constants).  E.g. `env.set_vehicle_randomization(**spec.DR_DEPLOYMENT_LOCK, seed=1)`."""
        if lo is None or hi is None:
            L.check(self._lib.rc_set_vehicle_randomization(self._h, None, None, C.c_uint64(0)))
            return
        lo_a = np.ascontiguousarray(np.asarray(lo, np.float32).reshape(len(spec.VEHICLE_PARAMS)))
        hi_a = np.ascontiguousarray(np.asarray(hi, np.float32).reshape(len(spec.VEHICLE_PARAMS)))
        L.check(self._lib.rc_set_vehicle_randomization(self._h, lo_a.ctypes.data, hi_a.ctypes.data, C.c_uint64(int(seed))))

    def set_vehicle_params(self, params: Optional[torch.Tensor]) -> None:
        """Fixed mode: float32 [n_cars, 5] (or [num_envs, cars_per_env, 5]) vehicle parameters that persist across resets and
        are never drawn (evaluation sweeps).  None: off."""
        if params is None:
            L.check(self._lib.rc_set_vehicle_params(self._h, None))
            return
        t = torch.as_tensor(params, dtype=torch.float32).to(self.device).reshape(self.n_cars, len(spec.VEHICLE_PARAMS)).contiguous()
        self._enter()
        L.check(self._lib.rc_set_vehicle_params(self._h, t.data_ptr()))
        self._exit()
        self._vp_source = t                  # (the copy is stream-ordered: keep the source alive until the next call)

    @property
    def vehicle_params(self) -> torch.Tensor:
        """Device view float32 [n_cars, 5] of every car's current vehicle parameters (nominal values while randomization is
        off) - state, not record: it changes at resets, so clone what must be kept."""
        return self._vehicle_params

    def set_lidar_noise(self, sigma: float = 0.0, p_drop: float = 0.0, seed: int = 0) -> None:
        """Gaussian-like range noise (standardised Irwin-Hall(4), `sigma` metres) and dropout (a beam reads 15 m, "no return",
        with probability `p_drop`) on the `lidar` scan, counter-based per (seed, global car, episode, sub-step, beam).
        sigma = p_drop = 0: off."""
        L.check(self._lib.rc_set_lidar_noise(self._h, float(sigma), float(p_drop), C.c_uint64(int(seed))))

    # ------------------------------------------------------------------ track set (include/racecar_hip.h, rc_set_track_set)
    @classmethod
    def with_track_set(cls, tracks, num_envs: int, cars_per_env: int = 1, order: str = "sequential", initial=None, weights=None,
                       seed: int = 0, **kw) -> "BatchedRaceEnv":
        """A batch whose envs switch track at every reset, on the device (the reference's ChangingTrackSingleAgentRaceEnv per env):
        `tracks` (names or Tracks, 1..8), order "sequential" (k + 1 mod T), "random" (Philox keyed by `seed`, the global env id and
        the episode; optional `weights`) or "manual" (`set_next_track`).  `initial`: int [num_envs] track per env, default
        contiguous blocks of near-equal size (MixedTrackEnv's split).  Each env's first reset keeps its initial track.  The handle
        is built on tracks[0]; every other keyword goes to the constructor (vehicle_randomization=, lidar_noise=, ...).
        `env.track_id` is a zero-copy int32 [num_envs] device view of the current tracks, `env.track_names` their names."""
        tracks = list(tracks)
        if not 1 <= len(tracks) <= 8:
            raise ValueError(f"a track set has 1..8 tracks, got {len(tracks)}")
        if order not in TRACK_ORDERS:
            raise ValueError(f"order must be one of {sorted(TRACK_ORDERS)}, got {order!r}")
        loaded = [load_track(t) if isinstance(t, str) else t for t in tracks]
        env = cls(loaded[0], num_envs, cars_per_env, **kw)
        dev = env.device.index or 0
        env._ts_sources = [cls(t, 1, 1, device=dev) for t in loaded[1:]]         # small handles: only their track tables are used
        handles = (C.c_void_p * len(loaded))(env._h, *[h._h for h in env._ts_sources])
        w = None
        if weights is not None:
            w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(len(loaded)))
        init_ptr = None
        if initial is not None:
            init_t = torch.as_tensor(initial, dtype=torch.int32).to(env.device).reshape(env.num_envs).contiguous()
            init_ptr = init_t.data_ptr()
        env._enter()
        L.check(env._lib.rc_set_track_set(env._h, handles, len(loaded), TRACK_ORDERS[order], None if w is None else w.ctypes.data,
                                          init_ptr, C.c_uint64(int(seed))))
        env._exit()
        env.track_names = [t.name for t in loaded]
        env.track_order = order
        ptr, nb = C.c_void_p(), C.c_size_t()
        L.check(env._lib.rc_track_ids(env._h, C.byref(ptr), C.byref(nb)))
        env._track_array = _BorrowedDeviceArray(ptr.value, (env.num_envs,), env.device, code=0)
        env.track_id = torch.utils.dlpack.from_dlpack(env._track_array)
        return env

    def set_next_track(self, ids) -> None:
        """Order "manual": int [num_envs] track of each env's next reset (persists; read at every reset)."""
        t = torch.as_tensor(ids, dtype=torch.int32).to(self.device).reshape(self.num_envs).contiguous()
        self._enter()
        L.check(self._lib.rc_set_next_track(self._h, t.data_ptr()))
        self._exit()
        self._next_source = t                # (the copy is stream-ordered: keep the source alive until the next call)

    def clear_track_set(self) -> None:
        """Turn the track set off (rc_set_track_set with n = 0): the production kernels run again, every env on the handle's own
        track (tracks[0]) - reset before stepping on."""
        L.check(self._lib.rc_set_track_set(self._h, None, 0, 0, None, None, C.c_uint64(0)))

    def set_raycast_variant(self, variant: int) -> None:
        """0 = plain traversal, 1 = free-rectangle skipping, 2 = tuned skipping, 3 = tuned + packed block table
        in LDS, 4 = the same reading the table through L1/L2, 5 = per-cell distance table through L1/L2,
        6 = per-cell, per-quadrant free rectangles through L1/L2,
        7 = the same with one wave per car (default).  All variants return identical results.  Variants 0-6 are not in the
        shipped library: they live in the lab library (csrc/racecar_lab.hip), which is compiled here on first request."""
        if int(variant) != 7:
            _ensure_lab()
        L.check(self._lib.rc_set_raycast_variant(self._h, int(variant)))

    # ------------------------------------------------------------------ half-size record + multi-GPU gather
    def enable_compact(self, buffers: int = 2) -> None:
        """Make the scan also store the LiDAR row as uint16, followed by the 76 B/car summary (`rc_set_compact_slab`):
        the 2 236 B/car record of the `full-u16` gather.  `buffers` slabs take turns (`rotate_compact`), so a gather
        of slab k overlaps the step that fills slab k + 1."""
        nbytes = self._lib.rc_compact_bytes(C.byref(self._cfg))
        slabs = []
        for _ in range(max(1, int(buffers))):
            raw = torch.zeros(nbytes + 64, dtype=torch.uint8, device=self.device)
            pad = (-raw.data_ptr()) % 64
            slabs.append((raw, raw[pad:pad + nbytes]))
        L.check(self._lib.rc_set_compact_slab(self._h, slabs[0][1].data_ptr(), nbytes))
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        L.check(self._lib.rc_compact_layout(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.compact_layout = (a.value, b.value, c.value)       # uint16 bytes, summary offset, summary bytes
        self._compact, self._compact_k = slabs, 0
        self.compact = slabs[0][1]

    def rotate_compact(self) -> torch.Tensor:
        """Point the next step's compact record at the next slab of the set; returns the slab just completed."""
        done = self.compact
        self._compact_k = (self._compact_k + 1) % len(self._compact)
        self.compact = self._compact[self._compact_k][1]
        L.check(self._lib.rc_set_compact_slab(self._h, self.compact.data_ptr(), self.compact.numel()))
        return done

    def disable_compact(self) -> None:
        L.check(self._lib.rc_set_compact_slab(self._h, None, 0))
        self.compact = None

    def gather_source(self, mode: str) -> torch.Tensor:
        """The bytes one gather mode sends: 'full' (fp32 record), 'full-u16' (compact slab), 'summary' (pose..time)."""
        if mode == "full":
            return self.slab
        if mode == "summary":
            return self.summary_slab
        if mode == "full-u16":
            if getattr(self, "compact", None) is None:
                raise L.RacecarHipError("gather mode 'full-u16' needs enable_compact() first")
            return self.compact
        raise ValueError(f"unknown gather mode {mode!r}")

    def comm_init(self, unique_id: bytes, rank: int, world: int) -> None:
        """RCCL communicator of this handle (`rc_comm_init`); `unique_id` from `comm_unique_id()` on rank 0."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        L.check(self._lib.rc_comm_init(self._h, buf, 128, int(rank), int(world)))
        self.comm_world = int(world)

    @staticmethod
    def comm_unique_id() -> bytes:
        lib = L.load_library()
        buf = C.create_string_buffer(128)
        L.check(lib.rc_comm_unique_id(buf, 128))
        return buf.raw

    def gather(self, mode: str, dst: torch.Tensor) -> None:
        """`rc_gather_trajectory`: asynchronous RCCL all-gather of the last step's record into `dst` (uint8,
        world x gather_bytes(mode))."""
        L.check(self._lib.rc_gather_trajectory(self._h, L.GATHER_MODES[mode], dst.data_ptr(), dst.numel()))

    def gather_bytes(self, mode: str) -> int:
        return int(self._lib.rc_gather_bytes(self._h, L.GATHER_MODES[mode]))

    def gather_wait(self, host_sync: bool = True) -> None:
        L.check(self._lib.rc_gather_wait(self._h, int(bool(host_sync))))

    # ---- the same gather as direct peer copies (rc_gather_trajectory_p2p: hipIpc handles, one copy stream per peer) ----
    def p2p_setup(self, mode: str, rank: int, world: int) -> bytes:
        """Allocate this rank's destination and flags for peer-copy gathers (sized for the largest payload) and select
        `mode`; returns the 256-byte blob the other ranks need.  Hand every rank's blob (in rank order) to `p2p_connect`
        on every rank.  Called again it only switches the payload: same buffers, same blob."""
        buf = C.create_string_buffer(L.P2P_EXPORT_BYTES)
        L.check(self._lib.rc_p2p_setup(self._h, L.GATHER_MODES[mode], int(rank), int(world), buf, L.P2P_EXPORT_BYTES))
        self._p2p_mode, self._p2p_world = mode, int(world)
        return buf.raw

    def p2p_connect(self, blobs) -> None:
        raw = b"".join(bytes(b) for b in blobs)
        L.check(self._lib.rc_p2p_connect(self._h, C.create_string_buffer(raw, len(raw)), len(raw)))

    def gather_p2p(self, mode: Optional[str] = None) -> None:
        """Send the last step's record into every rank's buffer (asynchronous, behind the work on the env's stream)."""
        if mode is not None and mode != self._p2p_mode:
            raise ValueError(f"the peer-copy gather was set up for {self._p2p_mode!r}, not {mode!r}")
        L.check(self._lib.rc_gather_trajectory_p2p(self._h))

    def gather_p2p_wait(self, host_sync: bool = True):
        """Order the env's stream (and the host) behind the arrival of the last issued gather; returns (device pointer,
        bytes) of the gathered slot: rank r's record at r * bytes / world."""
        ptr, nb = C.c_void_p(), C.c_size_t()
        L.check(self._lib.rc_gather_p2p_wait(self._h, int(bool(host_sync)), C.byref(ptr), C.byref(nb)))
        return ptr.value, nb.value

    def gathered_p2p_host(self, back: int = 0) -> np.ndarray:
        """Host copy of the last gathered slot (back = 1: of the gather before it) as uint8 [world, bytes per rank]
        (synchronising)."""
        ptr, nb = self.gather_p2p_wait(host_sync=True)
        if back:
            p2, n2 = C.c_void_p(), C.c_size_t()
            L.check(self._lib.rc_p2p_slot(self._h, int(back), C.byref(p2), C.byref(n2)))
            ptr, nb = p2.value, n2.value
        out = np.empty(nb, np.uint8)
        L.check(self._lib.rc_copy_from_device(self._h, ptr, out.ctypes.data, nb))
        # the slot's entries are sized for the largest payload: the current one fills the head of each
        return out.reshape(self._p2p_world, -1)[:, :self.gather_bytes(self._p2p_mode)]

    def p2p_disconnect(self) -> None:
        """Wait for this rank's copies and unmap the peers' buffers.  Every rank disconnects, the ranks synchronise (the
        caller's barrier), then they `p2p_teardown()`: exported memory must not be freed while a peer still maps it."""
        L.check(self._lib.rc_p2p_disconnect(self._h))

    def p2p_teardown(self) -> None:
        L.check(self._lib.rc_p2p_teardown(self._h))

    def comm_count(self) -> int:
        n = C.c_int32()
        L.check(self._lib.rc_comm_count(self._h, C.byref(n)))
        return int(n.value)

    def scan_kernel_name(self) -> str:
        buf = C.create_string_buffer(128)
        L.check(self._lib.rc_scan_kernel_name(self._h, buf, 128))
        return buf.value.decode()

    def scan_overruns(self) -> int:
        """Waves of this handle's BOUNDED scans that used up a round's trip budget (0 unless a band was mis-set)."""
        n = C.c_uint64()
        L.check(self._lib.rc_scan_overruns(self._h, C.byref(n)))
        return int(n.value)

    def debug_set(self, knob: str, value: int) -> None:
        """Experiment / validation knobs of the scan (`rc_debug_set`; 0 = production behaviour): ray_threads,
        ray_split, ray_wg_per_cu, band_log2.  Used by tools/knob_sweep.sh and the band-sensitivity check of
        tests/test_gpu_parity.py; the library itself reads nothing from the process environment."""
        L.check(self._lib.rc_debug_set(self._h, L.DEBUG_KNOBS[knob], int(value)))

    def debug_scan_stamps(self, n_waves: int = 0) -> Optional[torch.Tensor]:
        """In-kernel time stamps of the default scan (`rc_debug_scan_stamps`, analysis only; tools/scan_stamps.py): with
        n_waves > 0 the following scans run the instrumented kernel and its first n_waves waves fill the returned
        int64 [n_waves, 32] device tensor; n_waves = 0 switches back to the production kernel."""
        if n_waves <= 0:
            L.check(self._lib.rc_debug_scan_stamps(self._h, None, 0))
            self._stamps = None
            return None
        _ensure_lab()                    # the instrumented build is a lab kernel
        self._stamps = torch.zeros((n_waves, 32), dtype=torch.int64, device=self.device)
        L.check(self._lib.rc_debug_scan_stamps(self._h, self._stamps.data_ptr(), int(n_waves)))
        return self._stamps

    def follow_the_gap(self, motor_straight: float = 0.6, motor_corner: float = 0.3) -> torch.Tensor:
        """Batched follow-the-gap agent (dreamer/dream.py:211-216 prefill): fills and returns `action_in`
        from the current LiDAR scans; pass None to step() to apply it."""
        self._enter()
        L.check(self._lib.rc_follow_the_gap(self._h, motor_straight, motor_corner))
        self._exit()
        return self.views["action_in"]

    def follow_the_gap_reference(self, dt: Optional[float] = None, detail: bool = False):
        """The reference's own follow-the-gap law (ros_agent/agents/follow_the_gap/src/agent.py:128-234) as a device agent:
        fills and returns `action_in`; with detail=True also a float32 [n_cars, 4] tensor of heading, free distance,
        steering angle and speed.  dt defaults to the env's agent step (0.01 s x action_repeat)."""
        dt = 0.01 * self.action_repeat if dt is None else float(dt)
        det = torch.empty((self.n_cars, 4), dtype=torch.float32, device=self.device) if detail else None
        self._enter()
        L.check(self._lib.rc_follow_the_gap_reference(self._h, dt, det.data_ptr() if detail else None))
        self._exit()
        return (self.views["action_in"], det) if detail else self.views["action_in"]

    # ------------------------------------------------------------------ the reference's trained Dreamer agent
    def load_policy(self, weights) -> None:
        """Load a checkpoint of the reference's deployed Dreamer agent (mapping of float32 arrays with the keys of
        tests/golden/dreamer_policy_*.npz, or an .npz path) onto the device (`rc_policy_load`): the weights are copied, the agent's
        state starts at zero.  Shapes are checked by the library."""
        w, keep = L.policy_weights(weights)
        L.check(self._lib.rc_policy_load(self._h, C.byref(w)))
        del keep
        ptr, nb = C.c_void_p(), C.c_size_t()
        L.check(self._lib.rc_policy_state(self._h, C.byref(ptr), C.byref(nb)))
        # a second load keeps the first load's wrapper alive: torch reads the DLPack struct again when the tensor made from it
        # is released, which may be after this call (a view the caller still holds)
        self._policy_arrays = getattr(self, "_policy_arrays", []) + [_BorrowedDeviceArray(ptr.value, (self.n_cars, L.POLICY_STATE), self.device)]
        self._policy_state = torch.utils.dlpack.from_dlpack(self._policy_arrays[-1])
        self._policy_has_head = False                       # (rc_policy_load drops a head loaded before)
        heads = L.policy_heads(weights)
        if heads is not None:
            L.check(self._lib.rc_policy_load_heads(self._h, C.byref(heads[0])))
            self._policy_has_head = True
        self._policy_has_decoder = False                    # (and a decoder)
        decoder = L.policy_decoder(weights)
        if decoder is not None:
            L.check(self._lib.rc_policy_load_decoder(self._h, C.byref(decoder[0])))
            self._policy_has_decoder = True
        self._policy_has_lidar_decoder = False              # (and a LiDAR distance decoder)
        if L.policy_lidar_decoder(weights) is not None:
            self.load_lidar_decoder(weights)
        self._policy_has_value = self._policy_has_pcont = False      # (and a critic)
        if L.policy_critic(weights) is not None:
            self.load_critic(weights)

    def load_critic(self, weights) -> None:
        """Load the critic of a Dreamer agent beside the loaded policy (`rc_policy_load_critic`): a mapping (or an .npz path) with
        the value head's `value_h0_w` .. `value_hout_b` (DenseDecoder((), 3, 400): [230, 400], [400], 2 x ([400, 400], [400]),
        [400, 1], [1]) and, optionally, the pcont head's `pcont_*` of the same shapes - `critic.init_critic` makes a synthetic
        pair, `critic.critic_from_variables` picks a trained one out of the reference's `variables.pkl`.  None drops both heads;
        so do `load_policy` and `unload_policy`.  Shapes are checked by the library."""
        if weights is None:
            L.check(self._lib.rc_policy_load_critic(self._h, None))
            self._policy_has_value = self._policy_has_pcont = False
            return
        critic = L.policy_critic(weights)
        if critic is None:
            raise KeyError("critic weights lack the value_* arrays")
        L.check(self._lib.rc_policy_load_critic(self._h, C.byref(critic[0])))
        self._policy_has_value = True
        self._policy_has_pcont = bool(critic[0].pcont_hout_w.data)

    @property
    def policy_has_value_head(self) -> bool:
        """Whether a value head is loaded (`value_*` arrays: `load_critic`, or a checkpoint that holds them)."""
        return bool(getattr(self, "_policy_has_value", False))

    @property
    def policy_has_pcont_head(self) -> bool:
        """Whether a pcont head is loaded (`pcont_*` arrays); without one `policy_returns` uses the constant `discount`."""
        return bool(getattr(self, "_policy_has_pcont", False))

    def _returns(self, args: dict, tensors: dict, lo: int, hi: int) -> int:
        """rc_policy_returns on this handle: from its live latents, reading and writing rows [lo, hi) of the tensors (one row per
        car), or from a given state, the whole tensors."""
        a = L.RcPolicyReturnsArgs(C.sizeof(L.RcPolicyReturnsArgs), args["horizon"], args["mode"], args["mask"], args["lambda_"], args["discount"],
                                  args["seed"], args["starts"], args["row_offset"])
        for field, t in tensors.items():
            setattr(a, field, None if t is None else (t[lo:hi] if args["live"] else t).data_ptr())
        return self._lib.rc_policy_returns(self._h, C.byref(a))

    def policy_returns(self, horizon: int = 15, mode: str = "mean", seed: int = 0, lambda_: float = 0.95, discount: float = 0.99,
                       actions: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None, row_offset: int = 0, slots=None,
                       outputs=("returns", "weight"), out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """The forward half of the reference's behaviour learning (`rc_policy_returns`, one launch; dreamer/models.py:113-133):
        `policy_imagine`'s rollout - closed loop, or open loop under `actions` [S, horizon, 2] - with the reward, value and pcont
        heads on every imagined feature, then the lambda-return and the discount weights, all on the device.  The starts are
        every car's latent as `policy_act` last left it (S = n_cars, `policy_imagine`'s draws for the same seed; with `slots`,
        rows of the other cars are zero - or what `out` held), or `state` float32 [S, 232] = stoch | deter | (2 unused), whose
        draws in mode "sample" depend on (seed, `row_offset` + row, t) only, so shards of a batch reproduce the whole.  Without
        a pcont head pcont is the constant `discount`.  `outputs` names what to compute, each a device float32 tensor:
        `returns`, `weight` [S, H - 1] (H >= 2; returns[t] = R_t, weight = cumprod([1, pcont[:-2]])), `reward`, `value`, `pcont`
        [S, H], `actions` [S, H, 2], `features` [S, H, 230], `reward_start`, `value_start`, `pcont_start` [S] (the heads on the
        starting feature; horizon 0 asks for them alone).  Nothing else changes: not the agent's state, not `action_in`."""
        args, tensors, result = _returns_setup(self, horizon, mode, seed, lambda_, discount, actions, state, row_offset, slots, outputs, out)
        self._enter()
        try:
            L.check(self._returns(args, tensors, 0, self.n_cars))
        finally:
            self._exit()                 # a refused call still orders torch's stream after the env's
        return result

    def _returns_grad(self, args: dict, tensors: dict, lo: int, hi: int) -> int:
        """rc_policy_returns_grad on this handle: rows as `_returns` takes them."""
        a = L.RcPolicyReturnsGradArgs(C.sizeof(L.RcPolicyReturnsGradArgs), args["horizon"], args["mode"], args["mask"], args["lambda_"],
                                      args["discount"], args["scale"], 0, args["seed"], args["starts"] if not args["live"] else 0,
                                      args["row_offset"], args["chunk_rows"])
        for field, t in tensors.items():
            setattr(a, field, None if t is None else (t[lo:hi] if args["live"] else t).data_ptr())
        return self._lib.rc_policy_returns_grad(self._h, C.byref(a))

    def policy_returns_grad(self, horizon: int = 15, mode: str = "sample", seed: int = 0, lambda_: float = 0.95, discount: float = 0.99,
                            scale: Optional[float] = None, actions: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None,
                            row_offset: int = 0, slots=None, outputs=("grad_actions", "actor_features", "eps"),
                            out: Optional[Dict[str, torch.Tensor]] = None, chunk_rows: int = 0) -> Dict[str, torch.Tensor]:
        """The gradient of the reference's actor loss through the dream (`rc_policy_returns_grad`; dreamer/models.py:113-128):
        `policy_returns`' rollout with the same arguments, draws and bytes, then the backward pass of J = sum_t (scale weight[t])
        returns[t] per row - weight a constant, returns differentiated through the reward, value and pcont heads and the prior step.
        `scale` None is float32(-1 / (rows (H - 1))): the sum of J over the rows is then the reference's actor_loss.  The actor is
        not differentiated (the reference feeds it stop_gradient(feat)); `outputs` are the rows `actor_fit(grad_actions=...)` takes:
        `grad_actions` [S, H, 2] (dJ / d a_t; under `actions` exactly +0 where the raw action lies outside [-1, 1]), `actor_features`
        [S, H, 230] (what the actor read for a_t), `eps` [S, H, 2] (its draw's normals: mode "sample", closed loop), and `grad_state`
        [S, 230]; every output of `policy_returns` may be asked for beside them and is byte for byte what it returns.  At least one
        of `grad_actions` and `grad_state`; H >= 2; a reward head and a value head must be loaded.  `chunk_rows` as
        `dream_ahead_grad`'s.  Nothing else changes: not the agent's state, not `action_in`, not a weight."""
        args, tensors, result = _returns_grad_setup(self, horizon, mode, seed, lambda_, discount, scale, actions, state, row_offset, slots,
                                                    outputs, out, chunk_rows)
        self._enter()
        try:
            L.check(self._returns_grad(args, tensors, 0, self.n_cars))
        finally:
            self._exit()                 # a refused call still orders torch's stream after the env's
        return result

    def policy_value(self, features: Optional[torch.Tensor] = None, slots=None, outputs=("value",)) -> Dict[str, torch.Tensor]:
        """The heads on given features (a horizon-0 `policy_returns`): `features` float32 [..., 230] = stoch | deter, e.g.
        `dream_ahead(...)["final_feature"]`, or None for every car's live latent (with `slots`: the other cars' rows are zero).
        `outputs` among "value", "reward", "pcont"; each comes back as a device float32 tensor of the leading shape."""
        state, lead, names = _value_setup(self, features, slots, outputs)
        got = self.policy_returns(horizon=0, state=state, slots=slots, outputs=names)
        return {n[:-6]: got[n].reshape(lead) for n in names}

    def _fit(self, head, feat, tgt, wgt, status, hyper) -> int:
        a = L.RcPolicyFitArgs(C.sizeof(L.RcPolicyFitArgs), L.FIT_HEADS.get(head, head), feat.shape[0], feat.data_ptr(), tgt.data_ptr(),
                              None if wgt is None else wgt.data_ptr(), hyper["lr"], hyper["clip"], hyper["beta1"], hyper["beta2"],
                              hyper["epsilon"], None if status is None else status.data_ptr())
        return self._lib.rc_policy_fit_step(self._h, C.byref(a))

    def critic_fit_begin(self, head: str = "value") -> None:
        """Open the optimizer of a loaded head, "value" or "pcont" (`rc_policy_fit_begin`): Adam moments zero, step 0.  One per
        head; `load_critic`, `load_policy` and `unload_policy` close them."""
        if head not in L.FIT_HEADS:
            raise ValueError(f"head must be one of {sorted(L.FIT_HEADS)}, got {head!r}")
        cfg = L.RcPolicyFitConfig(C.sizeof(L.RcPolicyFitConfig), L.FIT_HEADS[head])
        self._enter()
        try:
            L.check(self._lib.rc_policy_fit_begin(self._h, C.byref(cfg)))
        finally:
            self._exit()

    def critic_fit(self, features: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, head: str = "value",
                   lr: float = 8e-5, clip: float = 1.0, beta1: float = 0.9, beta2: float = 0.999,
                   epsilon: float = 1e-7) -> Dict[str, torch.Tensor]:
        """One step of the reference's value update on the device (`rc_policy_fit_step`; dreamer/models.py:129-137,
        dreamer/tools.py:421-455): the head's forward and backward pass on `features` [..., 230] = stoch | deter against `target`
        [...] (for the value head `policy_returns`' returns on `features[:, :-1]`) under `weight` [...] or None, the global-norm
        clip (`clip` 0: none) and Adam, all on the device and in the env's stream: no synchronisation, no host copy.  Inputs
        that are not contiguous float32 are made so.  The defaults are the reference's value_lr and grad_clip and TF's Adam.
        Returns device scalars: `loss`, `grad_norm` (before the clip), `skipped` (1: the norm was not finite, nothing changed),
        `step` (the steps taken).  The fitted weights are what `policy_returns`, `policy_value` and the planners read next."""
        feat, tgt, wgt, status = _fit_setup(self, features, target, weight, head)
        hyper = dict(lr=lr, clip=clip, beta1=beta1, beta2=beta2, epsilon=epsilon)
        self._enter()
        try:
            L.check(self._fit(head, feat, tgt, wgt, status, hyper))
        finally:
            self._exit()
        return _fit_status(status)

    def critic_fit_end(self, head: str = "value") -> None:
        """Free the optimizer's state (`rc_policy_fit_end`); the fitted weights stay loaded."""
        if head not in L.FIT_HEADS:
            raise ValueError(f"head must be one of {sorted(L.FIT_HEADS)}, got {head!r}")
        L.check(self._lib.rc_policy_fit_end(self._h, L.FIT_HEADS[head]))

    def critic_weights(self) -> Dict[str, np.ndarray]:
        """The loaded critic as NumPy arrays under `VALUE_KEYS` (and `PCONT_KEYS` with a pcont head), as `load_critic` takes
        them (`rc_policy_read_critic`; waits for the env's stream)."""
        keys = L.VALUE_KEYS + (L.PCONT_KEYS if self.policy_has_pcont_head else ())
        out = {k: np.empty(shape, np.float32) for k, shape in zip(keys, L.CRITIC_SHAPES * 2)}
        c = L.RcPolicyCritic()
        c.struct_size = C.sizeof(L.RcPolicyCritic)
        for k, a in out.items():
            arr = getattr(c, k)
            arr.data = a.ctypes.data
            arr.rows, arr.cols = (1, a.shape[0]) if a.ndim == 1 else a.shape
        self._enter()
        try:
            L.check(self._lib.rc_policy_read_critic(self._h, C.byref(c)))
        finally:
            self._exit()
        return out

    # ---- the reward head's own fit (rc_policy_fit_* with RC_POLICY_FIT_REWARD): not one of critic_fit's heads
    def reward_fit_begin(self) -> None:
        """Open the optimizer of the loaded reward head (`rc_policy_fit_begin`, RC_POLICY_FIT_REWARD): Adam moments zero, step 0.
        Independent of the critic's optimizers; `load_reward_head`, `load_policy` and `unload_policy` close it."""
        cfg = L.RcPolicyFitConfig(C.sizeof(L.RcPolicyFitConfig), L.FIT_REWARD)
        self._enter()
        try:
            L.check(self._lib.rc_policy_fit_begin(self._h, C.byref(cfg)))
        finally:
            self._exit()

    def reward_fit(self, features: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, lr: float = 6e-4,
                   clip: float = 1.0, beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-7) -> Dict[str, torch.Tensor]:
        """One step of the reward head towards recorded rewards, on the device (`rc_policy_fit_step`, RC_POLICY_FIT_REWARD): the
        head's forward and backward pass on `features` [..., 230] = stoch | deter (e.g. `policy_observe`'s) against `target` [...]
        under `weight` [...] or None - loss = -mean(weight * Normal(head(features), 1).log_prob(target)) -, the global-norm clip
        (`clip` 0: none) and Adam, as `critic_fit` does for the value head: no synchronisation, no host copy.  The defaults are
        the reference's model_lr and grad_clip (dreamer/dream.py:85, 88) and TF's Adam.  Returns device scalars `loss`,
        `grad_norm` (before the clip), `skipped`, `step`.  The fitted head is what `policy_imagine`, `policy_observe`,
        `dream_ahead`, `policy_returns`, `dream_ahead_grad` and the planners read next; nothing else moves."""
        feat, tgt, wgt, status = _fit_setup(self, features, target, weight, None)
        hyper = dict(lr=lr, clip=clip, beta1=beta1, beta2=beta2, epsilon=epsilon)
        self._enter()
        try:
            L.check(self._fit(L.FIT_REWARD, feat, tgt, wgt, status, hyper))
        finally:
            self._exit()
        return _fit_status(status)

    def reward_fit_end(self) -> None:
        """Free the reward optimizer's state (`rc_policy_fit_end`); the fitted head stays loaded."""
        L.check(self._lib.rc_policy_fit_end(self._h, L.FIT_REWARD))

    def reward_head_weights(self) -> Dict[str, np.ndarray]:
        """The loaded reward head as NumPy arrays under `HEAD_KEYS`, as `load_reward_head` takes them (`rc_policy_read_heads`;
        waits for the env's stream)."""
        out = {k: np.empty(shape, np.float32) for k, shape in zip(L.HEAD_KEYS, L.HEAD_SHAPES)}
        h = L.RcPolicyHeads()
        h.struct_size = C.sizeof(L.RcPolicyHeads)
        for k, a in out.items():
            arr = getattr(h, k)
            arr.data = a.ctypes.data
            arr.rows, arr.cols = (1, a.shape[0]) if a.ndim == 1 else a.shape
        self._enter()
        try:
            L.check(self._lib.rc_policy_read_heads(self._h, C.byref(h)))
        finally:
            self._exit()
        return out

    def load_reward_head(self, weights) -> None:
        """Replace the reward head alone (`rc_policy_load_heads`): a mapping (or an .npz path) with `reward_h0_w` .. `reward_hout_b`.
        The policy, the latents and the critic stay as they are; the reward optimizer is closed."""
        heads = L.policy_heads(weights)
        if heads is None:
            raise KeyError("reward head weights lack the reward_* arrays")
        self._enter()
        try:
            L.check(self._lib.rc_policy_load_heads(self._h, C.byref(heads[0])))
        finally:
            self._exit()
        self._policy_has_head = True

    # ---- the actor's own fit (rc_policy_fit_begin / _end with RC_POLICY_FIT_ACTOR, rc_policy_actor_*)
    def _actor_fit(self, feat, t, gfeat, status, hyper) -> int:
        ptr = lambda x: None if x is None else x.data_ptr()
        a = L.RcPolicyActorFitArgs(C.sizeof(L.RcPolicyActorFitArgs), feat.shape[0], feat.data_ptr(), ptr(t["eps"]), ptr(t["weight"]),
                                   ptr(t["target"]), ptr(t["grad"]), ptr(gfeat), hyper["lr"], hyper["clip"], hyper["beta1"], hyper["beta2"],
                                   hyper["epsilon"], ptr(status))
        return self._lib.rc_policy_actor_fit_step(self._h, C.byref(a))

    def actor_fit_begin(self) -> None:
        """Open the optimizer of the loaded actor (`rc_policy_fit_begin`, RC_POLICY_FIT_ACTOR): Adam moments zero, step 0.
        Independent of the other optimizers; `load_actor`, `load_policy` and `unload_policy` close it.  The plain actor only: a
        checkpoint with `hnorm_*` arrays ("normalized") is refused."""
        cfg = L.RcPolicyFitConfig(C.sizeof(L.RcPolicyFitConfig), L.FIT_ACTOR)
        self._enter()
        try:
            L.check(self._lib.rc_policy_fit_begin(self._h, C.byref(cfg)))
        finally:
            self._exit()

    def actor_fit(self, features: torch.Tensor, target: Optional[torch.Tensor] = None, grad_actions: Optional[torch.Tensor] = None,
                  eps: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None, grad_features: bool = False,
                  lr: float = 8e-5, clip: float = 1.0, beta1: float = 0.9, beta2: float = 0.999,
                  epsilon: float = 1e-7) -> Dict[str, torch.Tensor]:
        """One step of the actor's optimizer on the device (`rc_policy_actor_fit_step`; the reference's ActionDecoder,
        dreamer/models.py:535-560, under actor_opt, dreamer/dream.py:87-88): the actor's forward pass on `features` [..., 230] =
        stoch | deter, the action act = tanh(mean + std * eps) (`eps` [..., 2] standard normal draws, or None: the mode action),
        then its backward pass from EITHER `target` [..., 2] raw actions in [-1, 1] - loss = mean(weight * 0.5 * |act - target|^2)
        - OR `grad_actions` [..., 2], the gradient of a loss of the caller's with respect to act (times `weight`; the reported loss
        is then 0); the global-norm clip (`clip` 0: none) and Adam, all in the env's stream: no synchronisation, no host copy.
        The defaults are the reference's actor_lr and grad_clip and TF's Adam.  Returns device scalars `loss`, `grad_norm`
        (before the clip), `skipped`, `step`, and with `grad_features` the gradient with respect to the features [..., 230]
        (before the clip, of the same loss).  The fitted actor is what `policy_act` (every mode), `policy_imagine`,
        `policy_returns` and `policy_action` read next; nothing else moves.  The closed-loop gradient through the dream is not
        computed here."""
        feat, t, gfeat, gshape, status = _actor_fit_setup(self, features, target, grad_actions, eps, weight, grad_features)
        hyper = dict(lr=lr, clip=clip, beta1=beta1, beta2=beta2, epsilon=epsilon)
        self._enter()
        try:
            L.check(self._actor_fit(feat, t, gfeat, status, hyper))
        finally:
            self._exit()
        out = _fit_status(status)
        if gfeat is not None:
            out["grad_features"] = gfeat.reshape(gshape)
        return out

    def actor_fit_end(self) -> None:
        """Free the actor optimizer's state (`rc_policy_fit_end`); the fitted actor stays loaded."""
        L.check(self._lib.rc_policy_fit_end(self._h, L.FIT_ACTOR))

    def _actor_forward(self, feat, eps, tensors) -> int:
        a = L.RcPolicyActorForwardArgs(C.sizeof(L.RcPolicyActorForwardArgs), feat.shape[0], feat.data_ptr(), None if eps is None else eps.data_ptr())
        for name, t in tensors.items():
            setattr(a, name, t.data_ptr())
        return self._lib.rc_policy_actor_forward(self._h, C.byref(a))

    def policy_action(self, features: torch.Tensor, eps: Optional[torch.Tensor] = None, outputs=("action",)) -> Dict[str, torch.Tensor]:
        """The actor on given features (`rc_policy_actor_forward`, one launch): `features` float32 [..., 230] = stoch | deter,
        e.g. `policy_state[:, :230]`; `eps` [..., 2] standard normal draws or None for the mode action, which is byte for byte
        what `policy_act` writes in mode "mean" for the same feature.  `outputs` among "action" (raw, in [-1, 1]), "mean", "std"
        (of the normal under the tanh); each comes back as a device float32 tensor [..., 2]."""
        names = tuple(outputs)
        unknown = [n for n in names if n not in L.ACTOR_OUTPUTS]
        if unknown or not names:
            raise ValueError(f"policy_action outputs must be among {sorted(L.ACTOR_OUTPUTS)}, got {list(names)}")
        feat, lead, t = _actor_rows(self, features, dict(eps=eps), {})
        tensors = {n: torch.empty((feat.shape[0], 2), dtype=torch.float32, device=self.device) for n in names}
        self._enter()
        try:
            L.check(self._actor_forward(feat, t["eps"], tensors))
        finally:
            self._exit()
        return {n: v.reshape(lead + (2,)) for n, v in tensors.items()}

    def actor_weights(self) -> Dict[str, np.ndarray]:
        """The loaded actor as NumPy arrays under `ACTOR_KEYS` (`h0_w` .. `hout_b`, the checkpoint's names), as `load_actor`
        takes them (`rc_policy_read_actor`; waits for the env's stream)."""
        out = {k: np.empty(shape, np.float32) for k, shape in zip(L.ACTOR_KEYS, L.ACTOR_SHAPES)}
        h = L.RcPolicyActor()
        h.struct_size = C.sizeof(L.RcPolicyActor)
        for k, a in out.items():
            arr = getattr(h, k)
            arr.data = a.ctypes.data
            arr.rows, arr.cols = (1, a.shape[0]) if a.ndim == 1 else a.shape
        self._enter()
        try:
            L.check(self._lib.rc_policy_read_actor(self._h, C.byref(h)))
        finally:
            self._exit()
        return out

    def load_actor(self, weights) -> None:
        """Replace the actor alone (`rc_policy_load_actor`): a mapping (or an .npz path) with `h0_w` .. `hout_b`.  The RSSM, the
        heads, the critic and the latents stay as they are; the actor's optimizer is closed."""
        actor = L.policy_actor(weights)
        self._enter()
        try:
            L.check(self._lib.rc_policy_load_actor(self._h, C.byref(actor[0])))
        finally:
            self._exit()

    @property
    def policy_has_decoder(self) -> bool:
        """Whether the loaded checkpoint brought a LidarOccupancyDecoder (`dec_*` arrays): `policy_decode` needs one."""
        return bool(getattr(self, "_policy_has_decoder", False))

    def _decode(self, features, mask: int, tensors: dict, lo: int, hi: int) -> int:
        """rc_policy_decode on this handle: of `features` [rows, 230] into the whole tensors, or (features None) of this handle's live
        latents into rows [lo, hi) of the tensors (one row per car)."""
        a = L.RcPolicyDecodeArgs(C.sizeof(L.RcPolicyDecodeArgs))
        if features is not None:
            a.features, a.rows, lo, hi = features.data_ptr(), features.shape[0], 0, features.shape[0]
        a.slot_mask = mask
        for field, t in tensors.items():
            setattr(a, field, None if t is None else t[lo:hi].data_ptr())
        return self._lib.rc_policy_decode(self._h, C.byref(a))

    def policy_decode(self, features: Optional[torch.Tensor] = None, slots=None, logits: bool = False, image: bool = True,
                      mismatch: bool = False, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """What the world model believes the car sees (`rc_policy_decode`, one launch): the reference's LidarOccupancyDecoder on
        every car's latent as `policy_act` last left it - the reconstruction - or on `features`, a device float32 [..., 230] =
        stoch | deter such as `policy_imagine(features=True)["feature"]` - the open-loop prediction; the leading dimensions
        are kept.  Returns device tensors: `logits` float32 [..., 64, 64] (the Bernoulli logits, >= 0), `image` uint8
        [..., 64, 64] = logits > 0 in the encoding of `lidar_occupancy` (1 = drivable), `mismatch` int32 [n_cars] = the number
        of pixels in which the image differs from the car's current `lidar_occupancy` (live latents, obs_type lidar_occupancy*).
        Nothing else changes.  With `slots` (live latents), rows of the other cars are zero - or what `out` (tensors to write
        into, by the same names) held."""
        feats, mask, tensors, result = _decode_setup(self, features, slots, logits, image, mismatch, out)
        self._enter()
        try:
            L.check(self._decode(feats, mask, tensors, 0, self.n_cars))
        finally:
            self._exit()                 # a refused call still orders torch's stream after the env's
        return result

    def _decode_loglik(self, features, mask: int, target, tensors: dict, lo: int, hi: int) -> int:
        """rc_policy_decode_loglik on this handle, as `_decode`."""
        a = L.RcPolicyDecodeLoglikArgs(C.sizeof(L.RcPolicyDecodeLoglikArgs))
        if features is not None:
            a.features, a.rows, lo, hi = features.data_ptr(), features.shape[0], 0, features.shape[0]
        a.slot_mask = mask
        a.target = None if target is None else target[lo:hi].data_ptr()
        for field, t in tensors.items():
            setattr(a, field, None if t is None else t[lo:hi].data_ptr())
        return self._lib.rc_policy_decode_loglik(self._h, C.byref(a))

    def policy_decode_loglik(self, target: Optional[torch.Tensor] = None, features: Optional[torch.Tensor] = None, slots=None,
                             outputs=("loglik",), out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """The LidarOccupancyDecoder's log-probability of an occupancy image (`rc_policy_decode_loglik`, one launch): `loglik`
        float32 [...] = the sum over the 64 x 64 pixels of x logit - softplus(logit), on `features` [..., 230] against `target`
        uint8 [..., 64, 64] (1 = drivable), or on every car's live latent against its own current `lidar_occupancy` (`target`
        stays None; obs_type lidar_occupancy*).  `outputs` may also name `logits` and `image`, as `policy_decode` returns them,
        from the same launch.  Nothing else changes; `slots` and `out` as `policy_decode`'s."""
        feats, mask, tgt, tensors, result = _decode_loglik_setup(self, target, features, slots, outputs, out)
        self._enter()
        try:
            L.check(self._decode_loglik(feats, mask, tgt, tensors, 0, self.n_cars))
        finally:
            self._exit()                 # a refused call still orders torch's stream after the env's
        return result

    def load_lidar_decoder(self, weights) -> None:
        """Load a LidarDistanceDecoder beside the loaded policy (`rc_policy_load_lidar_decoder`): a mapping (or an .npz path) with
        `ldec_dense1_w` [230, 256], `ldec_dense1_b` [256], `ldec_dense2_w` [256, 512], `ldec_dense2_b` [512], `ldec_params_w`
        [512, 2160], `ldec_params_b` [2160] - `decoder.init_lidar_decoder` makes a synthetic one,
        `decoder.lidar_decoder_from_variables` picks a trained one out of the reference's `variables.pkl`.  None drops it; so do
        `load_policy` and `unload_policy`.  Shapes are checked by the library."""
        if weights is None:
            L.check(self._lib.rc_policy_load_lidar_decoder(self._h, None))
            self._policy_has_lidar_decoder = False
            return
        dec = L.policy_lidar_decoder(weights)
        if dec is None:
            raise KeyError("decoder weights lack the ldec_* arrays")
        L.check(self._lib.rc_policy_load_lidar_decoder(self._h, C.byref(dec[0])))
        self._policy_has_lidar_decoder = True

    @property
    def policy_has_lidar_decoder(self) -> bool:
        """Whether a LidarDistanceDecoder is loaded (`ldec_*` arrays): `policy_decode_lidar` needs one."""
        return bool(getattr(self, "_policy_has_lidar_decoder", False))

    def _decode_lidar(self, features, mask: int, target, tensors: dict, lo: int, hi: int) -> int:
        """rc_policy_decode_lidar on this handle: of `features` [rows, 230] into the whole tensors, or (features None) of this
        handle's live latents into rows [lo, hi) of the tensors (one row per car)."""
        a = L.RcPolicyDecodeLidarArgs(C.sizeof(L.RcPolicyDecodeLidarArgs))
        if features is not None:
            a.features, a.rows, lo, hi = features.data_ptr(), features.shape[0], 0, features.shape[0]
        a.slot_mask = mask
        a.target = None if target is None else target[lo:hi].data_ptr()
        for field, t in tensors.items():
            setattr(a, field, None if t is None else t[lo:hi].data_ptr())
        return self._lib.rc_policy_decode_lidar(self._h, C.byref(a))

    def policy_decode_lidar(self, features: Optional[torch.Tensor] = None, slots=None, target: Optional[torch.Tensor] = None,
                            outputs=("mean",), out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """What scan the world model expects (`rc_policy_decode_lidar`, one launch): the reference's LidarDistanceDecoder on every
        car's latent as `policy_act` last left it, or on `features`, a device float32 [..., 230] = stoch | deter such as
        `policy_observe(...)["feature"]` or `policy_imagine(features=True)["feature"]`; the leading dimensions are kept.
        `outputs` among `mean`, `std` float32 [..., 1080] - loc and scale of the Normal over the beams, in the model's units
        scan_m / 15 - 0.5 - and `loglik` float32 [...], the log-probability of `target` float32 [..., 1080] in METRES (given
        features), or of the car's own current `lidar` (live latents; `target` stays None).  Nothing else changes.  With `slots`
        (live latents), rows of the other cars are zero - or what `out` (tensors to write into, by the same names) held."""
        feats, mask, tgt, tensors, result = _decode_lidar_setup(self, features, slots, target, outputs, out)
        self._enter()
        try:
            L.check(self._decode_lidar(feats, mask, tgt, tensors, 0, self.n_cars))
        finally:
            self._exit()                 # a refused call still orders torch's stream after the env's
        return result

    @property
    def policy_has_reward_head(self) -> bool:
        """Whether the loaded checkpoint brought a reward head (`reward_*` arrays): `policy_imagine` then returns rewards."""
        return bool(getattr(self, "_policy_has_head", False))

    def policy_observe(self, lidar: torch.Tensor, action: torch.Tensor, context: Optional[int] = None, mode: str = "mean", seed: int = 0,
                       state: Optional[torch.Tensor] = None, row_offset: int = 0, outputs=("feature",),
                       out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """The world model over RECORDED sequences (`rc_policy_observe`, one launch): the reference's `RSSM.observe` on `lidar`
        float32 [..., T, 1080] in metres and `action` float32 [..., T, 2], as `TrajectoryRing.sample(...)["lidar"]` / `["action"]`
        give them; T <= 64, the leading dimensions are kept in the results.  `action[..., t, :]` is the action that led to scan t
        (a window's first row after a reset carries action 0) and must be RAW, in [-1, 1] (values outside are clamped): that is
        what a ring records when the env was built with `remap_actions=True`.  An env built with it off records the remapped
        commands - convert them back before calling; nothing here converts silently.  Steps t < `context` (default: all) see
        their scan - the posterior -, the steps after it run the prior under the recorded actions: `context=5` is the
        reference's "observe 5, imagine the rest" summary.  mode "mean": stoch' = the mean, what `policy_act` computes step by
        step; "sample": stoch' ~ Normal(mean, std), a function of (seed, row_offset + row, t) only, so two shards of a batch
        called with their `row_offset` reproduce the whole.  `state` [..., 232] = stoch | deter | (2 unused) is the start
        state; None is `RSSM.initial`'s zeros.  `outputs` names what to compute, each a device float32 tensor: `feature`
        [..., T, 230] = stoch | deter, `post_mean`, `post_std`, `prior_mean`, `prior_std` [..., T, 30], `kl` [..., T] =
        KL(post || prior), `reward` [..., T] (the reward head on `feature`; needs a checkpoint with one), `state` [..., 232] =
        the last stoch | deter | action, in `policy_state`'s layout.  `post_*` and `kl` are written for t < context only: the
        entries after it are uninitialised - or what `out` (tensors to write into, by the same names) held.  Nothing else
        changes: not the agent's state, not `action_in`."""
        a, keep, result = _observe_setup(self, lidar, action, context, mode, seed, state, row_offset, outputs, out)
        self._enter()
        try:
            L.check(self._lib.rc_policy_observe(self._h, C.byref(a)))
        finally:
            self._exit()                 # a refused call still orders torch's stream after the env's
        del keep
        return result

    def _imagine(self, args: dict, tensors: dict, lo: int, hi: int) -> int:
        """rc_policy_imagine on this handle, reading and writing rows [lo, hi) of the tensors (one row per car)."""
        a = L.RcPolicyImagineArgs(C.sizeof(L.RcPolicyImagineArgs), args["horizon"], args["mode"], args["mask"], args["seed"])
        for field, t in tensors.items():
            setattr(a, field, None if t is None else t[lo:hi].data_ptr())
        return self._lib.rc_policy_imagine(self._h, C.byref(a))

    def policy_imagine(self, horizon: int = 15, mode: str = "mean", seed: int = 0, actions: Optional[torch.Tensor] = None, slots=None,
                       features: bool = False, start_reward: bool = False, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """Roll the world model `horizon` steps ahead from every car's latent as `policy_act` last left it (`rc_policy_imagine`,
        one launch): under the actor's own actions (the reference's `_imagine_ahead`), or under `actions` float32
        [n_cars, horizon, 2] raw in [-1, 1] (`RSSM.imagine`, open loop; clamped).  mode "mean": tanh of the actor's mean and the
        prior's mean; "sample": one tanh-normal action draw and a sampled prior, a function of (seed, global env id, slot,
        episode, agent step, t) only.  Returns device tensors: `action` [n_cars, horizon, 2], `reward` [n_cars, horizon] (when
        the checkpoint has a reward head), `feature` [n_cars, horizon, 230] = stoch | deter (features=True), `reward_start`
        [n_cars] = the head on the starting latent (start_reward=True).  Nothing else changes: not the agent's state, not
        `action_in`.  With `slots`, rows of the other cars are zero - or what `out` (tensors to write into, by the same names)
        held."""
        args, tensors, result = _imagine_setup(self, horizon, mode, seed, actions, slots, features, start_reward, out)
        self._enter()
        try:
            L.check(self._imagine(args, tensors, 0, self.n_cars))
        finally:
            self._exit()                 # a refused call still orders torch's stream after the env's
        return result

    def _dream_ahead(self, args: dict, tensors: dict, lo: int, hi: int) -> int:
        """rc_policy_dream_ahead on this handle: from its live latents, reading and writing rows [lo, hi) of the tensors (one row per
        car), or from a given state, the whole tensors."""
        a = L.RcPolicyDreamAheadArgs(C.sizeof(L.RcPolicyDreamAheadArgs), args["horizon"], args["mode"], args["candidates"], args["mask"],
                                     args["discount"], args["seed"], args["starts"], args["row_offset"])
        for field, t in tensors.items():
            setattr(a, field, None if t is None else (t[lo:hi] if args["live"] else t).data_ptr())
        return self._lib.rc_policy_dream_ahead(self._h, C.byref(a))

    def dream_ahead(self, actions: torch.Tensor, mode: str = "mean", seed: int = 0, state: Optional[torch.Tensor] = None, row_offset: int = 0,
                    slots=None, discount: float = 1.0, outputs=("return",), out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """Plan in the dream (`rc_policy_dream_ahead`, one launch): `actions` float32 [S, K, H, 2] raw in [-1, 1] (clamped) holds K
        candidate sequences of H steps per start latent; every one is carried through the world model open loop, exactly as
        `policy_imagine(actions=...)` would carry it, and scored by the reward head - `look_ahead`'s counterpart in the latent.
        The starts are every car's latent as `policy_act` last left it (S = n_cars; with `slots`, rows of the other cars are
        zero - or what `out` held), or `state` float32 [S, 232] = stoch | deter | (2 unused) in `policy_state`'s layout, e.g.
        `policy_observe(..., outputs=("state",))["state"]`: observe a replay window, then plan from its end.  mode "mean": the
        prior's mean; "sample": stoch' ~ Normal(mean, std), a function of (seed, start id, candidate, t) only - the start id is
        the global car id, or `row_offset` + the row of `state`, so shards of a batch reproduce the whole.  `outputs` names
        what to compute, each a device float32 tensor: `return` [S, K] = sum_t discount^t reward_t, `reward` [S, K, H],
        `final_feature` [S, K, 230] = stoch | deter after the last step (for a value head of the caller's).  `return` and
        `reward` need a checkpoint with a reward head.  Nothing else changes: not the agent's state, not `action_in`."""
        args, tensors, result = _dream_setup(self, actions, mode, seed, state, row_offset, slots, discount, outputs, out)
        self._enter()
        try:
            L.check(self._dream_ahead(args, tensors, 0, self.n_cars))
        finally:
            self._exit()                 # a refused call still orders torch's stream after the env's
        return result

    def _dream_grad(self, args: dict, tensors: dict, lo: int, hi: int) -> int:
        """rc_policy_dream_grad on this handle: rows as `_dream_ahead` takes them."""
        a = L.RcPolicyDreamGradArgs(C.sizeof(L.RcPolicyDreamGradArgs), args["horizon"], args["mode"], args["candidates"], args["mask"],
                                    args["discount"], args["seed"], args["starts"], args["row_offset"], args["chunk_rows"])
        for field, t in tensors.items():
            setattr(a, field, None if t is None else (t[lo:hi] if args["live"] else t).data_ptr())
        return self._lib.rc_policy_dream_grad(self._h, C.byref(a))

    def dream_ahead_grad(self, actions: torch.Tensor, mode: str = "mean", seed: int = 0, state: Optional[torch.Tensor] = None, row_offset: int = 0,
                         slots=None, discount: float = 1.0, outputs=("grad_actions", "return"), out: Optional[Dict[str, torch.Tensor]] = None,
                         chunk_rows: int = 0) -> Dict[str, torch.Tensor]:
        """The gradient of `dream_ahead`'s return (`rc_policy_dream_grad`): `actions`, `mode`, `seed`, `state`, `row_offset`, `slots`
        and `discount` are `dream_ahead`'s, and so are `return` [S, K] and `reward` [S, K, H], byte for byte.  `grad_actions`
        [S, K, H, 2] is d return / d actions - exactly zero where the raw action lies outside [-1, 1], where `dream_ahead` clamps
        it -, `grad_state` [S, K, 230] is d return / d (stoch | deter) of the start.  In mode "sample" the step's normals are
        held fixed (the reparameterised gradient).  The forward's activations are kept in a scratch the env owns (at most
        1 GiB, released with the policy); the rows go through it in chunks of `chunk_rows` (0: as many as fit), one launch per
        chunk, and the results do not depend on the chunking.  Needs a checkpoint with a reward head.  Nothing else changes."""
        args, tensors, result = _dream_setup(self, actions, mode, seed, state, row_offset, slots, discount, outputs, out, L.DREAM_GRAD_OUTPUTS,
                                             "dream_ahead_grad")
        args["chunk_rows"] = _chunk_rows(chunk_rows)
        self._enter()
        try:
            L.check(self._dream_grad(args, tensors, 0, self.n_cars))
        finally:
            self._exit()                 # a refused call still orders torch's stream after the env's
        return result

    def _look_ahead(self, args: dict, tensors: dict, lo: int, hi: int) -> int:
        """rc_look_ahead on this handle, reading and writing rows [lo, hi) of the tensors (one row per env)."""
        a = L.RcLookAheadArgs(C.sizeof(L.RcLookAheadArgs), args["candidates"], args["horizon"], args["repeat"])
        for field, t in tensors.items():
            setattr(a, field, t[lo:hi].data_ptr())
        return self._lib.rc_look_ahead(self._h, C.byref(a))

    def look_ahead(self, actions: torch.Tensor, repeat: Optional[int] = None, outputs=("reward", "flags", "return", "length"),
                   out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """What would really happen from here under these actions (`rc_look_ahead`, one launch): `actions` float32
        [num_envs, K, H, cars_per_env, 2] (or [num_envs, K, H, 2] with one car per env) holds K candidate sequences of H agent
        steps per env in `step`'s convention; every one is carried through the true dynamics from the env's live state, exactly
        as `step(actions, repeat)` on an env without auto-reset would - a finished env is frozen: reward +0.0, flags kept, no
        reset.  The env is not touched: no state, no view, not `action_in`, not the episode log, not the agent's latent.
        `repeat=None`: the env's default, as `step`.  Returns device tensors by name, those of `outputs`: `reward` float32
        [E, K, H, A], `flags` uint8 [E, K, H, A] (bit 0 done, 1 truncated, 2 wall, 3 opponent, 4 wrong_way, after step t), `return`
        float32 [E, K, A], `length` int32 [E, K] (steps until the env finished, that step counted; H if it did not; 0 if it
        was), `final_state` float32 [E, K, A, 8] (x, y, theta, v, delta, omega, lap - 1 + progress, time), `pose` float32
        [E, K, H, A, 3].  `out`: tensors to write into, by the same names."""
        args, tensors, result = _look_ahead_setup(self, actions, self.action_repeat if repeat is None else repeat, outputs, out)
        self._enter()
        try:
            L.check(self._look_ahead(args, tensors, 0, self.num_envs))
        finally:
            self._exit()
        return result

    def look_ahead_time(self):
        """(total ms, launches) of `look_ahead`'s kernel while profiling is on (behind `kernel_times()`, whose keys stay as they are)."""
        ms, n = C.c_double(), C.c_uint64()
        L.check(self._lib.rc_look_ahead_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    def policy_act(self, slots=None) -> torch.Tensor:
        """One step of the loaded agent, in the mode of `set_policy_sampling` (deterministic by default), for every car (or the cars in the listed slots = car indices within
        an env, e.g. `slots=(1, 2, 3)`: trained opponents B-D next to a learner in slot A): reads `lidar` and `fresh` in place,
        fills and returns `action_in` in this env's action convention, so `step(None)` applies it."""
        mask = (1 << self.cars_per_env) - 1 if slots is None else sum({1 << int(a) for a in slots})
        self._enter()
        L.check(self._lib.rc_policy_act(self._h, C.c_uint32(mask)))
        self._exit()
        return self.views["action_in"]

    def set_policy_sampling(self, mode: str = "mean", seed: int = 0, expl_amount: Optional[float] = None) -> None:
        """How `policy_act` runs the loaded agent from now on (`rc_policy_set_sampling`; `load_policy` resets it to "mean"):
        "mean" - posterior mean, tanh(mean), deterministic; "deploy" - the reference's deployed / evaluation agent: sampled
        posterior, the most probable of 100 action draws (racing_dreamer.py:61-80, tools.py:301-321); "explore" - its
        training-time collector: sampled posterior, one action draw, additive Gaussian noise of standard deviation
        `expl_amount`, clipped (models.py:189-202).  `expl_amount=None`: 0 for "deploy", 0.3 for "explore".  The draws depend
        on (seed, global env id, slot, episode, agent step) only."""
        if mode not in L.POLICY_MODES:
            raise ValueError(f"policy sampling mode must be one of {sorted(L.POLICY_MODES)}, got {mode!r}")
        amount = L.POLICY_EXPL_DEFAULT[mode] if expl_amount is None else float(expl_amount)
        s = L.RcPolicySampling(C.sizeof(L.RcPolicySampling), L.POLICY_MODES[mode], int(seed) & (2 ** 64 - 1), amount)
        L.check(self._lib.rc_policy_set_sampling(self._h, C.byref(s)))

    @property
    def policy_sampling(self) -> dict:
        """dict(mode, seed, expl_amount) as installed (`rc_policy_get_sampling`)."""
        s = L.RcPolicySampling()
        L.check(self._lib.rc_policy_get_sampling(self._h, C.byref(s)))
        return dict(mode={v: k for k, v in L.POLICY_MODES.items()}[s.mode], seed=int(s.seed), expl_amount=float(s.expl_amount))

    @property
    def policy_state(self) -> torch.Tensor:
        """Device view float32 [n_cars, 232] = stoch 30 | deter 200 | raw previous action 2 of the loaded agent: readable and
        writable between calls (on the env's stream, or after `sync()`)."""
        if getattr(self, "_policy_state", None) is None:
            raise L.RacecarHipError("no policy loaded (load_policy)")
        return self._policy_state

    def unload_policy(self) -> None:
        self._policy_state = None
        self._policy_has_head = False
        self._policy_has_decoder = False
        self._policy_has_lidar_decoder = False
        self._policy_has_value = self._policy_has_pcont = False
        L.check(self._lib.rc_policy_unload(self._h))

    # ------------------------------------------------------------------ episode log (include/racecar_hip.h, rc_episode_log_*)
    def enable_episode_log(self, capacity: int, max_episodes: int = 0) -> None:
        """Keep return, length, progress and time of every episode on the device (the reference's summarize_episode,
        dreamer/callbacks.py:56-100): per-car running sums and, in the call in which an env's episode ends, one row per car appended
        to a buffer of `capacity` rows in (call, env, slot) order.  `max_episodes` > 0: only each env's first `max_episodes`
        episodes get rows.  An env is followed from its next reset on (enabled mid-episode, nothing is logged for the partial
        episode).  Called again: clears, and resizes if the capacity differs."""
        L.check(self._lib.rc_episode_log_enable(self._h, C.c_int64(int(capacity)), int(max_episodes)))
        rows, cap, ctr, nb = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        L.check(self._lib.rc_episode_log(self._h, C.byref(rows), C.byref(cap), C.byref(ctr), C.byref(nb)))
        words = C.sizeof(L.RcEpisodeRow) // 4
        arrays = (_BorrowedDeviceArray(rows.value, (cap.value, words), self.device, code=0),
                  _BorrowedDeviceArray(ctr.value, (nb.value // 4,), self.device, code=0))
        # (the DLPack descriptors of earlier enables stay alive with the env: a caller may still hold views made from them)
        self._ep_arrays = getattr(self, "_ep_arrays", None) or []
        self._ep_arrays.extend(arrays)
        self._ep_rows = torch.utils.dlpack.from_dlpack(arrays[0])           # int32 [capacity, 12]: a structured view
        self._ep_counters = torch.utils.dlpack.from_dlpack(arrays[1])

    def _ep_check(self) -> None:
        if getattr(self, "_ep_rows", None) is None:
            raise L.RacecarHipError("the episode log is not enabled (enable_episode_log)")

    @property
    def episode_counters(self) -> Dict[str, int]:
        """written, dropped, skipped (rows), abandoned (episodes), envs_at_quota (envs), calls: one synchronising host read."""
        self._ep_check()
        self._enter()
        with torch.cuda.stream(self.stream):
            host = self._ep_counters.cpu().numpy()
        return dict(zip(L.EPISODE_COUNTERS, (int(v) for v in host.view(np.uint64))))

    @property
    def episode_rows(self) -> torch.Tensor:
        """The whole row buffer as int32 [capacity, 12] (48-byte rc_episode_row per row), zero-copy."""
        self._ep_check()
        return self._ep_rows

    def episode_log(self, clear: bool = False) -> Dict[str, torch.Tensor]:
        """The rows written so far as device tensors [written] named as rc_episode_row's fields - env, slot, track, episode, call,
        length, laps, flags (int32 views; flags: L.EP_WALL / EP_OPPONENT / EP_TRUNCATED / EP_WRONG_WAY / EP_OWN_DONE) and ret,
        progress, time (float32) - in (call, env, slot) order.  One host read (the counter); the columns are zero-copy strided
        views of the row buffer, valid until the log is cleared or resized (clear=True returns copies, then clears)."""
        n = self.episode_counters["written"]
        rows = self._ep_rows[:n]
        out = {}
        for k, (name, ctype) in enumerate(L.RcEpisodeRow._fields_):
            if name == "reserved":
                continue
            col = rows[:, k:k + 1]
            out[name] = (col.view(torch.float32) if ctype is C.c_float else col)[:, 0]
        if clear:
            with torch.cuda.stream(self.stream):
                out = {k: v.clone() for k, v in out.items()}
            self.clear_episode_log()
        return out

    def clear_episode_log(self) -> None:
        """Rows, counters and ordinals to zero (stream-ordered); running episodes keep their sums."""
        self._ep_check()
        self._enter()
        L.check(self._lib.rc_episode_log_clear(self._h))
        self._exit()

    def disable_episode_log(self) -> None:
        self._ep_rows = self._ep_counters = None
        L.check(self._lib.rc_episode_log_disable(self._h))

    def episode_log_time(self):
        """(total ms, steps) between events around the log's launches, summed over the steps taken while profiling was on."""
        ms, n = C.c_double(), C.c_uint64()
        L.check(self._lib.rc_episode_log_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    def fill_random_actions(self, seed: int, step: int) -> None:
        L.check(self._lib.rc_fill_random_actions(self._h, C.c_uint64(seed), C.c_uint32(step)))

    # ------------------------------------------------------------------ profiling
    def set_profiling(self, on, kernels=None) -> None:
        """HIP-event timing of the kernels: on/off, or only the listed kernel ids (L.K_*)."""
        mask = int(bool(on))
        if on and kernels is not None:
            mask = 0
            for k in kernels:
                mask |= 1 << k
            mask |= 1 << 31 if mask == 1 else 0      # keep a single-kernel mask distinct from "1 = all"
        L.check(self._lib.rc_set_profiling(self._h, mask))

    def reset_kernel_times(self) -> None:
        L.check(self._lib.rc_reset_kernel_times(self._h))

    def kernel_times(self) -> Dict[str, Dict[str, float]]:
        out = {}
        for k, name in L.KERNEL_NAMES.items():
            ms, n = C.c_double(), C.c_uint64()
            L.check(self._lib.rc_kernel_time(self._h, k, C.byref(ms), C.byref(n)))
            out[name] = {"total_ms": ms.value, "launches": int(n.value),
                         "avg_ms": ms.value / n.value if n.value else 0.0}
        return out

    @property
    def arena_nbytes(self) -> int:
        return int(self._arena_view.numel())

    def views_of(self, arena: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Typed views [num_envs, cars_per_env, ...] of every output field inside another arena-sized uint8 buffer."""
        out = {}
        for name, (off, nb, dtype, tail) in self._host_layout.items():
            out[name] = arena[off:off + nb].view(getattr(torch, dtype)).view(self.num_envs, self.cars_per_env, *tail)
        return out

    def set_arena(self, arena: Optional[torch.Tensor], views: Optional[Dict[str, torch.Tensor]] = None) -> None:
        """Re-point the outputs of the following reset()/step() calls at `arena` (uint8, >= arena_nbytes, 64-byte
        aligned, on the env's device); None = back to the env's own arena.  `action_in` stays where it is.  This is
        how `replay.TrajectoryRing` records trajectories on the device without copies."""
        if arena is None:
            L.check(self._lib.rc_set_arena(self._h, None, 0))
            self.views = self._own_views
            return
        if arena.dtype != torch.uint8 or arena.device != self.device or not arena.is_contiguous():
            raise ValueError("arena must be a contiguous uint8 tensor on the env's device")
        L.check(self._lib.rc_set_arena(self._h, arena.data_ptr(), arena.numel()))
        new = dict(views) if views is not None else self.views_of(arena)
        new["action_in"] = self._own_views["action_in"]
        self.views = new

    def gather_rows(self, ring: torch.Tensor, slot_bytes: int, slots: torch.Tensor, cars: torch.Tensor, names) -> Dict[str, torch.Tensor]:
        """`rc_gather_rows`: for every row r the record of car `cars[r]` in ring slot `slots[r]` (int32 device tensors),
        the fields `names`, as one launch.  Returns name -> tensor [rows, ...] (views of one fresh buffer)."""
        unknown = [n for n in names if not (n in _FIELD_VIEWS and n != "action_in" and n in self._host_layout)]
        if unknown:
            raise ValueError(f"fields {unknown} are not recorded by this env")
        order = sorted(names, key=lambda n: _FIELD_VIEWS[n][0])
        mask = 0
        for n in order:
            mask |= 1 << _FIELD_VIEWS[n][0]
        rows = int(slots.numel())
        nbytes = int(self._lib.rc_gather_rows_bytes(self._h, mask, rows))
        out = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        slots = slots.to(torch.int32).contiguous()
        cars = cars.to(torch.int32).contiguous()
        self._enter()
        L.check(self._lib.rc_gather_rows(self._h, ring.data_ptr(), int(slot_bytes), slots.data_ptr(), cars.data_ptr(), rows, mask,
                                         out.data_ptr(), nbytes))
        self._exit()
        res, off = {}, 0
        for n in order:
            fid, dtype, tail = _FIELD_VIEWS[n]
            per = self._host_layout[n][1] // self.n_cars
            res[n] = out[off:off + per * rows].view(dtype).view(rows, *tail)
            off = (off + per * rows + 63) // 64 * 64
        return res

    def sample_windows(self, ring: torch.Tensor, slot_bytes: int, capacity: int, oldest: int, count: int, length: int,
                       n_windows: int, seed: int, draw: int, max_tries: int = 16) -> Dict[str, torch.Tensor]:
        """`rc_sample_windows`: window starts of a replay sampler drawn on the device - no host round trip.  Returns int32
        device tensors `slots`, `slots_obs`, `cars` [n_windows * length] (rows for `gather_rows`), `meta` [n_windows, 4] =
        (t0, car, terminal, first) and `failed` [1] (windows that found no episode-internal start in `max_tries` draws)."""
        i32 = dict(dtype=torch.int32, device=self.device)
        out = dict(slots=torch.empty(n_windows * length, **i32), slots_obs=torch.empty(n_windows * length, **i32),
                   cars=torch.empty(n_windows * length, **i32), meta=torch.empty((n_windows, 4), **i32),
                   failed=torch.zeros(1, dtype=torch.int32, device=self.device))
        self._enter()
        L.check(self._lib.rc_sample_windows(self._h, ring.data_ptr(), int(slot_bytes), int(capacity), int(oldest), int(count),
                                            int(length), int(n_windows), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint32(int(draw) & 0xffffffff),
                                            int(max_tries), out["slots"].data_ptr(), out["slots_obs"].data_ptr(),
                                            out["cars"].data_ptr(), out["meta"].data_ptr(), out["failed"].data_ptr()))
        self._exit()
        return out

    def sample_batch_layout(self, names, n_windows: int, length: int) -> Dict[str, object]:
        """Layout of the ONE buffer `sample_batch` fills (include/racecar_hip.h, rc_sample_batch): field sections in field
        order (64-byte aligned), then meta int32 [n_windows, 4], then the 64-byte failure block - `payload` bytes in all, what
        a sharded store exchanges - then the sampler's row indices; `total` bytes to allocate."""
        unknown = [n for n in names if not (n in _FIELD_VIEWS and n != "action_in" and n in self._host_layout)]
        if unknown:
            raise ValueError(f"fields {unknown} are not recorded by this env")
        order = sorted(names, key=lambda n: _FIELD_VIEWS[n][0])
        mask = 0
        for n in order:
            mask |= 1 << _FIELD_VIEWS[n][0]
        payload, meta_off = C.c_size_t(), C.c_size_t()
        total = int(self._lib.rc_sample_batch_bytes(self._h, mask, int(n_windows), int(length), C.byref(payload), C.byref(meta_off)))
        if total == 0:
            raise ValueError(f"no recorded field among {list(names)}")
        rows, off, fields = int(n_windows) * int(length), 0, {}
        for n in order:
            fid, dtype, tail = _FIELD_VIEWS[n]
            per = self._host_layout[n][1] // self.n_cars
            fields[n] = (off, per * rows, dtype, tail)
            off = (off + per * rows + 63) // 64 * 64
        assert off == meta_off.value, (off, meta_off.value)
        return {"mask": mask, "total": total, "payload": int(payload.value), "meta": int(meta_off.value), "failed": int(meta_off.value) +
                (16 * int(n_windows) + 63) // 64 * 64, "fields": fields, "n_windows": int(n_windows), "length": int(length)}

    def sample_batch(self, ring: torch.Tensor, slot_bytes: int, capacity: int, oldest: int, count: int, layout: Dict[str, object],
                     seed: int, draw: int, reset_rows: bool = True, max_tries: int = 16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`rc_sample_batch`: one training batch - windows drawn, rows gathered, reset rows written - as one call into one
        packed uint8 buffer (`sample_batch_layout`); returns the buffer (`out`, or a fresh one)."""
        if out is None:
            out = torch.empty(layout["total"] + 64, dtype=torch.uint8, device=self.device)
            out = out[(-out.data_ptr()) % 64:][:layout["total"]]
        self._enter()
        L.check(self._lib.rc_sample_batch(self._h, ring.data_ptr(), int(slot_bytes), int(capacity), int(oldest), int(count), layout["length"],
                                          layout["n_windows"], C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint32(int(draw) & 0xffffffff),
                                          int(max_tries), layout["mask"], int(bool(reset_rows)), out.data_ptr(), int(out.numel())))
        self._exit()
        return out

    def host_snapshot(self) -> Dict[str, np.ndarray]:
        """Every output field on the host from ONE device-to-host copy of the arena (for small batches, e.g. the
        single-env shim): dict of NumPy views [num_envs, cars_per_env, ...] into one host buffer."""
        self.sync()
        buf = self._arena_view.cpu().numpy()
        out = {}
        for name, (off, nb, dtype, tail) in self._host_layout.items():
            out[name] = buf[off:off + nb].view(dtype).reshape(self.num_envs, self.cars_per_env, *tail)
        return out

    def host(self, name: str) -> np.ndarray:
        """Synchronised host copy of one output field."""
        self.sync()
        return self.views[name].cpu().numpy()


class MixedTrackEnv:
    """A batch that mixes tracks by blocks of envs (SURVEY.md 8e "per-env track"; BASELINE configs[4]'s track mix on ONE GPU):
    one `BatchedRaceEnv` handle per track, all of them filling their slice of ONE output arena, so the caller
    sees a single set of tensors `[total_envs, cars_per_env, ...]` and `track_id[total_envs]` (each handle on a stream of its own,
    forked from / joined to the caller's current stream around every call).  Env e of the batch is env e
    of the job: its reset stream is keyed by `first_env + e` whatever block it lies in, so a block of track T behaves
    exactly like the same envs in a single-track batch.  A step is one (dynamics, scan[, render]) launch set per track.

        env = MixedTrackEnv(["columbia", "austria", "barcelona"], [21846, 21845, 21845], auto_reset=True)
        out = env.reset(mode="random", seed=0); out = env.step(actions)       # actions float32 [65536, 1, 2] on the device
    """

    def __init__(self, tracks, envs_per_track, cars_per_env: int = 1, obs_type: str = "lidar", device: int = 0,
                 first_env: int = 0, **kw):
        if len(tracks) != len(envs_per_track) or not tracks:
            raise ValueError("one env count per track")
        self._lib = L.load_library()
        if not torch.cuda.is_available():
            raise L.RacecarHipError("no HIP device visible to torch; MixedTrackEnv has no CPU fallback")
        self.device = torch.device("cuda", device)
        self.num_envs, self.cars_per_env = int(sum(envs_per_track)), int(cars_per_env)
        self.n_cars = self.num_envs * self.cars_per_env
        cfg = L.RcConfig()
        self._lib.rc_default_config(C.byref(cfg))
        cfg.num_envs, cfg.cars_per_env, cfg.obs_type = self.num_envs, self.cars_per_env, OBS_TYPES[obs_type]
        nbytes = self._lib.rc_arena_bytes(C.byref(cfg))
        with torch.cuda.device(self.device):
            raw = torch.zeros(nbytes + 64, dtype=torch.uint8, device=self.device)
            self.stream = torch.cuda.Stream(device=self.device)      # a stream for callers that want one (bench.py works on it)
        pad = (-raw.data_ptr()) % 64
        self._raw, self.arena = raw, raw[pad:pad + nbytes]
        self.parts, self.blocks = [], []
        e0 = 0
        for track, n in zip(tracks, envs_per_track):
            self.parts.append(BatchedRaceEnv(track, int(n), cars_per_env, obs_type=obs_type, device=device, first_env=first_env + e0,
                                             shared_arena=self.arena, arena_total_cars=self.n_cars,
                                             arena_first_car=e0 * self.cars_per_env, stream=self.stream, **kw))
            self.blocks.append((e0, e0 + int(n)))
            e0 += int(n)
        self.track_id = torch.cat([torch.full((b - a,), i, dtype=torch.int32) for i, (a, b) in enumerate(self.blocks)]).to(self.device)
        self.views: Dict[str, torch.Tensor] = {}
        off, per = C.c_size_t(), C.c_size_t()
        for name, (fid, dtype, tail) in _FIELD_VIEWS.items():
            L.check(self._lib.rc_field_layout(C.byref(cfg), fid, C.byref(off), C.byref(per)))
            if per.value == 0:
                continue
            t = self.arena[off.value:off.value + per.value * self.n_cars].view(dtype)
            self.views[name] = t.view(self.num_envs, self.cars_per_env, *tail)

    @classmethod
    def from_track_ids(cls, tracks, track_id, **kw):
        """An ARBITRARY per-env track assignment (`track_id[e]` indexes `tracks`): the envs are laid out in the arena sorted by
        track (stable), because a workgroup of the render shares one bitmap in LDS and a wave's table lines should be its
        neighbours'; `row_of_env[e]` is the arena row of the caller's env e, `env_of_row` its inverse, and `to_rows` /
        `to_envs` reorder a leading-axis tensor between the two orders (one indexed copy).  Row r draws from reset stream
        `first_env + r`."""
        ids = torch.as_tensor(track_id, dtype=torch.int64).cpu().reshape(-1)
        if ids.numel() == 0 or int(ids.min()) < 0 or int(ids.max()) >= len(tracks):
            raise ValueError("track_id must index tracks")
        used = [i for i in range(len(tracks)) if bool((ids == i).any())]
        env = cls([tracks[i] for i in used], [int((ids == i).sum()) for i in used], **kw)
        env.env_of_row = torch.argsort(ids, stable=True).to(env.device)
        env.row_of_env = torch.empty_like(env.env_of_row)
        env.row_of_env[env.env_of_row] = torch.arange(ids.numel(), device=env.device)
        env.track_id = torch.as_tensor(used, dtype=torch.int32, device=env.device)[env.track_id.long()]   # ids as the caller numbered them
        return env

    def to_rows(self, x: torch.Tensor) -> torch.Tensor:
        """Caller order [num_envs, ...] -> arena order (e.g. actions before `step`)."""
        return x.to(self.device)[self.env_of_row]

    def to_envs(self, x: torch.Tensor) -> torch.Tensor:
        """Arena order -> caller order (e.g. `to_envs(out["lidar"])`)."""
        return x[self.row_of_env]

    # All blocks work on ONE stream (`self.stream`), ordered behind and before the caller's current stream around each call.  A
    # step is ONE dynamics and ONE scan launch over all blocks (`rc_step_group`: every wave works from the parameters of the
    # block it lies in): with a launch pair per block on streams of their own, each block's small dynamics kernel waited behind
    # the previous block's scan, the three scans shared the chip and 33 us passed between the join of one step and the first
    # kernel of the next (0.258 -> 0.208 ms per step of three blocks of 21 845 envs; the three tracks alone average 0.20;
    # EXPERIMENTS I.10).
    def _ordered(self, call):
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream != self.stream.cuda_stream:
            self.stream.wait_stream(cur)
        L.check(call())
        if cur.cuda_stream != self.stream.cuda_stream:
            cur.wait_stream(self.stream)
        return self.views

    def _fork_join(self, call):
        def every_block():
            for p, blk in zip(self.parts, self.blocks):
                rc = call(p, blk)
                if rc:
                    return rc
            return 0
        return self._ordered(every_block)

    def _handles(self):
        if getattr(self, "_handle_array", None) is None:
            self._handle_array = (C.c_void_p * len(self.parts))(*[p._h for p in self.parts])
        return self._handle_array

    def reset(self, mode: str = "grid", seed: Optional[int] = None):
        if mode not in spec.RESET_MODES:
            raise ValueError(f"reset mode must be one of {sorted(spec.RESET_MODES)}, got {mode!r}")
        for p in self.parts:
            if seed is not None:
                p.seed = int(seed)
        return self._fork_join(lambda p, blk: p._lib.rc_reset(p._h, None, spec.RESET_MODES[mode], C.c_uint64(p.seed)))

    def step(self, actions: Optional[torch.Tensor] = None, repeat: Optional[int] = None):
        """actions: float32 [total_envs, cars_per_env, 2] on the device (None: each block's `action_in`)."""
        if actions is not None:
            actions = actions.to(self.device, torch.float32).reshape(self.num_envs, self.cars_per_env, 2).contiguous()
        rep = self.parts[0].action_repeat if repeat is None else int(repeat)
        if len(self.parts) > 8:             # (more blocks than a group launch carries: one launch pair per block)
            return self._fork_join(lambda p, blk: p._lib.rc_step(p._h, None if actions is None else actions[blk[0]:blk[1]].data_ptr(), rep))
        return self._ordered(lambda: self._lib.rc_step_group(self._handles(), len(self.parts),
                                                             None if actions is None else actions.data_ptr(), rep))

    def step_random(self, seed: int, step: int, repeat: Optional[int] = None):
        rep = self.parts[0].action_repeat if repeat is None else int(repeat)
        if len(self.parts) > 8:
            return self._fork_join(lambda p, blk: p._lib.rc_step_random(p._h, C.c_uint64(seed), C.c_uint32(step), rep))
        return self._ordered(lambda: self._lib.rc_step_random_group(self._handles(), len(self.parts), C.c_uint64(seed), C.c_uint32(step), rep))

    # domain randomization: the same settings on every block (each block's handle keys its draws by its global env ids)
    def set_vehicle_randomization(self, lo=None, hi=None, seed: int = 0) -> None:
        for p in self.parts:
            p.set_vehicle_randomization(lo, hi, seed)

    def set_vehicle_params(self, params: Optional[torch.Tensor]) -> None:
        """float32 [n_cars, 5] in arena order (or None: off)."""
        if params is None:
            for p in self.parts:
                p.set_vehicle_params(None)
            return
        t = torch.as_tensor(params, dtype=torch.float32).to(self.device).reshape(self.n_cars, len(spec.VEHICLE_PARAMS))
        for p, (a, b) in zip(self.parts, self.blocks):
            p.set_vehicle_params(t[a * self.cars_per_env:b * self.cars_per_env])

    @property
    def vehicle_params(self) -> torch.Tensor:
        """float32 [n_cars, 5] in arena order: a COPY gathered from the blocks (each handle holds its own)."""
        return torch.cat([p.vehicle_params for p in self.parts])

    def set_lidar_noise(self, sigma: float = 0.0, p_drop: float = 0.0, seed: int = 0) -> None:
        for p in self.parts:
            p.set_lidar_noise(sigma, p_drop, seed)

    def follow_the_gap_reference(self, dt: Optional[float] = None):
        self._fork_join(lambda p, blk: p._lib.rc_follow_the_gap_reference(p._h, 0.01 * p.action_repeat if dt is None else float(dt), None))
        return self.views["action_in"]

    def load_policy(self, weights) -> None:
        """The reference's trained Dreamer agent on every block (BatchedRaceEnv.load_policy)."""
        if isinstance(weights, (str, os.PathLike)):
            weights = dict(np.load(weights))
        for p in self.parts:
            p.load_policy(weights)

    def policy_act(self, slots=None):
        mask = (1 << self.cars_per_env) - 1 if slots is None else sum({1 << int(a) for a in slots})
        self._fork_join(lambda p, blk: p._lib.rc_policy_act(p._h, C.c_uint32(mask)))
        return self.views["action_in"]

    @property
    def policy_has_reward_head(self) -> bool:
        return self.parts[0].policy_has_reward_head

    def policy_imagine(self, horizon: int = 15, mode: str = "mean", seed: int = 0, actions: Optional[torch.Tensor] = None, slots=None,
                       features: bool = False, start_reward: bool = False, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.policy_imagine over all blocks: each block writes its cars' rows of one tensor per output."""
        args, tensors, result = _imagine_setup(self, horizon, mode, seed, actions, slots, features, start_reward, out)
        k = self.cars_per_env
        self._fork_join(lambda p, blk: p._imagine(args, tensors, blk[0] * k, blk[1] * k))
        return result

    def dream_ahead(self, actions: torch.Tensor, mode: str = "mean", seed: int = 0, state: Optional[torch.Tensor] = None, row_offset: int = 0,
                    slots=None, discount: float = 1.0, outputs=("return",), out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.dream_ahead over all blocks: each block plans from its cars' latents into its rows of one tensor per
        output; a given `state` (every block holds the same weights) goes through the first block."""
        args, tensors, result = _dream_setup(self, actions, mode, seed, state, row_offset, slots, discount, outputs, out)
        k = self.cars_per_env
        if state is not None:
            self._ordered(lambda: self.parts[0]._dream_ahead(args, tensors, 0, 0))
        else:
            self._fork_join(lambda p, blk: p._dream_ahead(args, tensors, blk[0] * k, blk[1] * k))
        return result

    def dream_ahead_grad(self, actions: torch.Tensor, mode: str = "mean", seed: int = 0, state: Optional[torch.Tensor] = None, row_offset: int = 0,
                         slots=None, discount: float = 1.0, outputs=("grad_actions", "return"), out: Optional[Dict[str, torch.Tensor]] = None,
                         chunk_rows: int = 0) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.dream_ahead_grad over all blocks, forwarded the way `dream_ahead` is."""
        args, tensors, result = _dream_setup(self, actions, mode, seed, state, row_offset, slots, discount, outputs, out, L.DREAM_GRAD_OUTPUTS,
                                             "dream_ahead_grad")
        args["chunk_rows"] = _chunk_rows(chunk_rows)
        k = self.cars_per_env
        if state is not None:
            self._ordered(lambda: self.parts[0]._dream_grad(args, tensors, 0, 0))
        else:
            self._fork_join(lambda p, blk: p._dream_grad(args, tensors, blk[0] * k, blk[1] * k))
        return result

    def load_critic(self, weights) -> None:
        """The critic on every block (BatchedRaceEnv.load_critic)."""
        if isinstance(weights, (str, os.PathLike)):
            weights = dict(np.load(weights))
        for p in self.parts:
            p.load_critic(weights)

    @property
    def policy_has_value_head(self) -> bool:
        return self.parts[0].policy_has_value_head

    @property
    def policy_has_pcont_head(self) -> bool:
        return self.parts[0].policy_has_pcont_head

    def policy_returns(self, horizon: int = 15, mode: str = "mean", seed: int = 0, lambda_: float = 0.95, discount: float = 0.99,
                       actions: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None, row_offset: int = 0, slots=None,
                       outputs=("returns", "weight"), out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.policy_returns over all blocks: each block starts from its cars' latents and writes its rows of one tensor
        per output; a given `state` (every block holds the same weights) goes through the first block."""
        args, tensors, result = _returns_setup(self, horizon, mode, seed, lambda_, discount, actions, state, row_offset, slots, outputs, out)
        k = self.cars_per_env
        if state is not None:
            self._ordered(lambda: self.parts[0]._returns(args, tensors, 0, 0))
        else:
            self._fork_join(lambda p, blk: p._returns(args, tensors, blk[0] * k, blk[1] * k))
        return result

    def policy_returns_grad(self, horizon: int = 15, mode: str = "sample", seed: int = 0, lambda_: float = 0.95, discount: float = 0.99,
                            scale: Optional[float] = None, actions: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None,
                            row_offset: int = 0, slots=None, outputs=("grad_actions", "actor_features", "eps"),
                            out: Optional[Dict[str, torch.Tensor]] = None, chunk_rows: int = 0) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.policy_returns_grad over all blocks, forwarded the way `policy_returns` is (the default `scale` counts the
        rows of all blocks)."""
        args, tensors, result = _returns_grad_setup(self, horizon, mode, seed, lambda_, discount, scale, actions, state, row_offset, slots,
                                                    outputs, out, chunk_rows)
        k = self.cars_per_env
        if state is not None:
            self._ordered(lambda: self.parts[0]._returns_grad(args, tensors, 0, 0))
        else:
            self._fork_join(lambda p, blk: p._returns_grad(args, tensors, blk[0] * k, blk[1] * k))
        return result

    def policy_value(self, features: Optional[torch.Tensor] = None, slots=None, outputs=("value",)) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.policy_value: given features go through the first block, live latents through every block."""
        state, lead, names = _value_setup(self, features, slots, outputs)
        got = self.policy_returns(horizon=0, state=state, slots=slots, outputs=names)
        return {n[:-6]: got[n].reshape(lead) for n in names}

    def critic_fit_begin(self, head: str = "value") -> None:
        """BatchedRaceEnv.critic_fit_begin on every block."""
        for p in self.parts:
            p.critic_fit_begin(head)

    def critic_fit(self, features: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, head: str = "value",
                   lr: float = 8e-5, clip: float = 1.0, beta1: float = 0.9, beta2: float = 0.999,
                   epsilon: float = 1e-7) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.critic_fit on every block with the same inputs: the step is deterministic, so the blocks' critics stay
        byte-identical.  The status is the first block's."""
        feat, tgt, wgt, status = _fit_setup(self, features, target, weight, head)
        hyper = dict(lr=lr, clip=clip, beta1=beta1, beta2=beta2, epsilon=epsilon)
        self._fork_join(lambda p, blk: p._fit(head, feat, tgt, wgt, status if p is self.parts[0] else None, hyper))
        return _fit_status(status)

    def critic_fit_end(self, head: str = "value") -> None:
        for p in self.parts:
            p.critic_fit_end(head)

    def critic_weights(self) -> Dict[str, np.ndarray]:
        """The first block's critic (every block holds the same)."""
        return self.parts[0].critic_weights()

    def reward_fit_begin(self) -> None:
        """BatchedRaceEnv.reward_fit_begin on every block."""
        for p in self.parts:
            p.reward_fit_begin()

    def reward_fit(self, features: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, lr: float = 6e-4,
                   clip: float = 1.0, beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-7) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.reward_fit on every block with the same inputs: the step is deterministic, so the blocks' reward heads
        stay byte-identical.  The status is the first block's."""
        feat, tgt, wgt, status = _fit_setup(self, features, target, weight, None)
        hyper = dict(lr=lr, clip=clip, beta1=beta1, beta2=beta2, epsilon=epsilon)
        self._fork_join(lambda p, blk: p._fit(L.FIT_REWARD, feat, tgt, wgt, status if p is self.parts[0] else None, hyper))
        return _fit_status(status)

    def reward_fit_end(self) -> None:
        for p in self.parts:
            p.reward_fit_end()

    def reward_head_weights(self) -> Dict[str, np.ndarray]:
        """The first block's reward head (every block holds the same)."""
        return self.parts[0].reward_head_weights()

    def load_reward_head(self, weights) -> None:
        """The reward head on every block (BatchedRaceEnv.load_reward_head)."""
        if isinstance(weights, (str, os.PathLike)):
            weights = dict(np.load(weights))
        for p in self.parts:
            p.load_reward_head(weights)

    def actor_fit_begin(self) -> None:
        """BatchedRaceEnv.actor_fit_begin on every block."""
        for p in self.parts:
            p.actor_fit_begin()

    def actor_fit(self, features: torch.Tensor, target: Optional[torch.Tensor] = None, grad_actions: Optional[torch.Tensor] = None,
                  eps: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None, grad_features: bool = False,
                  lr: float = 8e-5, clip: float = 1.0, beta1: float = 0.9, beta2: float = 0.999,
                  epsilon: float = 1e-7) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.actor_fit on every block with the same inputs: the step is deterministic, so the blocks' actors stay
        byte-identical.  The status and `grad_features` are the first block's."""
        feat, t, gfeat, gshape, status = _actor_fit_setup(self, features, target, grad_actions, eps, weight, grad_features)
        hyper = dict(lr=lr, clip=clip, beta1=beta1, beta2=beta2, epsilon=epsilon)
        first = self.parts[0]
        self._fork_join(lambda p, blk: p._actor_fit(feat, t, gfeat if p is first else None, status if p is first else None, hyper))
        out = _fit_status(status)
        if gfeat is not None:
            out["grad_features"] = gfeat.reshape(gshape)
        return out

    def actor_fit_end(self) -> None:
        for p in self.parts:
            p.actor_fit_end()

    def policy_action(self, features: torch.Tensor, eps: Optional[torch.Tensor] = None, outputs=("action",)) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.policy_action through the first block (every block holds the same actor)."""
        return self.parts[0].policy_action(features, eps, outputs)

    def actor_weights(self) -> Dict[str, np.ndarray]:
        """The first block's actor (every block holds the same)."""
        return self.parts[0].actor_weights()

    def load_actor(self, weights) -> None:
        """The actor on every block (BatchedRaceEnv.load_actor)."""
        if isinstance(weights, (str, os.PathLike)):
            weights = dict(np.load(weights))
        for p in self.parts:
            p.load_actor(weights)

    def look_ahead(self, actions: torch.Tensor, repeat: Optional[int] = None, outputs=("reward", "flags", "return", "length"),
                   out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.look_ahead over all blocks: each block writes its envs' rows of one tensor per output."""
        args, tensors, result = _look_ahead_setup(self, actions, self.parts[0].action_repeat if repeat is None else repeat, outputs, out)
        self._fork_join(lambda p, blk: p._look_ahead(args, tensors, blk[0], blk[1]))
        return result

    def policy_observe(self, lidar: torch.Tensor, action: torch.Tensor, context: Optional[int] = None, mode: str = "mean", seed: int = 0,
                       state: Optional[torch.Tensor] = None, row_offset: int = 0, outputs=("feature",),
                       out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.policy_observe: recorded rows are not cars of a block (every block holds the same weights), so the
        call goes through the first block."""
        a, keep, result = _observe_setup(self, lidar, action, context, mode, seed, state, row_offset, outputs, out)
        self._ordered(lambda: self.parts[0]._lib.rc_policy_observe(self.parts[0]._h, C.byref(a)))
        del keep
        return result

    @property
    def policy_has_decoder(self) -> bool:
        return self.parts[0].policy_has_decoder

    def policy_decode(self, features: Optional[torch.Tensor] = None, slots=None, logits: bool = False, image: bool = True,
                      mismatch: bool = False, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.policy_decode over all blocks: each block decodes its cars' latents into its rows of one tensor per
        output; given `features` (every block holds the same decoder) go through the first block."""
        feats, mask, tensors, result = _decode_setup(self, features, slots, logits, image, mismatch, out)
        k = self.cars_per_env
        if feats is not None:
            self._ordered(lambda: self.parts[0]._decode(feats, mask, tensors, 0, 0))
        else:
            self._fork_join(lambda p, blk: p._decode(None, mask, tensors, blk[0] * k, blk[1] * k))
        return result

    def policy_decode_loglik(self, target: Optional[torch.Tensor] = None, features: Optional[torch.Tensor] = None, slots=None,
                             outputs=("loglik",), out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.policy_decode_loglik over all blocks, as `policy_decode`."""
        feats, mask, tgt, tensors, result = _decode_loglik_setup(self, target, features, slots, outputs, out)
        k = self.cars_per_env
        if feats is not None:
            self._ordered(lambda: self.parts[0]._decode_loglik(feats, mask, tgt, tensors, 0, 0))
        else:
            self._fork_join(lambda p, blk: p._decode_loglik(None, mask, tgt, tensors, blk[0] * k, blk[1] * k))
        return result

    def load_lidar_decoder(self, weights) -> None:
        """The LiDAR distance decoder on every block (BatchedRaceEnv.load_lidar_decoder)."""
        if isinstance(weights, (str, os.PathLike)):
            weights = dict(np.load(weights))
        for p in self.parts:
            p.load_lidar_decoder(weights)

    @property
    def policy_has_lidar_decoder(self) -> bool:
        return self.parts[0].policy_has_lidar_decoder

    def policy_decode_lidar(self, features: Optional[torch.Tensor] = None, slots=None, target: Optional[torch.Tensor] = None,
                            outputs=("mean",), out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """BatchedRaceEnv.policy_decode_lidar over all blocks: each block decodes its cars' latents into its rows of one tensor per
        output; given `features` (every block holds the same decoder) go through the first block."""
        feats, mask, tgt, tensors, result = _decode_lidar_setup(self, features, slots, target, outputs, out)
        k = self.cars_per_env
        if feats is not None:
            self._ordered(lambda: self.parts[0]._decode_lidar(feats, mask, tgt, tensors, 0, 0))
        else:
            self._fork_join(lambda p, blk: p._decode_lidar(None, mask, tgt, tensors, blk[0] * k, blk[1] * k))
        return result

    def set_policy_sampling(self, mode: str = "mean", seed: int = 0, expl_amount: Optional[float] = None) -> None:
        """The same mode and seed on every block (BatchedRaceEnv.set_policy_sampling): the draws are keyed by global env ids."""
        for p in self.parts:
            p.set_policy_sampling(mode, seed, expl_amount)

    @property
    def policy_sampling(self) -> dict:
        return self.parts[0].policy_sampling

    @property
    def policy_state(self) -> torch.Tensor:
        """float32 [n_cars, 232] in arena order: a COPY gathered from the blocks (each handle holds its own)."""
        return torch.cat([p.policy_state for p in self.parts])

    def unload_policy(self) -> None:
        for p in self.parts:
            p.unload_policy()

    # episode log: each block's handle keeps its own; the merged view is in (call, env, slot) order with `track` = the block's index
    def enable_episode_log(self, capacity: int, max_episodes: int = 0) -> None:
        """`capacity` rows for the whole batch, shared out by each block's share of the envs (rounded up)."""
        for p in self.parts:
            p.enable_episode_log(-(-int(capacity) * p.num_envs // self.num_envs), max_episodes)

    @property
    def episode_counters(self) -> Dict[str, int]:
        parts = [p.episode_counters for p in self.parts]
        out = {k: sum(c[k] for c in parts) for k in L.EPISODE_COUNTERS}
        out["calls"] = max(c["calls"] for c in parts)
        return out

    def episode_log(self, clear: bool = False) -> Dict[str, torch.Tensor]:
        """The blocks' logs merged (copies) into (call, env, slot) order: `env` in the batch's own numbering (first_env + row of the
        arena), `track` = the index of the env's block."""
        logs = [p.episode_log(clear=clear) for p in self.parts]
        for i, lg in enumerate(logs):
            lg["track"] = torch.full_like(lg["track"], i)
        cat = {k: torch.cat([lg[k] for lg in logs]) for k in logs[0]}
        # blocks hold disjoint, ascending env ranges and each is already ordered: a stable sort by call restores the order
        order = torch.sort(cat["call"].to(torch.int64) & 0xFFFFFFFF, stable=True).indices
        return {k: v[order] for k, v in cat.items()}

    def clear_episode_log(self) -> None:
        for p in self.parts:
            p.clear_episode_log()

    def disable_episode_log(self) -> None:
        for p in self.parts:
            p.disable_episode_log()

    def sync(self):
        for p in self.parts:
            p.sync()

    def close(self):
        for p in self.parts:
            p.close()
