"""The critic's arrays: the value head and the pcont head of the reference's Dreamer (dreamer/models.py:301-318 DenseDecoder((), 3,
400) each), as `BatchedRaceEnv.load_critic` takes them.  No shipped checkpoint holds them - the reference's own training does
(`pcont=True`, saved with the whole agent as `variables.pkl`) - so `init_critic` makes a synthetic pair and `critic_from_variables`
picks a trained pair out of such a list."""
from __future__ import annotations

import numpy as np

from ._lib import HEAD_KEYS, PCONT_KEYS, VALUE_KEYS

_SHAPES = ((230, 400), (400,), (400, 400), (400,), (400, 400), (400,), (400, 1), (1,))
_REWARD_SHAPES = ((230, 400), (400,), (400, 400), (400,), (400, 1), (1,))


def init_critic(seed: int, pcont: bool = True, pcont_bias: float = 3.0) -> dict:
    """A value head (and a pcont head) with Glorot-uniform weights from numpy.random.default_rng(seed) and zero biases;
    `pcont_hout_b = pcont_bias`, so pcont sits near sigmoid(3) = 0.95 without saturating the sigmoid."""
    rng = np.random.default_rng(seed)
    out = {}
    for keys in (VALUE_KEYS,) + ((PCONT_KEYS,) if pcont else ()):
        for k, shape in zip(keys, _SHAPES):
            if len(shape) == 2:
                limit = np.sqrt(6.0 / (shape[0] + shape[1]))
                out[k] = rng.uniform(-limit, limit, shape).astype(np.float32)
            else:
                out[k] = np.zeros(shape, np.float32)
    if pcont:
        out["pcont_hout_b"][:] = pcont_bias
    return out


def save_critic(path, env) -> None:
    """The env's loaded critic - as `critic_fit` last left it - into an .npz of `env.critic_weights()`."""
    np.savez(path, **env.critic_weights())


def load_critic_file(path) -> dict:
    """What `save_critic` wrote, as the mapping `BatchedRaceEnv.load_critic` takes."""
    with np.load(path) as f:
        return {k: np.ascontiguousarray(f[k], np.float32) for k in f.files if k in VALUE_KEYS + PCONT_KEYS}


def critic_from_variables(arrays) -> dict:
    """The critic out of a `variables.pkl`-ordered list of arrays (dreamer/models.py:30-50: ..., reward, [pcont,] value, actor):
    the reward head is found by its six shapes in a row ([230, 400], [400], [400, 400], [400], [400, 1], [1]); a pcont head
    (eight arrays, `pcont=True`) follows it when sixteen arrays of the critic's shapes do, else the value head alone does.
    Raises ValueError when the shapes say otherwise."""
    shapes = [tuple(np.shape(a)) for a in arrays]
    at = next((i for i in range(len(shapes) - 5) if tuple(shapes[i:i + 6]) == _REWARD_SHAPES), None)
    if at is None:
        raise ValueError(f"no reward head ({len(HEAD_KEYS)} arrays of shapes {_REWARD_SHAPES}) in the list")
    at += 6
    if tuple(shapes[at:at + 16]) == _SHAPES + _SHAPES:
        keys = PCONT_KEYS + VALUE_KEYS
    elif tuple(shapes[at:at + 8]) == _SHAPES:
        keys = VALUE_KEYS
    else:
        raise ValueError(f"the arrays after the reward head have shapes {shapes[at:at + 16]}: not a DenseDecoder((), 3, 400) or two")
    return {k: np.ascontiguousarray(arrays[at + i], np.float32) for i, k in enumerate(keys)}
