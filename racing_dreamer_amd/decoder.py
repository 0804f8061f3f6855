"""The LiDAR distance decoder's arrays: the observation decoder of the reference's `lidar` agents (dreamer/models.py:424-441
LidarDistanceDecoder: dense1 230 -> 256, dense2 256 -> 512, params 512 -> 2160), as `BatchedRaceEnv.load_lidar_decoder` takes
them.  No shipped checkpoint holds them (`decoder.pkl` exists only for the two occupancy agents; training saves the decoder with
the whole agent as `variables.pkl`), so `init_lidar_decoder` makes a synthetic one and `lidar_decoder_from_variables` picks a
trained one out of such a list."""
from __future__ import annotations

import numpy as np

from ._lib import LIDAR_DECODER_KEYS, LIDAR_DECODER_SHAPES

BEAMS = 1080


def init_lidar_decoder(seed: int, scale_bias: float = 0.0) -> dict:
    """Glorot-uniform weights from numpy.random.default_rng(seed) and zero biases; `ldec_params_b[1080:] = scale_bias`, the bias
    of the raw scale columns: 0 puts the scale near softplus(0) = 0.69, a negative one (through the leaky ReLU's slope 0.2)
    makes the distribution as narrow as a trained decoder's."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, shape in zip(LIDAR_DECODER_KEYS, LIDAR_DECODER_SHAPES):
        if len(shape) == 2:
            limit = np.sqrt(6.0 / (shape[0] + shape[1]))
            out[k] = rng.uniform(-limit, limit, shape).astype(np.float32)
        else:
            out[k] = np.zeros(shape, np.float32)
    out["ldec_params_b"][BEAMS:] = scale_bias
    return out


def save_lidar_decoder(path, weights) -> None:
    """The six arrays of `weights` into an .npz."""
    np.savez(path, **{k: np.ascontiguousarray(weights[k], np.float32) for k in LIDAR_DECODER_KEYS})


def load_lidar_decoder_file(path) -> dict:
    """What `save_lidar_decoder` wrote, as the mapping `BatchedRaceEnv.load_lidar_decoder` takes."""
    with np.load(path) as f:
        return {k: np.ascontiguousarray(f[k], np.float32) for k in LIDAR_DECODER_KEYS}


def lidar_decoder_from_variables(arrays) -> dict:
    """The decoder out of a `variables.pkl`-ordered list of arrays (dreamer/models.py:30-50: encoder, dynamics, decoder, reward,
    ...): found by its six shapes in a row ([230, 256], [256], [256, 512], [512], [512, 2160], [2160]).  Raises ValueError when no
    such run is in the list, or more than one."""
    shapes = [tuple(np.shape(a)) for a in arrays]
    hits = [i for i in range(len(shapes) - 5) if tuple(shapes[i:i + 6]) == LIDAR_DECODER_SHAPES]
    if len(hits) != 1:
        raise ValueError(f"{len(hits)} runs of a LidarDistanceDecoder's six shapes {LIDAR_DECODER_SHAPES} in the list (one expected)")
    return {k: np.ascontiguousarray(arrays[hits[0] + i], np.float32) for i, k in enumerate(LIDAR_DECODER_KEYS)}
