"""Test-side restatement of the track set (include/racecar_hip.h, rc_set_track_set / rc_set_next_track / rc_track_ids) on top of
the CPU oracle, which itself stays as it is.

TrackSetMixin goes in front of oracle.racecar_oracle.OracleRaceEnv (or tests/dr_oracle.DROracleEnv: the two compose):
  - the composite owns the per-env track, the started flags and the manual order's next-track array;
  - one base oracle per track provides that track's geometry (grids, centre line, origin, resolution and the cached spawn tables);
  - `_reset_envs` draws each env's next track (the first reset after the install keeps the initial one), then runs the base reset
    on the envs now on track k with track k's geometry installed, for every k;
  - `_substep`, `_raycast_cars` and `render_patch` run the base work on the envs / cars of each track in turn, the same way.
"""
import numpy as np

from oracle import racecar_oracle as ro
from oracle.racecar_oracle import i32, u32, u64, philox4x32

TRACK_TAG = 3
M32 = 0xFFFFFFFF
ORDERS = ("sequential", "random", "manual")
# what a base oracle holds of its track (the rest is state, owned by the composite)
_GEOMETRY = ("occ", "ring", "drv", "progress_grid", "centerline", "H", "W", "org_x", "org_y", "res", "inv_res", "tmax", "frame_track")


def weight_thresholds(weights):
    """uint32 c_1 .. c_{T-1} as rc_set_track_set computes them: c_k = min(floor(2^32 S_k / S + 0.5), 2^32 - 1), S_k the binary64
    partial sums of the binary32 weights, left to right."""
    w = [float(np.float32(v)) for v in weights]
    total = 0.0
    for v in w:
        total += v
    out, part = [], 0.0
    for k in range(1, len(w)):
        part += w[k - 1]
        c = np.floor(4294967296.0 * part / total + 0.5)
        out.append(M32 if c >= 4294967295.0 else int(c))
    return np.asarray(out, np.uint64)


def draw_tracks(seed, global_env, episode, T, thresholds=None):
    """int32 [n]: the random order's track for resets with these (global env id, episode value)."""
    g = np.asarray(global_env, np.uint64).astype(u32)
    ep = np.asarray(episode, u32)
    r = philox4x32(g, ep, u32(0), u32(TRACK_TAG), seed & M32, (seed >> 32) & M32)[0].astype(u64)
    if thresholds is None:
        return ((r * u64(T)) >> u64(32)).astype(i32)
    return (np.asarray(thresholds, u64)[None, :] <= r[:, None]).sum(1).astype(i32)


def contiguous_initial(num_envs, T):
    """The default initial assignment: contiguous blocks, the first num_envs % T one env longer."""
    return np.concatenate([np.full(num_envs // T + (1 if k < num_envs % T else 0), k, i32) for k in range(T)])


def _geometry(env, track):
    env.frame_track = track
    env.spawn_rows()
    env.spawn_safe()
    g = {k: getattr(env, k) for k in _GEOMETRY}
    g.update({k: v for k, v in env.__dict__.items() if k.startswith("_spawn")})
    return g


class TrackSetMixin:
    def set_track_set(self, geometries, order="sequential", initial=None, weights=None, seed=0):
        assert order in ORDERS and 1 <= len(geometries) <= 8
        self.ts_geom, self.ts_T, self.ts_order, self.ts_seed = list(geometries), len(geometries), order, int(seed)
        self.ts_thresholds = None if weights is None else weight_thresholds(weights)
        init = contiguous_initial(self.B, self.ts_T) if initial is None else np.asarray(initial, i32).reshape(self.B)
        assert ((init >= 0) & (init < self.ts_T)).all()
        self.track = init.astype(i32).copy()
        self.ts_next = self.track.copy()
        self.ts_started = np.zeros(self.B, bool)
        self._ts_use(0)

    def set_next_track(self, ids):
        self.ts_next = np.asarray(ids, i32).reshape(self.B).copy()

    def _ts_use(self, k):
        self.__dict__.update(self.ts_geom[k])

    def _next_tracks(self, envs, episode, cur):
        T = self.ts_T
        if self.ts_order == "sequential":
            return ((cur + 1) % T).astype(i32)
        if self.ts_order == "manual":
            nx = self.ts_next[envs]
            return np.where((nx >= 0) & (nx < T), nx, cur).astype(i32)
        return draw_tracks(self.ts_seed, envs + self.cfg.first_env, episode, T, self.ts_thresholds)

    def _by_track(self, envs):
        tr = self.track[envs]
        for k in range(self.ts_T):
            m = tr == k
            if m.any():
                self._ts_use(k)
                yield m

    # ---- reset: the next track before the spawn draw (the first reset after the install keeps the initial one)
    def _reset_envs(self, envs):
        envs = np.asarray(envs)
        if envs.size:
            cur = self.track[envs]
            nxt = self._next_tracks(envs, self.episode[envs].copy(), cur)
            self.track[envs] = np.where(self.ts_started[envs], nxt, cur)
            self.ts_started[envs] = True
        for m in self._by_track(envs):
            super()._reset_envs(envs[m])
        self.needs_reset[envs] = False

    def _substep(self, envs, motor, steer):
        for m in self._by_track(envs):
            super()._substep(envs[m], motor[m], steer[m])

    def _raycast_cars(self, cars):
        out = np.empty((cars.size, ro.N_BEAMS), ro.f32)
        for m in self._by_track(cars // self.A):
            out[m] = super()._raycast_cars(cars[m])
        return out

    def render_patch(self, cars=None):
        cars = np.arange(self.NC) if cars is None else cars
        out = np.zeros((cars.size, ro.PATCH, ro.PATCH), np.uint8)
        for m in self._by_track(cars // self.A):
            out[m] = super().render_patch(cars[m])
        return out

    def outputs(self):
        out = super().outputs()
        out["track_id"] = self.track.copy()
        return out

    def step(self, actions, repeat=1):
        out = super().step(actions, repeat)
        out["track_id"] = self.track.copy()
        return out


def make_track_set_oracle(tracks, order="sequential", initial=None, weights=None, seed=0, base=ro.OracleRaceEnv, **kw):
    """A track-set oracle over `tracks` (Track objects) with OracleConfig(**kw); base: OracleRaceEnv or DROracleEnv."""
    cls = type("TrackSet" + base.__name__, (TrackSetMixin, base), {})
    t0 = tracks[0]
    env = cls(t0.occ, t0.drivable, t0.progress, t0.centerline, t0.origin, t0.resolution, ro.OracleConfig(**kw))
    geo_cfg = dict(num_envs=1, cars_per_env=kw.get("cars_per_env", 1))
    geoms = [_geometry(ro.OracleRaceEnv(t.occ, t.drivable, t.progress, t.centerline, t.origin, t.resolution, ro.OracleConfig(**geo_cfg)), t)
             for t in tracks]
    env.set_track_set(geoms, order=order, initial=initial, weights=weights, seed=seed)
    return env
