"""Test-side restatement of per-episode domain randomization (include/racecar_hip.h, rc_set_vehicle_randomization /
rc_set_vehicle_params / rc_set_lidar_noise) on top of the CPU oracle, which itself stays as it is.

DROracleEnv subclasses oracle.racecar_oracle.OracleRaceEnv:
  - `_substep` is the base integrator with the five per-car vehicle parameters (`vp`, float32 [n_cars, 5]) as operands;
  - `_reset_envs` draws them (random mode) after the base reset, from the episode value the spawn draw used;
  - `raycast` applies range noise and dropout to the base scan (metres, before any lidar_transform scaling).
"""
import numpy as np

from oracle import racecar_oracle as ro
from oracle.racecar_oracle import f32, i32, u32, u64, clamp32, sincos32, exp32, philox4x32

VP_NOMINAL = np.array([0.19, 4.0, 0.8, 5.0, 0.032], np.float32)      # wheel_max, accel_max, drag, max_vel, steer_step
VP_TAG = 2
NOISE_Z_SCALE = np.float32(4.2286398820579052e-4)                      # sqrt(3 / (4096^2 - 1)) in binary32
M32 = 0xFFFFFFFF


def lowbias32(x):
    """C. Wellons' lowbias32 on uint32 arrays."""
    x = np.asarray(x, np.uint32).astype(np.uint64)
    x ^= x >> u64(16)
    x = (x * u64(0x7feb352d)) & u64(M32)
    x ^= x >> u64(15)
    x = (x * u64(0x846ca68b)) & u64(M32)
    x ^= x >> u64(16)
    return x.astype(np.uint32)


def noise_car_key(seed, global_car, episode, steps):
    s_lo, s_hi = np.uint32(seed & M32), np.uint32((seed >> 32) & M32)
    h = lowbias32(np.asarray(steps, np.uint32) ^ s_hi)
    h = lowbias32(np.asarray(episode, np.uint32) ^ h)
    h = lowbias32(np.asarray(global_car, np.uint32) ^ h)
    return lowbias32(s_lo ^ h)


def noise_words(key, beams=None):
    """w0, w1 [n, n_beams] for per-car keys [n]."""
    b = np.arange(ro.N_BEAMS, dtype=np.uint64) if beams is None else np.asarray(beams, np.uint64)
    x0 = (np.asarray(key, np.uint64)[:, None] + b[None, :] * u64(2 * 0x9E3779B9)) & u64(M32)
    return lowbias32(x0), lowbias32((x0 + u64(0x9E3779B9)) & u64(M32))


def noise_z_and_drop(w0, w1):
    """(k0 + k1 + k2 + k3 - 8190) as int, and the 16-bit dropout value d."""
    k = (w0 & 0xfff).astype(np.int64) + ((w0 >> 12) & 0xfff) + (w1 & 0xfff) + ((w1 >> 12) & 0xfff)
    d = ((w0 >> 16) & 0xff00) | (w1 >> 24)
    return (k - 8190).astype(np.int64), d.astype(np.uint32)


def noise_params(sigma, p_drop):
    """(scale, threshold) exactly as rc_set_lidar_noise derives them."""
    return f32(f32(sigma) * NOISE_Z_SCALE), int(np.floor(float(np.float32(p_drop)) * 65536.0 + 0.5))


def apply_noise(r, key, sigma, p_drop):
    """Noisy ranges [n, 1080] (metres) from clean ranges r and per-car keys."""
    scale, drop = noise_params(sigma, p_drop)
    w0, w1 = noise_words(key)
    kz, d = noise_z_and_drop(w0, w1)
    r = np.asarray(r, f32)
    n = kz.astype(f32) * scale
    out = np.where(r < ro.MAX_RANGE, clamp32((r + n).astype(f32), f32(0.0), ro.MAX_RANGE), r).astype(f32)
    return np.where(d < drop, ro.MAX_RANGE, out).astype(f32)


def draw_vehicle(seed, global_env, episode, lo, hi, A):
    """float32 [len(global_env), A, 5]: the parameters a reset with these episode values draws."""
    g = np.asarray(global_env, np.uint64).astype(u32)
    ep = np.asarray(episode, u32)
    n_calls = (5 * A + 3) // 4
    words = []
    for k in range(n_calls):
        words.extend(philox4x32(g, ep, u32(k), u32(VP_TAG), seed & M32, (seed >> 32) & M32))
    w = np.stack(words, 1)[:, :5 * A].reshape(-1, A, 5)
    u = (w >> u32(8)).astype(f32) * f32(5.9604644775390625e-8)
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    return (lo + u * (hi - lo)).astype(f32)


def transform(r, t):
    """The scan's fused lidar_transform scaling (include/racecar_hip.h, RC_LIDAR_*)."""
    r = np.asarray(r, f32)
    if t == 1:
        return (r / ro.MAX_RANGE - f32(0.5)).astype(f32)
    if t == 2:
        return (r * f32(1.0 / 15.0)).astype(f32)
    return r


class DROracleEnv(ro.OracleRaceEnv):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.vp = np.tile(VP_NOMINAL, (self.NC, 1))
        self.vp_mode, self.vp_lo, self.vp_hi, self.vp_seed = "off", None, None, 0
        self.noise = None                          # (sigma, p_drop, seed)

    # ---- settings (the C-ABI's entry points)
    def set_vehicle_randomization(self, lo=None, hi=None, seed=0):
        if lo is None or hi is None:
            self.vp_mode = "off"
            self.vp[:] = VP_NOMINAL
        else:
            self.vp_mode, self.vp_lo, self.vp_hi, self.vp_seed = "random", np.asarray(lo, f32), np.asarray(hi, f32), int(seed)

    def set_vehicle_params(self, params):
        if params is None:
            self.vp_mode = "off"
            self.vp[:] = VP_NOMINAL
        else:
            self.vp_mode = "fixed"
            self.vp[:] = np.asarray(params, f32).reshape(self.NC, 5)

    def set_lidar_noise(self, sigma=0.0, p_drop=0.0, seed=0):
        self.noise = None if (sigma == 0 and p_drop == 0) else (float(sigma), float(p_drop), int(seed))

    # ---- reset: the base law, then the new episode's vehicle parameters
    def _reset_envs(self, envs):
        ep = self.episode[envs].copy()             # the value the spawn draw uses (before the reset's increment)
        super()._reset_envs(envs)
        if self.vp_mode == "random" and envs.size:
            v = draw_vehicle(self.vp_seed, envs + self.cfg.first_env, ep, self.vp_lo, self.vp_hi, self.A)
            for a in range(self.A):
                self.vp[envs * self.A + a] = v[:, a]

    # ---- scan: the base scan, then noise and dropout (before the lidar_transform the device fuses into its store)
    def raycast(self, chunk_cars=2048):
        r = super().raycast(chunk_cars)
        if self.noise is None:
            return r
        sigma, p_drop, seed = self.noise
        cars = np.arange(self.NC)
        env = cars // self.A
        key = noise_car_key(seed, (cars + self.cfg.first_env * self.A).astype(np.uint64), self.episode[env], self.steps[env])
        return apply_noise(r, key, sigma, p_drop)

    # ---- dynamics: OracleRaceEnv._substep with the car's parameters as operands (same operations, same order)
    def _substep(self, envs, motor, steer):
        A = self.A
        for a in range(A):
            c = envs * A + a
            vp = self.vp[c]
            wheel_max, accel_max, drag, max_vel, steer_step = (vp[:, i] for i in range(5))
            m, s = motor[:, a], steer[:, a]
            v, delta, theta = self.v[c], self.delta[c], self.theta[c]
            force = np.abs(m) * accel_max
            acc = np.where(m >= f32(0.0), force, -force) - drag * v
            v = clamp32(v + acc * ro.DT, f32(0.0), max_vel)
            dd = clamp32(s * -wheel_max - delta, -steer_step, steer_step)
            delta = delta + dd
            sd, cd = sincos32(delta)
            omega = (v / ro.WHEELBASE) * (sd / cd)
            self.x[c] = self.x[c] + (v * self.ct[c]) * ro.DT
            self.y[c] = self.y[c] + (v * self.st[c]) * ro.DT
            theta = theta + omega * ro.DT
            theta = np.where(theta > ro.PI, theta - ro.TWO_PI, theta)
            theta = np.where(theta < -ro.PI, theta + ro.TWO_PI, theta)
            self.theta[c] = theta
            self.st[c], self.ct[c] = sincos32(theta)
            self.v[c], self.delta[c], self.omega[c] = v, delta, omega
            self.accel[c] = acc.astype(f32)
        self.steps[envs] += 1
        # --- collisions (H5)
        for a in range(A):
            c = envs * A + a
            self.wall[c] = self._wall_hit(c)
            self.opp[c] = 0
        for a in range(A):
            for b in range(a + 1, A):
                ca, cb_ = envs * A + a, envs * A + b
                o = self._obb_overlap(ca, cb_)
                self.opp[ca] |= o
                self.opp[cb_] |= o
        # --- progress / reward / done (H4, H15)
        cfg = self.cfg
        tlim = f32(cfg.time_limit)
        time = self.steps[envs].astype(f32) * ro.DT
        NC_ = ro.N_CHECKPOINTS
        for a in range(A):
            c = envs * A + a
            ix, iy = self._cell(self.x[c], self.y[c])
            p_new = self._lookup(self.progress_grid, ix, iy, f32(-1.0))
            p_old, lap_old, cp_old = self.progress[c], self.lap[c], self.cp[c]
            valid = p_new >= f32(0.0)
            p_new = np.where(valid, p_new, p_old)
            cp_new = np.minimum((p_new * f32(NC_)).astype(i32), NC_ - 1)
            d = np.mod(cp_new - cp_old, NC_)
            fwd = (d > 0) & (d <= NC_ // 2)
            bwd = d > NC_ // 2
            lap = lap_old + np.where(fwd & (cp_new < cp_old), 1, 0) - np.where(bwd & (cp_new > cp_old), 1, 0)
            lap = lap.astype(i32)
            self.wrong_way[c] = np.where(fwd, 0, np.where(bwd, 1, self.wrong_way[c]))
            self.cp[c] = np.where(fwd | bwd, cp_new, cp_old)
            self.lap[c], self.progress[c] = lap, p_new
            collided = (self.wall[c] | self.opp[c]).astype(bool)
            task = cfg.task_of(a)
            if task == ro.TASK_N_STEP_PROGRESS:
                slot = self.steps[envs] % cfg.n_steps
                total = (lap - 1).astype(f32) + p_new
                r = (total - self.nstep_hist[c, slot]) * ro.PROGRESS_REWARD
                self.nstep_hist[c, slot] = total
                done = np.zeros(envs.size, bool)
            elif task == ro.TASK_MAX_PROGRESS:
                delta_p = (lap - lap_old).astype(f32) + (p_new - p_old)
                r = delta_p * ro.PROGRESS_REWARD + np.where(collided, f32(cfg.collision_reward), f32(0.0))
                done = (collided & bool(cfg.terminate_on_collision)) | (lap > cfg.laps) | (time > tlim)
            else:
                r = np.where(self.wall[c].astype(bool), f32(-1.0), -exp32(np.abs(steer[:, a]) - self.v[c]))
                done = np.zeros(envs.size, bool)
            self.reward[c] = self.reward[c] + r.astype(f32)
            self.done[c] = done


def make_dr_oracle(track, **kw):
    env = DROracleEnv(track.occ, track.drivable, track.progress, track.centerline, track.origin, track.resolution,
                      ro.OracleConfig(**kw))
    env.frame_track = track
    return env
