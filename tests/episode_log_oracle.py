"""Test-side restatement of the episode log (include/racecar_hip.h, rc_episode_log_*) in NumPy: a pure function of the per-call
record - reward, done, truncated, wall_collision, opponent_collision, wrong_way, progress_total, time, lap, fresh as the step
leaves them in the arena, the env's track ids, and the reset events.  It produces the rows in order plus the counters.

What it restates (dreamer/callbacks.py:56-100 of the reference: return = reward.sum(), length = len(reward) - 1, progress =
max(progress), time = max(time), over an episode that starts with the reset row reward 0 / progress -1 / time 0):
  - an episode is an env's: it ends for all its cars in the call in which any car's done is 1;
  - an env is followed from a reset on (`on_reset`, or a call that ends with fresh = 1: the auto-reset inside a step);
  - without auto-reset (done = 1, fresh = 0) the env is frozen: one row per car, nothing more until it is reset;
  - `on_reset` of an env whose episode is running counts one abandoned episode and starts anew;
  - rows of one call by env, then slot; position = rows asked for so far; rows beyond the capacity are dropped, an episode whose
    ordinal has reached the quota is skipped.
"""
import numpy as np

ROW_DTYPE = np.dtype([("env", "<i4"), ("slot", "<i4"), ("track", "<i4"), ("episode", "<u4"), ("call", "<u4"), ("length", "<i4"),
                      ("ret", "<f4"), ("progress", "<f4"), ("time", "<f4"), ("laps", "<i4"), ("flags", "<u4"), ("reserved", "<u4")])
assert ROW_DTYPE.itemsize == 48
COLUMNS = tuple(n for n in ROW_DTYPE.names if n != "reserved")
COUNTERS = ("written", "dropped", "skipped", "abandoned", "envs_at_quota", "calls")
WALL, OPPONENT, TRUNCATED, WRONG_WAY, OWN_DONE = 1, 2, 4, 8, 16
RECORD_KEYS = ("reward", "done", "truncated", "wall_collision", "opponent_collision", "wrong_way", "progress_total", "time", "lap", "fresh")


class EpisodeLogOracle:
    def __init__(self, num_envs, cars_per_env, capacity, max_episodes=0, first_env=0):
        self.B, self.A, self.capacity, self.quota, self.first_env = int(num_envs), int(cars_per_env), int(capacity), int(max_episodes), int(first_env)
        self.active = np.zeros(self.B, bool)
        self.length = np.zeros(self.B, np.int32)
        self.track = np.zeros(self.B, np.int32)
        self.ret = np.zeros((self.B, self.A), np.float32)
        self.prog = np.zeros((self.B, self.A), np.float32)
        self.time = np.zeros((self.B, self.A), np.float32)
        self.wrong = np.zeros((self.B, self.A), bool)
        self.clear()

    def clear(self):
        """Rows, counters and ordinals to zero; running episodes keep their sums."""
        self.rows = np.zeros(self.capacity, ROW_DTYPE)
        self.ordinal = np.zeros(self.B, np.uint32)
        self.asked = 0
        self.counters = dict.fromkeys(COUNTERS, 0)

    def _start(self, envs, track):
        self.ret[envs] = np.float32(0.0)
        self.prog[envs] = np.float32(-1.0)
        self.time[envs] = np.float32(0.0)
        self.wrong[envs] = False
        self.length[envs] = 0
        self.track[envs] = 0 if track is None else np.asarray(track, np.int32).reshape(self.B)[envs]
        self.active[envs] = True

    def on_reset(self, mask=None, track=None):
        """rc_reset of the envs in `mask` (None = all); `track` = the track ids after that reset (None without a track set)."""
        sel = np.ones(self.B, bool) if mask is None else np.asarray(mask).reshape(self.B).astype(bool)
        self.counters["abandoned"] += int((sel & self.active).sum())
        self._start(np.nonzero(sel)[0], track)

    def on_step(self, rec, track=None):
        """One step call.  rec: mapping of RECORD_KEYS -> array [num_envs, cars_per_env] (or flat) as the call left them;
        `track` = the track ids after the call."""
        B, A = self.B, self.A
        r = {k: np.asarray(rec[k]).reshape(B, A) for k in RECORD_KEYS}
        call = self.counters["calls"]
        done = r["done"] != 0
        ended = done.any(1)
        act = self.active.copy()
        # sums of the running episodes, in call order, one binary32 rounding per addition
        ret = (self.ret + r["reward"].astype(np.float32)).astype(np.float32)
        prog = np.maximum(self.prog, r["progress_total"].astype(np.float32))
        time = np.maximum(self.time, r["time"].astype(np.float32))
        wrong = self.wrong | (r["wrong_way"] != 0)
        length = self.length + 1
        run = act & ~ended
        self.ret[run], self.prog[run], self.time[run], self.wrong[run], self.length[run] = ret[run], prog[run], time[run], wrong[run], length[run]
        in_quota = (self.ordinal < self.quota) if self.quota else np.ones(B, bool)
        logs = act & ended & in_quota
        skips = act & ended & ~in_quota
        self.counters["skipped"] += int(skips.sum()) * A
        if self.quota:
            self.counters["envs_at_quota"] += int((act & ended & (self.ordinal + 1 == self.quota)).sum())
        envs = np.nonzero(logs)[0]                       # ascending: by env, then slot
        if envs.size:
            rows = np.zeros((envs.size, A), ROW_DTYPE)
            rows["env"] = (self.first_env + envs)[:, None]
            rows["slot"] = np.arange(A)[None, :]
            rows["track"] = self.track[envs][:, None]
            rows["episode"] = self.ordinal[envs][:, None]
            rows["call"] = call & 0xFFFFFFFF
            rows["length"] = length[envs][:, None]
            rows["ret"], rows["progress"], rows["time"] = ret[envs], prog[envs], time[envs]
            rows["laps"] = r["lap"][envs].astype(np.int32) - 1
            rows["flags"] = ((r["wall_collision"][envs] != 0) * WALL + (r["opponent_collision"][envs] != 0) * OPPONENT +
                             (r["truncated"][envs] != 0) * TRUNCATED + wrong[envs] * WRONG_WAY + done[envs] * OWN_DONE).astype(np.uint32)
            rows = rows.reshape(-1)
            fit = max(0, min(rows.size, self.capacity - self.asked))
            self.rows[self.asked:self.asked + fit] = rows[:fit]
            self.asked += rows.size
        self.ordinal[act & ended] += 1
        self.counters["written"] = min(self.asked, self.capacity)
        self.counters["dropped"] = self.asked - self.counters["written"]
        self.counters["calls"] = call + 1
        # respawned inside the call: the next episode starts here, on the track the env has now; else frozen until a reset
        fresh = r["fresh"][:, 0] != 0
        self.active[ended & ~fresh] = False
        self._start(np.nonzero(ended & fresh)[0], track)

    def log(self):
        """The written rows (structured array, in order)."""
        return self.rows[:self.counters["written"]]


def reference_summary(ep):
    """dreamer/callbacks.py:56-100 on one recorded episode dict (trajectory.EpisodeRecorder): (return in binary64, length, progress,
    time)."""
    reward = np.asarray(ep["reward"], np.float32)
    return float(reward.astype(np.float64).sum()), len(reward) - 1, np.float32(np.max(ep["progress"])), np.float32(np.max(ep["time"]))
