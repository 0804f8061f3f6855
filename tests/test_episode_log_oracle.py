"""Episode log, CPU side: the NumPy restatement (tests/episode_log_oracle.py) that the GPU tests compare the device log with,
checked against the reference's own definitions (dreamer/callbacks.py:56-100) applied to `trajectory.EpisodeRecorder` episodes,
its rules on hand-built records, and the C-ABI surface (include/racecar_hip.h, rc_episode_log_*)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from episode_log_oracle import (COUNTERS, OPPONENT, OWN_DONE, RECORD_KEYS, ROW_DTYPE, TRUNCATED, WALL, WRONG_WAY, EpisodeLogOracle,
                                reference_summary)
from oracle import c_oracle
from oracle import racecar_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rc_episode_log_enable", "rc_episode_log_disable", "rc_episode_log", "rc_episode_log_clear", "rc_episode_log_time")


def _publish(out, B, A):
    """The oracle's outputs as [num_envs, cars_per_env, ...] tensors (what BatchedRaceEnv.views are)."""
    return {k: torch.from_numpy(np.asarray(v).reshape(B, A, *np.asarray(v).shape[1:]).copy()) for k, v in out.items()}


@pytest.mark.parametrize("cars", [1, 2])
def test_restatement_equals_the_reference_definitions_on_recorded_episodes(cars):
    """64 envs x {1, 2} cars of the CPU oracle with auto-reset and a 40-call time limit, random actions, 200 calls: every row of
    the restatement against summarize_episode's definitions on the EpisodeRecorder episode of the same env and car."""
    from racing_dreamer_amd.track_assets import load_track
    from racing_dreamer_amd.trajectory import EpisodeRecorder
    t = load_track("austria")
    B, A, calls = 64, cars, 200
    cfg = ro.OracleConfig(num_envs=B, cars_per_env=A, auto_reset=True, time_limit_steps=40)
    env = c_oracle.COracleEnv(t.occ, t.drivable, t.progress, t.centerline, t.origin, t.resolution, cfg)
    log = EpisodeLogOracle(B, A, capacity=B * A * calls)
    recorders = [EpisodeRecorder(B, A, range(B), car=a) for a in range(A)]
    episodes = [[[] for _ in range(B)] for _ in range(A)]          # [car][env] -> the episodes in order

    def record_view(views):
        # an episode is the env's (Collect fires for every agent when the env is done): the recorder of a car whose team-mate
        # ended the episode sees the env's done
        v = dict(views)
        v["done"] = views["done"].amax(1, keepdim=True).expand(B, A)
        return v

    views = _publish(env.reset(mode=2 if A > 1 else 1, seed=11), B, A)
    log.on_reset()
    for r in recorders:
        r.on_reset(views)
    for k in range(calls):
        act = env.random_actions(5, k)
        act[:, 0] = np.abs(act[:, 0])                                # throttle only, 8 sub-steps per call: cars reach the walls
        views = _publish(env.step(act, repeat=8), B, A)
        log.on_step({key: views[key].numpy() for key in RECORD_KEYS})
        v = record_view(views)
        for a, r in enumerate(recorders):
            # the recorder returns the finished episodes in env order; which envs finished is the env-level done
            ended = np.nonzero(v["done"][:, a].numpy())[0]
            eps = r.on_step(v)
            assert len(eps) == len(ended)
            for e, ep in zip(ended, eps):
                episodes[a][e].append(ep)
    rows = log.log()
    assert log.counters["written"] == len(rows) >= 5 * B * A          # time_limit_steps = 40: at least 5 episodes per env in 200 calls
    assert log.counters["dropped"] == log.counters["skipped"] == log.counters["abandoned"] == 0 and log.counters["calls"] == calls
    # ordered by call, then env, then slot - strictly
    key = rows["call"].astype(np.int64) * B * A + rows["env"].astype(np.int64) * A + rows["slot"]
    assert (np.diff(key) > 0).all()
    team_mate = crashed = 0
    for row in rows:
        ep = episodes[row["slot"]][row["env"]][row["episode"]]
        ret64, length, progress, time = reference_summary(ep)
        assert row["length"] == length and 1 <= length <= 40
        assert row["progress"] == progress and row["time"] == time
        bound = length * 2.0 ** -24 * float(np.abs(ep["reward"].astype(np.float64)).sum())      # sequential binary32 sum, first order
        assert abs(float(row["ret"]) - ret64) <= bound, (row, ret64, bound)
        assert bool(row["flags"] & TRUNCATED) == (length == 40)
        team_mate += not (row["flags"] & OWN_DONE)
        crashed += bool(row["flags"] & (WALL | OPPONENT))
    for a in range(A):
        for e in range(B):
            assert len(episodes[a][e]) == int((rows["env"] == e).sum()) // A
    assert crashed >= B                # not every episode ran into the time limit
    if A == 2:
        assert team_mate > 0          # some episodes ended on the other car's collision


def _rec(B, A, **kw):
    r = {k: np.zeros((B, A), np.float32 if k in ("reward", "progress_total", "time") else np.int32) for k in RECORD_KEYS}
    r["lap"] += 1
    for k, v in kw.items():
        r[k] = np.asarray(v, r[k].dtype).reshape(B, A)
    return r


def test_an_episode_is_logged_once_while_the_env_is_frozen():
    log = EpisodeLogOracle(2, 1, capacity=8)
    log.on_reset()
    log.on_step(_rec(2, 1, reward=[1, 2], progress_total=[0.1, 0.2], time=[0.01, 0.01]))
    log.on_step(_rec(2, 1, reward=[1, 2], progress_total=[0.3, 0.1], time=[0.02, 0.02], done=[1, 0], wall_collision=[1, 0], wrong_way=[0, 1]))
    for _ in range(3):                # env 0 frozen: done stays 1, reward 0, fresh 0
        log.on_step(_rec(2, 1, reward=[0, 2], progress_total=[0.3, 0.15], time=[0.02, 0.03], done=[1, 0]))
    rows = log.log()
    assert len(rows) == 1 and log.counters == dict(written=1, dropped=0, skipped=0, abandoned=0, envs_at_quota=0, calls=5)
    r = rows[0]
    assert (r["env"], r["slot"], r["track"], r["episode"], r["call"], r["length"], r["laps"]) == (0, 0, 0, 0, 1, 2, 0)
    assert r["ret"] == 2 and r["progress"] == np.float32(0.3) and r["time"] == np.float32(0.02) and r["flags"] == WALL | OWN_DONE
    # env 1 ends later: progress is the maximum (not the last value), wrong_way is remembered, the return has every call
    log.on_step(_rec(2, 1, reward=[0, 2], progress_total=[0.3, 0.05], time=[0.02, 0.04], done=[1, 1], truncated=[0, 1]))
    r = log.log()[1]
    assert (r["env"], r["call"], r["length"], r["ret"], r["progress"]) == (1, 5, 6, 12, np.float32(0.2))
    assert r["flags"] == TRUNCATED | WRONG_WAY | OWN_DONE
    # a reset of a frozen env abandons nothing and starts a new episode with ordinal 1
    log.on_reset(mask=[1, 0])
    assert log.counters["abandoned"] == 0
    log.on_step(_rec(2, 1, reward=[5, 0], done=[1, 1]))
    r = log.log()[2]
    assert len(log.log()) == 3 and (r["env"], r["episode"], r["length"], r["ret"], r["progress"]) == (0, 1, 1, 5, 0)


def test_reset_row_values_and_enabling_mid_episode():
    log = EpisodeLogOracle(1, 1, capacity=4)
    # no reset seen: the partial episode is not logged, the auto-reset inside the call (fresh = 1) starts the first one
    log.on_step(_rec(1, 1, reward=[3]))
    log.on_step(_rec(1, 1, reward=[3], done=[1], fresh=[1]))
    assert len(log.log()) == 0 and log.counters["calls"] == 2
    log.on_step(_rec(1, 1, reward=[-0.5], progress_total=[-2.0], time=[0.0], done=[1], fresh=[1]))
    r = log.log()[0]
    assert (r["episode"], r["call"], r["length"], r["ret"], r["progress"], r["time"]) == (0, 2, 1, -0.5, -1.0, 0.0)      # max with the reset row's -1


def test_masked_reset_mid_episode_is_abandoned():
    log = EpisodeLogOracle(3, 1, capacity=4)
    log.on_reset()
    log.on_step(_rec(3, 1, reward=[1, 1, 1]))
    log.on_reset(mask=[0, 1, 1])
    assert log.counters["abandoned"] == 2 and log.counters["written"] == 0
    log.on_step(_rec(3, 1, reward=[1, 1, 1], done=[1, 1, 0]))
    rows = log.log()
    assert list(rows["ret"]) == [2, 1] and list(rows["length"]) == [2, 1] and list(rows["episode"]) == [0, 0]


def test_capacity_overflow_keeps_the_first_rows_and_counts_the_rest():
    log = EpisodeLogOracle(4, 2, capacity=5)
    log.on_reset()
    log.on_step(_rec(4, 2, reward=np.arange(8), done=[1, 0, 0, 0, 1, 1, 0, 0], fresh=np.ones(8)))     # envs 0, 2: 4 rows
    first = log.log().copy()
    log.on_step(_rec(4, 2, reward=np.arange(8), done=np.ones(8), fresh=np.ones(8)))                   # 8 rows asked, 1 fits
    rows = log.log()
    assert log.counters["written"] == 5 and log.counters["dropped"] == 7
    assert np.array_equal(rows[:4], first) and list(first["env"]) == [0, 0, 2, 2] and list(first["slot"]) == [0, 1, 0, 1]
    assert (rows[4]["env"], rows[4]["slot"], rows[4]["episode"], rows[4]["call"]) == (0, 0, 1, 1)
    log.clear()
    assert log.counters == dict.fromkeys(COUNTERS, 0) and len(log.log()) == 0
    log.on_step(_rec(4, 2, reward=np.ones(8), done=np.ones(8), fresh=np.ones(8)))
    assert log.counters["written"] == 5 and log.counters["dropped"] == 3 and (log.log()["episode"] == 0).all() and (log.log()["call"] == 0).all()


def test_quota_skips_later_episodes_and_counts_the_envs_that_reached_it():
    log = EpisodeLogOracle(3, 1, capacity=6, max_episodes=2)
    log.on_reset()
    for k in range(4):                # env 0 ends every call, env 1 every second call, env 2 never
        log.on_step(_rec(3, 1, reward=[1, 1, 1], done=[1, k % 2, 0], fresh=[1, k % 2, 0]))
    assert log.counters["envs_at_quota"] == 2 and log.counters["skipped"] == 2 and log.counters["written"] == 4
    assert list(log.log()["env"]) == [0, 0, 1, 1] and list(log.log()["episode"]) == [0, 1, 0, 1] and list(log.log()["call"]) == [0, 1, 1, 3]


def test_team_mate_ending_and_terminal_flags():
    log = EpisodeLogOracle(1, 2, capacity=4)
    log.on_reset()
    log.on_step(_rec(1, 2, reward=[1, 2], lap=[2, 1], done=[0, 1], opponent_collision=[1, 1], fresh=[1, 1]))
    rows = log.log()
    assert list(rows["flags"]) == [OPPONENT, OPPONENT | OWN_DONE] and list(rows["laps"]) == [1, 0] and list(rows["slot"]) == [0, 1]


def test_track_is_latched_at_the_start_under_a_track_set():
    """Over tests/track_set_oracle.py: after an auto-reset the env's track id already names the next episode's track; the row
    carries the one the episode was driven on."""
    from racing_dreamer_amd.track_assets import load_track
    from track_set_oracle import make_track_set_oracle
    B = 7
    ts = make_track_set_oracle([load_track(n) for n in ("columbia", "austria", "barcelona")], num_envs=B, auto_reset=True, time_limit_steps=3)
    log = EpisodeLogOracle(B, 1, capacity=64)
    out = ts.reset(mode=1, seed=1)
    log.on_reset(track=out["track_id"])
    driven = [out["track_id"].copy()]
    for k in range(9):
        out = ts.step(np.zeros((B, 2), np.float32))
        log.on_step({key: np.asarray(out[key]) for key in RECORD_KEYS}, track=out["track_id"])
        driven.append(out["track_id"].copy())
    rows = log.log()
    assert len(rows) == 3 * B and list(rows["call"]) == [2] * B + [5] * B + [8] * B
    for s in range(3):                # sequential order: episode s of env e ran on (initial + s) mod 3, not on the id seen at its end
        assert list(rows["track"][s * B:(s + 1) * B]) == list((driven[0] + s) % 3)
        assert list(driven[3 * s + 3]) == list((driven[0] + s + 1) % 3)
    assert (rows["flags"] == TRUNCATED | OWN_DONE).all() and (rows["length"] == 3).all()


# ---- header / binding ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(hip_lib):
    from racing_dreamer_amd import _lib
    text = open(os.path.join(ROOT, "include", "racecar_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(hip_lib, name) and name in _lib.SYMBOLS, name
    assert "callbacks.py:56-100" in text
    assert "RC_K_POLICY = 6, RC_K_COUNT = 7" in code and "#define RC_ABI_VERSION 3" in code       # no new timer, no ABI bump
    assert hip_lib.rc_abi_version() == 3


def test_row_is_48_bytes_and_matches_the_restatement():
    from racing_dreamer_amd import _lib
    assert C.sizeof(_lib.RcEpisodeRow) == 48 == ROW_DTYPE.itemsize
    assert [n for n, _ in _lib.RcEpisodeRow._fields_] == list(ROW_DTYPE.names)
    for name, ctype in _lib.RcEpisodeRow._fields_:
        assert getattr(_lib.RcEpisodeRow, name).offset == ROW_DTYPE.fields[name][1]
        assert np.dtype(ctype) == ROW_DTYPE.fields[name][0]
    assert _lib.EPISODE_COUNTERS == COUNTERS
    assert (_lib.EP_WALL, _lib.EP_OPPONENT, _lib.EP_TRUNCATED, _lib.EP_WRONG_WAY, _lib.EP_OWN_DONE) == (WALL, OPPONENT, TRUNCATED, WRONG_WAY, OWN_DONE)
    header = open(os.path.join(ROOT, "include", "racecar_hip.h")).read()
    body = re.search(r"typedef struct rc_episode_row \{(.*?)\} rc_episode_row;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == list(ROW_DTYPE.names)


def test_misuse_returns_codes_with_messages(hip_lib):
    """The paths that need no device: NULL env on every entry point, capacity < 1 (checked before the handle).  A log that is
    read before it is enabled needs a handle: tests/test_gpu_episode_log.py."""
    assert hip_lib.rc_episode_log_enable(None, 16, 0) == -1 and b"env is NULL" in hip_lib.rc_last_error()
    assert hip_lib.rc_episode_log_enable(None, 0, 0) == -1 and b"capacity_rows" in hip_lib.rc_last_error()
    assert hip_lib.rc_episode_log_enable(None, 16, -1) == -1 and b"max_episodes" in hip_lib.rc_last_error()
    rows, cap, ctr, nb = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
    assert hip_lib.rc_episode_log(None, C.byref(rows), C.byref(cap), C.byref(ctr), C.byref(nb)) == -1 and b"env is NULL" in hip_lib.rc_last_error()
    assert hip_lib.rc_episode_log_clear(None) == -1 and hip_lib.rc_episode_log_disable(None) == -1
    assert hip_lib.rc_episode_log_time(None, None, None) == -1
    assert rows.value is None and ctr.value is None
