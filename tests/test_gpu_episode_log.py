"""The episode log on the MI355X (include/racecar_hip.h, rc_episode_log_*): the device log against the NumPy restatement
(tests/episode_log_oracle.py) fed with the device's own per-call outputs - every column and every counter, unsorted - over the
ways a batch can be stepped; the ordering guarantee (byte-identical logs of two runs); overflow, quota and clear; that the log
only observes; and evaluate()."""
import ctypes as C

import numpy as np
import pytest

from episode_log_oracle import COLUMNS, COUNTERS, RECORD_KEYS, ROW_DTYPE, TRUNCATED, EpisodeLogOracle

pytestmark = pytest.mark.gpu

TRACKS = ("columbia", "austria", "barcelona")
WIDE_LO = (0.168, 2.0, 0.4, 3.0, 0.02)
WIDE_HI = (0.294, 8.0, 1.6, 8.0, 0.05)


def _record(env):
    """What the last call left in the (current) arena, on the host."""
    import torch
    torch.cuda.synchronize()
    return {k: env.views[k].cpu().numpy() for k in RECORD_KEYS}


def _tracks_of(env):
    tid = getattr(env, "track_id", None)
    return None if tid is None else tid.cpu().numpy()


def _raw_rows(env, n):
    import torch
    torch.cuda.synchronize()
    return env.episode_rows[:n].cpu().numpy().view(ROW_DTYPE).reshape(-1)


def _assert_log_equals(env, ora, what=""):
    """torch.equal on every column, every counter, and the raw bytes of the written rows - no sorting."""
    import torch
    counters = env.episode_counters
    assert counters == ora.counters, (what, counters, ora.counters)
    dev, rows = env.episode_log(), ora.log()
    assert set(dev) == set(COLUMNS)
    for name in COLUMNS:
        want = rows[name]
        want = torch.from_numpy(want.view(np.int32).copy() if want.dtype.kind == "u" else want.copy())
        got = dev[name].cpu()
        assert got.dtype == want.dtype and got.shape == want.shape, (what, name, got.dtype, got.shape, want.shape)
        assert torch.equal(got, want), (what, name)
    if hasattr(env, "episode_rows"):
        assert _raw_rows(env, counters["written"]).tobytes() == rows.tobytes(), what
    return rows


def _roll(env, ora, calls, step, first_call=0):
    for k in range(first_call, first_call + calls):
        step(k)
        ora.on_step(_record(env), track=_tracks_of(env))


@pytest.mark.parametrize("track,n,cars,car_tasks", [("austria", 4096, 1, None), ("columbia", 2048, 2, None),
                                                    ("austria", 1024, 4, ["maximize_progress", "n_step_progress", "max_speed", None])])
def test_log_equals_the_restatement(track, n, cars, car_tasks):
    """step_random, auto-reset, a 50-call time limit, 300 calls: at least 6 episodes per env."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv(track, n, cars, auto_reset=True, time_limit_steps=50, action_repeat=4, car_tasks=car_tasks)
    ora = EpisodeLogOracle(n, cars, capacity=n * cars * 24)
    env.enable_episode_log(n * cars * 24)
    env.reset(mode="random_ball" if cars > 1 else "random", seed=3)
    ora.on_reset()
    _roll(env, ora, 300, lambda k: env.step_random(17, k))
    rows = _assert_log_equals(env, ora, track)
    assert ora.counters["dropped"] == 0 and len(rows) >= 6 * n * cars
    assert np.bincount(rows["env"], minlength=n).min() >= 6 * cars
    assert ((rows["flags"] & TRUNCATED) == 0).any()          # crashes, not only time limits
    env.close()


def test_first_env_numbers_the_rows_and_a_second_enable_clears():
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n = 300
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, time_limit_steps=5, first_env=1000)
    ora = EpisodeLogOracle(n, 1, capacity=4 * n, first_env=1000)
    env.enable_episode_log(7)
    env.reset(mode="random", seed=1)
    ora.on_reset()
    env.enable_episode_log(4 * n)                # resize: clears, running episodes keep their sums
    _roll(env, ora, 12, lambda k: env.step_random(2, k))
    rows = _assert_log_equals(env, ora)
    assert rows["env"].min() == 1000 and rows["env"].max() == 1299 and len(rows) >= 2 * n
    env.close()


def test_auto_reset_off_a_frozen_tail_and_a_masked_reset():
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n, cars = 512, 2
    env = BatchedRaceEnv("columbia", n, cars, auto_reset=False, time_limit_steps=30, action_repeat=4)
    ora = EpisodeLogOracle(n, cars, capacity=8 * n * cars)
    env.enable_episode_log(8 * n * cars)
    env.reset(mode="random_ball", seed=5)
    ora.on_reset()
    _roll(env, ora, 20, lambda k: env.step_random(9, k))
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)          # running and finished envs alike
    env.reset(mask=mask, mode="random_ball", seed=6)
    ora.on_reset(mask=mask)
    assert 0 < ora.counters["abandoned"] <= int(mask.sum())
    _roll(env, ora, 45, lambda k: env.step_random(9, k), first_call=20)          # every env ends by call 50; the rest is frozen tail
    rows = _assert_log_equals(env, ora)
    assert len(rows) == (n + int(mask.sum()) - ora.counters["abandoned"]) * cars
    assert torch.all(env.views["done"].amax(1) == 1)
    env.close()


def test_track_set_in_random_order_latches_the_track():
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    n = 1024
    env = BatchedRaceEnv.with_track_set([load_track(t) for t in TRACKS], n, 1, order="random", seed=(5 << 32) | 3, auto_reset=True,
                                        time_limit_steps=25, action_repeat=4)
    ora = EpisodeLogOracle(n, 1, capacity=n * 16)
    env.enable_episode_log(n * 16)
    env.reset(mode="random", seed=13)
    ora.on_reset(track=_tracks_of(env))
    _roll(env, ora, 200, lambda k: env.step_random(4, k))
    rows = _assert_log_equals(env, ora)
    assert set(np.unique(rows["track"])) == {0, 1, 2} and len(rows) >= 8 * n
    env.close()


def test_mixed_track_env_merges_its_blocks():
    from racing_dreamer_amd.batched_env import MixedTrackEnv
    sizes = [300, 500, 224]
    env = MixedTrackEnv(list(TRACKS), sizes, auto_reset=True, time_limit_steps=20, action_repeat=4)
    n = sum(sizes)
    ora = EpisodeLogOracle(n, 1, capacity=n * 24)
    env.enable_episode_log(n * 24)
    env.reset(mode="random", seed=2)
    ora.on_reset(track=_tracks_of(env))
    _roll(env, ora, 100, lambda k: env.step_random(8, k))
    rows = _assert_log_equals(env, ora)
    assert len(rows) >= 5 * n and set(np.unique(rows["track"])) == {0, 1, 2}
    env.close()


def test_with_vehicle_randomization_and_lidar_noise():
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n = 1024
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, time_limit_steps=40, action_repeat=4,
                         vehicle_randomization=(WIDE_LO, WIDE_HI, 21), lidar_noise=(0.2, 0.03, 8))
    ora = EpisodeLogOracle(n, 1, capacity=n * 12)
    env.enable_episode_log(n * 12)
    env.reset(mode="random", seed=3)
    ora.on_reset()
    _roll(env, ora, 150, lambda k: env.step_random(5, k))
    assert len(_assert_log_equals(env, ora)) >= 3 * n
    env.close()


def test_under_a_trajectory_ring():
    """The arena is re-pointed before every step: the log reads whichever is current."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.replay import TrajectoryRing
    n = 512
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, time_limit_steps=30, action_repeat=4)
    ring = TrajectoryRing(env, 5)
    ora = EpisodeLogOracle(n, 1, capacity=n * 8)
    env.enable_episode_log(n * 8)
    ring.reset(mode="random", seed=3)
    ora.on_reset()
    _roll(env, ora, 100, lambda k: ring.step_random(5, k))
    assert len(_assert_log_equals(env, ora)) >= 3 * n
    env.close()


@pytest.mark.parametrize("agent", ["policy_act", "follow_the_gap_reference"])
def test_driven_by_the_device_agents(agent):
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from test_golden_policy import weights
    n = 512
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, time_limit_steps=60, action_repeat=8, remap_actions=True)
    if agent == "policy_act":
        env.load_policy(weights("austria"))
    ora = EpisodeLogOracle(n, 1, capacity=n * 16)
    env.enable_episode_log(n * 16)
    env.reset(mode="random", seed=3)
    ora.on_reset()

    def step(k):
        getattr(env, agent)()
        env.step(None)
    _roll(env, ora, 130, step)
    rows = _assert_log_equals(env, ora, agent)
    assert len(rows) >= 2 * n and rows["progress"].max() > 0.05
    env.close()


def _run_twice_bytes(n, cars, calls):
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    out = []
    for _ in range(2):
        env = BatchedRaceEnv("austria", n, cars, auto_reset=True, time_limit_steps=20, action_repeat=4)
        env.enable_episode_log(n * cars * 8)
        env.reset(mode="random_ball" if cars > 1 else "random", seed=3)
        for k in range(calls):
            env.step_random(17, k)
        torch.cuda.synchronize()
        out.append((env.episode_rows.cpu().numpy().tobytes(), env.episode_counters))
        env.close()
    return out


def test_two_runs_give_byte_identical_row_buffers():
    """The ordering guarantee: 20 000 envs (79 workgroups, 313 waves) whose episodes end in bursts and in between."""
    (a, ca), (b, cb) = _run_twice_bytes(20000, 2, 90)
    assert ca == cb and ca["written"] >= 4 * 20000 * 2 and ca["dropped"] == 0
    assert a == b
    rows = np.frombuffer(a, ROW_DTYPE)[:ca["written"]]
    key = rows["call"].astype(np.int64) * 40000 + rows["env"].astype(np.int64) * 2 + rows["slot"]
    assert (np.diff(key) > 0).all()


def test_overflow_quota_and_clear_on_the_device():
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n, cars = 1000, 2
    env = BatchedRaceEnv("austria", n, cars, auto_reset=True, time_limit_steps=10, action_repeat=4)
    # overflow: room for one and a half bursts
    ora = EpisodeLogOracle(n, cars, capacity=3001)
    env.enable_episode_log(3001)
    env.reset(mode="random_ball", seed=3)
    ora.on_reset()
    _roll(env, ora, 35, lambda k: env.step_random(1, k))
    _assert_log_equals(env, ora, "overflow")
    assert ora.counters["written"] == 3001 and ora.counters["dropped"] >= 2 * n * cars - 1001
    # clear mid-run: ordinals and calls restart, the running episodes keep their sums
    env.clear_episode_log()
    ora.clear()
    _roll(env, ora, 7, lambda k: env.step_random(1, k), first_call=35)
    rows = _assert_log_equals(env, ora, "clear")
    assert len(rows) > 0 and (rows["episode"] == 0).all() and rows["call"].max() < 7 and rows["length"].max() == 10
    # quota: the first 2 episodes of every env, exactly
    ora = EpisodeLogOracle(n, cars, capacity=2 * n * cars, max_episodes=2)
    env.enable_episode_log(2 * n * cars, max_episodes=2)
    env.reset(mode="random_ball", seed=4)
    ora.on_reset()
    assert env.episode_counters["abandoned"] == n          # the second enable cleared the counters, the reset after it abandoned
    ora.counters["abandoned"] = n                          # the n episodes that were running (the fresh restatement saw none)
    _roll(env, ora, 35, lambda k: env.step_random(2, k))
    rows = _assert_log_equals(env, ora, "quota")
    assert len(rows) == 2 * n * cars and ora.counters["envs_at_quota"] == n and ora.counters["skipped"] >= n * cars
    assert ora.counters["dropped"] == 0 and rows["episode"].max() == 1
    env.close()


def test_off_is_off():
    """The log observes, it never changes a step: after 50 calls every arena byte of an env that never had a log, of one whose
    log was enabled and then disabled, and of one with the log on is the same; rc_arena_bytes does not depend on it."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n, cars = 2048, 2
    kw = dict(auto_reset=True, time_limit_steps=15, action_repeat=4, obs_type="lidar_occupancy")
    never, toggled, on = (BatchedRaceEnv("columbia", n, cars, **kw) for _ in range(3))
    before = never._lib.rc_arena_bytes(C.byref(never._cfg))
    on.enable_episode_log(n * cars * 4)
    toggled.enable_episode_log(64)
    for env in (never, toggled, on):
        env.reset(mode="random_ball", seed=3)
    for k in range(50):
        if k == 10:
            toggled.disable_episode_log()
        for env in (never, toggled, on):
            env.step_random(5, k)
    torch.cuda.synchronize()
    assert on.episode_counters["written"] >= 3 * n * cars
    assert torch.equal(never._arena_view, on._arena_view) and torch.equal(never._arena_view, toggled._arena_view)
    assert never._lib.rc_arena_bytes(C.byref(on._cfg)) == before == on.arena_nbytes
    with pytest.raises(Exception, match="not enabled"):
        toggled.episode_log()
    for env in (never, toggled, on):
        env.close()


def test_reading_before_enable_is_an_error_code():
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 4, 1)
    rows, cap, ctr, nb = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
    assert env._lib.rc_episode_log(env._h, C.byref(rows), C.byref(cap), C.byref(ctr), C.byref(nb)) == -1
    assert b"not enabled" in env._lib.rc_last_error()
    assert env._lib.rc_episode_log_clear(env._h) == -1 and b"not enabled" in env._lib.rc_last_error()
    assert env._lib.rc_episode_log_enable(env._h, 0, 0) == -1 and b"capacity_rows" in env._lib.rc_last_error()
    assert env._lib.rc_episode_log_disable(env._h) == 0
    env.close()


def test_evaluate_on_a_track_set():
    """512 envs on a 3-track set, the reference's follow-the-gap agent, 2 episodes per env: evaluate()'s statistics against the same
    quantities computed from the raw log with NumPy on the host."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.evaluate import evaluate
    from racing_dreamer_amd.track_assets import load_track
    n = 512
    env = BatchedRaceEnv.with_track_set([load_track(t) for t in TRACKS], n, 1, order="sequential", auto_reset=True, time_limit_steps=150,
                                        action_repeat=8, remap_actions=True)
    res = evaluate(env, lambda e: e.follow_the_gap_reference(), episodes=2, seed=7, reset_mode="random")
    counters = env.episode_counters
    assert counters["written"] == 2 * n and counters["envs_at_quota"] == n and counters["dropped"] == 0
    assert res["unfinished_envs"] == 0 and res["tracks"] == 3 and res["calls"] <= 2 * 150 + 32
    rows = _raw_rows(env, counters["written"])
    assert len(rows) == 2 * n and rows["episode"].max() == 1 and np.bincount(rows["env"], minlength=n).tolist() == [2] * n
    for t in range(3):
        g = rows[rows["track"] == t]
        assert res["episodes"][t, 0].item() == len(g) > 0
        for name in ("ret", "length", "progress", "time"):
            x = g[name].astype(np.float64)
            for stat, want in (("mean", x.mean()), ("std", x.std()), ("min", x.min()), ("max", x.max())):
                got = res[f"{name}_{stat}"][t, 0].item()
                assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (t, name, stat, got, want)       # binary64 on both sides
        for cause, bit in (("wall", 1), ("opponent", 2), ("truncated", 4), ("wrong_way", 8), ("own_done", 16)):
            assert abs(res[f"share_{cause}"][t, 0].item() - ((g["flags"] & bit) != 0).mean()) <= 1e-12
    assert res["progress_mean"].max().item() > 0.02          # the agent drives
    env.close()


@pytest.mark.gpu_slow
def test_log_equals_the_restatement_at_65536_envs():
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n = 65536
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, time_limit_steps=50, action_repeat=4)
    ora = EpisodeLogOracle(n, 1, capacity=n * 8)
    env.enable_episode_log(n * 8)
    env.reset(mode="random", seed=3)
    ora.on_reset()
    _roll(env, ora, 200, lambda k: env.step_random(17, k))
    assert len(_assert_log_equals(env, ora)) >= 4 * n
    env.close()
