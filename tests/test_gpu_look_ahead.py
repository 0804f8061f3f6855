"""The look-ahead on the MI355X (include/racecar_hip.h, rc_look_ahead): every output against the test-side
restatement (tests/look_ahead_oracle.py) bit for bit, against the device's own step, its purity, the planner built on it and
the refusals.  The cases, their seeds and what they cover: tests/look_ahead_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import look_ahead_cases as lc
from look_ahead_oracle import DONE, OUTPUTS, WALL, flags_of, look_ahead

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICY = os.path.join(ROOT, "tests", "golden", "dreamer_policy_austria.npz")
RC_ERR_INVALID, RC_ERR_NEEDS_RESET = -1, -4          # include/racecar_hip.h
WIDE_LO = (0.168, 2.0, 0.4, 3.0, 0.02)
WIDE_HI = (0.294, 8.0, 1.6, 8.0, 0.05)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_equal(got, want, context=""):
    """Device tensors by name against the restatement's arrays: dtype, shape and every bit (a +0.0 is not a -0.0)."""
    import torch
    torch.cuda.synchronize()
    for name in want:
        d, o = got[name].cpu().numpy(), want[name]
        assert d.dtype == o.dtype and d.shape == o.shape, (context, name, d.dtype, d.shape, o.dtype, o.shape)
        bad = np.argwhere(_bits(d) != _bits(o))
        assert bad.size == 0, f"{context}: {name} differs in {len(bad)} places, first at {bad[0].tolist()}: {d[tuple(bad[0])]!r} != {o[tuple(bad[0])]!r}"


def _look(env, actions, **kw):
    import torch
    return env.look_ahead(torch.from_numpy(np.array(actions)).to(env.device), repeat=lc.REPEAT, outputs=OUTPUTS, **kw)      # (a copy: the cases' arrays are read-only)


# ---- 1, 2: bit-exact against the restatement, and what the cases cover
@pytest.mark.parametrize("name", list(lc.CASES))
def test_every_output_equals_the_restatement(name):
    ora, actions, want = lc.case(name)
    end = lc.endings(want)
    if name == "wide":
        assert end["wall"] >= 1 and end["unfinished"] >= 1, end
        assert actions.shape[0] * actions.shape[1] == 259                # more lanes than one workgroup holds
    if name == "a2":
        assert end["opponent"] >= 1 and end["unfinished"] >= 1, end
    if name in ("a4", "nstep", "long"):
        assert end["wall"] + end["opponent"] >= 1, end
    if name == "time_limit":
        assert end["truncated"] >= 1 and (want["length"] < actions.shape[2]).any(), end
    env = lc.device_env(name)
    _assert_equal(_look(env, actions), want, name)
    if actions.shape[3] == 1:                                            # [E, K, H, 2] is accepted with one car per env
        _assert_equal(_look(env, actions[:, :, :, 0]), want, name + " 4-d")
    env.close()


# ---- 3: against the device's own step
@pytest.mark.parametrize("name", ["wide", "a2", "nstep"])
def test_the_live_env_under_candidate_1_follows_the_look_ahead(name):
    import torch
    E, K, H, A = lc.CASES[name][:4]
    _ora, actions, want = lc.case(name)
    env = lc.device_env(name)
    got = {k: v.cpu().numpy() for k, v in _look(env, actions).items()}
    k = 1
    alive, finished = np.ones(E, bool), 0
    for t in range(H):
        out = env.step(torch.from_numpy(np.array(actions[:, k, t])).to(env.device), repeat=lc.REPEAT)
        torch.cuda.synchronize()
        reward = out["reward"].cpu().numpy().reshape(E, A)
        flags = sum(out[n].cpu().numpy().reshape(E, A).astype(np.uint8) << b for b, n in
                    enumerate(("done", "truncated", "wall_collision", "opponent_collision", "wrong_way"))).astype(np.uint8)
        assert np.array_equal(_bits(reward[alive]), _bits(got["reward"][alive, k, t])), t
        assert np.array_equal(flags[alive], got["flags"][alive, k, t]), t
        fin = (flags & DONE).any(axis=1)
        assert (got["length"][alive & fin, k] == t + 1).all(), t
        finished += int((alive & fin).sum())
        alive &= ~fin
        later = (got["length"][:, k] <= t)
        assert (_bits(got["reward"][later, k, t]) == 0).all(), t                                   # +0.0f
        assert np.array_equal(got["flags"][later, k, t], got["flags"][later, k, got["length"][later, k] - 1]), t
    assert (got["length"][alive, k] == H).all()
    assert finished == int((want["length"][:, k] < H).sum()) and finished >= 1
    env.close()


# ---- 4: purity
def test_a_look_ahead_leaves_no_trace():
    """Two identical envs - a track set on two tracks, two cars (slot B on n_step_progress), randomized vehicles, the episode
    log on, a policy loaded in deploy mode - of which one looks ahead: byte-equal afterwards and over 20 further steps."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    E, A, K, H = 24, 2, 5, 6

    def make():
        env = BatchedRaceEnv.with_track_set(["columbia", "austria"], E, A, order="sequential", seed=5, auto_reset=True,
                                            time_limit_steps=30, car_tasks=[None, "n_step_progress"], n_steps=10,
                                            vehicle_randomization=(WIDE_LO, WIDE_HI, 21))
        env.load_policy(POLICY)
        env.set_policy_sampling("deploy", seed=9)
        env.enable_episode_log(4096)
        env.reset(mode="random_ball", seed=13)
        for k in range(25):
            env.policy_act()
            env.step(None, repeat=lc.REPEAT)
        return env

    def state(env):
        snap = env.host_snapshot()
        snap.update(policy_state=env.policy_state.cpu().numpy(), vehicle_params=env.vehicle_params.cpu().numpy(),
                    track_id=env.track_id.cpu().numpy(), episode_counters=np.array(list(env.episode_counters.values())),
                    episode_rows=env.episode_rows.cpu().numpy())
        return snap

    def same(a, b, context):
        sa, sb = state(a), state(b)
        assert sa.keys() == sb.keys() and "action_in" in sa
        for k in sa:
            assert sa[k].tobytes() == sb[k].tobytes(), (context, k)

    looker, twin = make(), make()
    same(looker, twin, "before")
    actions = torch.from_numpy(lc.candidate_actions(4, E, K, H, A)).to(looker.device)
    out = looker.look_ahead(actions, repeat=lc.REPEAT, outputs=OUTPUTS)
    assert int((out["length"] < H).sum()) >= 1                        # (the time limit falls inside the horizon for most envs)
    same(looker, twin, "after the look-ahead")
    for k in range(20):
        for env in (looker, twin):
            env.policy_act()
            env.step(None, repeat=lc.REPEAT)
        if k % 5 == 0:
            looker.look_ahead(actions, repeat=lc.REPEAT, outputs=("return", "length"))
        same(looker, twin, f"step {k}")
    assert looker.episode_counters["written"] > 0
    looker.close(); twin.close()


# ---- 5: envs that are already finished
def test_finished_envs_are_frozen_from_the_first_step():
    import torch
    from helpers import make_oracle
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    E, K, H = 12, 2, 3
    ora = lc.no_scan(make_oracle(load_track(lc.TRACK), num_envs=E, cars_per_env=1, auto_reset=False))
    lc.settle_oracle(ora, 1, 6, steps=120)
    env = lc.settle_device(BatchedRaceEnv(lc.TRACK, E, 1, auto_reset=False), 6, steps=120)
    done0 = ora.done.astype(bool)
    assert done0.any() and not done0.all()
    assert np.array_equal(env.views["done"].cpu().numpy().reshape(E).astype(bool), done0)
    actions = lc.candidate_actions(5, E, K, H, 1)
    got = _look(env, actions)
    _assert_equal(got, look_ahead(ora, actions, lc.REPEAT), "finished envs")
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert (g["length"][done0] == 0).all() and (g["length"][~done0] > 0).all()
    assert (_bits(g["reward"][done0]) == 0).all() and (_bits(g["return"][done0]) == 0).all()
    assert (g["flags"][done0] == flags_of(ora)[done0][:, None, None, None]).all()
    # a tie: every candidate of a finished env returns +0.0, so the planner takes the lowest index, candidate 0
    from racing_dreamer_amd.planning import first_best, shooting_act
    seq = torch.from_numpy(actions).to(env.device)
    best = first_best(got["return"][:, :, 0])
    assert (best.cpu().numpy()[done0] == 0).all()
    shooting_act(env, candidates=seq, repeat=lc.REPEAT)
    assert torch.equal(env.views["action_in"].reshape(E, 2), seq[torch.arange(E, device=env.device), best, 0, 0])
    assert not np.array_equal(actions[done0][:, 0, 0], actions[done0][:, 1, 0])            # (the candidates' first actions differ)
    env.close()


# ---- 6: randomized vehicles
@pytest.mark.parametrize("mode", ["fixed", "random"])
def test_randomized_vehicles_equal_the_dr_restatement(mode):
    import torch
    from dr_oracle import VP_NOMINAL, make_dr_oracle
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    E, A, K, H = 9, 2, 3, 5
    env = BatchedRaceEnv(lc.TRACK, E, A, auto_reset=True)
    ora = lc.no_scan(make_dr_oracle(load_track(lc.TRACK), num_envs=E, cars_per_env=A, auto_reset=True))
    if mode == "fixed":
        rng = np.random.default_rng(2)
        lo, hi = np.asarray(WIDE_LO, np.float32), np.asarray(WIDE_HI, np.float32)
        vp = (lo + rng.uniform(0, 1, (E * A, 5)).astype(np.float32) * (hi - lo)).astype(np.float32)
        env.set_vehicle_params(torch.from_numpy(vp).to(env.device))
        ora.set_vehicle_params(vp)
    else:
        env.set_vehicle_randomization(WIDE_LO, WIDE_HI, seed=(9 << 32) | 21)
        ora.set_vehicle_randomization(WIDE_LO, WIDE_HI, seed=(9 << 32) | 21)
    lc.settle_device(env, 11)
    lc.settle_oracle(ora, A, 11)
    torch.cuda.synchronize()
    assert np.array_equal(env.vehicle_params.cpu().numpy(), ora.vp) and (ora.vp != VP_NOMINAL).any()
    actions = lc.candidate_actions(7, E, K, H, A)
    want = look_ahead(ora, actions, lc.REPEAT)
    _assert_equal(_look(env, actions), want, mode)
    assert np.array_equal(env.vehicle_params.cpu().numpy(), ora.vp)
    env.close()


# ---- 7: a track set
def test_a_track_set_uses_each_envs_current_track():
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.track_assets import load_track
    from track_set_oracle import make_track_set_oracle
    E, A, K, H = 10, 1, 3, 5
    tracks = [load_track(n) for n in ("columbia", "austria")]
    kw = dict(auto_reset=True, time_limit_steps=25)          # (one switch inside the settling run)
    env = BatchedRaceEnv.with_track_set(tracks, E, A, order="sequential", seed=3, **kw)
    ora = lc.no_scan(make_track_set_oracle(tracks, order="sequential", seed=3, num_envs=E, cars_per_env=A, **kw))
    lc.settle_device(env, 8)
    lc.settle_oracle(ora, A, 8)
    torch.cuda.synchronize()
    assert np.array_equal(env.track_id.cpu().numpy(), ora.track) and len(set(ora.track.tolist())) == 2
    assert (ora.track != np.repeat([0, 1], E // 2)).any()                 # (envs have switched: not the initial blocks)
    actions = lc.candidate_actions(9, E, K, H, A)
    _assert_equal(_look(env, actions), look_ahead(ora, actions, lc.REPEAT), "track set")
    assert np.array_equal(env.track_id.cpu().numpy(), ora.track)
    env.close()


# ---- 8: MixedTrackEnv
def test_mixed_track_env_equals_separate_envs():
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    names, counts, A, K, H = ["columbia", "austria"], [7, 5], 2, 3, 4
    E = sum(counts)
    mixed = MixedTrackEnv(names, counts, cars_per_env=A, auto_reset=True)
    parts, e0 = [], 0
    for n, c in zip(names, counts):
        parts.append(BatchedRaceEnv(n, c, A, auto_reset=True, first_env=e0))
        e0 += c
    mixed.reset(mode="random_ball", seed=4)
    for p in parts:
        p.reset(mode="random_ball", seed=4)
    for k in range(20):
        act = torch.from_numpy(lc.settle_actions(4, k, E * A)).to(mixed.device).reshape(E, A, 2)
        mixed.step(act, repeat=lc.REPEAT)
        e0 = 0
        for p, c in zip(parts, counts):
            p.step(act[e0:e0 + c], repeat=lc.REPEAT)
            e0 += c
    actions = torch.from_numpy(lc.candidate_actions(12, E, K, H, A)).to(mixed.device)
    got = mixed.look_ahead(actions, repeat=lc.REPEAT, outputs=OUTPUTS)
    e0 = 0
    for p, c in zip(parts, counts):
        want = p.look_ahead(actions[e0:e0 + c], repeat=lc.REPEAT, outputs=OUTPUTS)
        _assert_equal({k: v[e0:e0 + c] for k, v in got.items()}, {k: v.cpu().numpy() for k, v in want.items()}, p.track.name)
        e0 += c
        p.close()
    assert float(got["reward"].abs().sum()) > 0
    mixed.close()


# ---- 9: refusals
def test_error_codes_and_messages():
    import torch
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv(lc.TRACK, 4, 1)
    lib, K, H = env._lib, 2, 3
    actions = torch.zeros((4, K, H, 1, 2), device=env.device)
    ret = torch.zeros((4, K, 1), device=env.device)

    def call(**kw):
        a = L.RcLookAheadArgs(C.sizeof(L.RcLookAheadArgs), K, H, 1)
        a.actions, a.ret = actions.data_ptr(), ret.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.rc_look_ahead(env._h, C.byref(a))
        return rc, (lib.rc_last_error() or b"").decode()

    rc, msg = call()
    assert rc == RC_ERR_NEEDS_RESET and msg == "Must reset environment."
    with pytest.raises(L.RacecarHipError, match="Must reset environment"):
        env.look_ahead(actions)
    env.reset(mode="random", seed=1)
    assert call()[0] == 0
    for kw, text in ((dict(struct_size=8), "struct_size"), (dict(candidates=0), "candidates"), (dict(horizon=0), "horizon"),
                     (dict(horizon=L.LOOK_AHEAD_MAX_HORIZON + 1), "horizon"), (dict(repeat=0), "repeat"),
                     (dict(candidates=2 ** 30), "int32"), (dict(actions=None), "actions"), (dict(ret=None), "no output")):
        rc, msg = call(**kw)
        assert rc == RC_ERR_INVALID and text in msg, (kw, rc, msg)
    assert call(horizon=L.LOOK_AHEAD_MAX_HORIZON, actions=torch.zeros((4, K, 64, 1, 2), device=env.device).data_ptr())[0] == 0
    with pytest.raises(ValueError):
        env.look_ahead(actions, outputs=("speed",))
    with pytest.raises(ValueError):
        env.look_ahead(actions[:3])
    with pytest.raises(ValueError):
        env.look_ahead(actions, outputs=("return",), out={"return": torch.zeros((4, K), device=env.device)})
    env.set_profiling(True)
    before = set(env.kernel_times())
    env.look_ahead(actions, outputs=("return",))
    ms, n = env.look_ahead_time()
    assert n == 1 and ms > 0 and set(env.kernel_times()) == before                 # its own accumulator: the public keys stay
    env.close()


# ---- 10: the planner
def test_shooting_act_takes_the_argmax_candidates_first_action():
    import torch
    from racing_dreamer_amd.planning import first_best, shooting_act, shooting_candidates
    name = "a2"
    E, _K, _H, A = lc.CASES[name][:4]
    env = lc.device_env(name)
    held = env.views["action_in"].clone()
    cands = shooting_candidates(env, 16, 8, hold=4, seed=5)
    assert torch.equal(cands[:, 0], held.reshape(E, 1, A, 2).expand(E, 8, A, 2))
    want = cands.clone()
    want[:, :, :, 1:] = held.reshape(E, 1, 1, A, 2)[:, :, :, 1:]                                  # others="hold"
    ret = env.look_ahead(want, repeat=lc.REPEAT, outputs=("return",))["return"][:, :, 0]
    best = first_best(ret)
    assert int(best.max()) > 0                                           # (not every env keeps what it was doing)
    chosen = shooting_act(env, candidates=16, horizon=8, hold=4, seed=5, repeat=lc.REPEAT)
    assert chosen.data_ptr() == env.views["action_in"].data_ptr()
    assert torch.equal(chosen, want[torch.arange(E, device=env.device), best, 0])
    assert torch.equal(chosen[:, 1:], held[:, 1:])                       # the other slot stays on its action
    env.close()


def test_shooting_act_takes_the_candidate_that_survives():
    """Cars set square to the track on the starting grid, the wall 23 agent steps of full throttle ahead: every candidate but one
    drives into it inside the horizon, one stays where it is."""
    import torch
    from oracle import racecar_oracle as ro
    from helpers import make_oracle
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.planning import shooting_act
    from racing_dreamer_amd.track_assets import load_track
    E, K, H = 6, 5, 24
    t = load_track(lc.TRACK)
    ora = lc.no_scan(make_oracle(t, num_envs=E, cars_per_env=1, auto_reset=False))
    ora.reset(mode=ro.RESET_GRID, seed=2)
    pose = np.stack([ora.x, ora.y, ora.theta + np.float32(np.pi / 2)], 1).astype(np.float32)
    env = BatchedRaceEnv(t, E, 1, auto_reset=False)
    env.reset(mode="grid", seed=2)
    env.set_pose(pose.reshape(E, 1, 3))
    seq = torch.zeros((E, K, H, 1, 2), device=env.device)
    seq[..., 0] = 1.0                                                    # full throttle, straight on ...
    survivor = torch.tensor([3, 0, 4, 1, 2, 3], device=env.device)
    seq[torch.arange(E, device=env.device), survivor, :, 0, 0] = -1.0    # ... but one that stays where it is
    out = env.look_ahead(seq, repeat=lc.REPEAT, outputs=("flags", "length", "return"))
    last = out["flags"][:, :, -1, 0]
    hit = (last & WALL) != 0
    assert bool(hit.sum(dim=1).eq(K - 1).all()), hit.sum(dim=1).tolist()               # all but one end at the wall
    assert bool(out["length"].lt(H).sum(dim=1).eq(K - 1).all())
    assert bool((~hit).long().argmax(dim=1).eq(survivor).all())
    shooting_act(env, candidates=seq, repeat=lc.REPEAT)
    assert torch.equal(env.views["action_in"].reshape(E, 2), seq[torch.arange(E, device=env.device), survivor, 0, 0])
    env.close()


# ---- 11: the dream beside the simulator
def test_imagined_vs_simulated_equals_imagining_then_driving_a_twin():
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    from racing_dreamer_amd.world_model import imagined_vs_simulated
    E, A, H = 33, 1, 15

    def make():
        env = BatchedRaceEnv("austria", E, A, auto_reset=True, remap_actions=True, time_limit_steps=45)
        env.load_policy(POLICY)
        env.reset(mode="random", seed=1)
        for _ in range(36):
            env.policy_act()
            env.step(None, repeat=lc.REPEAT)
        env.policy_act()
        return env

    env, twin = make(), make()
    assert env.policy_has_reward_head
    pairs = imagined_vs_simulated(env, H, "mean", repeat=lc.REPEAT)
    dream = twin.policy_imagine(H, "mean")
    assert torch.equal(pairs["predicted"], dream["reward"]) and torch.equal(pairs["action"], dream["action"])
    assert pairs["simulated"].shape == (E * A, H) and pairs["alive"].shape == (E * A, H) and pairs["alive"].dtype == torch.bool
    alive = torch.ones(E * A, dtype=torch.bool, device=env.device)
    compared = 0
    for t in range(H):
        out = twin.step(dream["action"][:, t].reshape(E, A, 2), repeat=lc.REPEAT)
        was_alive = alive.clone()
        alive &= out["fresh"].reshape(E * A) == 0                        # (a reset: the env has left the imagined episode)
        assert torch.equal(pairs["alive"][:, t], alive), t
        real = out["reward"].reshape(E * A)
        assert torch.equal(real[was_alive].view(torch.int32), pairs["simulated"][was_alive, t].view(torch.int32)), t
        compared += int(was_alive.sum())
    assert compared > E * H // 2 and not bool(pairs["alive"][:, -1].all())       # (the time limit ends every episode inside the horizon)
    # pure: the env the pairs were taken from stands where its twin stood before it drove
    again = imagined_vs_simulated(env, H, "mean", repeat=lc.REPEAT)
    assert all(torch.equal(pairs[k], again[k]) for k in pairs)
    env.close(); twin.close()
