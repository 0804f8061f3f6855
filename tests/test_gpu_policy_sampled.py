"""rc_policy_act in the sampled modes (rc_policy_set_sampling: `deploy`, `explore`) against their binary32 specification
(tests/policy_sample_spec.c): bit for bit, one step and closed loop, every checkpoint, both action conventions, partial tiles,
resets inside a run, slot masks, mixed tracks, a noisy track set under domain randomization; shards, mode switches, determinism,
the noise amount and the refusals."""
import ctypes as C

import numpy as np
import pytest

from oracle import racecar_oracle as ro
from racing_dreamer_amd import spec
from policy_sample_spec import EpisodeClock, PolicySampleSpec
from policy_spec import PolicySpec
from test_golden_policy import c_env, weights
from test_gpu_policy import DeviceEnv
from test_gpu_policy_device import CHECKPOINTS, _device_step, _recorded_inputs

pytestmark = pytest.mark.gpu
MODES = [("deploy", None), ("explore", None)]


@pytest.mark.parametrize("remap", [True, False])
@pytest.mark.parametrize("name", CHECKPOINTS)
def test_one_step_is_the_spec_bit_for_bit(name, remap):
    """test_gpu_policy_device's one-step test in both sampled modes: recorded (scan, state, fresh) in the device views, one
    policy_act after the reset (episode 1, agent step 0, global env = row), 1, 33 and 4 097 cars."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    assert len(CHECKPOINTS) == 4
    for n in (1, 33, 4097):
        scan, state, fresh = _recorded_inputs(min(n, 97), seed=3)
        reps = -(-n // len(scan))
        scan, state, fresh = (np.concatenate([x] * reps)[:n] for x in (scan, state, fresh))
        state = state * (1.0 + 0.001 * (np.arange(n) // 97))[:, None].astype(np.float32)
        env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=remap)
        env.reset(mode="random", seed=1)
        env.load_policy(weights(name))
        clock = EpisodeClock(n)
        clock.reset()
        for mode, amount in MODES:
            env.set_policy_sampling(mode, seed=77, expl_amount=amount)
            spec_pol = PolicySampleSpec(weights(name), mode, seed=77, expl_amount=amount)
            env.views["action_in"].view(n, 2).copy_(torch.full((n, 2), 7.0, device=env.device))
            got_a, got_s = _device_step(env, scan, state, fresh)
            want_raw, want_s = spec_pol.act_packed(scan, state, fresh, clock.keys())
            want_a = want_raw if remap else spec_pol.postprocess(want_raw)
            assert got_s.tobytes() == want_s.tobytes(), (name, n, mode, float(np.abs(got_s - want_s).max()))
            assert got_a.tobytes() == want_a.tobytes(), (name, n, mode, float(np.abs(got_a - want_a).max()))
            assert np.abs(want_raw).max() <= 1.0 and np.abs(want_raw).max() > 0.01
        env.close()


@pytest.mark.parametrize("mode,amount,start", [("deploy", None, ro.RESET_GRID), ("explore", 1.0, ro.RESET_RANDOM)])
def test_closed_loop_is_the_spec_on_the_c_oracle_step_for_step(mode, amount, start):
    """The device agent on the HIP env and the spec on the C oracle, the spec keyed by the ORACLE's own episode and agent-step
    counters: scans, actions and poses identical for 200 agent steps at repeat 4 with auto-reset (explore at 1.0 from random starts
    drives cars into the wall: 13 resets inside the run on the oracle); deploy from the grid drives without a wall contact at a mean
    speed above 3 m/s over agent steps 50 .. 200 - the measure of test_golden_policy.drive, not the speed at the last step: the 16
    cars leave the grid together and at step 200 stand in the same slow corner, where the port's own sample=True agent does
    2.45 .. 2.75 m/s (four seeds, its mean over steps 50 .. 200: 3.75 .. 3.84) and this mode 2.70 (mean 3.74)."""
    n = 16
    dev, ora = DeviceEnv("austria", n), c_env("austria", n)
    dev.env.load_policy(weights("austria"))
    dev.env.set_policy_sampling(mode, seed=9, expl_amount=amount)
    po = PolicySampleSpec(weights("austria"), mode, seed=9, expl_amount=amount)
    od, oo = dev.reset(start, 1), ora.reset(mode=start, seed=1)
    so = po.initial(n)
    crashes = resets = 0
    speeds = []
    for k in range(200):
        assert np.array_equal(od["lidar"].reshape(n, -1), np.asarray(oo["lidar"]).reshape(n, -1)), f"scan differs at agent step {k}"
        ad = dev.env.policy_act().view(n, 2).cpu().numpy()
        keys = np.stack([np.arange(n), ora.arr["episode"], ora.arr["agent_steps"], np.zeros(n)], 1).astype(np.uint32)
        fresh = np.asarray(oo["fresh"]).reshape(n) != 0
        resets += int(fresh.sum()) if k else 0
        ao, so = po.act(np.asarray(oo["lidar"]).reshape(n, -1), so, reset=fresh, keys=keys)
        assert ad.tobytes() == ao.tobytes(), f"action differs at agent step {k}"
        od = dev._out(dev.env.step(None, repeat=4))
        oo = ora.step(ao, repeat=4)
        assert np.array_equal(od["pose"].reshape(n, 6), np.asarray(oo["pose"]).reshape(n, 6))
        crashes += int(np.count_nonzero(od["wall_collision"]))
        speeds.append(float(od["speed"].mean()))
    speed = float(np.mean(speeds[50:]))
    print(f"{mode}: {crashes} wall contacts, {resets} resets, mean speed {speed:.3f}")
    if mode == "deploy":
        assert crashes == 0 and speed > 3.0
    else:
        assert resets > 0
    dev.env.close()


def _follow(env, spec_pol, steps, clock, slots=None, check_rows=None):
    """test_gpu_policy_device._follow with the draw's keys from `clock` (reset by the caller with the env)."""
    import torch
    n = env.n_cars
    rows = np.arange(n) if check_rows is None else check_rows
    st = np.zeros((n, 232), np.float32)
    n_fresh = 0
    for k in range(steps):
        torch.cuda.synchronize()
        scan = env.views["lidar"].view(n, 1080).cpu().numpy()
        fresh = env.views["fresh"].view(n).cpu().numpy()
        if k:
            clock.step(fresh)
            n_fresh += int(fresh[rows].sum())
        got_a = env.policy_act(slots).view(n, 2).cpu().numpy()
        want_a, st_new = spec_pol.act_packed(scan, st, fresh, clock.keys())
        st[rows] = st_new[rows]
        got_s = env.policy_state.cpu().numpy()
        assert got_a[rows].tobytes() == want_a[rows].tobytes(), f"action differs at agent step {k}"
        assert got_s[rows].tobytes() == st[rows].tobytes(), f"state differs at agent step {k}"
        env.step(None, repeat=4)
    return n_fresh


@pytest.mark.parametrize("mode", ["deploy", "explore"])
def test_episodes_restart_the_latent_and_the_stream(mode):
    """Random starts, terminate_on_collision and a time limit of 7 agent steps: every car is reset five times inside 40 agent
    steps; the latent restarts from zero and the draws go on under the next episode counter at agent step 0."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 48, 1, auto_reset=True, remap_actions=True, terminate_on_collision=True, time_limit_steps=7)
    env.reset(mode="random", seed=5)
    env.load_policy(weights("austria"))
    env.set_policy_sampling(mode, seed=3)
    clock = EpisodeClock(48)
    clock.reset()
    assert _follow(env, PolicySampleSpec(weights("austria"), mode, seed=3), 40, clock) >= 4 * 48
    env.close()


@pytest.mark.parametrize("mode", ["deploy", "explore"])
def test_slot_mask_leaves_the_other_cars_alone(mode):
    """slots=(1, 2, 3) of four cars per env: slot A keeps the caller's action and state rows, the others equal the spec - whose
    draws carry the slot in their counter, so they are what a call over all four slots gives those cars."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n_envs, cars = 19, 4
    env = BatchedRaceEnv("austria", n_envs, cars, auto_reset=True, remap_actions=True)
    env.reset(mode="grid", seed=2)
    env.load_policy(weights("austria"))
    env.set_policy_sampling(mode, seed=14)
    n = env.n_cars
    slot = np.arange(n) % cars
    env.views["action_in"].view(n, 2)[::cars] = torch.tensor([0.25, -0.125], device=env.device)
    clock = EpisodeClock(n_envs, cars)
    clock.reset()
    _follow(env, PolicySampleSpec(weights("austria"), mode, seed=14), 12, clock, slots=(1, 2, 3), check_rows=np.flatnonzero(slot != 0))
    assert np.all(env.policy_state[::cars].cpu().numpy() == 0.0)
    env.close()


def test_mixed_tracks_and_a_noisy_randomized_track_set():
    """A MixedTrackEnv of three tracks (its blocks' handles key the draws by their global env ids), and a with_track_set env with
    LiDAR noise and vehicle randomization on: 40 agent steps each in deploy mode, equal to the spec fed the same device scans."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    spec_pol = PolicySampleSpec(weights("austria"), "deploy", seed=21)
    env = MixedTrackEnv(["columbia", "austria", "barcelona"], [13, 20, 7], auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=4)
    env.load_policy(weights("austria"))
    env.set_policy_sampling("deploy", seed=21)
    assert env.policy_sampling == dict(mode="deploy", seed=21, expl_amount=0.0)
    clock = EpisodeClock(40)
    clock.reset()
    _follow(env, spec_pol, 40, clock)
    env.close()
    env = BatchedRaceEnv.with_track_set(["austria", "columbia"], 40, order="random", seed=9, auto_reset=True, remap_actions=True,
                                        terminate_on_collision=True, time_limit_steps=15)
    env.set_lidar_noise(0.02, 0.01, seed=11)
    env.set_vehicle_randomization(**spec.DR_DEPLOYMENT_LOCK, seed=12)
    env.reset(mode="random", seed=6)
    env.load_policy(weights("austria"))
    env.set_policy_sampling("deploy", seed=21)
    clock = EpisodeClock(40)
    clock.reset()
    assert _follow(env, spec_pol, 40, clock) >= 40
    env.close()


@pytest.mark.parametrize("mode", ["deploy", "explore"])
def test_two_shards_are_the_full_batch(mode):
    """Envs [0, 40) on one handle, and [0, 17) and [17, 40) on two handles with first_env offsets: 20 closed-loop agent steps from
    random starts give the same action and state rows."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    def run(n, first):
        env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True, terminate_on_collision=True, time_limit_steps=8, first_env=first)
        env.reset(mode="random", seed=5)
        env.load_policy(weights("austria"))
        env.set_policy_sampling(mode, seed=31)
        acts = []
        for _ in range(20):
            acts.append(env.policy_act().view(n, 2).cpu().numpy().copy())
            env.step(None, repeat=4)
        state = env.policy_state.cpu().numpy()
        env.close()
        return np.stack(acts, 1), state
    full_a, full_s = run(40, 0)
    for lo, hi in ((0, 17), (17, 40)):
        a, s = run(hi - lo, lo)
        assert np.array_equal(a, full_a[lo:hi]) and np.array_equal(s, full_s[lo:hi])


def _run(env, steps):
    n = env.n_cars
    acts = []
    for _ in range(steps):
        acts.append(env.policy_act().view(n, 2).cpu().numpy().copy())
        env.step(None, repeat=4)
    return np.stack(acts), env.policy_state.cpu().numpy()


def test_mode_switches_determinism_and_the_noise_amount():
    """`mean` after `deploy` is a run that never left `mean` (given the same state and scans); a second load_policy resets the
    mode; two runs with one seed are identical, another seed changes the actions; two calls without a step draw the same
    numbers; explore with expl_amount 0 is the unperturbed clipped sample (the spec's, bit for bit), 0.3 differs from it."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n = 33
    def fresh_env():
        env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True)
        env.reset(mode="random", seed=8)
        env.load_policy(weights("austria"))
        return env
    env = fresh_env()
    assert env.policy_sampling["mode"] == "mean"
    want_a, want_s = _run(env, 6)
    env.close()
    env = fresh_env()
    env.set_policy_sampling("deploy", seed=1)
    env.policy_act()
    first = env.views["action_in"].view(n, 2).cpu().numpy().copy()
    env.policy_act()                                                  # no step in between: the same draws ...
    state_twice = env.policy_state.cpu().numpy()
    env.policy_state.zero_()
    env.policy_act()                                                  # ... and from the same (zero) state the same action
    assert np.array_equal(env.views["action_in"].view(n, 2).cpu().numpy(), first) and np.abs(state_twice).max() > 0
    env.set_policy_sampling("mean")
    env.policy_state.zero_()
    got_a, got_s = _run(env, 6)
    assert got_a.tobytes() == want_a.tobytes() and got_s.tobytes() == want_s.tobytes()
    env.set_policy_sampling("explore", seed=2)
    assert env.policy_sampling == dict(mode="explore", seed=2, expl_amount=pytest.approx(0.3))
    env.load_policy(weights("austria"))
    assert env.policy_sampling == dict(mode="mean", seed=0, expl_amount=0.0)
    env.close()
    runs = {}
    for tag, mode, seed, amount in (("a", "deploy", 5, None), ("b", "deploy", 5, None), ("c", "deploy", 6, None),
                                    ("e0", "explore", 5, 0.0), ("e3", "explore", 5, 0.3)):
        env = fresh_env()
        env.set_policy_sampling(mode, seed=seed, expl_amount=amount)
        runs[tag] = _run(env, 6)
        env.close()
    assert runs["a"][0].tobytes() == runs["b"][0].tobytes() and runs["a"][1].tobytes() == runs["b"][1].tobytes()
    assert not np.array_equal(runs["a"][0], runs["c"][0])
    assert not np.array_equal(runs["e0"][0][0], runs["e3"][0][0]) and np.abs(runs["e3"][0]).max() <= 1.0
    # expl_amount 0: the spec's explore step with no noise, i.e. clip(tanh(mu + sd n)) of the one draw
    env = fresh_env()
    env.set_policy_sampling("explore", seed=5, expl_amount=0.0)
    torch.cuda.synchronize()
    scan, fresh = env.views["lidar"].view(n, 1080).cpu().numpy(), env.views["fresh"].view(n).cpu().numpy()
    clock = EpisodeClock(n)
    clock.reset()
    spec_pol = PolicySampleSpec(weights("austria"), "explore", seed=5, expl_amount=0.0)
    want, _, d = spec_pol.act_packed(scan, np.zeros((n, 232), np.float32), fresh, clock.keys(), detail=True)
    mu, sd = d["dist"][:, :2].astype(np.float64), d["dist"][:, 2:].astype(np.float64)
    assert np.allclose(want, np.tanh(mu + sd * d["normals"][:, 32:34]), atol=1e-5)
    assert env.policy_act().view(n, 2).cpu().numpy().tobytes() == want.tobytes()
    env.close()


def test_refusals():
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 4, 1, auto_reset=True)
    env.reset(mode="grid", seed=1)
    lib = env._lib
    s = L.RcPolicySampling(C.sizeof(L.RcPolicySampling), 1, 0, 0.0)
    assert lib.rc_policy_set_sampling(env._h, C.byref(s)) == -1 and b"no policy loaded" in lib.rc_last_error()
    assert lib.rc_policy_get_sampling(env._h, C.byref(s)) == -1 and b"no policy loaded" in lib.rc_last_error()
    env.load_policy(weights("austria"))
    assert lib.rc_policy_set_sampling(env._h, C.byref(s)) == 0 and env.policy_sampling["mode"] == "deploy"
    for field, value, text in (("struct_size", 8, b"struct_size"), ("mode", 3, b"unknown mode"), ("mode", -1, b"unknown mode"),
                               ("expl_amount", -0.1, b"expl_amount"), ("expl_amount", float("nan"), b"expl_amount"),
                               ("expl_amount", float("inf"), b"expl_amount")):
        bad = L.RcPolicySampling(C.sizeof(L.RcPolicySampling), 2, 0, 0.3)
        setattr(bad, field, value)
        assert lib.rc_policy_set_sampling(env._h, C.byref(bad)) == -1 and text in lib.rc_last_error(), field
        assert env.policy_sampling["mode"] == "deploy"                   # (a refused call changes nothing)
    assert lib.rc_policy_set_sampling(env._h, None) == 0 and env.policy_sampling["mode"] == "mean"
    with pytest.raises(ValueError):
        env.set_policy_sampling("greedy")
    env.unload_policy()
    assert lib.rc_policy_set_sampling(env._h, C.byref(s)) == -1 and b"no policy loaded" in lib.rc_last_error()
    env.close()
