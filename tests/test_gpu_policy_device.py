"""rc_policy_act - the reference's trained Dreamer agent on the device - against its binary32 specification (tests/policy_spec.c):
bit for bit, one step and closed loop, every checkpoint, both action conventions, partial tiles, resets inside a run, slot masks,
mixed tracks, a track set under LiDAR noise; and the refusals."""
import glob
import os

import numpy as np
import pytest

from oracle import racecar_oracle as ro
from policy_spec import PolicySpec
from test_golden_policy import GOLDEN, c_env, drive, weights
from test_gpu_policy import DeviceEnv

pytestmark = pytest.mark.gpu
CHECKPOINTS = sorted(os.path.basename(p)[len("dreamer_policy_"):-4] for p in glob.glob(os.path.join(GOLDEN, "dreamer_policy_*.npz")))


def _recorded_inputs(n, seed):
    """(scan, state, fresh) as a run produces them: scans of cars on austria (C oracle, random starts, a few steps of the
    spec's own driving), the state the spec carries by then, and every fifth car marked fresh."""
    m = 16
    env, pol = c_env("austria", m), PolicySpec(weights("austria"))
    out = env.reset(mode=ro.RESET_RANDOM, seed=seed)
    st = np.zeros((m, 232), np.float32)
    scans, states = [], []
    for k in range(-(-n // m) + 2):
        scan = np.asarray(out["lidar"]).reshape(m, 1080)
        if k >= 2:
            scans.append(scan.copy())
            states.append(st.copy())
        a, st = pol.act_packed(scan, st)
        out = env.step(a, repeat=4)
    scan, state = np.concatenate(scans)[:n], np.concatenate(states)[:n]
    fresh = (np.arange(n) % 5 == 3).astype(np.uint8)
    return scan, state, fresh


def _device_step(env, scan, state, fresh, slots=None):
    import torch
    n = len(scan)
    env.views["lidar"].view(n, 1080).copy_(torch.from_numpy(scan))
    env.views["fresh"].view(n).copy_(torch.from_numpy(fresh))
    env.policy_state.copy_(torch.from_numpy(state))
    env.policy_act(slots)
    torch.cuda.synchronize()
    return env.views["action_in"].view(n, 2).cpu().numpy(), env.policy_state.cpu().numpy()


@pytest.mark.parametrize("remap", [True, False])
@pytest.mark.parametrize("name", CHECKPOINTS)
def test_one_step_is_the_spec_bit_for_bit(name, remap):
    """Recorded (scan, state, fresh) written into the device views, one policy_act: action_in and policy_state equal PolicySpec
    in every row, for 1, 33 and 4 097 cars (sizes that leave a partial tile of 32), both action conventions."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    assert len(CHECKPOINTS) == 4
    spec_pol = PolicySpec(weights(name))
    for n in (1, 33, 4097):
        scan, state, fresh = _recorded_inputs(min(n, 97), seed=3)
        reps = -(-n // len(scan))
        scan, state, fresh = (np.concatenate([x] * reps)[:n] for x in (scan, state, fresh))
        state = state * (1.0 + 0.001 * (np.arange(n) // 97))[:, None].astype(np.float32)      # (the repeats are not copies)
        env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=remap)
        env.reset(mode="random", seed=1)
        env.load_policy(weights(name))
        guard = torch.full((n, 2), 7.0, device=env.device)
        env.views["action_in"].view(n, 2).copy_(guard)
        got_a, got_s = _device_step(env, scan, state, fresh)
        want_raw, want_s = spec_pol.act_packed(scan, state, fresh)
        want_a = want_raw if remap else spec_pol.postprocess(want_raw)
        assert got_s.tobytes() == want_s.tobytes(), (name, n, float(np.abs(got_s - want_s).max()))
        assert got_a.tobytes() == want_a.tobytes(), (name, n, float(np.abs(got_a - want_a).max()))
        assert np.abs(want_raw).max() <= 1.0 and np.abs(want_raw).max() > 0.01
        env.close()


def test_closed_loop_is_the_spec_on_the_c_oracle_step_for_step():
    """The loop of test_gpu_policy's first test with the device agent on the HIP env and PolicySpec on the C oracle: scans,
    actions and poses identical for 300 agent steps at repeat 4, auto_reset, 16 cars; no wall contact, mean speed > 3."""
    import torch
    n = 16
    dev, ora = DeviceEnv("austria", n), c_env("austria", n)
    dev.env.load_policy(weights("austria"))
    po = PolicySpec(weights("austria"))
    od, oo = dev.reset(ro.RESET_GRID, 1), ora.reset(mode=ro.RESET_GRID, seed=1)
    so = po.initial(n)
    crashes = 0
    for k in range(300):
        assert np.array_equal(od["lidar"].reshape(n, -1), np.asarray(oo["lidar"]).reshape(n, -1)), f"scan differs at agent step {k}"
        ad = dev.env.policy_act().view(n, 2).cpu().numpy()
        ao, so = po.act(np.asarray(oo["lidar"]).reshape(n, -1), so, reset=np.asarray(oo["fresh"]).reshape(n) != 0)
        assert ad.tobytes() == ao.tobytes(), f"action differs at agent step {k}"
        od = dev._out(dev.env.step(None, repeat=4))
        oo = ora.step(ao, repeat=4)
        assert np.array_equal(od["pose"].reshape(n, 6), np.asarray(oo["pose"]).reshape(n, 6))
        crashes += int(np.count_nonzero(od["wall_collision"]))
    assert crashes == 0 and float(od["speed"].mean()) > 3.0
    dev.env.close()


def _follow(env, spec_pol, steps, slots=None, check_rows=None):
    """Drive `env` with the device agent; at every step feed the spec the device's own scan and fresh flags and compare the
    rows in `check_rows` (all by default) of action_in and of the state.  Returns the number of fresh rows seen after step 0."""
    import torch
    n = env.n_cars
    rows = np.arange(n) if check_rows is None else check_rows
    st = np.zeros((n, 232), np.float32)
    n_fresh = 0
    for k in range(steps):
        torch.cuda.synchronize()
        scan = env.views["lidar"].view(n, 1080).cpu().numpy()
        fresh = env.views["fresh"].view(n).cpu().numpy()
        n_fresh += int(fresh[rows].sum()) if k else 0
        got_a = env.policy_act(slots).view(n, 2).cpu().numpy()
        want_a, st_new = spec_pol.act_packed(scan, st, fresh)
        st[rows] = st_new[rows]
        got_s = env.policy_state.cpu().numpy()
        assert got_a[rows].tobytes() == want_a[rows].tobytes(), f"action differs at agent step {k}"
        assert got_s[rows].tobytes() == st[rows].tobytes(), f"state differs at agent step {k}"
        env.step(None, repeat=4)
    return n_fresh


def test_episodes_restart_the_latent_as_the_spec_does():
    """Random starts, terminate_on_collision and a time limit of 7 agent steps: every car is reset five times inside 40 agent
    steps, and the state of a fresh car restarts from zero exactly as PolicySpec.act(reset=fresh) does."""
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 48, 1, auto_reset=True, remap_actions=True, terminate_on_collision=True, time_limit_steps=7)
    env.reset(mode="random", seed=5)
    env.load_policy(weights("austria"))
    assert _follow(env, PolicySpec(weights("austria")), 40) >= 4 * 48
    env.close()


@pytest.mark.parametrize("cars", [2, 4])
def test_slot_mask_leaves_the_other_cars_alone(cars):
    """Trained opponents: slot_mask = cars B.. only.  Slot A's action_in and state rows keep the caller's values, the others
    equal the spec."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n_envs = 19
    env = BatchedRaceEnv("austria", n_envs, cars, auto_reset=True, remap_actions=True)
    env.reset(mode="grid", seed=2)
    env.load_policy(weights("austria"))
    n = env.n_cars
    slot = np.arange(n) % cars
    mine = np.float32([0.25, -0.125])
    for k in range(12):
        env.views["action_in"].view(n, 2)[::cars] = torch.from_numpy(mine).to(env.device)
        env.policy_state[::cars] = 0.5
        torch.cuda.synchronize()
        if k == 0:
            st = np.zeros((n, 232), np.float32)
            spec_pol = PolicySpec(weights("austria"))
        scan = env.views["lidar"].view(n, 1080).cpu().numpy()
        fresh = env.views["fresh"].view(n).cpu().numpy()
        got_a = env.policy_act(slots=range(1, cars)).view(n, 2).cpu().numpy()
        got_s = env.policy_state.cpu().numpy()
        want_a, st_new = spec_pol.act_packed(scan, st, fresh)
        st[slot != 0] = st_new[slot != 0]
        assert np.array_equal(got_a[slot == 0], np.tile(mine, (n_envs, 1))) and np.all(got_s[slot == 0] == 0.5)
        assert got_a[slot != 0].tobytes() == want_a[slot != 0].tobytes() and got_s[slot != 0].tobytes() == st[slot != 0].tobytes()
        env.step(None, repeat=4)
    env.close()


def test_mixed_tracks_and_a_noisy_track_set():
    """A MixedTrackEnv of three tracks, and a with_track_set env with LiDAR noise on: 50 agent steps each, equal to the spec fed
    the same device scans (the agent reads only the scan and `fresh`: no special case)."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv, MixedTrackEnv
    spec_pol = PolicySpec(weights("austria"))
    env = MixedTrackEnv(["columbia", "austria", "barcelona"], [13, 20, 7], auto_reset=True, remap_actions=True)
    env.reset(mode="random", seed=4)
    env.load_policy(weights("austria"))
    _follow(env, spec_pol, 50)
    env.close()
    env = BatchedRaceEnv.with_track_set(["austria", "columbia"], 40, order="random", seed=9, auto_reset=True, remap_actions=True,
                                        terminate_on_collision=True, time_limit_steps=60)
    env.set_lidar_noise(0.02, 0.01, seed=11)
    env.reset(mode="random", seed=6)
    env.load_policy(weights("austria"))
    _follow(env, spec_pol, 50)
    env.close()


def test_refusals():
    from racing_dreamer_amd import _lib as L
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    env = BatchedRaceEnv("austria", 4, 2, auto_reset=True)
    env.reset(mode="grid", seed=1)
    lib = env._lib
    assert lib.rc_policy_act(env._h, 1) == -1 and b"no policy loaded" in lib.rc_last_error()
    env.load_policy(weights("austria"))
    assert lib.rc_policy_act(env._h, 0) == -1 and b"empty" in lib.rc_last_error()
    assert lib.rc_policy_act(env._h, 0b101) == -1 and b"beyond cars_per_env" in lib.rc_last_error()
    assert lib.rc_policy_act(env._h, 0b11) == 0
    env.unload_policy()
    assert lib.rc_policy_act(env._h, 1) == -1 and b"no policy loaded" in lib.rc_last_error()
    env.close()
    env = BatchedRaceEnv("austria", 4, 1, auto_reset=True, lidar_transform="dreamer")
    env.reset(mode="grid", seed=1)
    env.load_policy(weights("austria"))
    assert lib.rc_policy_act(env._h, 1) == -1 and b"metres" in lib.rc_last_error()
    env.close()


@pytest.mark.gpu_slow
def test_the_agent_drives_65536_cars():
    """65 536 cars on austria from random poses, 100 agent steps: fewer than one wall contact per 5 000 agent steps and mean speed
    > 3.0 (the bounds of test_reference_agent_drives_a_thousand_cars_on_the_device), and the final state of 4 096 of the cars
    equal to the spec run on their recorded scans for the last step."""
    import torch
    from racing_dreamer_amd.batched_env import BatchedRaceEnv
    n, steps, m = 65536, 100, 4096
    env = BatchedRaceEnv("austria", n, 1, auto_reset=True, remap_actions=True)
    out = env.reset(mode="random", seed=1)
    env.load_policy(weights("austria"))
    crashes, speeds = 0, []
    pick = torch.arange(0, n, n // m, device=env.device)
    for k in range(steps):
        if k == steps - 1:
            before = env.policy_state[pick].cpu().numpy()
            scan = out["lidar"].view(n, 1080)[pick].cpu().numpy()
            fresh = out["fresh"].view(n)[pick].cpu().numpy()
        env.policy_act()
        out = env.step(None, repeat=4)
        crashes += int(out["wall_collision"].sum().item())
        speeds.append(float(out["speed"].mean().item()))
    speed = float(np.mean(speeds[50:]))
    print(f"65536 cars: {crashes} wall contacts in {n * steps} agent steps, mean speed {speed:.3f} m/s")
    assert crashes * 5000 <= n * steps and speed > 3.0, (crashes, speed)
    _, want = PolicySpec(weights("austria")).act_packed(scan, before, fresh)
    assert env.policy_state[pick].cpu().numpy().tobytes() == want.tobytes()
    env.close()
