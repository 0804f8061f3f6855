"""bench.py contract on a real GPU: one JSON line with the required keys; the N > 1 path end to end with two
ranks sharing the one GPU of the test box (gloo backend - RCCL itself needs one GPU per rank)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline"}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _errtext(stderr):
    """The ranks' own tracebacks come first, the launcher's summary last: show both ends."""
    lines = [l for l in stderr.splitlines() if "Traceback" in l or "Error" in l or "error" in l]
    return "\n".join(lines[:30]) + "\n...\n" + stderr[-1500:]


def _json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_bench_single_gpu_contract():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "8", "--warmup", "2", "--envs", "4096", "--track",
                        "columbia", "--cpu-envs", "4096", "--numpy-envs", "256", "--observable-seconds", "2", "--full"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, _errtext(r.stderr)
    d = _json_line(r.stdout)
    assert REQUIRED <= set(d) and d["n_gpus"] == 1 and d["steps"] == 8 and d["warmup"] == 2
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["value"] > 1e6 and d["config"]["workload"].startswith("4096 envs")
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and rf["launches"] == 8
    # the symbol rocprofv3 lists for the scan this run launched (4 096 cars: several waves per car, the overlapped build),
    # and PMC figures only for the workload they were profiled on - this is not it
    assert rf["kernel"] == "rc_raycast_car_kernel<1, true, false>" and rf["traffic"] is None and rf["traffic_source"] is None
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    # the threads the baseline ran on are the cores the process really has (cgroup quota / measured share), and the
    # all-thread rate is a real multiple of the one-thread rate measured in the same leg
    assert cb["cores"] == cb["cores_effective"] <= cb["cpu_share"]["sched_getaffinity"]
    assert cb["speedup_all_over_one_thread"] >= 0.5 * cb["cores_effective"] or cb["cores_effective"] == 1
    assert cb["numpy_batch"]["value"] > 0 and "256 envs" in cb["numpy_batch"]["sample"]
    # the other single-GPU configurations of BASELINE.json ride in the same line
    cfgs = d["configs"]
    assert [c["envs"] * c["cars_per_env"] for c in cfgs] == [4096, 65536, 65536, 65536]
    assert cfgs[3]["track"] == "mixed: columbia / austria / barcelona" and cfgs[3]["kernels_ms"]["rc_raycast_kernel"] > 0 and "rc_step_group" in cfgs[3]["workload"]
    cfgs = cfgs[:3]
    assert cfgs[1]["obs_type"] == "lidar_occupancy" and "rc_patch_kernel" in cfgs[1]["kernels_ms"]
    assert cfgs[2]["cars_per_env"] == 2 and cfgs[2]["track"] == "treitlstrasse_v2"
    for c in cfgs:
        r = c["roofline"]
        assert c["ms_per_step"] > 0 and 0 < r["step_frac"] < 1 and 0 < r["raycast_frac"] < 1
        assert r["step_bytes"] == c["envs"] * c["cars_per_env"] * (4479 + (4096 if c["obs_type"] == "lidar_occupancy" else 0))
    # the scan across tracks at the headline's batch size, and the first steps after a reset
    assert [t["track"] for t in d["tracks"]] == ["columbia", "barcelona", "gbr"] and d["tracks"][0]["headline"] is True
    assert all(t["raycast_ms"] > 0 and 0 < t["raycast_frac"] < 1 for t in d["tracks"])
    lo, hi = rf["raycast_ms_range_over_tracks"]
    assert lo <= rf["avg_launch_ms"] * 1.01 and hi >= lo and len(rf["frac_range_over_tracks"]) == 2
    assert d["fresh_reset"]["steps"] == 20 and d["fresh_reset"]["raycast_ms"] > 0
    assert "issue_frac" in rf and rf["issue_frac"] is None          # (PMC figures only for the profiled workload)
    assert "leg_errors" not in d and "aborted" not in d and "legs_skipped" not in d and "headline_pending" not in d
    # the window an outside observer can see: the headline's loop for --observable-seconds without a pause
    sl = d["steady_long"]
    assert 1.5 < sl["seconds"] < 6.0 and sl["steps"] > d["steady"]["steps"] and sl["env_steps_per_s"] > 0.5 * d["steady"]["env_steps_per_s"]


def test_bench_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """Without --full the line carries the headline and nothing that takes runs of its own; --steps sets the timed steps (one
    scan launch each); --dump-outputs writes the last timed step's outputs, identical from run to run with the same arguments."""
    import numpy as np
    lines = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, "bench.py", "--steps", "7", "--warmup", "2", "--envs", "4096", "--track", "columbia",
                            "--dump-outputs", str(tmp_path / name)], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, _errtext(r.stderr)
        lines.append(_json_line(r.stdout))
    d = lines[0]
    assert REQUIRED <= set(d) and d["steps"] == 7 and d["roofline"]["launches"] == 7 and d["value"] > 1e6
    assert d["ms_per_step"] == pytest.approx(4096 / d["value"] * 1e3, rel=1e-9) and d["config"]["full"] is False
    assert not {"cpu_baseline", "configs", "tracks", "fresh_reset", "steady", "steady_long", "action_repeat_4", "follow_the_gap",
                "exact_render", "leg_errors", "aborted"} & set(d)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and {"lidar.npy", "pose.npy", "reward.npy", "done.npy", "sampled_cars.npy"} <= set(files)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y, equal_nan=True), f
    assert np.load(tmp_path / "a" / "pose.npy").shape == (4096, 1, 6)
    lidar, rows = np.load(tmp_path / "a" / "lidar.npy"), np.load(tmp_path / "a" / "sampled_cars.npy")
    assert lidar.shape == (len(rows), 1080) and 0 < len(rows) <= 4096 and np.all(np.diff(rows) > 0) and lidar.max() > 0


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2 ...` with NO launcher around it (the way the driver starts the N = 1 line): the process
    starts its two ranks itself, rank 0's single JSON line comes through, and the communicator's own rank count is in it."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--backend", "gloo", "--steps", "6", "--warmup", "2",
                        "--envs", "2048", "--full"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, _errtext(r.stderr)
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["config"]["total_envs"] == 4096 and d["config"]["comm_ranks"] == 2
    assert d["config"]["comm_backend"] == "gloo" and d["config"]["rccl_ranks"] is None      # (RCCL needs a GPU per rank)
    assert set(d["gather_modes"]) == {"sharded", "full-u16", "full", "summary", "none", "batch"}
    # every payload's collective checked by the run itself: both ranks' shards of the gathered records against the senders' checksums
    gc = d["gather_check"]
    assert gc["ok"] is True and set(gc["payloads"]) == {"sharded", "batch", "full-u16", "full", "summary", "full-u16@repeat4", "full@repeat4"}
    assert all(c["ok"] is True and c["ranks"] == 2 and c["via"] == "torch" for c in gc["payloads"].values())
    assert gc["payloads"]["sharded"]["records_verified"] == 3 and gc["payloads"]["full"]["records_verified"] == 2
    assert "aborted" not in d and "leg_errors" not in d


def test_bench_sees_one_flipped_bit_in_a_gathered_record():
    """The self-check is live: one bit flipped in rank 1's record after its checksum was taken, before the collective -
    the line says so and the run fails (each rank exits 4; the launcher reports the failure)."""
    import os
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--backend", "gloo", "--steps", "4", "--warmup", "1",
                        "--envs", "1024", "--no-gather-modes", "--full"], cwd=ROOT, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, RC_BENCH_CORRUPT_GATHER="1"))
    assert r.returncode != 0, _errtext(r.stderr)
    d = _json_line(r.stdout)
    assert d["gather_check"]["ok"] is False and d["gather_check"]["payloads"]["sharded"]["ok"] is False
    assert "differs from what its sender sent" in r.stderr


def test_a_secondary_leg_that_raises_or_hangs_does_not_cost_the_headline():
    """VERDICT r3 #1a: the legs after the headline have never run across devices.  One of them raising on one rank (the others
    are then inside a collective it never joins), or hanging, ends the run with the ONE line: the headline, the legs
    measured before it, and `aborted` naming the leg - and exit code 5 (a leg was lost; VERDICT r5 #1b: not 0)."""
    import os
    base = [sys.executable, "bench.py", "--gpus", "2", "--backend", "gloo", "--steps", "4", "--warmup", "1", "--envs", "1024", "--full"]
    r = subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=900, env=dict(os.environ, RC_BENCH_FAIL_LEG="summary:1"))
    assert r.returncode == 5, _errtext(r.stderr)
    d = _json_line(r.stdout)
    assert d["value"] > 0 and d["config"]["gather"] == "sharded" and d["gather_check"]["payloads"]["sharded"]["ok"] is True
    assert d["aborted"]["leg"] == "summary" and "RC_BENCH_FAIL_LEG" in d["aborted"]["reason"]
    assert {"sharded", "none", "batch"} <= set(d["gather_modes"]) and "full" not in d["gather_modes"]
    r = subprocess.run(base + ["--leg-timeout", "10"], cwd=ROOT, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, RC_BENCH_HANG_LEG="batch:1"))
    assert r.returncode == 5, _errtext(r.stderr)
    d = _json_line(r.stdout)
    assert d["value"] > 0 and d["aborted"]["leg"] == "batch" and "deadline" in d["aborted"]["reason"] and d["aborted"]["exit_code"] == 5
    assert "none" in d["gather_modes"] and "summary" not in d["gather_modes"]
    assert "headline_pending" not in d and d["rank0_alone_before_the_rendezvous"]["env_steps_per_s_this_rank"] > 0


def test_a_headline_that_hangs_on_first_contact_prints_the_provisional_line():
    """VERDICT r5 #1b on the real env: rank 1 never enters the headline leg (the ring prefill and the timed window: the first
    collectives on the data path), rank 0 sits in a collective nobody joins.  The leg's deadline ends the run with the line
    rank 0 armed BEFORE the rendezvous - its own simulation-only window on the GPU, marked `headline_pending` - and exit code
    3: a code of its own, not a success and not the driver's time-out."""
    import os
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--backend", "gloo", "--steps", "4", "--warmup", "1", "--envs", "1024",
                        "--leg-timeout", "10"], cwd=ROOT, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, RC_BENCH_HANG_LEG="headline:1"))
    assert r.returncode == 3, _errtext(r.stderr)
    d = _json_line(r.stdout)
    assert REQUIRED - {"roofline"} <= set(d) and d["headline_pending"] is True and d["n_gpus"] == 2
    assert d["aborted"]["leg"] == "headline" and d["aborted"]["exit_code"] == 3 and "PROVISIONAL" in d["config"]["workload"]
    assert d["provisional"]["env_steps_per_s_this_rank"] > 1e5 and d["value"] == pytest.approx(2 * d["provisional"]["env_steps_per_s_this_rank"])
    assert "gather_modes" not in d and "roofline" not in d


def test_legs_are_budgeted_from_the_time_left():
    """VERDICT r5 #1c: with a time budget that has room for the headline and little else (a two-rank run of 1 024 envs takes
    about 5 s; 12 s of any budget are kept back for printing and leaving), the later legs are SKIPPED (listed
    in `legs_skipped`, every rank taking the same branch) instead of running into the launcher's time-out; that is not an
    error: exit 0, headline and self-check present."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--backend", "gloo", "--steps", "4", "--warmup", "1", "--envs", "1024",
                        "--time-budget", "30", "--full"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, _errtext(r.stderr)
    d = _json_line(r.stdout)
    assert d["value"] > 0 and d["gather_check"]["payloads"]["sharded"]["ok"] is True and "aborted" not in d
    assert d["legs_skipped"] and all("time budget" in why for why in d["legs_skipped"].values())
    assert "full" in d["legs_skipped"] or "full" in d["gather_modes"]


def test_bench_two_ranks_peer_copy_transport():
    """The same two ranks with the gather as direct peer copies (hipIpc works between processes on one device)."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--backend", "gloo", "--gather-via", "p2p", "--steps", "6",
                        "--warmup", "2", "--envs", "2048", "--full"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, _errtext(r.stderr)
    d = _json_line(r.stdout)
    # (the headline stays the sharded store over torch.distributed; the per-step record gathers go over the peer copies)
    assert d["config"]["gather"] == "sharded" and d["config"]["gather_via"] == "torch"
    gm = d["gather_modes"]
    assert all(gm[m]["ms_per_step"] > 0 for m in ("sharded", "full-u16", "full", "summary", "none", "batch"))
    gc = d["gather_check"]
    assert gc["ok"] is True and all(gc["payloads"][m]["ok"] is True and gc["payloads"][m]["via"] == "p2p" and
                                    gc["payloads"][m]["records_verified"] == 2 for m in ("full-u16", "full", "summary"))


def test_bench_two_ranks_functional():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2", "--steps", "6", "--warmup",
           "2", "--envs", "2048", "--backend", "gloo", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, _errtext(r.stderr)
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["config"]["total_envs"] == 4096 and d["scaling"] == "weak"
    # the headline of an N > 1 run is the sharded trajectory store (summary per step + a 50 x 50 batch every 10th step), and
    # says so; the per-step gathers of whole records are timed beside it; the CPU baseline is a pointer to the N = 1 line
    assert d["config"]["gather"] == "sharded"
    assert "sharded" in d["config"]["workload"] and "ShardedReplay" in d["config"]["gather_detail"]
    assert d["cpu_baseline"]["measured_in_this_run"] is False and "N = 1" in d["cpu_baseline"]["see"]
    gm = d["gather_modes"]
    assert set(gm) == {"sharded", "full-u16", "full", "summary", "none", "batch"} and gm["sharded"]["headline"] is True
    assert gm["sharded"]["batch_every"] == 10 and gm["sharded"]["batch_windows"] == 50 and gm["sharded"]["batch_length"] == 50
    # the pure-simulation leg really is that: nothing of the uint16 record is produced in it
    assert "simulation alone" in gm["none"]["includes"] and "in place" in gm["full"]["includes"]
    assert gm["batch"]["bytes_per_gpu_per_step"] == 25 * 50 * (1080 * 4 + 8 + 4 + 4) // 10       # one batch every 10th step
    assert gm["sharded"]["bytes_per_gpu_per_step"] == pytest.approx(2048 * 76 + gm["batch"]["bytes_per_gpu_per_step"], rel=0.05)
    assert gm["full-u16"]["bytes_per_gpu_per_step"] == pytest.approx(2048 * 2236, rel=0.01)
    assert gm["full"]["bytes_per_gpu_per_step"] == pytest.approx(2048 * 4396, rel=0.01)
    assert gm["summary"]["bytes_per_gpu_per_step"] == pytest.approx(2048 * 76, rel=0.05)
    assert all(gm[m]["ms_per_step"] > 0 for m in gm) and gm["none"]["link_bound_ms_per_step"] == 0.0
    assert gm["full"]["link_bound_ms_per_step"] == pytest.approx(2 * gm["full-u16"]["link_bound_ms_per_step"], rel=0.02)
    # the plain `--gpus N` line carries the north star's workload - the whole-record gathers at the reference's
    # cadence (one record per agent step of 4 sub-steps) with their byte counts and link bounds, and configs[4]'s track mix
    r4 = d["gather_modes_repeat_4"]
    assert set(r4) == {"full-u16", "full"}
    for m, per_car in (("full-u16", 2236), ("full", 4396)):
        e = r4[m]
        assert e["action_repeat"] == 4 and e["bytes_per_gpu_per_agent_step"] == pytest.approx(2048 * per_car, rel=0.01)
        assert e["ms_per_agent_step"] > 0 and e["env_steps_per_s"] == pytest.approx(4 * e["agent_steps_per_s"], rel=1e-6)
        assert e["link_bound_ms_per_agent_step"] == pytest.approx(gm[m]["link_bound_ms_per_step"], rel=1e-6)
        assert e["check"]["ok"] is True and "agent step" in e["cadence"]
    mix = d["configs4_track_mix"]
    assert mix["tracks_by_rank"] == ["columbia", "austria"] and mix["gather"] == "sharded" and mix["env_steps_per_s"] > 0
    assert "configs[4]" in mix["workload"] and "`value` is timed with THIS payload" in d["config"]["workload"]
    assert d["gather_check"]["ok"] is True and {"full@repeat4", "full-u16@repeat4"} <= set(d["gather_check"]["payloads"])
