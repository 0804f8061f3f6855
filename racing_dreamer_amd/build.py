"""Build libracecar_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libracecar_hip.so")
# one unit per subsystem ("where things live"); SCAN_SOURCE holds the scan kernels that verify_scan_assembly reads
SCAN_SOURCE = "racecar_kernels.hip"
SOURCES = [SCAN_SOURCE, "racecar_tracks.hip", "racecar_agents.hip", "racecar_gather.hip", "racecar_abi.hip", "racecar_policy.hip", "racecar_imagine.hip", "racecar_dream.hip", "racecar_dream_grad.hip", "racecar_returns.hip", "racecar_returns_grad.hip", "racecar_fit.hip", "racecar_observe.hip", "racecar_decode.hip", "racecar_decode_lidar.hip", "racecar_episode.hip", "racecar_lookahead.hip"]
HEADERS = ["racecar_device.h", "racecar_internal.h", "racecar_env.h", "racecar_car.h", "racecar_step.h", "racecar_substep.inc", "racecar_spec.h", "racecar_scan.h", "racecar_beam_pairs.h", "racecar_patch_exact.h", "racecar_policy.h", "racecar_policy_math.h", "racecar_policy_tiles.h", "racecar_rollout.h", "racecar_dream_grad.h", "racecar_episode.h", os.path.join("..", "..", "include", "racecar_hip.h")]
# The lab library: scan variants 0-6 and the instrumented build of the scan (racecar_lab.hip).  NOT part of the shipped
# library; built by build_lab() - which tools/ and the variant tests call - and loaded by libracecar_hip.so on first use.
LAB_PATH = os.path.join(LIB_DIR, "libracecar_lab.so")
LAB_SOURCES = ["racecar_lab.hip"]
# -ffp-contract=off: the env spec is "one IEEE fp32 operation per written operator" (DESIGN.md §2);
# a fused multiply-add would break bit-exact parity with the CPU oracle.
# -fno-slp-vectorize: packed fp32 (v_pk_*_f32) issues at half rate on gfx950, i.e. buys nothing over two scalar
# operations, and costs register-pair copies, explicit |x| / -x operands and wait states (tools/ubench/valu_issue4.hip);
# the places where a packed form does help are written as explicit vector types.
# -fvisibility=hidden: the libraries export their C interface (rc_*, rclab_*: declared under a visibility pragma) and nothing else.
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-shared", "-std=c++17", "-Wall",
         "-Wno-unused-function", "-fvisibility=hidden"]


def find_hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (looked on PATH and in /opt/rocm/bin)")


BUILD_ID_MARK = b"RC_BUILD_ID="


def source_hash(csrc: str = CSRC, flags=None, sources=None) -> str:
    """sha256 over the flags and the CONTENT of every source and header the library is made of (in a fixed order, each
    preceded by its name): the identity of a build.  It is compiled into the library (`-DRC_BUILD_ID`, `rc_build_id()`),
    so whether a library on disk belongs to the sources beside it is a question about contents, not about file times - a
    tree pushed with a stale `.so` that happens to be newer than its sources is rebuilt."""
    import hashlib
    h = hashlib.sha256()
    h.update("\0".join(FLAGS if flags is None else flags).encode())
    for name in (SOURCES if sources is None else sources) + HEADERS:
        with open(os.path.join(csrc, name), "rb") as f:
            h.update(b"\0" + os.path.basename(name).encode() + b"\0" + f.read())
    return h.hexdigest()[:32]


def headers_hash(csrc: str = CSRC) -> str:
    """sha256 over the CONTENT of the headers alone: what the shipped library and the lab library must have in common (RcParams,
    RcLaunchInfo and RcLabTables cross between them by pointer).  Compiled into both as -DRC_HEADERS_ID; the loader compares."""
    import hashlib
    h = hashlib.sha256()
    for name in HEADERS:
        with open(os.path.join(csrc, name), "rb") as f:
            h.update(b"\0" + os.path.basename(name).encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def _tmp_beside(path: str) -> str:
    """A temporary name next to `path` that no other process uses: N ranks may build the same library at once (the lab on first
    use of a variant), and a shared `.new` let one replace or remove the file another was still writing."""
    import tempfile
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".new", dir=os.path.dirname(path))
    os.close(fd)
    return tmp


def library_build_id(path: str = LIB_PATH):
    """The build id a library file carries (the string behind `rc_build_id()`), read from the file's bytes - no dlopen, so
    asking does not load a stale library into the process.  None if the file is missing or carries none."""
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError:
        return None
    at = blob.find(BUILD_ID_MARK)
    if at < 0:
        return None
    tail = blob[at + len(BUILD_ID_MARK):at + len(BUILD_ID_MARK) + 32]
    return tail.decode("ascii", "replace") if len(tail) == 32 and all(c in b"0123456789abcdef" for c in tail) else None


def needs_build(lib_path: str = LIB_PATH, csrc: str = CSRC) -> bool:
    return library_build_id(lib_path) != source_hash(csrc)


# Kernels that hand a register to an asynchronous load through inline assembly and wait for it in a LATER assembly
# statement (the scan's table request, racecar_scan.h: trip_head / trip_tail): between the two the compiler believes
# the value is there.  That is safe as long as it keeps the value where the load will write it - it does not copy a live
# register without need - but a spill of that register to scratch would store it BEFORE the load has landed.  So the build
# refuses a library in which one of these kernels spills or uses scratch at all, and one that has fallen below the
# occupancy the launch geometry assumes.
# One row per checked kernel: (name, minimum waves per SIMD or None, its in-flight loads are checked, the library that must
# show it: "shipped" | "lab" | None).  Every row is a no-spill kernel.
CHECKED_KERNELS = (
    ("rc_raycast_car_kernel", 8, True, "shipped"),
    ("rc_raycast_car_stamps_kernel", None, True, "lab"),
    ("rc_raycast_kernel", None, True, "lab"),
    ("rc_patch_car_kernel", 8, False, "shipped"),
    # (the exact prefilter holds a line per lane in 161 + registers: one wave per SIMD by design - what it must not do is spill)
    ("rc_patch_exact_prefilter_kernel", None, False, "shipped"),
    ("rc_patch_exact_sample_kernel", 4, False, "shipped"),
    ("rc_raycast_car_noise_kernel", 8, True, "shipped"),        # (the scan with LiDAR noise: same trip loop)
    ("rc_raycast_group_noise_kernel", None, True, "shipped"),
    ("rc_raycast_ts_kernel", 8, True, "shipped"),               # (a track set: the same scan and render)
    ("rc_patch_ts_kernel", 8, False, "shipped"),
    ("rc_policy_kernel", None, False, "shipped"),               # (the Dreamer agent: 4 to 6 MFMA accumulator tiles per wave - a spill would sit in its k loops)
    ("rc_policy_sampled_kernel", None, False, "shipped"),       # (its sampled modes: the same body, plus the draws)
    ("rc_policy_imagine_kernel", None, False, "shipped"),       # (imagination: the same tiles in a loop over the horizon)
    ("rc_policy_imagine_sampled_kernel", None, False, "shipped"),
    ("rc_policy_dream_kernel", None, False, "shipped"),         # (planning in the latent: imagination's prior and head over (start, candidate) rows)
    ("rc_policy_dream_sampled_kernel", None, False, "shipped"),
    ("rc_policy_dream_grad_kernel", None, False, "shipped"),    # (the dream's backward pass: the forward's tiles, then the transposed products' two to four)
    ("rc_policy_dream_grad_sampled_kernel", None, False, "shipped"),
    ("rc_policy_returns_kernel", None, False, "shipped"),       # (imagination with the critic's heads and the lambda-return behind it)
    ("rc_policy_returns_sampled_kernel", None, False, "shipped"),
    ("rc_policy_returns_grad_kernel", None, False, "shipped"),  # (the actor loss's backward pass: item 20's forward, then three heads' and the prior's transposed products)
    ("rc_policy_returns_grad_sampled_kernel", None, False, "shipped"),
    ("rc_policy_fit_rows_kernel", None, False, "shipped"),      # (the critic's fit: the head forward and backward on the same tiles)
    ("rc_policy_fit_reward_rows_kernel", None, False, "shipped"),     # (the reward head's: the same body at two hidden layers)
    ("rc_policy_fit_wgrad_kernel", None, False, "shipped"),     # (its weight gradients: one accumulator tile per wave over all rows)
    ("rc_policy_observe_kernel", None, False, "shipped"),       # (recorded sequences: imagination's tiles and the agent's staged scan)
    ("rc_policy_observe_sampled_kernel", None, False, "shipped"),
    ("rc_look_ahead_kernel", None, False, "shipped"),           # (a look-ahead keeps an env's cars in registers through the horizon: a spill would sit in its sub-step)
    ("rc_policy_decode_kernel", 4, False, "shipped"),           # (the decoder: two workgroups of eight waves per CU; a spill would sit in its tap loops)
    ("rc_policy_decode_loglik_kernel", 4, False, "shipped"),    # (the same body with the Bernoulli log-likelihood)
    ("rc_policy_decode_lidar_kernel", None, False, "shipped"),  # (the LiDAR decoder: four MFMA accumulator tiles per wave and their prefetched operands)
)
NO_SPILL_KERNELS = tuple(k for k, _, _, _ in CHECKED_KERNELS)
MIN_WAVES_PER_SIMD = {k: w for k, w, _, _ in CHECKED_KERNELS if w is not None}
ASYNC_LOAD_KERNELS = tuple(k for k, _, load, _ in CHECKED_KERNELS if load)


def required_kernels(library: str):
    return tuple(k for k, _, _, lib in CHECKED_KERNELS if lib == library)


def check_resource_usage(remarks: str, required=("rc_raycast_car_kernel", "rc_patch_car_kernel"), min_waves=None) -> None:
    """Parse `-Rpass-analysis=kernel-resource-usage` remarks; raise if a kernel of NO_SPILL_KERNELS spills."""
    min_waves = MIN_WAVES_PER_SIMD if min_waves is None else min_waves
    import re
    name, problems, seen = None, [], set()
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", line)
        if not m or name is None:
            continue
        kernel = next((k for k in NO_SPILL_KERNELS if k + "I" in name or name.endswith(k) or k + "E" in name or re.search(k + r"\d", name)), None)
        if kernel is None:
            continue
        seen.add(kernel)
        key, val = m.group(1), int(m.group(2))
        if key.startswith("Occupancy"):
            if val < min_waves.get(kernel, 1):
                problems.append(f"{name}: {val} waves/SIMD < {min_waves[kernel]}")
        elif key != "SGPRs Spill" and val != 0:
            problems.append(f"{name}: {key} = {val}")
    missing = [k for k in required if k not in seen]
    if missing:
        raise RuntimeError(f"resource-usage remarks not found for {missing}: cannot verify that the scan does not spill")
    if problems:
        raise RuntimeError("build refused (see racing_dreamer_amd/build.py, NO_SPILL_KERNELS):\n  " + "\n  ".join(problems))


def check_async_load_registers(asm_text: str, kernels=ASYNC_LOAD_KERNELS) -> int:
    """The scan requests a table entry with an inline-assembly `global_load_ushort` and waits for it in a LATER statement
    (`s_waitcnt vmcnt(0)`): until then the destination register is not the compiler's to read, copy or overwrite, and
    nothing tells it so.  This walks the generated assembly of the scan kernels and raises if any instruction between such
    a load and the next wait for it (in layout order) touches the destination register.  Returns the number of loads
    checked."""
    import re
    checked, problems = 0, []
    kernel, pending, in_asm = None, None, False
    for raw in asm_text.splitlines():
        line = raw.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            kernel = m.group(1) if any(k in m.group(1) for k in kernels) else None
            pending = None
            continue
        if kernel is None or not line or line.startswith((";", ".", "//")) and "#ASM" not in line:
            if ";;#ASMSTART" in line:
                in_asm = True
            elif ";;#ASMEND" in line:
                in_asm = False
            continue
        if ";;#ASMSTART" in line:
            in_asm = True
            continue
        if ";;#ASMEND" in line:
            in_asm = False
            continue
        if "s_endpgm" in line:
            kernel, pending = None, None
            continue
        code = line.split(";")[0].strip()
        if not code or code.endswith(":"):
            continue
        if pending is not None:
            if code.startswith("s_waitcnt") and "vmcnt(0)" in code:
                pending = None
            else:
                regs = set(int(r) for r in re.findall(r"\bv(\d+)\b", code))
                for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", code):
                    regs.update(range(int(a), int(b) + 1))
                if pending[0] in regs:
                    problems.append(f"{kernel}: `{code}` touches v{pending[0]} while `{pending[1]}` is in flight")
                    pending = None
        m = re.match(r"^global_load_ushort v(\d+),", code)
        if m and in_asm:
            pending = (int(m.group(1)), code)
            checked += 1
    if problems:
        raise RuntimeError("build refused: a register with an asynchronous load in flight is used before its wait\n  " + "\n  ".join(problems[:8]))
    if checked == 0:
        raise RuntimeError("no inline-assembly table request found in the scan kernels: the check does not see what it should")
    return checked


def verify_scan_assembly(verbose: bool = True, csrc: str = CSRC, source: str = None) -> int:
    """Compile the unit that holds the scan kernels to assembly once more (device only) and run check_async_load_registers on it."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "kernels.s")
        flags = [f for f in FLAGS if f not in ("-fPIC", "-shared")]
        cmd = [find_hipcc(), *flags, "-S", "--cuda-device-only", os.path.join(csrc, source or SCAN_SOURCE), "-o", out]
        r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise subprocess.CalledProcessError(r.returncode, cmd)
        with open(out) as f:
            n = check_async_load_registers(f.read())
    if verbose:
        print(f"[racing_dreamer_amd.build] scan assembly: {n} in-flight table requests, none touched before its wait", flush=True)
    return n


LAST_BUILD = {"action": None, "build_id": None}      # what the last build() call did: "compiled" | "reused"


def _compile(what: str, sources, want: str, out_path: str, csrc: str, verbose: bool, required, min_waves, scan_source: str) -> None:
    """One hipcc command over `sources` into `out_path` (through a temporary beside it), refused if a checked kernel spills, has
    fallen below its occupancy or touches a register under an asynchronous load."""
    import time
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    tmp = _tmp_beside(out_path)
    cmd = [find_hipcc(), *FLAGS, f'-DRC_BUILD_ID="{want}"', f'-DRC_HEADERS_ID="{headers_hash(csrc)}"', "-Rpass-analysis=kernel-resource-usage",
           *[os.path.join(csrc, s) for s in sources], "-o", tmp]
    if verbose:
        print("[racing_dreamer_amd.build]", " ".join(cmd), flush=True)
    t0 = time.time()
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    other = [l for l in r.stderr.splitlines() if "kernel-resource-usage" not in l and not l.startswith(("      |", " ")) and "hip-link" not in l]
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-8000:])
        if os.path.exists(tmp):
            os.remove(tmp)
        raise subprocess.CalledProcessError(r.returncode, cmd)
    if other and verbose:
        print("\n".join(other), file=sys.stderr)
    try:
        check_resource_usage(r.stderr, required=required, min_waves=min_waves)
        verify_scan_assembly(verbose, csrc, source=scan_source)
    except RuntimeError:
        os.remove(tmp)
        raise
    os.chmod(tmp, 0o755)
    os.replace(tmp, out_path)
    if library_build_id(out_path) != want:
        raise RuntimeError(f"{out_path} does not carry the build id it was compiled with ({library_build_id(out_path)} != {want})")
    if verbose:
        print(f"[racing_dreamer_amd.build] compiled {out_path} in {time.time() - t0:.1f} s ({what}, build id {want})", flush=True)


def build(force: bool = False, verbose: bool = True, csrc: str = CSRC, lib_path: str = LIB_PATH) -> str:
    """Compile `csrc` into `lib_path` unless the library there already carries the hash of those sources and the flags
    (`LAST_BUILD["action"]` says which happened).  The defaults are the package's own tree; the tests build copies."""
    want = source_hash(csrc)
    LAST_BUILD.update(action="reused", build_id=want)
    if not force and library_build_id(lib_path) == want:
        if verbose:
            print(f"[racing_dreamer_amd.build] reused {lib_path}: its build id {want} is the hash of the sources and flags", flush=True)
        return lib_path
    _compile("the shipped library", SOURCES, want, lib_path, csrc, verbose, required_kernels("shipped"), None, SCAN_SOURCE)
    LAST_BUILD.update(action="compiled")
    return lib_path


def build_lab(force: bool = False, verbose: bool = True, csrc: str = CSRC, lab_path: str = LAB_PATH) -> str:
    """Compile the lab library (scan variants 0-6, the stamps build) unless the one at `lab_path` already carries the hash of
    its sources: same flags, same refusals (no spills in a scan kernel, no register touched under an asynchronous load)."""
    want = source_hash(csrc, sources=LAB_SOURCES)
    if not force and library_build_id(lab_path) == want:
        if verbose:
            print(f"[racing_dreamer_amd.build] reused {lab_path}: its build id {want} is the hash of the lab's sources and flags", flush=True)
        return lab_path
    _compile("the lab library", LAB_SOURCES, want, lab_path, csrc, verbose, required_kernels("lab"), {}, LAB_SOURCES[0])
    return lab_path


def lab_needs_build(lab_path: str = LAB_PATH, csrc: str = CSRC) -> bool:
    return library_build_id(lab_path) != source_hash(csrc, sources=LAB_SOURCES)


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB_PATH)
    if "--lab" in sys.argv:
        print(build_lab(force="--force" in sys.argv))
