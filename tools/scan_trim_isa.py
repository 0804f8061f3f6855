#!/usr/bin/env python
"""The vector instructions of the scan's trip loop and of its rounds, per kernel (profiles/scan_trim_isa.txt).

  python tools/scan_trim_isa.py                      # compiles racing_dreamer_amd/csrc/racecar_kernels.hip with the build's flags
  python tools/scan_trim_isa.py --csrc DIR           # the same for another tree's csrc (the parent commit's, say)
  python tools/scan_trim_isa.py --asm kernels.s      # reads a listing made before (hipcc ... -S --cuda-device-only)
  python tools/scan_trim_isa.py --full PIECE ...     # kernels whose mangled name contains PIECE, every instruction printed

The scan (racecar_scan.h, scan_car) is bound by the rate at which a SIMD issues vector instructions, so what this prints is
its cost: for every kernel that goes through scan_car

  * the TRIP LOOPS - the innermost loops that hold the inline-assembly table request (global_load_ushort): the vector
    instructions a trip always executes, and apart from them those of the blocks it enters behind an exec-mask skip (the exact
    path: few trips take it);
  * the ROUND LOOP outside its trip loops - the loop body holds two rounds (two register sets take turns) -, block by block;
    blocks of the IEEE division (axis-parallel beams, lidar_transform 1) are marked, they run for few rounds or none;
  * registers, scratch, occupancy.

The first kernel named on the command line (default: the production kernel, one wave per car, no overlap, no bound) is printed
in full, the others as counts.  Needs hipcc, no GPU.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRODUCTION = "rc_raycast_car_kernelILi1ELb0ELb0E"
SCAN_KERNELS = ("rc_raycast_car_kernel", "rc_raycast_car_noise_kernel", "rc_raycast_group_kernel", "rc_raycast_group_noise_kernel",
                "rc_raycast_ts_kernel")


def compile_listing(csrc):
    from racing_dreamer_amd import build as rb
    flags = [f for f in rb.FLAGS if f not in ("-fPIC", "-shared")]
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "kernels.s")
    cmd = [rb.find_hipcc(), *flags, "-S", "--cuda-device-only", os.path.join(csrc, rb.SCAN_SOURCE), "-o", out]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(r.returncode)
    with open(out) as f:
        text = f.read()
    os.remove(out)
    os.rmdir(tmp)
    return text


def kernels_of(lines):
    """(name, first line, line of .end_amdhsa_kernel) of every kernel of SCAN_KERNELS in the listing."""
    found = []
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m and any(k + "I" in m.group(1) for k in SCAN_KERNELS):
            end = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
            found.append((m.group(1), i, end))
    return found


class Block:
    def __init__(self, label, depth, skipped):
        self.label, self.depth, self.skipped = label, depth, skipped     # skipped: entered behind an exec-mask skip
        self.code = []                                                    # (instruction text, is inline assembly)


def blocks_of(body):
    """The kernel's code as basic blocks in layout order.  A block's loop depth comes from the compiler's own comments
    ("in Loop: Header=BBn_m Depth=d", "Loop Header: Depth=d", "Parent Loop ... Depth=d" + "Inner Loop Header: Depth=d")."""
    blocks = [Block("entry", 0, False)]
    after_exec_skip, in_asm = False, False
    pending_label = None
    for raw in body:
        line = raw.strip()
        if ";;#ASMSTART" in line:
            in_asm = True
            continue
        if ";;#ASMEND" in line:
            in_asm = False
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        bbm = re.match(r"^; %bb\.(\d+):", line)
        if m or bbm:
            label = m.group(1) if m else "%bb." + bbm.group(1)
            depth = 0
            dm = re.search(r"Depth=(\d+)", line)
            if dm:
                depth = int(dm.group(1))
            blocks.append(Block(label, depth, after_exec_skip and bbm is not None))
            after_exec_skip = False
            pending_label = blocks[-1]
            continue
        if line.startswith(";") and pending_label is not None and not pending_label.code:
            dm = re.search(r"(?:Inner Loop Header|Loop Header): Depth=(\d+)", line)     # (a header's own depth is on its later comment lines)
            if dm:
                pending_label.depth = max(pending_label.depth, int(dm.group(1)))
            continue
        code = line.split(";")[0].strip()
        if not code or code.startswith("."):
            continue
        blocks[-1].code.append((code, in_asm))
        after_exec_skip = code.startswith(("s_cbranch_execz", "s_cbranch_execnz"))
    return blocks


def is_vector(code):
    return code.startswith("v_")


def loops(blocks, depth):
    """Runs of consecutive blocks at `depth` or deeper, each run starting at a block that is a header of that depth."""
    runs, cur = [], None
    for b in blocks:
        if b.depth >= depth:
            if cur is None:
                cur = []
                runs.append(cur)
            cur.append(b)
        else:
            cur = None
    return runs


def has_request(run):
    return any(a and c.startswith("global_load_ushort") for b in run for c, a in b.code)


def resources(tail):
    keep = {}
    for l in tail:
        m = re.search(r"; (NumVgprs|NumAgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize|codeLenInByte)\b[^0-9]*(\d+)", l)
        if m and m.group(1) not in keep:
            keep[m.group(1)] = int(m.group(2))
    return keep


def describe(name, lines, start, end, full):
    blocks = blocks_of(lines[start:end])
    res = resources(lines[end:end + 80])
    out = [f"== {name}"]
    trip_loops = [r for r in loops(blocks, 2) if has_request(r)]
    counts = []
    for n, run in enumerate(trip_loops):
        always = [c for b in run if not b.skipped for c, _ in b.code if is_vector(c)]
        behind = [c for b in run if b.skipped for c, _ in b.code if is_vector(c)]
        counts.append((len(always), len(behind)))
        if full:
            out.append(f"  trip loop {n} ({run[0].label} ..): {len(always)} vector instructions in every trip, {len(behind)} more behind an exec-mask skip")
            for b in run:
                for c, a in b.code:
                    if is_vector(c) or c.startswith(("global_load", "s_cbranch", "s_waitcnt")):
                        out.append(f"      {'?' if b.skipped else ' '} {c}{'    (asm)' if a else ''}")
    round_runs = [r for r in loops(blocks, 1) if any(has_request([b]) for b in r)]
    round_total = round_div = 0
    for run in round_runs:
        outside = [b for b in run if b.depth == 1]
        for b in outside:
            vec = [c for c, _ in b.code if is_vector(c)]
            division = any(c.startswith(("v_div_scale", "v_div_fmas")) for c in vec)
            round_total += len(vec)
            round_div += len(vec) if division else 0
            if full and vec:
                out.append(f"  round loop, block {b.label}{' behind an exec-mask skip' if b.skipped else ''}{' (IEEE division)' if division else ''}: {len(vec)}")
                if not division:
                    out.extend(f"        {c}" for c in vec)
    trips = ", ".join(f"{a} (+{b})" for a, b in counts)
    out.append(f"  trip loops: {trips} vector instructions per trip (+ behind a skip); round loop outside them, two rounds: "
               f"{round_total - round_div} vector instructions + {round_div} in division blocks")
    out.append("  -- " + "; ".join(f"{k}: {v}" for k, v in res.items()))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=os.path.join(ROOT, "racing_dreamer_amd", "csrc"))
    ap.add_argument("--asm", default=None)
    ap.add_argument("--full", nargs="*", default=[PRODUCTION])
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            text = f.read()
    else:
        text = compile_listing(a.csrc)
    lines = text.splitlines()
    found = kernels_of(lines)
    if not found:
        raise SystemExit("no scan kernel in the listing")
    found.sort(key=lambda k: (not any(p in k[0] for p in a.full), k[0]))
    for name, start, end in found:
        print("\n".join(describe(name, lines, start, end, any(p in name for p in a.full))))
        print()


if __name__ == "__main__":
    main()
