#!/usr/bin/env python
"""The order of memory groups and waits in a compiled kernel (profiles/step_entry_isa.txt).

  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -std=c++17 -S --cuda-device-only \
      racing_dreamer_amd/csrc/racecar_kernels.hip -o kernels.s
  python tools/step_entry_isa.py kernels.s rc_dynamics_kernelILi1E rc_raycast_car_kernelILi1ELb0ELb0E

For each kernel whose mangled name contains one of the given pieces: consecutive scalar loads, vector loads, vector stores and
LDS operations are folded into one line each ("s_load x5", "global_load x19"), every s_waitcnt is its own line, and so are
branches, the long-latency division helpers (v_rcp_iflag_f32) and the end of the program; then the kernel's resource usage.
"""
import re
import sys


def kernel_body(lines, piece):
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and piece in l), None)
    if start is None:
        raise SystemExit(f"no kernel with {piece!r} in its name")
    end = next(i for i in range(start, len(lines)) if ".end_amdhsa_kernel" in lines[i])
    return lines[start].split(":")[0], lines[start:end]


def group_of(op):
    if op.startswith(("s_load_", "s_buffer_load")):
        return "s_load"
    if op.startswith(("global_load", "buffer_load", "flat_load")):
        return "global_load"
    if op.startswith(("global_store", "buffer_store", "flat_store")):
        return "global_store"
    if op.startswith("global_atomic"):
        return "global_atomic"
    if op.startswith("ds_"):
        return "lds"
    return None


def summarise(body):
    out, run, count, first = [], None, 0, 0
    def flush():
        nonlocal run, count
        if run is not None:
            out.append(f"  {first:6d}  {run} x{count}")
        run, count = None, 0
    in_asm = False
    for n, raw in enumerate(body):
        line = raw.strip()
        if ";;#ASMSTART" in line:
            in_asm = True
        if ";;#ASMEND" in line:
            in_asm = False
        code = line.split(";")[0].strip()
        if not code or code.startswith(".") or code.endswith(":"):
            continue
        op = code.split()[0]
        g = group_of(op)
        if g is not None:
            if g != run:
                flush()
                run, first = g, n
            count += 1
            continue
        if op == "s_waitcnt" or op.startswith(("s_cbranch", "s_branch", "s_endpgm", "v_rcp_iflag", "s_barrier", "s_memtime", "s_memrealtime")):
            flush()
            out.append(f"  {n:6d}  {code}{'   (inline asm)' if in_asm else ''}")
    flush()
    return out


def resources(body_and_tail):
    keep = []
    for l in body_and_tail:
        m = re.search(r"; (codeLenInByte|NumVgprs|NumAgprs|TotalNumVgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize)\b.*", l)
        if m:
            keep.append(m.group(0)[2:].strip())
    return keep


def main():
    path, pieces = sys.argv[1], sys.argv[2:]
    with open(path) as f:
        lines = f.read().splitlines()
    for piece in pieces:
        name, body = kernel_body(lines, piece)
        start = lines.index(body[0])
        tail = lines[start + len(body):start + len(body) + 80]
        print(f"== {name}")
        print("  (line in kernel, instruction or folded group)")
        print("\n".join(summarise(body)))
        print("  -- " + "; ".join(resources(tail)))
        print()


if __name__ == "__main__":
    main()
