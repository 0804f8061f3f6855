#!/usr/bin/env python3
"""Is the device code of two trees the same, kernel by kernel?  (No GPU needed: hipcc cross-compiles.)

    python tools/device_code_identity.py dump TREE OUT.json     # compile every unit of TREE, one block per kernel symbol
    python tools/device_code_identity.py compare A.json B.json  # same symbols, byte-identical blocks?

Every unit of TREE's build.SOURCES and build.LAB_SOURCES is compiled with the build's flags less `-fPIC -shared`, plus
`-S --cuda-device-only`.  The assembly is cut into one block per kernel symbol: the label to its `.end_amdhsa_kernel` (the
code, `s_endpgm`, the kernel descriptor) and its entry of the `amdhsa.kernels` metadata.  A kernel may move between units, so
what depends on its position in a unit is masked: the function index in local labels (`.LBB12_3` -> `.LBB_3`) and the
padding in front of a label's comment.  Lines that carry
the compilation-unit id or a source file name are dropped.  Device functions that are not inlined (`bin_usable`) get a block
of their own, so that a kernel's callee cannot change unseen.
"""
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile

LOCAL_LABEL = re.compile(r"(\.L[A-Za-z_]+?|\bBB)\d+_(\d+)")
FUNC_END = re.compile(r"\.Lfunc_(begin|end)\d+")
PADDING = re.compile(r"[ \t]+;")          # a label's comment is aligned by the label's length
DROPPED = ("__hip_cuid_", "\t.file\t", ".hip", "\t.ident\t")


def load_build(tree):
    path = os.path.join(tree, "racing_dreamer_amd", "build.py")
    spec = importlib.util.spec_from_file_location("rc_build_" + hashlib.md5(path.encode()).hexdigest(), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def normalise(lines):
    out = []
    for line in lines:
        if any(d in line for d in DROPPED):
            continue
        out.append(PADDING.sub(" ;", FUNC_END.sub(r".Lfunc_\1", LOCAL_LABEL.sub(r"\1_\2", line))))
    return "\n".join(out) + "\n"


def blocks_of(asm):
    """{symbol: (kind, text)} of one unit's device assembly."""
    lines = asm.splitlines()
    kernels = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel (\S+)", l) for l in lines) if m}
    functions = [m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", l) for l in lines) if m]
    found = {}
    for name in functions:
        start = lines.index(next(l for l in lines if l.startswith(name + ":")))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        found[name] = ["kernel" if name in kernels else "function", lines[start:end]]
    # the metadata entry of every kernel (a YAML list under amdhsa.kernels:, items start with "  - .")
    try:
        a = lines.index("amdhsa.kernels:")
    except ValueError:
        a = None
    if a is not None:
        item = []
        for l in lines[a + 1:] + ["end"]:
            if l.startswith("  - ") or not l.startswith("  "):
                if item:
                    name = next(x.split(":", 1)[1].strip() for x in item if x.strip().startswith(".name:"))
                    found[name][1] += ["; metadata"] + item
                item = []
                if not l.startswith("  - "):
                    break
            item.append(l)
    return {k: (kind, normalise(body)) for k, (kind, body) in found.items()}


def dump(tree, out_path):
    b = load_build(tree)
    csrc = os.path.join(tree, "racing_dreamer_amd", "csrc")
    flags = [f for f in b.FLAGS if f not in ("-fPIC", "-shared")]
    result = {"units": {}, "blocks": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for lib, sources in (("shipped", b.SOURCES), ("lab", b.LAB_SOURCES)):
            for src in sources:
                s_path = os.path.join(tmp, src + ".s")
                subprocess.run([b.find_hipcc(), *flags, "-S", "--cuda-device-only", os.path.join(csrc, src), "-o", s_path], cwd=csrc,
                               check=True, capture_output=True)
                with open(s_path) as f:
                    blocks = blocks_of(f.read())
                result["units"][src] = {"library": lib, "kernels": sum(1 for k, _ in blocks.values() if k == "kernel"),
                                        "functions": sum(1 for k, _ in blocks.values() if k == "function")}
                for name, (kind, text) in blocks.items():
                    key = lib + ":" + name
                    if key in result["blocks"]:
                        raise SystemExit(f"{name} is emitted by two units of the {lib} library")
                    result["blocks"][key] = {"unit": src, "kind": kind, "sha256": hashlib.sha256(text.encode()).hexdigest(), "text": text}
    with open(out_path, "w") as f:
        json.dump(result, f)
    for src, u in result["units"].items():
        print(f"{u['library']:8s} {src:24s} {u['kernels']:4d} kernels {u['functions']:3d} device functions")
    for lib in ("shipped", "lab"):
        print(f"{lib}: {sum(u['kernels'] for u in result['units'].values() if u['library'] == lib)} kernels")


def compare(a_path, b_path):
    with open(a_path) as f:
        a = json.load(f)["blocks"]
    with open(b_path) as f:
        b = json.load(f)["blocks"]
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    for blocks in (a, b):
        for v in blocks.values():
            v["text"] = PADDING.sub(" ;", v["text"])
    differ = sorted(k for k in set(a) & set(b) if a[k]["text"] != b[k]["text"])
    moved = sum(1 for k in set(a) & set(b) if a[k]["unit"] != b[k]["unit"])
    for k in only_a:
        print("only in", a_path, ":", k)
    for k in only_b:
        print("only in", b_path, ":", k)
    for k in differ:
        import difflib
        d = list(difflib.unified_diff(a[k]["text"].splitlines(), b[k]["text"].splitlines(), lineterm="", n=0))
        print(f"DIFFERS: {k} ({a[k]['unit']} -> {b[k]['unit']}), {len(d)} diff lines; first:")
        print("\n".join(d[:12]))
    print(f"{len(a)} symbols against {len(b)}: {len(set(a) & set(b)) - len(differ)} identical, {len(differ)} differ, "
          f"{len(only_a)} + {len(only_b)} unmatched; {moved} changed unit")
    if only_a or only_b or differ:
        raise SystemExit(1)
    print("identical")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
