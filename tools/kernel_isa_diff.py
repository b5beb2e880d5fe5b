#!/usr/bin/env python3
"""Compare the device code of two source trees, kernel by kernel (host only: nothing here touches a GPU).

    tools/kernel_isa_diff.py TREE_A TREE_B [--dev] [--renames FILE] [--only NAME.hip ...] [--jobs N]

Each tree's parq_amd/csrc/*.hip is compiled for the device alone

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only --no-gpu-bundle-output -c   (--dev adds -DPARQ_DEV_PROBES)

and the code objects are read with llvm-readelf -s (symbols), -S (where .text lies in the file) and --notes (the per-kernel
resource metadata).  Reported per source file: functions only in A, functions only in B, and the functions in both whose code
bytes or resources (registers, LDS, scratch, spills, workgroup size, kernel-argument size, the kernel descriptor apart from its
entry offset) differ; where bytes differ, a diff of the two disassemblies (llvm-objdump -d) without addresses and encodings follows.

--renames FILE: one `REGEX => REPLACEMENT` per line (blank lines and # comments skipped), applied with re.sub to A's mangled
names before matching: a kernel that lost a template parameter keeps its identity.  Exit status 1 when any kernel in both trees
differs, 0 otherwise (only-in-A / only-in-B lists are for the reader to judge).

Needs PyYAML (the metadata note is YAML) beside hipcc and the llvm-* tools of ROCm; the package itself depends on neither."""
from __future__ import annotations

import argparse
import concurrent.futures
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

try:
    import yaml
except ImportError:
    sys.exit("kernel_isa_diff.py needs PyYAML to read the kernels' metadata notes (llvm-readelf --notes prints YAML)")

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output", "-c"]
RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".vgpr_spill_count", ".sgpr_spill_count", ".uses_dynamic_stack", ".max_flat_workgroup_size", ".wavefront_size",
             ".kernarg_segment_size", ".kernarg_segment_align")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), check=True, capture_output=True, text=True).stdout


def compile_one(src, obj, dev):
    cmd = [HIPCC] + FLAGS + (["-DPARQ_DEV_PROBES"] if dev else []) + [src, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stderr))
    return obj


def read_object(obj):
    """{mangled name: {"code": bytes, "res": {...} or None, "kd": bytes or None}} of one code object."""
    raw = open(obj, "rb").read()
    sections = {}                  # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s+[0-9a-f]+", tool("llvm-readelf", "-S", "-W", obj), re.M):
        sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    syms = {}
    for line in tool("llvm-readelf", "-s", "-W", obj).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            addr, off = sections[int(f[6])]
            start = int(f[1], 16) - addr + off
            syms[f[7]] = (f[3], raw[start:start + int(f[2])])
    notes = tool("llvm-readelf", "--notes", obj)
    meta = yaml.safe_load(notes[notes.index("---"):notes.rindex("...")]) if "---" in notes else {}
    res = {k[".name"]: {r: k.get(r) for r in RESOURCES} for k in (meta or {}).get("amdhsa.kernels", [])}
    out = {}
    for name, (kind, data) in syms.items():
        if kind == "FUNC":
            kd = syms.get(name + ".kd")
            out[name] = {"code": data, "res": res.get(name), "kd": kd[1] if kd else None}
    return out


def disassembly(obj, name, renames=()):
    """The instructions of one function as text, without addresses and encodings (the bytes are compared separately) and with
    `renames` applied to the symbol names in branch targets."""
    text = tool("llvm-objdump", "-d", "--disassemble-symbols=" + name, obj)
    lines = []
    for line in text.splitlines():
        if not line.startswith("\t"):
            continue                                                    # file name, section and symbol headers
        line = re.sub(r"\s*//.*$", "", line)
        for rx, rep in renames:
            line = rx.sub(rep, line)
        lines.append(line.strip())
    return lines


def build_tree(tree, tmp, tag, dev, only, jobs):
    srcs = sorted(glob.glob(os.path.join(tree, "parq_amd", "csrc", "*.hip")))
    if only:
        srcs = [s for s in srcs if os.path.basename(s) in only]
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        futs = {os.path.basename(s): pool.submit(compile_one, s, os.path.join(tmp, tag + "_" + os.path.basename(s)[:-4] + ".co"), dev)
                for s in srcs}
        return {k: f.result() for k, f in futs.items()}


def load_renames(path):
    pairs = []
    for line in open(path) if path else []:
        line = line.strip()
        if line and not line.startswith("#"):
            a, b = line.split(" => ")
            pairs.append((re.compile(a.strip()), b.strip()))
    return pairs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--dev", action="store_true", help="compile with -DPARQ_DEV_PROBES")
    ap.add_argument("--renames", help="file of `REGEX => REPLACEMENT` lines applied to A's mangled names")
    ap.add_argument("--only", nargs="*", default=[], help="source file names to compare (default: all)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    renames = load_renames(a.renames)
    differ = 0
    totals = [0, 0, 0, 0]          # kernels in A, in B, only in A, only in B
    with tempfile.TemporaryDirectory() as tmp:
        objs_a = build_tree(a.tree_a, tmp, "a", a.dev, a.only, a.jobs)
        objs_b = build_tree(a.tree_b, tmp, "b", a.dev, a.only, a.jobs)
        print("# A = %s\n# B = %s\n# build: %s" % (a.tree_a, a.tree_b, "development (-DPARQ_DEV_PROBES)" if a.dev else "product"))
        for src in sorted(set(objs_a) | set(objs_b)):
            fa = read_object(objs_a[src]) if src in objs_a else {}
            fb = read_object(objs_b[src]) if src in objs_b else {}
            orig = {}              # name in B's terms -> A's own name
            for name in fa:
                new = name
                for rx, rep in renames:
                    new = rx.sub(rep, new)
                assert new not in orig, "two functions of A renamed to " + new
                orig[new] = name
            only_a = sorted(n for n in orig if n not in fb)
            only_b = sorted(n for n in fb if n not in orig)
            both = sorted(n for n in orig if n in fb)
            renamed = [n for n in both if orig[n] != n]
            kern = lambda d, names: sum(1 for n in names if d[n]["kd"] is not None)
            totals[0] += kern(fa, fa)
            totals[1] += kern(fb, fb)
            totals[2] += kern(fa, [orig[n] for n in only_a])
            totals[3] += kern(fb, only_b)
            bad = []
            for n in both:
                x, y = fa[orig[n]], fb[n]
                why = []
                if x["code"] != y["code"]:
                    why.append("code bytes (%d -> %d)" % (len(x["code"]), len(y["code"])))
                if x["res"] != y["res"]:
                    why.append("resources " + ", ".join("%s %s -> %s" % (r, x["res"][r], y["res"][r]) for r in RESOURCES
                                                         if x["res"] and y["res"] and x["res"][r] != y["res"][r]))
                kx, ky = x["kd"], y["kd"]
                # (bytes 16..23 of a descriptor are kernel_code_entry_byte_offset: where the code lies, not what it is)
                if (kx is None) != (ky is None) or (kx and kx[:16] + kx[24:] != ky[:16] + ky[24:]):
                    why.append("kernel descriptor")
                if why:
                    bad.append((n, why))
            print("\n== %s: %d functions in A (%d kernels), %d in B (%d kernels); %d in both (%d renamed), %d differ"
                  % (src, len(fa), kern(fa, fa), len(fb), kern(fb, fb), len(both), len(renamed), len(bad)))
            for n in only_a:
                print("  only in A: %s  (%d bytes)" % (orig[n], len(fa[orig[n]]["code"])))
            for n in only_b:
                print("  only in B: %s  (%d bytes)" % (n, len(fb[n]["code"])))
            for n in renamed:
                print("  renamed:   %s\n          -> %s" % (orig[n], n))
            for n, why in bad:
                differ += 1
                print("  DIFFERS:   %s: %s" % (n, "; ".join(why)))
                if fa[orig[n]]["code"] != fb[n]["code"]:
                    da, db = disassembly(objs_a[src], orig[n], renames), disassembly(objs_b[src], n)
                    for line in list(difflib.unified_diff(da, db, "A", "B", lineterm="", n=0))[2:]:
                        print("      " + line)
        print("\n# kernels: %d in A, %d in B; %d only in A, %d only in B; %d in both differ" % (*totals, differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
