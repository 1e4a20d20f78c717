#!/usr/bin/env python3
"""Is the gfx950 code of the kernels in two source trees the same, byte for byte?

    python tools/solver_identity.py                      # HEAD (git archive) against the working tree
    python tools/solver_identity.py --parent REV         # another parent commit
    python tools/solver_identity.py --a DIR --b DIR      # any two trees
    python tools/solver_identity.py --out profiles/x.txt # write the report to a file as well
    python tools/solver_identity.py --units frp_occmap_render.hip frp_occmap_render_scan.hip   # other units than the solver's five
    python tools/solver_identity.py --units frp_occmap_fuse_points.hip:frp_occmap_fuse_batch.hip --rename fuse::points::=fuse::batch:: --common
                                                         # side A's unit against ANOTHER unit of side B, kernel by namesake

For each translation unit (by default the five of the solver), and for each flag set that ships -- the unit's PER_SOURCE_FLAGS of its own
tree's build.py and, for the main unit, the same without the -mllvm switches (build_default_flags_lib) -- the unit is compiled
device-only, its code object unbundled, and compared: the raw bytes of .text and .rodata (as sha256), the kernel symbols with
their demangled names, and each kernel's metadata from the notes (registers, LDS, scratch, spills, workgroup size).  Whole
ELF files are not compared: they carry a compilation-unit id derived from the output path.

Kernels are paired by demangled name.  --rename OLD=NEW rewrites side A's names first, so that a kernel that moved to another
namespace meets its namesake; --common compares the kernels both sides have and only lists the others (a unit that lost or gained
kernels: the sections then differ by construction and are not compared).

A refactoring of the sources is harmless when every unit reports "identical".  Exit status 1 otherwise.
The tool needs a compiler and a parent commit and no GPU; it is not part of the test suite.
"""
import argparse
import concurrent.futures
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

UNITS = ["frp_ipm_lds.hip", "frp_ipm_lds_mem.hip", "frp_ipm_lds_q4.hip", "frp_ipm_lds_q30.hip", "frp_ipm_lds_s2.hip"]
META = [".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".vgpr_spill_count", ".sgpr_spill_count", ".max_flat_workgroup_size"]


def load_build(tree):
    spec = importlib.util.spec_from_file_location("frp_build_" + hashlib.md5(tree.encode()).hexdigest(),
                                                  os.path.join(tree, "forces_resilient_planner_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def llvm_bin(B):
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(B.hipcc()))), "lib", "llvm", "bin")
    return d if os.path.exists(os.path.join(d, "clang-offload-bundler")) else "/opt/rocm/lib/llvm/bin"


def flag_sets(B, unit):
    """(label, flags): what build_native and, for the main unit, build_default_flags_lib give the compiler."""
    flags = list(B.PER_SOURCE_FLAGS.get(unit, []))
    sets = [("shipped", flags)]
    if unit == UNITS[0]:
        sets.append(("compiler-default", [f for i, f in enumerate(flags) if f != "-mllvm" and (i == 0 or flags[i - 1] != "-mllvm")]))
    return sets


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(" ".join(cmd) + "\n" + r.stderr)
    return r.stdout


def inspect(tree, B, unit, label, flags, work):
    """Compile one unit device-only and describe its code object."""
    llvm = llvm_bin(B)
    stem = os.path.join(work, unit + "." + label)
    bundle, co = stem + ".bundle", stem + ".co"
    src = os.path.join(tree, "forces_resilient_planner_amd", "csrc", unit)
    run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
         "-I" + os.path.join(tree, "include")] + flags + ["--cuda-device-only", "-c", src, "-o", bundle])
    run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + bundle,
         "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    out = {"sections": {}, "kernels": {}}
    raw = {}
    for sec in (".text", ".rodata"):
        f = stem + sec
        run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", sec + "=" + f, co, stem + ".copy"])
        raw[sec] = open(f, "rb").read()
        out["sections"][sec] = (len(raw[sec]), hashlib.sha256(raw[sec]).hexdigest())
    # kernels = the functions that have a kernel descriptor NAME.kd; their bytes inside .text
    syms = {}
    text_addr = None
    for line in run([os.path.join(llvm, "llvm-readelf"), "--sections", "--symbols", "--wide", co]).splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)", line)
        if m:
            text_addr = int(m.group(1), 16)
        m = re.match(r"\s*(\d+):\s+([0-9a-f]+)\s+(\d+)\s+(\w+)\s+\w+\s+\w+\s+\S+\s+(\S+)$", line)
        if m:
            syms[m.group(5)] = (int(m.group(2), 16), int(m.group(3)), m.group(4), m.group(1))
    names = sorted(n for n in syms if n + ".kd" in syms and syms[n][2] == "FUNC")
    by_num = {}  # the same table once more, demangled (a demangled name has blanks: the rest of the line)
    for line in run([os.path.join(llvm, "llvm-readelf"), "--symbols", "--wide", "--demangle", co]).splitlines():
        m = re.match(r"\s*(\d+):\s+[0-9a-f]+\s+\d+\s+\w+\s+\w+\s+\w+\s+\S+\s+(.+)$", line)
        if m:
            by_num[m.group(1)] = m.group(2)
    demangled = [by_num[syms[n][3]] for n in names]
    meta = kernel_metadata(run([os.path.join(llvm, "llvm-readelf"), "--notes", co]))
    for n, d in zip(names, demangled):
        addr, size = syms[n][:2]
        code = raw[".text"][addr - text_addr: addr - text_addr + size]
        out["kernels"][d] = {"symbol": n, "size": size, "sha256": hashlib.sha256(code).hexdigest(), "meta": meta.get(n, {})}
    return out


def kernel_metadata(notes):
    """{kernel symbol: {key: value}} from the amdhsa.kernels list of the code object's metadata note (printed as YAML)."""
    out, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"^(\s*)(- )?(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        indent, dash, key, val = len(m.group(1)), m.group(2), m.group(3), m.group(4).strip()
        if dash and indent == 2:  # a new entry of a top-level list (amdhsa.kernels)
            cur = {}
        if cur is None or indent + (2 if dash else 0) != 4:  # the kernel's own keys, not those of its .args
            continue
        if key == ".name":
            out[val.strip("'\"")] = cur
        elif key in META:
            cur[key] = int(val)
    return out


def renamed(r, renames):
    """Side A's description with its kernels under the names they have on side B."""
    def name(d):
        for old, new in renames:
            d = d.replace(old, new)
        return d
    return {"sections": r["sections"], "kernels": {name(d): k for d, k in r["kernels"].items()}}


def compare(a, b, common=False):
    """'' when identical, else what differs first.  common: only the kernels both sides have, and not the sections."""
    if not common and sorted(a["kernels"]) != sorted(b["kernels"]):
        only = sorted(set(a["kernels"]) ^ set(b["kernels"]))
        return "kernel sets differ: " + ", ".join(only[:4])
    both = sorted(set(a["kernels"]) & set(b["kernels"]))
    if not both:
        return "no kernel in common"
    for n in both:
        ka, kb = a["kernels"][n], b["kernels"][n]
        if ka["meta"] != kb["meta"]:
            return f"metadata of {n} differs: {ka['meta']} / {kb['meta']}"
        if ka["sha256"] != kb["sha256"] or ka["size"] != kb["size"]:
            return f"code of {n} differs ({ka['size']} / {kb['size']} bytes)"
    for sec in () if common else (".text", ".rodata"):
        if a["sections"][sec] != b["sections"][sec]:
            return f"{sec} differs outside the kernels' own code (device functions, tables)"
    return ""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="HEAD", help="commit whose tree is side A (default HEAD)")
    ap.add_argument("--a", help="side A: a source tree (instead of --parent)")
    ap.add_argument("--b", help="side B: a source tree (default: the tree this script is in)")
    ap.add_argument("--out", help="write the report here as well")
    ap.add_argument("--units", nargs="+", default=UNITS, metavar="UNIT[:UNIT_B]",
                    help="translation units under csrc/ (default: the solver's five); UNIT:UNIT_B compares side A's UNIT with side B's UNIT_B")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="replace OLD by NEW in side A's demangled kernel names before pairing (repeatable)")
    ap.add_argument("--common", action="store_true", help="compare the kernels both sides have; list the others without failing")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("-v", "--verbose", action="store_true", help="list every kernel with its metadata")
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    b_tree = os.path.abspath(args.b or here)
    with tempfile.TemporaryDirectory() as tmp:
        if args.a:
            a_tree, a_name = os.path.abspath(args.a), os.path.abspath(args.a)
        else:
            a_tree = os.path.join(tmp, "parent")
            os.makedirs(a_tree)
            rev = run(["git", "-C", here, "rev-parse", args.parent]).strip()
            tar = os.path.join(tmp, "parent.tar")
            run(["git", "-C", here, "archive", "-o", tar, rev, "forces_resilient_planner_amd", "include"])
            run(["tar", "-xf", tar, "-C", a_tree])
            a_name = "commit " + rev
        sides = []
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            for tag, tree in (("a", a_tree), ("b", b_tree)):
                B = load_build(tree)
                work = os.path.join(tmp, tag)
                os.makedirs(work)
                units = [u.split(":")[0 if tag == "a" else -1] for u in args.units]
                sides.append({(pair, l): pool.submit(inspect, tree, B, u, l, f, work) for pair, u in zip(args.units, units) for l, f in flag_sets(B, u)})
            res = [{k: f.result() for k, f in s.items()} for s in sides]
        renames = [r.split("=", 1) for r in args.rename]
        B = load_build(b_tree)
        lines = ["kernels: device code of two source trees, gfx950",
                 "compiler: " + run([B.hipcc(), "--version"]).splitlines()[1].strip(),
                 "A = " + a_name, "B = " + ("the tree of this report" if not args.b else b_tree), ""]
        bad = 0
        for key in res[0]:
            a, b = renamed(res[0][key], renames), res[1][key]
            diff = compare(a, b, args.common)
            bad += bool(diff)
            lines.append(f"{key[0]} [{key[1]} flags]: " + ("IDENTICAL" if not diff else "DIFFERENT -- " + diff))
            for sec in (".text", ".rodata"):
                lines.append(f"  {sec:8s} A {a['sections'][sec][0]:8d} B  sha256 {a['sections'][sec][1]}")
                lines.append(f"  {sec:8s} B {b['sections'][sec][0]:8d} B  sha256 {b['sections'][sec][1]}")
            lines.append(f"  kernels: A {len(a['kernels'])}, B {len(b['kernels'])}")
            if args.verbose or diff:
                for side, r in (("A", a), ("B", b)):
                    for n in sorted(r["kernels"]):
                        k = r["kernels"][n]
                        lines.append(f"    {side} {n}\n        {k['symbol']}  {k['size']} B  " +
                                     " ".join(f"{m[1:]}={k['meta'].get(m)}" for m in META))
            else:
                for n in sorted(set(a["kernels"]) & set(b["kernels"])):
                    k = a["kernels"][n]
                    lines.append(f"    {n}: {k['size']} B " + " ".join(f"{m[1:]}={k['meta'].get(m)}" for m in META))
                for side, r, other in (("A", a, b), ("B", b, a)):
                    for n in sorted(set(r["kernels"]) - set(other["kernels"])):
                        lines.append(f"    only in {side}: {n}")
        lines.append("")
        lines.append("RESULT: " + ("all units identical" if not bad else f"{bad} unit / flag set(s) differ"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
