#!/usr/bin/env python3
"""Kernel by kernel, the gfx950 instruction streams and resources of two source trees (a parent checkout and this one).  No GPU involved.

    python scripts/isa_diff.py PARENT_TREE THIS_TREE [--out profiles/NAME_isa_diff.txt] [--jobs 8]

Every .hip file of norlab_icp_mapper_amd/csrc of both trees is compiled with the Makefile's flags and --cuda-device-only -S.  A kernel counts
as the parent's when its instruction stream (labels renamed, comments dropped) and its VGPRs, AGPRs, SGPRs, scratch, LDS and occupancy --
read from the compiler's own summary behind the kernel, not measured -- are the parent's.  Kernels that were added, changed or removed are
listed with those figures."""
import argparse
import concurrent.futures as cf
import os
import re
import shutil
import subprocess
import sys
import tempfile

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]
FIELDS = (("NumVgprs", "VGPRs"), ("NumAgprs", "AGPRs"), ("TotalNumSgprs", "SGPRs"), ("ScratchSize", "scratch"), ("LDSByteSize", "LDS"), ("Occupancy", "occupancy"))


def compile_file(hipcc, src, out):
    subprocess.check_call([hipcc] + FLAGS + [src, "-o", out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


def kernels_of(asm_path, cxxfilt):
    """{demangled kernel name: (normalised instruction lines, {figure: value})}"""
    text = open(asm_path).read()
    text = re.sub(r"\.intern\.[0-9a-f]+|__intern__[0-9a-f]+", "", text)      # (the unique suffix of a kernel with internal linkage depends on the file's path)
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    dem = subprocess.run([cxxfilt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n") if cxxfilt else names
    out = {}
    for name, pretty in zip(names, dem):
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
        if not m:
            continue
        labels, lines = {}, []
        for ln in m.group(1).split("\n"):
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith(".") and not ln.startswith(".LBB"):
                continue
            lines.append(ln)
        body = "\n".join(lines)
        for lab in re.findall(r"\.LBB\d+_\d+", body):
            labels.setdefault(lab, "L%d" % len(labels))
        body = re.sub(r"\.LBB\d+_\d+", lambda mm: labels[mm.group(0)], body)
        tail = text[m.end():m.end() + 4000]
        figs = {}
        for key, _ in FIELDS:
            fm = re.search(r";\s*%s:\s*(\d+)" % key, tail)
            figs[key] = int(fm.group(1)) if fm else -1
        insts = [ln for ln in body.split("\n") if not ln.endswith(":")]
        out[pretty] = (body, figs, len(insts))
    return out


def figures(figs, insts):
    f = dict(figs)
    return "VGPRs %d, AGPRs %d, SGPRs %d, scratch %d bytes/lane, LDS %d bytes/workgroup, occupancy %d waves/SIMD, insts %d" % (
        f["NumVgprs"], f["NumAgprs"], f["TotalNumSgprs"], f["ScratchSize"], f["LDSByteSize"], f["Occupancy"], insts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--cxxfilt", default=shutil.which("c++filt") or shutil.which("llvm-cxxfilt"))   # (neither: the names stay mangled)
    a = ap.parse_args()
    sub = os.path.join("norlab_icp_mapper_amd", "csrc")
    files = sorted(f for f in os.listdir(os.path.join(a.this, sub)) if f.endswith(".hip"))
    lines = []
    total = same_total = 0
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(a.jobs) as pool:
        jobs = {}
        for side, tree in (("parent", a.parent), ("this", a.this)):
            for f in files:
                src = os.path.join(tree, sub, f)
                if os.path.exists(src):
                    jobs[(side, f)] = pool.submit(compile_file, a.hipcc, src, os.path.join(tmp, side + "_" + f + ".s"))
        for f in files:
            new = kernels_of(jobs[("this", f)].result(), a.cxxfilt)
            old = kernels_of(jobs[("parent", f)].result(), a.cxxfilt) if ("parent", f) in jobs else {}
            same = [k for k in old if k in new and old[k] == new[k]]
            changed = [k for k in old if k in new and old[k] != new[k]]
            gone = [k for k in old if k not in new]
            added = [k for k in new if k not in old]
            total += len(old)
            same_total += len(same)
            lines.append("== %s: %d kernels in the parent, %d with the parent's instruction stream and resources, %d changed, %d gone, %d added"
                         % (f, len(old), len(same), len(changed), len(gone), len(added)))
            for k in changed:
                lines.append("  changed %s\n      parent: %s\n      this:   %s" % (k, figures(*old[k][1:]), figures(*new[k][1:])))
            for k in gone:
                lines.append("  gone %s" % k)
            for k in added:
                lines.append("  added %s\n      %s" % (k, figures(*new[k][1:])))
    lines.append("")
    lines.append("total: %d of the parent's %d kernels have the parent's instruction stream (labels renamed) and its VGPRs, AGPRs, SGPRs, scratch, LDS "
                 "and occupancy" % (same_total, total))
    text = "\n".join(lines) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
