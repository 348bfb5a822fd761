#!/usr/bin/env python
"""Static instruction counts of the headline stem kernels, read from their gfx950 assembly:
tools/stem_asm_counts.py [--csrc DIR] [--out FILE]

Every kernel is compiled on its own (-DCTG_STEM_DEV_ONE=<template arguments>, a few seconds each) and its depth-1 loops
that hold matrix instructions -- the tile loop, one per role in a specialised-wave kernel -- are counted: vector (VALU,
without the MFMAs), MFMA, LDS, global memory, scalar, wait and nop instructions, with the most frequent vector mnemonics.
Counts are STATIC (both sides of a branch inside the loop are counted, an inner loop once); they compare two builds of
the same kernel, they are not cycles.  VGPR / AGPR / scratch / spills come from the kernel's notes, LDS is dynamic (host)."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the stem kernels one slice of sycamore_m20_native launches (profiles/r6_steps_sycamore_m20_native.txt, stem_shared_rows.txt)
HEADLINE = [
    ("h2", "false,false,1,1,2,1,true,0,false,true,false,false,0,false,true,false,true"),
    ("h2", "false,false,1,2,4,1,false,0,false,true,false,false,0,false,true,false,true"),
    ("h2", "false,false,1,1,8,1,false,0,false,true,false,false,0,false,true,false,true"),
    ("h2", "false,true,1,2,4,2,false,0,false,true,false,false,0,false,true,false,true"),
    ("h2", "false,false,1,2,2,1,false,0,false,true,false,false,0,false,true,false,true"),
    ("h2", "true,false,2,1,1,1,true,0,true,true,false,false,0,false,true,false,true"),
    ("h2", "true,false,2,1,1,1,true,0,false,true,false,false,0,false,true,false,true"),
    ("h2", "false,true,1,1,2,2,true,0,false,true,false,false,0,false,true,false,true"),
    ("h2", "false,false,1,1,4,1,false,0,false,true,false,false,0,false,true,false,true"),
    ("h2", "false,false,1,1,2,1,true,0,true,true,false,false,0,false,true,false,true"),
    ("h2", "true,true,2,1,4,1,false,0,false,true,false,false,0,false,true,false,true"),
    ("h2", "false,false,1,1,2,0,true,0,false,true,false,true,0,false,true,false"),
    ("h2", "false,false,1,4,4,0,false,0,false,true,false,true,0,false,true,false"),
    ("h2", "false,false,1,2,8,0,false,0,false,true,false,true,0,false,true,false"),
    ("h2", "false,false,1,1,8,0,false,0,false,true,false,true,0,false,true,false"),
    # the paired-store forms of the three kernels above whose consumers hold a row tile's two column groups (stem2h_kernel_p16)
    ("h2p", "false,false,1,1,2,1,true,0,false,true,false,false,0,false,true,false,true"),
    ("h2p", "false,false,1,2,2,1,false,0,false,true,false,false,0,false,true,false,true"),
    ("h2p", "false,false,1,1,4,1,false,0,false,true,false,false,0,false,true,false,true"),
    ("bf3", "false,false,1,1,2,2,true,0,false,true,false,false,0,false,true,false,false"),
    ("bf3", "false,false,1,1,1,2,true,0,false,true,false,false,0,false,true,false,false"),
    ("bf3", "false,true,1,1,2,2,true,0,false,true,false,false,0,false,true,false,false"),
]


def compile_one(job):
    csrc, tmp, i, (ar, targs) = job
    src = "ctg_stem_h2.hip" if ar in ("h2", "h2p") else "ctg_stem.hip"
    out = os.path.join(tmp, f"k{i}.s")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "--cuda-device-only", "-Wno-unused-command-line-argument", "-S", f"-DCTG_STEM_DEV_ONE={targs}", src, "-o", out]
                   + (["-DCTG_STEM_DEV_P16"] if ar == "h2p" else []),
                   check=True, cwd=csrc)
    return open(out).read().split("\n")


def kind(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_nop"):
        return "nop"
    if op.startswith("s_"):
        return "salu"
    return None


def count(L, i, j):
    c, ops = collections.Counter(), collections.Counter()
    for k in range(i, j + 1):
        l = L[k].split(";")[0].strip()
        if not l or l.startswith(".") or l.endswith(":"):
            continue
        op = l.split()[0]
        kd = kind(op)
        if kd:
            c[kd] += 1
            if kd == "valu":
                ops[re.sub(r"_(e32|e64|sdwa|dpp)$", "", op)] += 1
    return c, ops


def report(L):
    """The depth-1 loops with MFMAs: (first line, last line, counts, vector mnemonics)."""
    heads = [i for i, l in enumerate(L) if re.match(r"\.LBB\d+_\d+:.*Loop Header: Depth=1", l)]
    out = []
    for h in heads:
        name = L[h].split(":")[0]
        short = name[2:]   # "BB0_39" as the comments of the loop's other blocks spell it
        last = h
        for k in range(h + 1, len(L)):
            if L[k].startswith(".Lfunc_end"):
                break
            if re.search(r"s_c?branch\w*\s+" + re.escape(name) + r"\b", L[k]) or ("Header=" + short + " ") in L[k]:
                last = k
        # (the loop's last block runs to the next label or branch after its header comment)
        k = last
        while k + 1 < len(L) and not re.match(r"\.LBB\d+_\d+:", L[k + 1]) and not L[k + 1].startswith(".Lfunc_end"):
            k += 1
        c, ops = count(L, h, k)
        if c["mfma"]:
            out.append((h, k, c, ops))
    return out


def note(L, key):
    for l in L:
        m = re.match(r"\s+\." + key + r":\s+(\d+)", l)
        if m:
            return int(m.group(1))
    return -1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "cotengra_amd", "csrc"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(min(16, len(HEADLINE))) as pool:
        texts = list(pool.map(compile_one, [(a.csrc, tmp, i, k) for i, k in enumerate(HEADLINE)]))
    for (ar, targs), L in zip(HEADLINE, texts):
        lines.append(f"{ {'h2': 'stem2h_kernel', 'h2p': 'stem2h_kernel_p16'}.get(ar, 'stem2_kernel') }<{targs}>")
        lines.append(f"   vgpr {note(L, 'vgpr_count')}  agpr {note(L, 'agpr_count')}  scratch {note(L, 'private_segment_fixed_size')} B"
                     f"  spilled vgprs {note(L, 'vgpr_spill_count')}  static lds {note(L, 'group_segment_fixed_size')} B")
        # (most MFMAs first: the order in which the compiler lays the roles out changes from build to build)
        for n, (i, j, c, ops) in enumerate(sorted(report(L), key=lambda r: (-r[2]["mfma"], -r[2]["valu"]))):
            top = "  ".join(f"{op[2:]} {v}" for op, v in ops.most_common(9))
            lines.append(f"   loop {n} (lines {i}-{j}): valu {c['valu']}  mfma {c['mfma']}  valu/mfma {c['valu'] / c['mfma']:.2f}"
                         f"  lds {c['lds']}  vmem {c['vmem']}  salu {c['salu']}  wait {c['wait']}  nop {c['nop']}")
            lines.append(f"      {top}")
    text = "\n".join(lines) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
