#!/usr/bin/env python
"""Register, scratch, LDS and occupancy figures of every kernel of the result-tensor sources, at a git revision
and in the working tree, side by side: tools/result_resources.py [REV, default HEAD] > profiles/result_refactor_resources.txt

No device is needed: the sources are compiled for gfx950 with the flags of build() plus
-Rpass-analysis=kernel-resource-usage; the remarks are compared per kernel instantiation and the device assembly
per source.  Exit status 1 when a line differs."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ["ctg_sample.hip", "ctg_reduce.hip", "ctg_rdm.hip", "ctg_rdm_wide.hip", "ctg_pauli.hip", "ctg_pauli_apply.hip", "ctg_op_apply.hip",
           "ctg_pauli_spectrum.hip", "ctg_cost.hip"]
FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ")]


def remarks(csrc, src):
    """{kernel: figures} of one source, and its device assembly without comments and the compilation unit's id"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(os.path.join(csrc, src)):   # (a source the revision does not have yet)
        return {"": None}
    with tempfile.NamedTemporaryFile(suffix=".s") as asm:
        err = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", src,
                              "-o", asm.name, "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, check=True,
                             capture_output=True, text=True).stderr
        text = [ln for ln in open(asm.name).read().splitlines()
                if not re.match(r"\s*(;|\.ident|\.file)", ln) and "__hip_cuid_" not in ln]
    out, name = {"": text}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        for label, key in FIELDS:
            m = re.search(r"remark: .*\s" + re.escape(label) + r": (\d+)", line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def tree(csrc):
    with ThreadPoolExecutor(len(SOURCES)) as pool:
        return dict(zip(SOURCES, pool.map(lambda s: remarks(csrc, s), SOURCES)))


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "archive", rev, "cotengra_amd/csrc", "include"], cwd=ROOT, check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        parent = tree(os.path.join(tmp, "cotengra_amd", "csrc"))
    head = tree(os.path.join(ROOT, "cotengra_amd", "csrc"))
    demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip() or n   # noqa: E731
    keys = [k for _, k in FIELDS]
    print("# parent | head per kernel: " + " ".join(keys))
    differ = 0
    for s in SOURCES:
        asm_same = parent[s].pop("") == head[s].pop("")
        differ += not asm_same
        print(f"{s}: device assembly, comments and the compilation unit's id apart: {'same' if asm_same else 'DIFFERENT'}")
        for name in sorted(set(parent[s]) | set(head[s])):
            p, h = parent[s].get(name), head[s].get(name)
            fmt = lambda r: "absent" if r is None else " ".join(str(r.get(k, "?")) for k in keys)   # noqa: E731
            same = p == h
            differ += not same
            print(f"{s}: {demangle(name)}: {fmt(p)} | {fmt(h)} {'same' if same else 'DIFFERENT'}")
    print(f"# {differ} lines differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
