#!/usr/bin/env python
"""Drive cotengra_amd/csrc/tools/ctg_probe.hip: HBM rate of a streaming-kernel-shaped
copy for each store width / pattern, grid size and operand size."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = C.CDLL(os.path.join(ROOT, "cotengra_amd", "lib", "exp", "libctg_probe.so"))
lib.ctg_probe_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int]
names = {0: "16B load, 16B store", 1: "16B load, 8B store", 2: "16B load, 8B store (epilogue rows)",
         3: "16B load only", 4: "16B store only", 5: "8B store only"}
for gib in (8,):
    n = gib << 30
    src = torch.empty(n // 4, device="cuda", dtype=torch.float32).normal_()
    dst = torch.empty_like(src)
    nt = n // 4096
    for blocks, tpw in ((256 * 3, 0), (0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (0, 64)):
        if tpw:
            blocks = (nt + 4 * tpw - 1) // (4 * tpw)
        for mode in (0, 3, 4):
            def run():
                lib.ctg_probe_copy(src.data_ptr(), dst.data_ptr(), n, mode, blocks, None, tpw)
            run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 3
            moved = n * (2 if mode < 3 else 1)
            print(f"{gib:2d} GiB  blocks {blocks:7d} tasks/wave {tpw:2d}  {names[mode]:36s} {ms:8.3f} ms  {moved / ms / 1e9:6.2f} TB/s", flush=True)
    # the elementwise reference on the same buffers
    torch.mul(src, 2.0, out=dst); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        torch.mul(src, 2.0, out=dst)
    e1.record(); torch.cuda.synchronize()
    print(f"{gib:2d} GiB  torch.mul 1R:1W {2 * n / (e0.elapsed_time(e1) / 3) / 1e9:6.2f} TB/s")
    del src, dst

# ---- one stem workgroup: gather / store portions, start skew, cache policy, gather depth ----
# (profiles/stem_mempath_probe.txt; the kernel is described in ctg_probe.hip)
lib.ctg_probe_stemwg.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int] * 7 + [C.c_void_p]
n = 4 << 30
src = torch.empty(n // 4, device="cuda", dtype=torch.float32).normal_()
dst = torch.empty_like(src)
cus = torch.cuda.get_device_properties(0).multi_processor_count
tiles_per_wg = n // 65536 / cus


def stemwg(gf, sp, gd=2, nt=0, nm=3, skew=0, reps=3):
    def run():
        rc = lib.ctg_probe_stemwg(src.data_ptr(), dst.data_ptr(), n, gf, sp, gd, nt, nm, skew, cus, None)
        if rc:
            raise SystemExit(f"ctg_probe_stemwg({gf}, {sp}, {gd}, {nt}, {nm}, {skew}) -> {rc}")
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    return ms, 2 * n / ms / 1e9


print(f"\nstem workgroup model: {cus} workgroups of 8 waves, 4 GiB in + 4 GiB out, {tiles_per_wg:.0f} tiles per workgroup; TB/s (ms)")
for nm in (0, 2, 3, 6):
    print(f"MFMAs per group nm = {nm} ({16 * nm} per tile and gather wave, {32 * nm} per tile and store wave); rows: fire2 at a time, columns: stores at a time")
    print("            " + "".join(f"{sp:>16d}" for sp in (16, 8, 4, 2)))
    for gf in (4, 2, 1):
        cells = [stemwg(gf, sp, nm=nm) for sp in (16, 8, 4, 2)]
        print(f"   fire2 x{gf} " + "".join(f"{tb:8.2f} ({ms:5.3f})" for ms, tb in cells), flush=True)
base_ms = stemwg(4, 16)[0]
period = base_ms * 1e-3 / tiles_per_wg * 1e8   # tile period in ticks of the 100 MHz wall clock
print(f"start skew, nm = 3 (tile period {period:.0f} ticks of 10 ns): workgroup b starts (b & 7) / 8 of the skew late")
for frac in (0.0, 0.5, 1.0, 4.0):
    row = [stemwg(gf, sp, skew=int(frac * period)) for gf, sp in ((4, 16), (1, 2))]
    print(f"   skew {frac:3.1f} tile   bursts {row[0][1]:5.2f} ({row[0][0]:5.3f})   finest {row[1][1]:5.2f} ({row[1][0]:5.3f})", flush=True)
print("cache policy, nm = 3")
for nt, name in ((0, "plain"), (1, "non-temporal loads"), (2, "non-temporal stores"), (3, "non-temporal both")):
    row = [stemwg(gf, sp, nt=nt) for gf, sp in ((4, 16), (1, 2))]
    print(f"   {name:20s} bursts {row[0][1]:5.2f} ({row[0][0]:5.3f})   finest {row[1][1]:5.2f} ({row[1][0]:5.3f})", flush=True)
print("gather depth, nm = 3")
for gd in (2, 4):
    row = [stemwg(gf, sp, gd=gd) for gf, sp in ((4, 16), (1, 2))]
    print(f"   depth {gd}              bursts {row[0][1]:5.2f} ({row[0][0]:5.3f})   finest {row[1][1]:5.2f} ({row[1][0]:5.3f})", flush=True)
torch.mul(src, 2.0, out=dst)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(3):
    torch.mul(src, 2.0, out=dst)
e1.record()
torch.cuda.synchronize()
print(f"torch.mul 1R:1W on the same buffers {2 * n / (e0.elapsed_time(e1) / 3) / 1e9:6.2f} TB/s")
