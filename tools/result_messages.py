#!/usr/bin/env python
"""The text of ``ctg_last_error()`` for every refusal of the entry points that read the result tensor -- the rows of
the three ``test_refusals_through_the_c_abi`` lists (tests/test_gpu_pauli.py, test_gpu_pauli_apply.py,
test_gpu_op_apply.py), the rdm and marginal refusals, top-k, the draws and the NaN member -- on 2^13-element complex64
and float32 resident results.  One line per case: ``<entry point> <case>: <return code> <message>``.

    python tools/result_messages.py                        # the library in use (CTG_LIB, else the built one)
    python tools/result_messages.py --libs A.so B.so --out profiles/result_refactor_messages.txt

``--libs`` runs every library in a fresh process of its own and writes the one output if all agree; else it prints the
lines that differ and exits 1.  Needs the device (an executor)."""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def walk():
    import numpy as np
    import torch

    import cotengra_amd as ca
    from cotengra_amd import runtime
    from cotengra_amd.contractor import _tree_contractor

    lib = runtime.load()
    n = 2 ** 13
    i64p, i32p, u8p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)

    def resident(x):
        ex = _tree_contractor(ca.ContractionTree(["a"], "a", {"a": x.size})).setup(x)["exec"]
        ex.zero_result()
        ex.run_slices()
        return ex

    def ptr(a, t):
        return None if a is None else np.ascontiguousarray(a).ctypes.data_as(t)

    def say(what, case, rc):
        print(f"{what} {case}: {rc} {lib.ctg_last_error().decode('utf-8', 'replace') if rc else ''}".rstrip(), flush=True)

    rng = np.random.default_rng(13)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype("complex64")
    xr = rng.standard_normal(n).astype("float32")
    nanx = x.copy()
    nanx[4097] = np.nan
    ex, exr, exn = resident(x), resident(xr), resident(nanx)
    exz = resident(np.zeros(n, "complex64"))
    i64 = lambda *v: np.array(v, np.int64)   # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)   # noqa: E731
    own = ex.handle
    over = i64(2 ** 21, 2 ** 21, 2)          # the running product passes 2^40 before the last axis

    # -- ctg_exec_result_pauli -- #
    ext = i64(2, 2, 2048)
    ops = np.array([[1, 3, 0], [2, 2, 0]], np.uint8)
    out = np.full(4097, 7.0)
    big = np.zeros((4097, 3), np.uint8)
    rows = [(None, 3, ext, 2, ops, out), (own, 3, None, 2, ops, out), (own, 3, ext, 2, None, out), (own, 3, ext, 2, ops, None),
            (own, -1, ext, 2, ops, out), (own, 3, i64(2, 2, 2047), 2, ops, out), (own, 2, ext, 2, ops, out),
            (own, 3, i64(2, 2, 0), 2, ops, out), (own, 3, over, 2, ops, out), (own, 3, ext, -1, ops, out),
            (own, 3, ext, 4097, big, out), (own, 3, ext, 2, np.array([[1, 3, 0], [2, 4, 0]], np.uint8), out),
            (own, 3, ext, 2, np.array([[1, 3, 0], [0, 255, 0]], np.uint8), out),
            (own, 3, ext, 2, np.array([[1, 3, 0], [0, 0, 1]], np.uint8), out),
            (own, 3, i64(4, 1, 2048), 2, np.array([[0, 3, 0], [0, 0, 0]], np.uint8), out),
            (exn.handle, 3, ext, 2, ops, out)]
    for i, (h, rank, e_, m, o_, out_) in enumerate(rows):
        say("pauli", i, lib.ctg_exec_result_pauli(h, rank, ptr(e_, i64p), m, ptr(o_, u8p), ptr(out_, dp)))

    # -- ctg_exec_result_pauli_apply -- #
    cs = np.array([0.5, -1.25])
    dev = torch.full((n,), 7.0 + 7.0j, dtype=torch.complex64, device="cuda")
    devr = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    host, hostr = np.full(n, 7.0 + 7.0j, dtype=np.complex64), np.full(n, 7.0, dtype=np.float32)
    d, res = dev.data_ptr(), ex.result_ptr()
    rows = [(None, 3, ext, 2, ops, cs, d, host), (own, 3, None, 2, ops, cs, d, host), (own, 3, ext, 2, None, cs, d, host),
            (own, 3, ext, 2, ops, None, d, host), (own, 3, ext, 2, ops, cs, None, None), (own, 3, ext, 2, ops, cs, res, host),
            (own, 3, ext, 2, ops, cs, res + 8 * (n - 1), host), (own, 3, ext, 2, ops, cs, res - 8 * (n - 1), host),
            (own, -1, ext, 2, ops, cs, d, host), (own, 3, i64(2, 2, 2047), 2, ops, cs, d, host), (own, 2, ext, 2, ops, cs, d, host),
            (own, 3, i64(2, 2, 0), 2, ops, cs, d, host), (own, 3, over, 2, ops, cs, d, host), (own, 3, ext, -1, ops, cs, d, host),
            (own, 3, ext, 4097, big, np.ones(4097), d, host),
            (own, 3, ext, 2, np.array([[1, 3, 0], [2, 4, 0]], np.uint8), cs, d, host),
            (own, 3, ext, 2, np.array([[1, 3, 0], [0, 0, 1]], np.uint8), cs, d, host),
            (own, 3, ext, 2, ops, np.array([0.5, np.nan]), d, host), (own, 3, ext, 2, ops, np.array([np.inf, 1.0]), d, host),
            (exr.handle, 3, ext, 2, np.array([[1, 3, 0], [2, 0, 0]], np.uint8), cs, devr.data_ptr(), hostr),
            (exn.handle, 3, ext, 2, ops, cs, None, host)]
    for i, (h, rank, e_, m, o_, c_, dev_, host_) in enumerate(rows):
        say("pauli_apply", i, lib.ctg_exec_result_pauli_apply(h, rank, ptr(e_, i64p), m, ptr(o_, u8p), ptr(c_, dp), C.c_void_p(dev_),
                                                              C.c_void_p(None if host_ is None else host_.ctypes.data)))

    # -- ctg_exec_result_op_apply -- #
    ext = i64(2, 2, 2, 1024)
    ms = rng.standard_normal(2 * (16 + 4))
    na, ax = i32(2, 1), i32(0, 2, 1)
    nan, inf = ms.copy(), ms.copy()
    nan[5], inf[-1] = np.nan, np.inf
    many = 4097
    rows = [(None, 4, ext, 2, na, ax, ms, d, host), (own, 4, None, 2, na, ax, ms, d, host), (own, 4, ext, 2, None, ax, ms, d, host),
            (own, 4, ext, 2, na, None, ms, d, host), (own, 4, ext, 2, na, ax, None, d, host), (own, 4, ext, 2, na, ax, ms, None, None),
            (own, 4, ext, 2, na, ax, ms, res, host), (own, 4, ext, 2, na, ax, ms, res + 8 * (n - 1), host),
            (own, 4, ext, 2, na, ax, ms, res - 8 * (n - 1), host), (own, -1, ext, 2, na, ax, ms, d, host),
            (own, 4, i64(2, 2, 2, 1023), 2, na, ax, ms, d, host), (own, 3, ext, 2, na, ax, ms, d, host),
            (own, 4, i64(2, 2, 2, 0), 2, na, ax, ms, d, host), (own, 4, i64(2 ** 21, 2 ** 21, 2, 2), 2, na, ax, ms, d, host),
            (own, 4, ext, -1, na, ax, ms, d, host),
            (own, 4, ext, many, np.ones(many, np.int32), np.zeros(many, np.int32), np.zeros(8 * many), d, host),
            (own, 4, ext, 2, i32(2, 0), ax, ms, d, host), (own, 4, ext, 2, na, i32(0, 4, 1), ms, d, host),
            (own, 4, ext, 2, na, i32(-1, 2, 1), ms, d, host), (own, 4, ext, 2, na, i32(2, 0, 1), ms, d, host),
            (own, 4, ext, 2, na, i32(2, 2, 1), ms, d, host), (own, 4, ext, 1, i32(1), i32(3), np.zeros(2 * 1024 * 1024), d, host),
            (own, 4, ext, 2, na, ax, nan, d, host), (own, 4, ext, 2, na, ax, inf, d, host),
            (own, 13, i64(*[2] * 13), 257, np.full(257, 6, np.int32), np.tile(np.arange(6, dtype=np.int32), 257),
             np.zeros(257 * 64 * 64 * 2), d, host),
            (exr.handle, 4, ext, 2, na, ax, ms, devr.data_ptr(), hostr), (exn.handle, 4, ext, 2, na, ax, ms, None, host)]
    for i, (h, rank, e_, m, n_, a_, m_, dev_, host_) in enumerate(rows):
        say("op_apply", i, lib.ctg_exec_result_op_apply(h, rank, ptr(e_, i64p), m, ptr(n_, i32p), ptr(a_, i32p), ptr(m_, dp),
                                                        C.c_void_p(dev_), C.c_void_p(None if host_ is None else host_.ctypes.data)))

    # -- ctg_exec_result_rdm, ctg_exec_result_marginal: the same split of the axes -- #
    big_out = np.zeros(128 * 128 * 2)
    rows = [(None, 2, i64(64, 128), i32(1, 0), big_out), (own, 2, i64(64, 128), i32(1, 0), None), (own, -1, i64(64, 128), i32(1, 0), big_out),
            (own, 2, None, i32(1, 0), big_out), (own, 2, i64(64, 128), None, big_out), (own, 2, i64(n // 2, 3), i32(1, 0), big_out),
            (own, 1, i64(n), i32(2), big_out), (own, 2, i64(n, 0), i32(1, 1), big_out), (own, 1, i64(n), i32(-1), big_out),
            (own, 3, over, i32(0, 0, 1), big_out), (own, 2, i64(128, 64), i32(1, 0), big_out),
            # two faults at once: which one is named
            (own, 2, i64(n, 0), i32(2, 1), big_out), (own, 2, i64(0, n), i32(2, 1), big_out), (own, 3, over, i32(0, 2, 1), big_out),
            (own, 3, over, i32(0, 0, 2), big_out), (own, 2, i64(n // 2, 3), i32(1, 2), big_out),
            (exn.handle, 2, i64(64, 128), i32(1, 0), big_out)]
    for i, (h, rank, e_, k_, out_) in enumerate(rows):
        say("rdm", i, lib.ctg_exec_result_rdm(h, rank, ptr(e_, i64p), ptr(k_, i32p), C.c_void_p(None if out_ is None else out_.ctypes.data)))
        say("marginal", i, lib.ctg_exec_result_marginal(h, rank, ptr(e_, i64p), ptr(k_, i32p), ptr(out_, dp)))

    # -- ctg_exec_result_topk, ctg_exec_sample_result, ctg_exec_result_stats -- #
    idx, u = np.zeros(8, np.int64), np.array([0.5])
    for i, (h, k) in enumerate([(None, 3), (own, 0), (own, n + 1), (exn.handle, 3)]):
        say("topk", i, lib.ctg_exec_result_topk(h, k, ptr(idx, i64p), None, None))
    say("topk", "null idx", lib.ctg_exec_result_topk(own, 3, None, None, None))
    for i, (h, u_, nd, idx_) in enumerate([(None, u, 1, idx), (own, u, -1, idx), (own, None, 1, idx), (own, u, 1, None),
                                           (own, np.array([1.0]), 1, idx), (own, np.array([np.nan]), 1, idx),
                                           (exn.handle, u, 1, idx), (exz.handle, u, 1, idx)]):
        say("sample", i, lib.ctg_exec_sample_result(h, ptr(u_, dp), nd, ptr(idx_, i64p), None, None))
    say("stats", "null exec", lib.ctg_exec_result_stats(None, None, None, None, None))
    assert ex.download_result().tobytes() == x.tobytes() and np.all(host == 7.0 + 7.0j) and np.all(out == 7.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not args.libs:
        return walk()
    texts = []
    for lib in args.libs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, CTG_LIB=os.path.abspath(lib)),
                           capture_output=True, text=True, timeout=300)
        if r.returncode:
            sys.exit(f"{lib}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        texts.append(r.stdout)
    for lib, t in zip(args.libs[1:], texts[1:]):
        if t != texts[0]:
            a, b = texts[0].splitlines(), t.splitlines()
            print("\n".join(f"{args.libs[0]}: {p}\n{lib}: {q}" for p, q in zip(a, b) if p != q) or f"{len(a)} and {len(b)} lines")
            sys.exit(1)
    head = f"# {len(texts[0].splitlines())} refusals, the same text from {len(args.libs)} libraries: {' '.join(os.path.basename(p) for p in args.libs)}\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(head + texts[0])
    print(head + texts[0], end="")


if __name__ == "__main__":
    main()
