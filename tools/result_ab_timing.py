#!/usr/bin/env python
"""Host time per call of the result-tensor entry points under two builds of the library, A (the parent's) and B:
the timing tools of this directory at their committed sizes, each in the order A B B A, every run a process of its
own under its own time limit; the first run that fails ends the sequence.

    python tools/result_ab_timing.py --a cotengra_amd/lib/exp/libctg_parent.so --b cotengra_amd/lib/libctg_hip.so \\
        [--tools rdm_timing ...] [--dir build/result_timing] [--out profiles/result_refactor_timing.json]
    python tools/result_ab_timing.py --assemble-only        # from the runs already in --dir

Per case of a tool the figure is the median the tool reports for the call itself: ``wall_ms`` (a host clock around the
synchronous call), else ``op_apply_ms`` / ``energy_ms``.  A case passes when both B figures lie inside the closed
interval of the two A figures -- the spread A shows against itself, which with two runs is often a fraction of a
percent; the four numbers are written whatever the verdict, with the spread B shows against itself next to A's and
the count of cases where both B runs are below / above both A runs."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ["pauli_apply_timing", "op_apply_timing", "pauli_timing", "rdm_timing", "result_reduce_timing"]
RUNS = ["A1", "B1", "B2", "A2"]
FIGURES = ["wall_ms", "op_apply_ms", "energy_ms"]
LABEL = ["what", "call", "route", "keep", "shape", "k", "data", "D", "dtype", "log2_n", "elements"]


def figure(row):
    for k in FIGURES:
        if k in row:
            return k, row[k]["median_ms"] if isinstance(row[k], dict) else row[k]
    return None, None


def assemble(d, tools):
    cases = []
    for tool in tools:
        runs = [json.load(open(os.path.join(d, f"{tool}_{r}.json"))) for r in RUNS]
        assert len({len(r) for r in runs}) == 1, tool
        for rows in zip(*runs):
            key, _ = figure(rows[0])
            if key is None:
                continue
            a1, b1, b2, a2 = (figure(r)[1] for r in rows)
            lo, hi = min(a1, a2), max(a1, a2)
            blo, bhi = min(b1, b2), max(b1, b2)
            cases.append({"tool": tool, "case": {k: rows[0][k] for k in LABEL if k in rows[0]}, "figure": key,
                          "a1_ms": a1, "b1_ms": b1, "b2_ms": b2, "a2_ms": a2, "a_spread_percent": 100.0 * (hi - lo) / lo,
                          "b_spread_percent": 100.0 * (bhi - blo) / blo, "b_below_a": bhi < lo, "b_above_a": blo > hi,
                          "b_mean_over_a_mean": (b1 + b2) / (a1 + a2), "b_within_a_spread": lo <= b1 <= hi and lo <= b2 <= hi})
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a")
    ap.add_argument("--b")
    ap.add_argument("--tools", nargs="*", default=TOOLS)
    ap.add_argument("--dir", default=os.path.join(ROOT, "build", "result_timing"))
    ap.add_argument("--limit", type=int, default=420, help="seconds per run")
    ap.add_argument("--assemble-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "result_refactor_timing.json"))
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    if not args.assemble_only:
        for tool in args.tools:
            for run in RUNS:
                lib = os.path.abspath(args.a if run[0] == "A" else args.b)
                t0 = time.time()
                with open(os.path.join(args.dir, f"{tool}_{run}.log"), "w") as log:
                    rc = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + ".py"), "--out",
                                         os.path.join(args.dir, f"{tool}_{run}.json")], env=dict(os.environ, CTG_LIB=lib),
                                        stdout=log, stderr=subprocess.STDOUT, timeout=args.limit).returncode
                print(f"{tool} {run} rc={rc} {time.time() - t0:.0f}s", flush=True)
                if rc:
                    sys.exit(f"{tool} {run} failed: nothing more is started")
    have = [t for t in TOOLS if all(os.path.exists(os.path.join(args.dir, f"{t}_{r}.json")) for r in RUNS)]
    cases = assemble(args.dir, have)
    inside = sum(c["b_within_a_spread"] for c in cases)
    ratios = sorted(c["b_mean_over_a_mean"] for c in cases)
    summary = {"tools": have, "order": "A B B A, A = the parent's library, B = this one", "cases": len(cases),
               "b_within_a_spread": inside, "b_below_both_a": sum(c["b_below_a"] for c in cases),
               "b_above_both_a": sum(c["b_above_a"] for c in cases), "b_mean_over_a_mean": {"min": ratios[0], "median": ratios[len(ratios) // 2], "max": ratios[-1]}}
    with open(args.out, "w") as f:
        json.dump({"summary": summary, "cases": cases}, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
