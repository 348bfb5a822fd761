"""Paired stores of the stem kernels (csrc/ctg_stem_impl.h: stem2h_kernel_p16), the host side: WHICH steps take them.

A consumer of a specialised-wave kernel that holds both 32-column groups of a row tile can write two adjacent columns
of a row as one 16-byte store.  Whether a step's result allows that is read off the step's own tables by the runtime
(csrc/ctg_runtime.hip: stem_pair16_ok); which launches then use it is the kernel's rule (stem_pair16_shape and the
form of the pair).  Both are restated here in Python and compared

* with the library's verdict on the very plans (``ctg_plan_stem_pair16``: host memory only, no device) -- on the cases
  of tests/stem_paired_cases.py, on every stem step of the headline plan, and on tables damaged on purpose: paired
  columns that are not adjacent, an odd column, row, tile or slice offset, an odd place in the arena;
* with what the cases say they are: paired, the 8-byte path because the tables say no, or the 8-byte path because the
  kernel family (the symmetric kernels: two items of 32 columns per wave) keeps it.
"""
import json
import os

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import runtime
from cotengra_amd.plan import KIND_STEM2, SPACE_ARENA, compile_tree

import golden_util as G
import stem_paired_cases as P
import stem_variant_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def open_model(monkeypatch):
    """Every pair the kernel can run is fused (tests/test_stem_variant_plans.py)."""
    from cotengra_amd import stem
    G.fuse_whatever_fits(monkeypatch, h2_all=True)
    monkeypatch.setattr(stem, "single_seconds", lambda *a, **k: 0.0)


def plan_of(case):
    return compile_tree(case.tree(), "complex64", fuse=True, fuse_min_elems=1 << 10, stem_bf16x3=True)


def library_says(plan, serial=None):
    """ctg_plan_stem_pair16 per step, of ``plan`` or of the damaged serialisation ``serial`` of it."""
    if serial is not None:
        class Damaged:
            inputs_elems = plan.inputs_elems
            steps = plan.steps

            def serialise(self):
                return serial
        plan = Damaged()
    dp = runtime.DevicePlan(plan)
    try:
        return dp.stem_pair16()
    finally:
        dp.close()


@pytest.mark.parametrize("case", P.CASES, ids=repr)
def test_cases_are_planned_as_they_say(case, open_model):
    plan = plan_of(case)
    stems = [(i, s) for i, s in enumerate(plan.steps) if s.kind == KIND_STEM2]
    assert [(s.stem["K1"], s.stem["N1"], s.stem["K2"], s.stem["N2"]) for _, s in stems] == case.shapes, case.id
    assert plan.nslices == 1 << case.sliced
    assert [s.stem["n_tiles"] for _, s in stems] == case.tiles
    tables = [P.tables_allow(plan, s) for _, s in stems]
    kernels = [P.kernel_pairs(s.stem) for _, s in stems]
    assert tables == case.tables_ok, (case.id, tables)
    assert [t and k for t, k in zip(tables, kernels)] == case.paired, (case.id, tables, kernels)
    # the library reads the same verdict off the same tables
    lib = library_says(plan)
    assert [lib[i] for i, _ in stems] == tables, case.id
    assert not any(v for i, v in enumerate(lib) if plan.steps[i].kind != KIND_STEM2)


def test_what_the_cases_cover():
    """The table of the issue: the three shapes of the headline's dominant kernels paired, a symmetric pair and a
    128-column pair on the 8-byte path by family, two tiles per workgroup, a sliced index, tables that say no."""
    by = {c.id: c for c in P.CASES}
    assert by["k32n32_k64n64"].paired == [True] and by["k32n64_k64n64"].paired == [True]
    assert by["k64n32_k64n64"].paired == [True]
    assert by["k32n32_k32n64_sym"].tables_ok == [True] and by["k32n32_k32n64_sym"].paired == [False]
    assert by["k32n32_k64n128_sym"].tables_ok == [True] and by["k32n32_k64n128_sym"].paired == [False]
    assert by["deep512"].tiles == [512] and by["deep512"].paired == [True]
    assert by["sliced"].sliced == 1 and by["sliced"].paired == [True]
    assert by["scattered"].tables_ok == [False] and by["scattered"].paired == [False]
    assert by["chain"].paired == [True, True]
    assert len({c.id for c in P.CASES}) == len(P.CASES)


def damaged(plan, step, what):
    """A serialisation of ``plan`` whose stem step ``step`` has one thing wrong."""
    s = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in plan.serialise().items()}
    steps = s["steps"].reshape(-1, P.STEP_WORDS)
    h = int(steps[step, P.W_STEM])
    t = s["tables"]
    tab = lambda name: int(t[h + 20 + P.TAB_ORDER.index(name)])   # noqa: E731
    N2 = int(t[h + P.SW_N2])
    if what == "swapped columns":          # (still a permutation of the same addresses: every store stays in bounds)
        oc = tab("out_col")
        t[oc + 1], t[oc + 2] = t[oc + 2], t[oc + 1]
    elif what == "pairs two apart":        # columns 2 j, 2 j + 1 <-> the even and the odd ones
        oc = tab("out_col")
        cols = t[oc:oc + N2].copy()
        t[oc:oc + N2 // 2], t[oc + N2 // 2:oc + N2] = cols[0::2], cols[1::2]
    elif what == "odd columns":            # adjacent, but the left one of every pair is odd (the last pair wraps)
        oc = tab("out_col")
        t[oc:oc + N2] = np.roll(t[oc:oc + N2], 1)
    elif what == "odd row":                # (rows 1 and 2 trade one element: still inside the result)
        orow = tab("out_row")
        t[orow + 1] += 1
        t[orow + 2] -= 1
    elif what == "odd tile":
        g = tab("gC_lo")
        assert int(t[h + P.SW_GLO]) >= 2
        t[g + 1] -= 1
    elif what == "odd place":
        assert steps[step, P.W_C_OFF] >= 2
        steps[step, P.W_C_OFF] -= 1
    elif what == "odd arena":              # (the stride of the replicas of a slice batch)
        assert steps[step, P.W_C_SPACE] == SPACE_ARENA
        s["arena_elems"] = int(s["arena_elems"]) + 1
    else:
        raise AssertionError(what)
    return s


DAMAGE = ("swapped columns", "pairs two apart", "odd columns", "odd row", "odd tile", "odd place", "odd arena")


@pytest.mark.parametrize("what", DAMAGE)
def test_damaged_tables_do_not_qualify(what, open_model):
    """Tables arrive through the C ABI and are not trusted: the library's verdict is read off them.  Each damage keeps
    every address inside the result (the plan still validates) and must turn the verdict to no -- in the library and
    in the rule restated here."""
    case = P.by_id("k32n32_k64n64_tail")
    plan = plan_of(case)
    (step,) = [i for i, s in enumerate(plan.steps) if s.kind == KIND_STEM2]
    assert library_says(plan)[step] and P.tables_allow(plan, plan.steps[step])
    s = damaged(plan, step, what)
    assert not P.serial_allows(s, step), what
    assert not library_says(plan, s)[step], what
    # (and nothing else changed its mind)
    assert sum(library_says(plan, s)) == 0


def test_headline_plan(monkeypatch):
    """The flagship plan (bench.py: sycamore_m20_native): every stem step's result is laid out [rows][N2] with even
    offsets -- the tables allow pairs on all of them -- and the launches that pair are the specialised-wave kernels with
    one row tile's two column groups per consumer: the k64 n64 second steps.  The symmetric pairs (two items per wave)
    and the single steps keep 8-byte stores."""
    for k in G.ARITH_ENV:
        monkeypatch.delenv(k, raising=False)
    tree = ca.tree_from_record(ca.load_network(os.path.join(ROOT, "tests", "golden", "trees", "sycamore_m20_native.json")))
    plan = compile_tree(tree, "complex64")
    stems = [(i, s) for i, s in enumerate(plan.steps) if s.kind == KIND_STEM2]
    pairs = [(i, s) for i, s in stems if not s.stem.get("one")]
    assert len(stems) == 24
    for i, s in pairs:
        assert P.tables_allow(plan, s), i
    lib = library_says(plan)
    assert [lib[i] for i, s in pairs] == [True] * len(pairs)
    assert not any(lib[i] for i, s in stems if s.stem.get("one"))
    paired = [(s.stem["K1"], s.stem["N1"], s.stem["K2"], s.stem["N2"]) for i, s in pairs if P.kernel_pairs(s.stem)]
    print("paired:", json.dumps(paired))
    assert sorted(set(paired)) == [(32, 32, 64, 64), (32, 64, 64, 64), (64, 32, 64, 64)]
    assert all(k2 == 64 and n2 == 64 for _, _, k2, n2 in paired)
