"""Host side of the LDS step-form audit (tests/lds_variant_cases.py): the planner gives every row the components and
the shadow records its table writes down, in all four types; the numpy interpretation of the shadow lowering
(oracle/plan_interp.py) equals the ordinary steps and numpy's einsum in double precision; the integer operands of
the bit-for-bit GPU check keep every partial sum below 2^24; every form the kernel has is in the table, by a row
or as unreachable, and the reasons given for the unreachable ones hold against the planner's constants.  No GPU."""
import numpy as np
import pytest

import golden_util as G
import lds_variant_cases as V
from cotengra_amd import ldsrun as L, plan as P
from oracle import plan_interp as PI

WIDE = {"complex64": "complex128", "complex128": "complex128", "float32": "float64", "float64": "float64"}


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("row", V.ALL_ROWS, ids=repr)
def test_planner_gives_the_recorded_components(row, dtype):
    plan = P.compile_tree(row.tree(), dtype)
    assert plan.nslices == int(np.prod([row.sizes[ix] for ix in row.sliced], dtype=np.int64))
    assert len(plan.lds_runs) == len(row.recs), [len(r["steps"]) for r in plan.lds_runs]
    for run, recs, names in zip(plan.lds_runs, row.shapes(), row.forms(dtype)):
        assert run["cls"] == "slice" and len(run["steps"]) == len(recs)
        for sh, want, name in zip(run["steps"], recs, names):
            s, form = sh["step"], G.lds_form(name)
            assert sh["kind"] == (L.KIND_LOAD if form["kernel"] == "load" else L.KIND_LPAIR), (row, name)
            assert (s.R, s.K, s.N, s.row_lo, sh["phase"]) == want, (row, name, (s.R, s.K, s.N, s.row_lo, sh["phase"]))
            # (one high entry: UNREACHABLE["ROW_HI"]); the division the name states is the one row_lo asks for
            assert all(len(hi) == 1 for hi, _ in s.rows.values())
            assert form["magic"] == bool(s.row_lo & (s.row_lo - 1)), (row, name)
            # a load of K = 1 is the plain gather; the columns per lane of a VALU pair follow N
            if form["kernel"] == "load":
                assert (form["arg"] == "gather") == (s.K == 1)
            elif form["kernel"] == "pair":
                assert form["arg"] == (4 if s.N >= 3 else s.N)
            else:
                assert dtype == "complex64" and s.N >= 8 and s.R >= 16
    # the last pair record of a component is its root (the global store), every other one stays in LDS
    for run in plan.lds_runs:
        pairs = [sh for sh in run["steps"] if sh["kind"] == L.KIND_LPAIR]
        assert [sh["global_operand"] for sh in pairs] == [-1] * (len(pairs) - 1) + [2]


@pytest.mark.parametrize("dtype", ["complex128", "float64"])
@pytest.mark.parametrize("row", V.ALL_ROWS, ids=repr)
def test_shadow_lowering_equals_the_ordinary_steps_and_einsum(row, dtype):
    plan = P.compile_tree(row.tree(), dtype)
    arrays = row.arrays(dtype)
    a = PI.run_plan(plan, arrays, lds=False)
    b = PI.run_plan(plan, arrays, lds=True)
    assert np.array_equal(a, b) or np.allclose(a, b, rtol=1e-13, atol=0)
    ref = np.einsum(row.eq, *arrays, optimize=True)
    assert G.relerr(b, ref) <= 1e-12, G.relerr(b, ref)


@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "real"])
@pytest.mark.parametrize("row", V.ALL_ROWS, ids=repr)
def test_integer_operands_stay_exact_in_single_precision(row, cplx):
    """Whole numbers from [-3, 3]: the int64 reference, the bound on every partial sum below 2^24 (so float32 adds
    them without rounding, in any order), numpy's einsum in double precision equal to the int64 result, and the
    interpreter of the shadow lowering -- in SINGLE precision -- equal to it bit for bit."""
    ref, bound = V.int_reference(row, cplx)
    print(f"BOUND {row.id} {'complex' if cplx else 'real'} {bound}")
    assert bound < 2 ** 24, bound
    wide = "complex128" if cplx else "float64"
    arrays = row.arrays(wide, integer=True)
    for x in arrays:
        assert np.array_equal(x.real, np.rint(x.real)) and np.abs(x.real).max() <= 3
    assert np.array_equal(np.einsum(row.eq, *arrays, optimize=True), ref)
    single = "complex64" if cplx else "float32"
    got = PI.run_plan(P.compile_tree(row.tree(), single), row.arrays(single, integer=True), lds=True)
    assert got.dtype == np.dtype(single) and np.array_equal(got, ref.astype(single))


# Every form section 2 of the audit lists: what a record's name and shape must say, and the least number of rows.
def _records(dtype):
    for row in V.ALL_ROWS:
        for comp, names in zip(row.recs, row.forms(dtype)):
            pairs = [i for i, (f, _, _) in enumerate(comp) if not f.startswith("load")]
            for i, ((_, _, shape), name) in enumerate(zip(comp, names)):
                yield row, G.lds_form(name), shape, (bool(pairs) and i == pairs[-1])


def _has(dtype, **want):
    """Rows with a record whose parsed name (and ``R``, ``K``, ``N``, ``root``) satisfies every ``want``."""
    hits = []
    for row, form, (R, K, N, _, _), root in _records(dtype):
        have = dict(form, R=R, K=K, N=N, root=root)
        if all(v(have[k]) if callable(v) else have[k] == v for k, v in want.items()):
            hits.append(row.id)
    return hits


def test_every_listed_form_has_a_row():
    c64 = "complex64"
    for lanes in ("rows", "cols"):
        for magic in (False, True):
            assert _has(c64, kernel="pair_mfma", arg=lanes, magic=magic), (lanes, magic)
        assert _has(c64, kernel="pair_mfma", arg=lanes, root=True) and _has(c64, kernel="pair_mfma", arg=lanes, root=False)
        assert _has(c64, kernel="pair_mfma", arg=lanes, wave=-1) and _has(c64, kernel="pair_mfma", arg=lanes, wave=0)
    # the three k loops in sequence (K >= 21, K % 4 != 0), K < 4, K = 16 exactly, the loop of four alone
    assert _has(c64, kernel="pair_mfma", arg="rows", K=lambda k: k >= 21 and k % 4)
    assert _has(c64, kernel="pair_mfma", arg="cols", K=lambda k: k >= 21 and k % 4)
    assert _has(c64, kernel="pair_mfma", K=lambda k: k < 4) and _has(c64, kernel="pair_mfma", K=16)
    assert _has(c64, kernel="pair_mfma", K=lambda k: k in (4, 8, 12))
    # ragged tiles in both axes; more tiles than waves; a start rotation; one clamped tile dealt to a wave
    assert _has(c64, kernel="pair_mfma", R=lambda r: r % 32, N=lambda n: n % 16)
    assert any(-(-R // 32) * -(-N // 16) > 16 for _, f, (R, K, N, _, _), _ in _records(c64)
               if f["kernel"] == "pair_mfma" and f["wave"] < 0)
    assert _has(c64, kernel="pair_mfma", rot=lambda r: r is not None and r > 0)
    assert _has(c64, kernel="pair_mfma", wave=0, R=lambda r: 16 <= r < 32, N=8)
    # matrix-core records are VALU records in the other three types
    for dtype in V.DTYPES[1:]:
        assert not _has(dtype, kernel="pair_mfma")
    for dtype in V.DTYPES:
        for tn in (1, 2, 4):
            for magic in (False, True):
                assert _has(dtype, kernel="pair", arg=tn, magic=magic), (tn, magic)
            assert _has(dtype, kernel="pair", arg=tn, wave=-1) and _has(dtype, kernel="pair", arg=tn, wave=lambda w: w >= 0)
            assert _has(dtype, kernel="pair", arg=tn, root=True, wave=-1) and _has(dtype, kernel="pair", arg=tn, root=False)
            assert _has(dtype, kernel="pair", arg=tn, root=True, wave=lambda w: w >= 0)
            assert _has(dtype, kernel="pair", arg=tn, K=lambda k: k < 4), tn
            assert _has(dtype, kernel="pair", arg=tn, K=lambda k: k >= 4 and k % 4 == 0), tn
            assert _has(dtype, kernel="pair", arg=tn, K=lambda k: k > 4 and k % 4), tn
        for n in (3, 5, 7, 21):
            assert _has(dtype, kernel="pair", arg=4, N=n), n
        for arg in ("gather", "sum"):
            for magic in (False, True):
                assert _has(dtype, kernel="load", arg=arg, magic=magic), (arg, magic)
        # a gather whose last round of 4 x 64 outputs is partial, and one of whole rounds
        assert _has(dtype, kernel="load", arg="gather", R=lambda r: r % 256) and _has(dtype, kernel="load", arg="gather", R=lambda r: r % 256 == 0)
        assert _has(dtype, kernel="load", arg="sum", K=lambda k: k > 256)
        assert not _has(dtype, kernel="load", wave=-1)        # UNREACHABLE["LOAD_SHARED"]
    marks = {m for r in V.ALL_ROWS for m in r.marks}
    assert {"batch", "sliced", "load sum trace", "load sum index", "group-shared operand"} <= marks
    batch = [r for r in V.ALL_ROWS if "batch" in r.marks]
    assert all(all(r.out[0] in t for t in r.terms) for r in batch)


def test_a_component_gathers_what_its_slice_group_shares():
    """G_shared: g is a group index, the first step does not carry it and is shared by the three slices of a group; the
    per-slice component gathers that step's result from the arena like a leaf (on the device: LdsStepDev.gzq = 3 in a
    batched launch, the operand lives with the first slice of its group)."""
    row = V.by_id("G_shared")
    for dtype in V.DTYPES:
        plan = P.compile_tree(row.tree(), dtype)
        assert plan.group_inds == ("g",) and plan.group_size == 3 and plan.nslices == 6
        shared = [s for s in plan.steps if s.kind == P.KIND_PAIR and s.group]
        assert len(shared) == 1 and shared[0].lds_comp < 0 and not shared[0].invariant
        (run,) = plan.lds_runs
        loads = [sh for sh in run["steps"] if sh["kind"] == L.KIND_LOAD]
        reads = [(plan.steps[sh["main"]].a, plan.steps[sh["main"]].b)[sh["global_operand"]] for sh in loads]
        assert sum(r is shared[0].c for r in reads) == 1


def test_the_unreachable_forms_are_unreachable():
    """The reasons of lds_variant_cases.UNREACHABLE against the planner's constants, and two trees just under and
    over the limit."""
    assert set(V.UNREACHABLE) == {"LOAD_SHARED", "ROW_HI", "MAGIC_R_65536"}
    members = 1
    budget_words = (L.LDS_TABLE_BYTES - members * 3 * 128) // 4
    assert 2 * 4096 > budget_words                        # a load the packer would share: more than 4096 outputs
    assert L._table_words(P.LO_MAX + 1, 1, 1) > budget_words and 3 * P.LO_MAX > budget_words   # two-level rows
    assert L.MAX_EXTERNAL_ELEMS <= 8192 < 65536
    for a, found in ((50, True), (63, False)):
        row = V.Row("limit", "ab,bc,cd,de->ae", dict(a=a, b=65, c=2, d=3, e=4), V.CHAIN, [])
        plan = P.compile_tree(row.tree(), "float32")
        assert bool(plan.lds_runs) is found, a
        for run in plan.lds_runs:
            assert all(sh["step"].R <= P.LO_MAX for sh in run["steps"])


def test_the_equal_bits_clause_is_not_lost():
    """The GPU suite compares a component's bits with its steps launched one by one where those run on the
    thread-per-output kernels with K < 256 -- a condition on what the step path runs.  In every row but the two named
    here every member has K < 256, so the clause can only fall away through the kernel the step path names, which the
    suite prints (SAME_ORDER)."""
    long_k = {"L_sum", "L_sum_p2"}   # (a leaf's sum over 300: single_kernel adds in another order from K = 256 on)
    for row in V.ALL_ROWS:
        plan = P.compile_tree(row.tree(), "complex64")
        members = [s for s in plan.steps if s.lds_comp >= 0]
        assert members and (all(s.K < 256 for s in members) != (row.id in long_k)), row


@pytest.mark.parametrize("magic", [False, True], ids=["shift", "magic"])
@pytest.mark.parametrize("ident", V.RECUT_IDS)
def test_recut_rows_are_the_same_rows_and_the_c_abi_takes_them(ident, magic):
    """Two-level rows (lds_variant_cases.recut_rows): every re-cut record addresses what it addressed before, the
    C ABI accepts the plan, and over the rows of RECUT_IDS loads, VALU pairs and matrix-core pairs are all re-cut in
    both kinds."""
    from cotengra_amd import runtime

    row = V.by_id(ident)
    plan = P.compile_tree(row.tree(), "complex64")
    recut, cuts = V.recut_rows(plan, magic)
    old, new = plan.serialise()["tables"], recut.serialise()["tables"]
    # (the new tables stand behind the old ones, which stay)
    assert np.array_equal(new[: 8], old[: 8]) and (len(new) > len(old)) == any(
        d < R for ds, sh in zip(cuts, row.shapes()) for d, (R, *_) in zip(ds, sh))
    H, W = L.LR_HEAD_WORDS, L.LR_WORDS
    steps = recut.serialise()["steps"].reshape(-1, P.STEP_WORDS)
    descs = sorted({int(s[P.W_LDS_DESC]) for s in steps if s[P.W_LDS_COMP] > 0})
    for d0, comp_cuts, shapes in zip(descs, cuts, row.shapes()):
        for i, (d, (R, _, _, _, _)) in enumerate(zip(comp_cuts, shapes)):
            q, q0 = new[d0 + H + i * W: d0 + H + (i + 1) * W], old[d0 + H + i * W: d0 + H + (i + 1) * W]
            assert q[10] == R and q[13] == d and q[13] * q[14] == R and (d == R or bool(d & (d - 1)) == magic)
            for w_hi, w_lo in ((17, 18), (19, 20), (21, 22)):
                if q[w_lo] < 0:
                    continue
                was = old[q0[w_hi]] + old[q0[w_lo]: q0[w_lo] + R]
                now = (new[q[w_hi]: q[w_hi] + R // d][:, None] + new[q[w_lo]: q[w_lo] + d][None, :]).reshape(-1)
                assert np.array_equal(was, now)
    runtime.DevicePlan(recut).close()


def test_recut_rows_reach_every_kind_of_record():
    seen = set()
    for ident in V.RECUT_IDS:
        row = V.by_id(ident)
        for magic in (False, True):
            _, cuts = V.recut_rows(P.compile_tree(row.tree(), "complex64"), magic)
            for comp_cuts, names, shapes in zip(cuts, row.forms("complex64"), row.shapes()):
                for d, name, shape in zip(comp_cuts, names, shapes):
                    if d < shape[0]:
                        f = G.lds_form(name)
                        seen.add((f["kernel"], f["arg"], magic))
    for magic in (False, True):
        assert {("load", "gather", magic), ("load", "sum", magic), ("pair", 1, magic), ("pair", 2, magic),
                ("pair", 4, magic), ("pair_mfma", "rows", magic), ("pair_mfma", "cols", magic)} <= seen, seen


def test_form_names_parse():
    assert G.lds_form("load<gather> wave=3 shift") == dict(kernel="load", arg="gather", wave=3, rot=None, magic=False)
    assert G.lds_form("pair<4> all magic") == dict(kernel="pair", arg=4, wave=-1, rot=None, magic=True)
    assert G.lds_form("pair_mfma<rows> all rot=5 shift") == dict(kernel="pair_mfma", arg="rows", wave=-1, rot=5, magic=False)
    assert G.lds_form("pair_mfma<cols> wave=0 magic")["wave"] == 0
    for bad in ("pair<3> all shift", "load<gather> all rot=1 shift", "pair_mfma<rows> all shift", "pair<4> wave=16 magic"):
        with pytest.raises(AssertionError):
            G.lds_form(bad)
    for row in V.ALL_ROWS:
        for dtype in V.DTYPES:
            for names in row.forms(dtype):
                for n in names:
                    G.lds_form(n)


def test_the_binding_declares_the_symbol():
    import os

    from cotengra_amd import runtime

    header = open(os.path.join(os.path.dirname(G.HERE), "include", "ctg_hip.h")).read()
    assert ("int ctg_exec_lds_form(ctg_exec* exec, int64_t comp, int64_t rec, int64_t* main_step, char* buf, "
            "int64_t buflen);") in header
    assert "#define CTG_ABI_VERSION 10" in header
    assert "ctg_exec_lds_form" in runtime.SYMBOLS and hasattr(runtime.load(), "ctg_exec_lds_form")
