"""The plans the device tests of the single-term kernels rely on, checked without a device.  Every row of
tests/single_variant_cases.py (run by tests/test_gpu_single_variants.py) must compile to exactly one single-term
step of the recorded shape, on the side of ``K >= 256 and R <= 2^14`` its kernel stands for; the plan, run through
the numpy plan interpreter, must equal ``numpy.einsum``; and the table must keep every edge it was written for.

The interpreter shares the plan with the device and nothing of the kernels: what a wrong lane stride or a dropped
``kA.hi`` in a kernel would break is decided here only in so far as the table holds a row on which it shows (K not a
multiple of 64; k_hi_len > 1 with non-zero hi offsets), which the property tests below pin.

The gradient of a one-input tree (cotengra_amd/vjp.py, the ``N == 1`` branch: the cotangent spread over the summed
indices, or put on a diagonal, by one accumulate step) is run for every row against torch autograd."""
import numpy as np
import pytest

from cotengra_amd.plan import KIND_ACCUM, KIND_PAIR, KIND_SINGLE, compile_tree
from cotengra_amd.vjp import compile_vjp
from oracle.plan_interp import run_plan

import golden_util as G
import single_variant_cases as V
import vjp_util as U

HI = {"float32": "float64", "float64": "float64", "complex64": "complex128", "complex128": "complex128"}


def single_steps(plan):
    return [s for s in plan.steps if s.kind == KIND_SINGLE]


def shape_of(s):
    return (s.R, s.K, s.k_lo, len(s.k_tabs["A"][0]))


def routed_to(s):
    return V.WAVE if s.K >= V.WAVE_MIN_K and s.R <= V.WAVE_MAX_R else V.THREAD


def test_rows_have_one_id_each():
    ids = [c.id for c in V.ALL_CASES + [V.LEAF_CASE]]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("dtype", V.ALL_DTYPES)
@pytest.mark.parametrize("case", V.ALL_CASES, ids=repr)
def test_table_rows_are_one_single_step(case, dtype):
    plan = compile_tree(case.tree(), dtype)
    assert plan.nslices == case.nslices
    steps = single_steps(plan)
    assert len(steps) == 1 and not [s for s in plan.steps if s.kind == KIND_PAIR], plan.steps
    s = steps[0]
    assert shape_of(s) == case.step
    assert s.K == s.k_lo * len(s.k_tabs["A"][0]) and len(s.k_tabs["A"][1]) == s.k_lo
    assert routed_to(s) == case.kernel
    if case.row is not None:
        assert (s.row_lo, len(s.rows["A"][0])) == case.row
    assert s.lds_comp < 0   # (the step launches on its own kernel, not inside an LDS-resident subtree)


@pytest.mark.parametrize("dtype", V.ALL_DTYPES)
def test_leaf_preprocessing_row(dtype):
    """``aab,bc->c``: the single-term step of the first leaf takes the wave form inside a two-input tree."""
    case = V.LEAF_CASE
    plan = compile_tree(case.tree(), dtype)
    steps = single_steps(plan)
    assert len(steps) == 1 and len([s for s in plan.steps if s.kind == KIND_PAIR]) == 1
    assert shape_of(steps[0]) == case.step and routed_to(steps[0]) == case.kernel == V.WAVE
    assert steps[0].lds_comp < 0


@pytest.mark.parametrize("case", V.ALL_CASES + [V.LEAF_CASE], ids=repr)
def test_plan_equals_einsum(case):
    for dtype in ("complex128", "float64"):
        arrays = case.arrays(dtype)
        tree = case.tree()
        got = np.asarray(run_plan(compile_tree(tree, dtype), arrays)).reshape(tree.gathered_shape())
        ref = np.einsum(case.eq, *arrays, optimize=True)
        assert G.relerr(got, ref) <= 1e-12, (case.id, dtype)


def _step(case):
    return single_steps(compile_tree(case.tree(), "complex128"))[0]


def test_table_reaches_both_kernels_and_every_edge():
    """Properties of the table itself: a later edit cannot thin it without notice."""
    rows = [(c, _step(c)) for c in V.ALL_CASES]
    wave = [(c, s) for c, s in rows if c.kernel == V.WAVE]
    thread = [(c, s) for c, s in rows if c.kernel == V.THREAD]
    assert wave and thread and {c.kernel for c in V.ALL_CASES} == {V.WAVE, V.THREAD}
    pow2 = lambda n: n & (n - 1) == 0  # noqa: E731
    khl = lambda s: len(s.k_tabs["A"][0])  # noqa: E731
    # the wave form: a lane tail, both forms of split_k under a two-level table with non-zero hi offsets
    assert any(s.K % 64 for _, s in wave)
    assert any(khl(s) > 1 and not pow2(s.k_lo) and np.any(s.k_tabs["A"][0] != 0) for _, s in wave)
    assert any(khl(s) > 1 and pow2(s.k_lo) and np.any(s.k_tabs["A"][0] != 0) for _, s in wave)
    assert any(khl(s) == 1 and not pow2(s.k_lo) for _, s in wave)
    # both sides of either threshold, each one step apart
    ks = lambda sel: {s.K for _, s in sel}  # noqa: E731
    assert 256 in ks(wave) and 257 in ks(wave) and 255 in ks(thread)
    assert any(s.R == 1 << 14 and s.K == 256 for _, s in wave)
    assert any(s.R == (1 << 14) + 1 and s.K == 256 for _, s in thread)
    assert any(s.K > 256 and s.R > 1 << 14 for _, s in thread)
    assert any(s.R == 1 and s.K == 1 << 20 for _, s in wave)
    # summed indices that are not the fastest in memory
    assert any(min(abs(int(x)) for x in np.diff(s.k_tabs["A"][1])) > 1 and s.R > 1 for _, s in wave)
    # row tables of two levels, row_lo no power of two; a scattered output
    assert any(len(s.rows["C"][0]) > 1 and not pow2(s.row_lo) for _, s in thread)
    assert any(s.K == 1 and np.any(np.diff(s.rows["A"][1]) != 1) for _, s in thread)
    # sliced launches on either kernel: a summed index, an output index, both, and one under a diagonal
    for kernel in (V.WAVE, V.THREAD):
        sl = [c for c in V.SLICED_CASES if c.kernel == kernel]
        assert any(set(c.sliced) and not set(c.sliced) & set(c.out) for c in sl)
        assert any(set(c.sliced) and set(c.sliced) <= set(c.out) for c in sl)
        assert any(set(c.sliced) & set(c.out) and set(c.sliced) - set(c.out) for c in sl)
        assert any(c.sliced and len(set(c.terms[0])) < len(c.terms[0]) for c in sl)
    # every operand stays small (the largest row the table was asked to hold is 20000 x 255)
    assert max(c.elems for c in V.ALL_CASES) <= 20000 * 255


def test_serial_fold_of_the_long_thread_rows_stays_inside_the_single_gate():
    """single_kernel adds the K >= 256 of rows T2 and T9 serially in the type.  The device test's single-precision
    gate is numpy's own error times eight (or 1e-5): a serial float32 fold of the same data must lie inside it, so
    that gate cannot fail because of the fold order alone."""
    for ident in ("T2", "T9"):
        case = V.by_id(ident)
        for dtype in ("float32", "complex64"):
            (x,) = case.arrays(dtype)
            ref = np.einsum(case.eq, x.astype(HI[dtype]))
            gate = G.single_gate(ref, np.einsum(case.eq, x))
            fold = np.add.accumulate(x, axis=1, dtype=x.dtype)[:, -1]
            assert fold.dtype == x.dtype
            assert G.relerr(fold, ref) <= gate, (ident, dtype, G.relerr(fold, ref), gate)


def test_the_two_slicing_orders_differ_in_what_consecutive_slices_share():
    """What tests/test_gpu_slice_sum.py relies on for ``stab->tb`` with s (summed) and t (kept) sliced: the tree keeps
    its sliced indices sorted, kept ones before summed ones, whatever the order of slicing -- so consecutive slice ids
    share their result elements in runs of five in BOTH orders (t changes twice over the 15 slices), and slices that
    alternate between result elements have to be asked for by a list of ids (``t_fast_ids``: t changes at every
    slice, and every result element still meets its five slices in rising s)."""
    import cotengra_amd as ca
    t_fast_ids = V.t_fast_ids

    keys = []
    for order in ("st", "ts"):
        tree = ca.ContractionTree.from_path(["stab"], "tb", dict(s=5, t=3, a=7, b=11), path=[])
        for ix in order:
            tree.remove_ind_(ix)
        keys.append([tree.slice_key(i) for i in range(tree.nslices)])
        ts = [k["t"] for k in keys[-1]]
        assert sum(1 for a, b in zip(ts, ts[1:]) if a != b) == 2
    assert keys[0] == keys[1]
    ids = t_fast_ids(5, 3)
    assert sorted(ids) == list(range(15))
    ts = [keys[0][i]["t"] for i in ids]
    assert all(a != b for a, b in zip(ts, ts[1:]))
    for t in range(3):
        assert [keys[0][i]["s"] for i in ids if keys[0][i]["t"] == t] == list(range(5))


@pytest.mark.parametrize("case", V.ALL_CASES + [V.LEAF_CASE], ids=repr)
def test_vjp_plan_matches_autograd(case):
    """The gradient of a one-input tree: one accumulate step per leaf, against torch autograd."""
    tree = case.tree()
    arrays = case.arrays("complex128")
    h = U.cotangent(tree, "complex128")
    plan = compile_vjp(tree, "complex128")
    assert sum(s.kind == KIND_ACCUM for s in plan.steps) == tree.N
    got = U.split_grads(plan, run_plan(plan, list(arrays) + [h]), [a.shape for a in arrays])
    ref = U.reference_vjp(tree, arrays, h)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert G.relerr(g, r) <= 1e-10, (case.id, i)
    if len(set(case.terms[0])) < len(case.terms[0]) and tree.N == 1:
        # a diagonal: nothing off it
        mask = np.ones(arrays[0].shape, bool)
        np.einsum(case.eq.split("->")[0] + "->" + "".join(dict.fromkeys(case.terms[0])), mask)[...] = False
        assert np.all(got[0][mask] == 0)
