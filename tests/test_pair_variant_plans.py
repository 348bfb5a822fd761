"""The plans tests/test_gpu_pair_variants.py relies on, checked without a device: every row of its tables must
reach the planner's matrix-core route (or, the long contractions, the VALU route with lanes along k) with the
step shape the table records.  A case that drifts off its kernel -- as the float32 / float64 cases of
tests/test_gpu_round3.py once did when the planner's threshold moved -- fails here."""
import pytest

from cotengra_amd.plan import KERNEL_MFMA, KERNEL_VALU, KIND_PAIR, compile_tree

import pair_variant_cases as V


def pair_steps(tree, dtype):
    return [s for s in compile_tree(tree, dtype).steps if s.kind == KIND_PAIR]


def the_pair_step(tree, dtype):
    steps = pair_steps(tree, dtype)
    assert len(steps) == 1, steps
    return steps[0]


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("case", V.TILE_CASES + V.GATHER_CASES, ids=repr)
def test_table_rows_are_one_matrix_core_step(case, dtype):
    s = the_pair_step(case.tree(), dtype)
    assert s.kernel == KERNEL_MFMA
    assert (s.R, s.Bt, s.K, s.N) == case.step
    assert case.tiles is not None and set(case.tiles) == set(V.DTYPES)


@pytest.mark.parametrize("fast", [False, True], ids=["slow", "fast"])
@pytest.mark.parametrize("dtype", ("float32", "float64"))
@pytest.mark.parametrize("case", V.GATHER_CASES, ids=repr)
def test_gather_rows_with_part_of_the_contraction_sliced(case, dtype, fast):
    """The contracted index split and one part sliced, as the device test does: still one matrix-core step, the
    contraction shorter by the sliced extent.  (Slicing the whole index would leave K = 1, an outer product on
    the VALU kernel, and the slice strides would never reach the check of the 16-byte gathers.)"""
    cut = V.split_contracted(case, fast)
    plan = compile_tree(cut.tree(sliced=("s",)), dtype)
    assert plan.nslices == cut.sizes["s"] >= 2
    steps = [s for s in plan.steps if s.kind == KIND_PAIR]
    assert len(steps) == 1 and steps[0].kernel == KERNEL_MFMA
    assert (steps[0].R, steps[0].Bt, steps[0].K, steps[0].N) == cut.step


@pytest.mark.parametrize("ident,dtype", [(i, d) for i, per in V.SLICED_ROWS.items() for d in per])
def test_sliced_tall_rows(ident, dtype):
    case = V.sliced_case(ident, dtype)
    plan = compile_tree(case.tree(sliced=("s",)), dtype)
    assert plan.nslices == 4
    steps = [s for s in plan.steps if s.kind == KIND_PAIR]
    assert len(steps) == 1 and steps[0].kernel == KERNEL_MFMA
    assert (steps[0].R, steps[0].Bt, steps[0].K, steps[0].N) == case.step


def _pairwise_case(index):
    import test_gpu_pairwise as TP

    eq, sizes = TP.CASES[index]
    return V.Case(f"pairwise{index}", eq, sizes, (0, 0, 0, 0))


@pytest.mark.parametrize("dtype", V.ALL_DTYPES)
@pytest.mark.parametrize("row", V.KRED_PAIRWISE, ids=lambda r: r[1])
def test_long_contractions_of_test_pairwise(row, dtype):
    index, eq, _, _ = row
    case = _pairwise_case(index)
    assert case.eq == eq
    s = the_pair_step(case.tree(), dtype)
    assert s.kernel == KERNEL_VALU and s.K >= 256 and s.R * s.N <= 1 << 15


@pytest.mark.parametrize("dtype", V.ALL_DTYPES)
@pytest.mark.parametrize("row", V.THREAD_PAIRWISE, ids=lambda r: r[1])
def test_short_contractions_of_test_pairwise(row, dtype):
    index, eq = row
    case = _pairwise_case(index)
    assert case.eq == eq
    s = the_pair_step(case.tree(), dtype)
    assert s.kernel == KERNEL_VALU and s.K < 256


@pytest.mark.parametrize("dtype", V.ALL_DTYPES)
@pytest.mark.parametrize("row", V.FINISH_CASES, ids=lambda r: r[0].id)
def test_finish_pass_shapes(row, dtype):
    case = row[0]
    s = the_pair_step(case.tree(), dtype)
    assert s.kernel == KERNEL_VALU and s.K >= 256 and s.R * s.N <= 1 << 15
    assert (s.R, s.Bt, s.K, s.N) == case.step
