"""The plans the device tests of the pair-kernel variants rely on, checked without a device.  Every row of the
tables in tests/pair_variant_cases.py (run by tests/test_gpu_pair_variants.py) and tests/pair_variant_cases_c64.py
(run by tests/test_gpu_pair_variants_c64.py) must reach the planner's matrix-core route (or, the long
contractions, the VALU route with lanes along k) with the step shape its table records.  A case that drifts off
its kernel -- as the float32 / float64 cases of tests/test_gpu_round3.py once did when the planner's threshold
moved -- fails here."""
import pytest

from cotengra_amd.plan import KERNEL_MFMA, KERNEL_VALU, KIND_PAIR, compile_tree

import pair_variant_cases as V
import pair_variant_cases_c64 as C


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


# ---- complex64 (tests/pair_variant_cases_c64.py): the variant is asserted on the device, by name ------------------ #

def c64_step(case, nslices=1):
    plan = compile_tree(case.tree(sliced=case.sliced), "complex64")
    assert plan.nslices == nslices
    steps = [s for s in plan.steps if s.kind == KIND_PAIR]
    assert len(steps) == 1 and steps[0].kernel == KERNEL_MFMA, steps
    return (steps[0].R, steps[0].Bt, steps[0].K, steps[0].N)


def test_c64_rows_have_one_id_each():
    ids = [c.id for c in C.ALL_CASES]
    assert len(set(ids)) == len(ids)
    for ident in C.STRIP_IDS + C.SLICE_BATCH_IDS + C.SPLIT_K_IDS:
        assert C.by_id(ident).id == ident


@pytest.mark.parametrize("case", C.ALL_CASES, ids=repr)
def test_c64_rows_are_one_matrix_core_step(case):
    nslices = 1
    for ix in case.sliced:
        nslices *= case.sizes[ix]
    assert c64_step(case, nslices) == case.step


def test_c64_streaming_rows_name_thirty_instantiations():
    """The table's own bookkeeping: thirty different streaming instantiations, none of them one of the six that no
    step can reach; all nine skinny and all twelve row-wise ones."""
    stream = {c.args for c in C.STREAM_CASES}
    assert len(stream) == 30 and not stream & set(C.STREAM_UNREACHABLE)
    assert {c.args for c in C.DEEP_CASES} <= stream
    assert len({c.args for c in C.SKINNY_CASES}) == 9 == len(C.SKINNY_CASES)
    assert len({c.args for c in C.ROWWISE_CASES}) == 12 == len(C.ROWWISE_CASES)
    assert len({c.args for c in C.KSTREAM_CASES}) == 4


@pytest.mark.parametrize("ident", C.SLICE_BATCH_IDS)
def test_c64_rows_with_the_row_index_sliced(ident):
    case = C.sliced_rows(C.by_id(ident))
    assert c64_step(case, 4) == case.step == C.by_id(ident).step


@pytest.mark.parametrize("fast", [False, True], ids=["slow", "fast"])
@pytest.mark.parametrize("ident", C.SPLIT_K_IDS)
def test_c64_rows_with_part_of_the_contraction_sliced(ident, fast):
    base = C.by_id(ident)
    cut = C.split_contracted(base, fast)
    cut = base.like(cut.id, cut.eq, cut.sizes, cut.step, sliced=("s",))
    R, Bt, K, N = base.step
    assert c64_step(cut, 2) == cut.step == (R, Bt, K // 2, N)
