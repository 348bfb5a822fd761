"""GPU suite: every variant of the pair kernels in float32, float64 and complex128 -- the tiles of the matrix-core
kernels (csrc/ctg_pair_mfma_f64.hip), their 16-byte gathers, launches of several slices on the large tiles, and
the long-contraction kernels with both forms of their finish pass (csrc/ctg_kernels_valu.hip).

Every case first asserts the kernel the executor names for its step (tests/golden_util.py: pair_flags) and then
compares the result element-wise with ``numpy.einsum`` in float64 / complex128: 1e-12 of the largest element for
the double types, ``G.single_gate`` against numpy's own single-precision einsum for the others.  One wrong element,
one dropped k or one transposed accumulator register is an error of order 1 against these gates.  The tables are in
tests/pair_variant_cases.py; tests/test_pair_variant_plans.py pins their plans on the host."""
import numpy as np
import pytest

import golden_util as G
import pair_variant_cases as V
from cotengra_amd.contractor import HipContractor

pytestmark = pytest.mark.gpu

MFMA_KERNEL = {"complex128": ("pair_mfma_c128_kernel", "c128"), "float32": ("pair_mfma_real_kernel", "float"),
               "float64": ("pair_mfma_real_kernel", "double")}

_DATA = {}


def data(case, dtype):
    """``(operands, reference, gate)`` of a case: computed once, shared by the tests that follow one another on the
    same case (the last two are kept: the references of the large cases are hundreds of megabytes)."""
    key = (case.id, case.eq, tuple(sorted(case.sizes.items())), dtype)
    if key not in _DATA:
        while len(_DATA) >= 2:
            _DATA.pop(next(iter(_DATA)))
        arrays = case.arrays(dtype)
        hi = "complex128" if "complex" in dtype else "float64"
        ref = np.einsum(case.eq, *[x.astype(hi) for x in arrays], optimize=True)
        tol = 1e-12
        if dtype in ("float32", "complex64"):
            tol = G.single_gate(ref, np.einsum(case.eq, *arrays, optimize=True))
        ref.setflags(write=False)
        _DATA[key] = (arrays, ref, tol)
    return _DATA[key]


def contract(case, dtype, sliced=(), strip_exponent=False):
    """``(flags of the pair step, result, slices per launch)`` -- the name is read before anything runs."""
    arrays, _, _ = data(case, dtype)
    fn = HipContractor(case.tree(sliced=sliced))
    try:
        ex = fn.setup(*arrays)["exec"]
        names = [n for n in ex.step_kernels() if n.startswith("pair_")]
        assert len(names) == 1, names
        print(f"KERNEL {case.id} {dtype} {'strip ' if strip_exponent else ''}{names[0]}")
        flags = G.pair_flags(names[0])
        batch = ex.batch
        if strip_exponent:
            m, e = fn(*arrays, strip_exponent=True)
            got = np.asarray(m) * 10.0 ** e
        else:
            got = np.asarray(fn(*arrays))
    finally:
        fn.close()
    return flags, got, batch


def assert_tile(flags, case, dtype):
    kernel, t = MFMA_KERNEL[dtype]
    assert (flags["kernel"], flags["dtype"]) == (kernel, t), flags
    assert (flags["tm"], flags["tn"]) == case.tiles[dtype], (flags, case.tiles[dtype])


def assert_close(got, case, dtype):
    _, ref, tol = data(case, dtype)
    err = G.relerr(got, ref)
    print(f"ERROR {case.id} {dtype} {err:.3e} gate {tol:.3e}")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("case", V.TILE_CASES + V.GATHER_CASES, ids=repr)
def test_tile_variant(case, dtype):
    """Every row of both tables in the three types, on the tile the table records for it."""
    flags, got, _ = contract(case, dtype)
    assert_tile(flags, case, dtype)
    if case.vec is not None and dtype in case.vec:
        assert flags["vec"] is case.vec[dtype], flags
    assert_close(got, case, dtype)


@pytest.mark.parametrize("dtype", ("float32", "float64"))
@pytest.mark.parametrize("case", V.GATHER_CASES, ids=repr)
def test_gather_variant(case, dtype):
    """The 16-byte gathers of the real kernels: VEC as the table says, and -- part of the contraction sliced, so that
    the slice strides enter the host's check -- the same result.  Slices that start at odd elements of an operand
    gathered along k must not be fetched in 16-byte pieces."""
    flags, got, _ = contract(case, dtype)
    assert_tile(flags, case, dtype)
    assert flags["vec"] is case.vec[dtype], flags
    assert_close(got, case, dtype)
    for fast in (False, True):
        cut = V.split_contracted(case, fast)
        flags, got, _ = contract(cut, dtype, sliced=("s",))
        assert_tile(flags, cut, dtype)
        if fast and (cut.ta[-1] == "s" or cut.tb[-1] == "s"):
            assert flags["vec"] is False, flags
        assert_close(got, cut, dtype)


TALL = [(ident, dtype) for ident, per in V.SLICED_ROWS.items() for dtype in per]


@pytest.mark.parametrize("ident,dtype", TALL)
def test_tall_tile_strip_exponent(ident, dtype):
    """The large tiles scale what they store by 1 / (facA facB) under strip_exponent (step_alpha): mantissa times
    10^exponent meets the same gate."""
    case = next(c for c in V.TILE_CASES if c.id == ident)
    assert case.tiles[dtype] != (2, 2)
    flags, got, _ = contract(case, dtype, strip_exponent=True)
    assert_tile(flags, case, dtype)
    assert_close(got, case, dtype)


@pytest.mark.parametrize("ident,dtype", TALL)
def test_tall_tile_slice_batches(ident, dtype, monkeypatch):
    """Four slices of the row index through one launch (gridDim.y = 4) and one by one: the same bits, and the
    unsliced reference's numbers.  One slice alone still fills the large tile's threshold: asserted by name."""
    case = V.sliced_case(ident, dtype)
    outs = []
    for cap in ("1", "4"):
        monkeypatch.setenv("CTG_SLICE_BATCH", cap)
        flags, got, batch = contract(case, dtype, sliced=("s",))
        assert batch == int(cap)
        assert_tile(flags, case, dtype)
        assert case.tiles[dtype] != (2, 2)
        outs.append(got)
    assert np.array_equal(outs[0], outs[1])
    assert_close(outs[1], case, dtype)


def _pairwise_case(index):
    import test_gpu_pairwise as TP

    eq, sizes = TP.CASES[index]
    return V.Case(f"pairwise{index % len(TP.CASES)}", eq, sizes, (0, 0, 0, 0), seed=index % len(TP.CASES))


def step_flags(case, dtype):
    arrays = case.arrays(dtype)
    fn = HipContractor(case.tree())
    try:
        names = [n for n in fn.setup(*arrays)["exec"].step_kernels() if n.startswith("pair_")]
    finally:
        fn.close()
    assert len(names) == 1, names
    print(f"KERNEL {case.id} {dtype} {names[0]}")
    return G.pair_flags(names[0]), names[0]


@pytest.mark.parametrize("dtype", V.ALL_DTYPES)
@pytest.mark.parametrize("row", V.KRED_PAIRWISE, ids=lambda r: r[1])
def test_long_contractions_take_the_k_reduction_kernels(row, dtype):
    """The cases of test_pairwise that are meant for pair_kred_kernel and pair_kred_multi_kernel<2|3|4> take them,
    in all four types (their numbers are test_pairwise's)."""
    index, eq, kernel, no = row
    case = _pairwise_case(index)
    assert case.eq == eq
    flags, _ = step_flags(case, dtype)
    assert (flags["kernel"], flags["no"]) == (kernel, no), flags
    assert flags["finish_wave"] is True, flags   # (K >= 65537: 128 chunks or more, at most four outputs)


@pytest.mark.parametrize("dtype", V.ALL_DTYPES)
@pytest.mark.parametrize("row", V.THREAD_PAIRWISE, ids=lambda r: r[1])
def test_short_contractions_take_a_thread_per_output(row, dtype):
    index, eq = row
    case = _pairwise_case(index)
    assert case.eq == eq
    _, name = step_flags(case, dtype)
    assert name == "pair_valu_kernel"


@pytest.mark.parametrize("dtype", V.ALL_DTYPES)
@pytest.mark.parametrize("row", V.FINISH_CASES, ids=lambda r: r[0].id)
def test_finish_pass_forms(row, dtype):
    """Both forms of the pass that adds the partial sums of a long contraction, in all four types."""
    case, kernel, no, wave = row
    flags, got, _ = contract(case, dtype)
    assert (flags["kernel"], flags["no"]) == (kernel, no), flags
    assert flags["finish_wave"] is wave, flags
    assert_close(got, case, dtype)
