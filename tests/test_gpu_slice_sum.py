"""GPU suite: the slice sum of a forward plan (csrc/ctg_kernels_valu.hip: accum_kernel / accum_rows).

(a) The value the kernel's comment defines, bit for bit: the slices added in slice order -- for float32 / complex64
    in a double-precision copy of the result, rounded once -- whatever the slice batch and however the caller cuts
    the run.  ``sa->a`` with s = 1003 = 15 * 64 + 43, 43 = 5 * 8 + 3: every slice is a copy of one row of the
    operand, the default batch of 64 ends on a launch that is no multiple of the eight slices fetched together.
(b) Slices that share a result element and slices that do not, in one launch: ``stab->tb`` with s (summed) and t
    (kept) both sliced, in both orders of slicing, and with the output transposed.
(c) The exponent-aware sum under ``strip_exponent`` (strip_prepare_kernel, rescale_kernel, StripState.coefM /
    coefm): slices whose magnitudes rise, fall or jump by factors of 100, and one of them zero."""
import numpy as np
import pytest

import cotengra_amd as ca
import golden_util as G
import single_variant_cases as V
from cotengra_amd.contractor import HipContractor
from cotengra_amd.plan import KIND_ACCUM, KIND_SINGLE

pytestmark = pytest.mark.gpu

ALL_DTYPES = ("float32", "float64", "complex64", "complex128")
HI = {"float32": "float64", "float64": "float64", "complex64": "complex128", "complex128": "complex128"}


def normal(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    if "complex" in dtype:
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dtype)


def tree_of(eq, sizes, sliced):
    terms, out = ca.eq_to_inputs_output(eq)
    tree = ca.ContractionTree.from_path(list(terms), out, sizes, path=[] if len(terms) == 1 else [(0, 1)])
    for ix in sliced:
        tree.remove_ind_(ix)
    return tree


def gate_of(eq, arrays, dtype):
    """``(reference, gate)``: the gates of tests/test_gpu_single_variants.py."""
    ref = np.asarray(np.einsum(eq, *[x.astype(HI[dtype]) for x in arrays], optimize=True))
    tol = 1e-12 if dtype == HI[dtype] else G.single_gate(ref, np.einsum(eq, *arrays, optimize=True))
    ref.setflags(write=False)
    return ref, tol


def slice_ids(parts):
    return [first + i * stride for first, count, stride in parts for i in range(count)]


def run(tree, arrays, monkeypatch, cap, parts=None, want_single=None):
    """The contraction with at most ``cap`` slices per launch; ``parts``: the run cut by the caller into
    ``run_slices(first, count, stride)`` calls that cover every slice once.  The forward plan keeps its one
    ``accum_kernel``."""
    monkeypatch.setenv("CTG_SLICE_BATCH", str(cap))
    fn = HipContractor(tree)
    try:
        ex = fn.setup(*arrays)["exec"]
        names = ex.step_kernels()
        assert [n for n, s in zip(names, ex.plan.steps) if s.kind == KIND_ACCUM] == ["accum_kernel"], names
        if want_single is not None:
            assert [n for n, s in zip(names, ex.plan.steps) if s.kind == KIND_SINGLE] == [want_single], names
        assert ex.batch == min(cap, tree.nslices)
        if parts is None:
            return np.asarray(fn(*arrays))
        ex.set_strip_exponent(False, False)
        ex.zero_result()
        assert sorted(slice_ids(parts)) == list(range(tree.nslices))
        for first, count, stride in parts:
            ex.run_slices(first, count, stride)
        return np.asarray(ex.download_result())
    finally:
        fn.close()


# ---- (a) ------------------------------------------------------------------------------------------------------------ #

S, A = 1003, 37


def defined_sum(x):
    """The left fold over the slices in slice order: in double for the single types, rounded once."""
    acc = np.zeros(x.shape[1:], HI[x.dtype.name])
    for s in range(x.shape[0]):
        acc = acc + x[s].astype(acc.dtype)
    return acc.astype(x.dtype)


def fold_in_type(x):
    acc = np.zeros(x.shape[1:], x.dtype)
    for s in range(x.shape[0]):
        acc = acc + x[s]
    assert acc.dtype == x.dtype
    return acc


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_slice_sum_is_the_double_left_fold_rounded_once(dtype, monkeypatch):
    x = normal((S, A), dtype, seed=0)
    G.assert_in_upload_window(x)   # (no prescale, no coefficient: the slices are the operand's rows exactly)
    want = defined_sum(x)
    assert want.dtype == x.dtype
    if dtype in ("float32", "complex64"):
        # a build that lost the double-precision copy adds in the type: that differs nearly everywhere
        differs = int(np.count_nonzero(fold_in_type(x) != want))
        print(f"FOLD {dtype} the fold in the type differs in {differs} of {A}")
        assert differs >= (A + 1) // 2
    else:
        assert np.array_equal(fold_in_type(x), want)
    tree = tree_of("sa->a", dict(s=S, a=A), "s")
    assert tree.nslices == S
    for cap in (1, 8, 12, 64):
        got = run(tree, [x], monkeypatch, cap)
        assert got.dtype == x.dtype and got.shape == want.shape
        assert np.array_equal(got, want), (dtype, cap, int(np.count_nonzero(got != want)))
    # the run cut by the caller in two uneven parts (417 = 6 * 64 + 33; 586 = 9 * 64 + 10)
    got = run(tree, [x], monkeypatch, 64, parts=[(0, 417, 1), (417, 586, 1)])
    assert np.array_equal(got, want), (dtype, "two parts")


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_slice_sum_of_wave_kernel_slices(dtype, monkeypatch):
    """``sab->b`` with a = 300 on the same s: the slice value comes from single_wave_kernel."""
    sizes = dict(s=S, a=300, b=5)
    x = normal((S, 300, 5), dtype, seed=1)
    ref, tol = gate_of("sab->b", [x], dtype)
    tree = tree_of("sab->b", sizes, "s")
    outs = [run(tree, [x], monkeypatch, cap, want_single="single_wave_kernel") for cap in (1, 8, 12, 64)]
    for got in outs[1:]:
        assert np.array_equal(outs[0], got)
    err = G.relerr(outs[0], ref)
    print(f"ERROR sab->b {dtype} {err:.3e} gate {tol:.3e}")
    assert err <= tol, (err, tol)


# ---- (b) ------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("eq", ["stab->tb", "stab->bt"])
@pytest.mark.parametrize("order", ["st", "ts"])
def test_shared_and_unshared_result_elements_in_one_launch(order, eq, dtype, monkeypatch):
    """15 slices over s (summed, 5) and t (kept, 3), sliced in either order: consecutive slices of a launch share
    their result elements in runs of five (the tree sorts its sliced indices, kept before summed, whatever the order
    of slicing: tests/test_single_variant_plans.py).  The slices asked for with t running fastest (five strided
    runs of three) change their result element at every slice of a launch -- the kernel flushes its register each
    time -- and every element still adds its five slices in rising s: the same bits.  ``->bt``: the rows of the
    result are strided."""
    sizes = dict(s=5, t=3, a=7, b=11)
    x = normal((5, 3, 7, 11), dtype, seed=2)
    ref, tol = gate_of(eq, [x], dtype)
    tree = tree_of(eq, sizes, order)
    assert tree.nslices == 15
    outs = [run(tree, [x], monkeypatch, cap) for cap in (1, 4, 15)]
    strided = [(s, 3, 5) for s in range(5)]
    assert slice_ids(strided) == V.t_fast_ids(5, 3)
    outs += [run(tree, [x], monkeypatch, cap, parts=strided) for cap in (1, 4, 15)]
    for got in outs[1:]:
        assert np.array_equal(outs[0], got)
    err = G.relerr(outs[0], ref)
    print(f"ERROR {eq} {order} {dtype} {err:.3e} gate {tol:.3e}")
    assert outs[0].shape == ref.shape and err <= tol, (err, tol)


# ---- (c) ------------------------------------------------------------------------------------------------------------ #

NS = 6
ORDERS = {"rising": [0, 2, 4, 6, 8, 10], "falling": [0, -2, -4, -6, -8, -10], "mixed": [4, 0, 10, 2, 8, 6]}
ZEROED = (None, 0, 3, NS - 1)


def scaled_operand(dtype, order, zeroed):
    x = normal((NS, 9, 5), HI[dtype], seed=3)
    x = x * (10.0 ** np.array(ORDERS[order], dtype=np.float64))[:, None, None]
    if zeroed is not None:
        x[zeroed] = 0
    return x.astype(dtype)


def strip_run(fn, arrays):
    m, e = fn(*arrays, strip_exponent=True, check_zero=True)
    return np.asarray(m), float(e)


def is_zero_with_no_exponent(out):
    m, e = out
    return np.ndim(m) == 0 and m == 0 and e == float("-inf")


def exponent_aware_sum(eq, dtype, sizes, others, monkeypatch):
    """Every order of magnitudes and every zeroed slice through ``strip_exponent`` and ``check_zero`` with one and
    with six slices per launch asked for: equal bits, mantissa times 10^exponent against numpy on the scaled operand
    -- a result that keeps s row by row, each row against its own largest element --, and (0, -inf) for the all-zero
    operand."""
    tree = tree_of(eq, sizes, "s")
    by_row = "s" in eq.split("->")[1]
    results, zeros = {}, {}
    for cap in (1, NS):
        monkeypatch.setenv("CTG_SLICE_BATCH", str(cap))
        fn = HipContractor(tree)
        try:
            for order in ORDERS:
                for zeroed in ZEROED:
                    results[cap, order, zeroed] = strip_run(fn, [scaled_operand(dtype, order, zeroed)] + others)
            zeros[cap] = fn(np.zeros((NS, 9, 5), dtype), *others, strip_exponent=True, check_zero=True)
        finally:
            fn.close()
    hi = [y.astype(HI[dtype]) for y in others]
    for order in ORDERS:
        for zeroed in ZEROED:
            (m1, e1), (m6, e6) = results[1, order, zeroed], results[NS, order, zeroed]
            assert e1 == e6 and np.array_equal(m1, m6), (order, zeroed)
            x = scaled_operand(dtype, order, zeroed)
            got = m1.astype(HI[dtype]) * 10.0 ** e1
            ref = np.einsum(eq, x.astype(HI[dtype]), *hi)
            low = np.einsum(eq, x, *others)
            assert got.shape == ref.shape
            rows = [(got[i], ref[i], low[i]) for i in range(NS)] if by_row else [(got, ref, low)]
            for i, (g, r, l) in enumerate(rows):
                if not np.any(r):
                    assert by_row and i == zeroed and not np.any(g), (order, zeroed, i)   # (the zero slice's own row)
                    continue
                tol = 1e-12 if dtype == HI[dtype] else G.single_gate(r, l)
                err = G.relerr(g, r)
                print(f"ERROR {eq} {dtype} {order} zero={zeroed} row {i}: {err:.3e} gate {tol:.3e}")
                assert err <= tol, (order, zeroed, i, err, tol)
    for cap in (1, NS):
        print(f"ZERO {eq} {dtype} batch {cap}: {zeros[cap]!r}")
        assert is_zero_with_no_exponent(zeros[cap]), zeros[cap]


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("eq", ["sab->b", "sab->sb"])
def test_exponent_aware_slice_sum(eq, dtype, monkeypatch):
    """Six slices 10^2 apart, rising, falling and out of order, each again with its first, a middle or its last
    slice zero.  A one-input tree has no pair step: nothing is normalised, every slice carries the exponent of the
    upload, and ``check_zero`` tests the slice output itself."""
    exponent_aware_sum(eq, dtype, dict(s=NS, a=9, b=5), [], monkeypatch)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("eq", ["sab,bc->c", "sab,bc->sc"])
def test_exponent_aware_slice_sum_with_a_pair_step(eq, dtype, monkeypatch):
    """The same set on a two-input tree: every slice has a pair step, hence a factor and an exponent of its own
    that rises, falls or jumps with the slice, and a zero slice is met by ``check_zero`` -- the sum rescales what
    it holds (coefM) and what it adds (coefm) at nearly every slice."""
    exponent_aware_sum(eq, dtype, dict(s=NS, a=9, b=5, c=4), [normal((5, 4), dtype, seed=4)], monkeypatch)
