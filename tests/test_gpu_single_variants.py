"""GPU suite: the single-term kernels (csrc/ctg_kernels_valu.hip: single_wave_kernel, single_kernel) on every row of
tests/single_variant_cases.py, in float32, float64, complex64 and complex128.

Every case first asserts the kernel the executor names for its single-term step -- read before anything runs -- and
then compares the result element-wise with ``numpy.einsum`` in float64 / complex128: 1e-12 of the largest element
for the double types, ``G.single_gate`` against numpy's own single-precision einsum for the others.  One dropped
lane tail, one wrong ``kA.hi`` offset or one wrong slice offset is an error of order 1 against these gates.  Sliced
rows run with 1, 4 and all slices per launch (gridDim.y = nz) and must give the same bits.
tests/test_single_variant_plans.py pins the plans and the table's edges on the host."""
import numpy as np
import pytest

import golden_util as G
import single_variant_cases as V
import vjp_util as U
from cotengra_amd.contractor import HipContractor
from cotengra_amd.plan import KIND_SINGLE
from cotengra_amd.vjp import compile_vjp
from oracle.plan_interp import run_plan

pytestmark = pytest.mark.gpu

HI = {"float32": "float64", "float64": "float64", "complex64": "complex128", "complex128": "complex128"}

_DATA = {}


def data(case, dtype):
    """``(operands, reference, gate)`` of a case: computed once, shared by the tests that follow one another on
    the same case (the last two are kept), the reference read-only."""
    key = (case.id, dtype)
    if key not in _DATA:
        while len(_DATA) >= 2:
            _DATA.pop(next(iter(_DATA)))
        arrays = case.arrays(dtype)
        ref = np.asarray(np.einsum(case.eq, *[x.astype(HI[dtype]) for x in arrays], optimize=True))
        tol = 1e-12
        if dtype in ("float32", "complex64"):
            tol = G.single_gate(ref, np.einsum(case.eq, *arrays, optimize=True))
        ref.setflags(write=False)
        _DATA[key] = (arrays, ref, tol)
    return _DATA[key]


def contract(case, dtype):
    """``(name of the single-term step, result, slices per launch)`` -- the name is read before anything runs."""
    arrays, _, _ = data(case, dtype)
    fn = HipContractor(case.tree())
    try:
        ex = fn.setup(*arrays)["exec"]
        kernels = ex.step_kernels()
        names = [n for n, s in zip(kernels, ex.plan.steps) if s.kind == KIND_SINGLE]
        assert len(names) == 1, kernels
        print(f"KERNEL {case.id} {dtype} {names[0]}")
        batch = ex.batch
        got = np.asarray(fn(*arrays))
    finally:
        fn.close()
    return names[0], got, batch


def assert_close(got, case, dtype):
    _, ref, tol = data(case, dtype)
    assert got.dtype == np.dtype(dtype)
    err = G.relerr(got, ref)
    print(f"ERROR {case.id} {dtype} {err:.3e} gate {tol:.3e}")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("dtype", V.ALL_DTYPES)
@pytest.mark.parametrize("case", V.UNSLICED_CASES + [V.LEAF_CASE], ids=repr)
def test_single_variant(case, dtype):
    """Every unsliced row, and the leaf preprocessing inside a two-input tree, on the kernel the table records."""
    name, got, _ = contract(case, dtype)
    assert name == case.kernel
    assert_close(got, case, dtype)


@pytest.mark.parametrize("dtype", V.ALL_DTYPES)
@pytest.mark.parametrize("case", V.SLICED_CASES, ids=repr)
def test_single_variant_slice_batches(case, dtype, monkeypatch):
    """The slices of a row one by one, four per launch and all in one launch: the kernel the table records, the
    same bits, and the unsliced reference's numbers."""
    outs = []
    for cap in (1, 4, case.nslices):
        monkeypatch.setenv("CTG_SLICE_BATCH", str(cap))
        name, got, batch = contract(case, dtype)
        assert name == case.kernel
        assert batch == min(cap, case.nslices)
        outs.append(got)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert_close(outs[0], case, dtype)


VJP_CASES = [c for c in V.UNSLICED_CASES if c.elems <= V.VJP_MAX_ELEMS]


@pytest.mark.parametrize("dtype", V.ALL_DTYPES)
@pytest.mark.parametrize("case", VJP_CASES, ids=repr)
def test_single_variant_vjp(case, dtype):
    """The device gradient of a one-input tree (the ``N == 1`` branch of cotengra_amd/vjp.py) against torch autograd,
    under the gate of tests/test_gpu_vjp.py; off a diagonal the gradient is exactly zero."""
    wide = HI[dtype]
    tree = case.tree()
    arrays = case.arrays(wide)
    h = U.cotangent(tree, wide)
    ref = U.reference_vjp(tree, arrays, h)
    xs, hx = [a.astype(dtype) for a in arrays], h.astype(dtype)
    fn = HipContractor(tree)
    try:
        got = fn.vjp(*xs, cotangent=hx)
    finally:
        fn.close()
    gate = 1e-10
    if dtype != wide:
        plan = compile_vjp(tree, dtype)
        npy = U.split_grads(plan, run_plan(plan, xs + [hx]), [a.shape for a in xs])
        gate = max(1e-5, 8 * G.relerr(npy[0], ref[0]))
    (g,), (r,) = got, ref
    assert g.dtype == np.dtype(dtype) and g.shape == r.shape
    err = G.relerr(g, r)
    print(f"VJP {case.id} {dtype} {err:.3e} gate {gate:.3e}")
    assert err <= gate, (err, gate)
    term = case.terms[0]
    if len(set(term)) < len(term):
        off = np.ones(g.shape, bool)
        np.einsum("".join(term) + "->" + "".join(dict.fromkeys(term)), off)[...] = False   # (a writable view of the diagonal)
        assert off.sum() > 0 and np.all(g[off] == 0)
