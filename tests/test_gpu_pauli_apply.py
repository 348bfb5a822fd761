"""GPU suite: a Pauli sum applied to the result tensor on the device and the energy gradients built on it
(csrc/ctg_pauli_apply.hip) -- ``Executor.pauli_apply_result``, ``HipContractor.apply_paulis`` /
``energy``, ``ContractionTree.contract_apply_paulis`` / ``contract_energy``, ``ContractExpression.energy``,
``circuits.energy_gradient`` and the torch autograd route.

Data reaches the result tensor bit for bit through a one-tensor tree, as in tests/test_gpu_pauli.py.  Reference and
tolerance are in tests/pauli_apply_util.py, derived from the roundings of the two associations and never from what the
device returns.

The power-of-two route works on output chunks of 4096 elements with grid = min(512, ceil(chunks / 3)): 2^12 elements
are one chunk; 2^13 two chunks on one workgroup, which an X letter on bit 12 pairs; 2^15 elements 8 chunks on 3
workgroups and 2^18 elements 64 chunks on 22, the last round partial in both."""
import ctypes as C

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import HipContractor
from cotengra_amd.vjp import compile_vjp
from oracle.plan_interp import run_plan

import golden_util as G
import pauli_apply_util as au
import pauli_util as pu
import vjp_util as V
from test_gpu_pauli import circuit_tree, strings_for
from test_gpu_result_reduce import resident
from test_gpu_sample import gaussian, random_circuit

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "complex64", "complex128"]
TAG = {"float32": "float", "float64": "double", "complex64": "c64", "complex128": "c128"}


def strings_and_coeffs(L, dtype, seed=0):
    ops = strings_for(L)
    if np.dtype(dtype).kind != "c":
        ops = ops[(ops == 2).sum(axis=1) % 2 == 0]          # P x of a real tensor must be real
    coeffs = np.random.default_rng(17000 + 10 * L + seed).standard_normal(len(ops))
    return ops, coeffs


def _close(tree):
    for fn in tree.contraction_cores.values():
        if isinstance(fn, HipContractor):
            fn.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [6, 12, 13, 15, 18])
def test_power_of_two_shapes_against_the_reference(L, dtype):
    """2^6: the general route; 2^12: one chunk; 2^13: two chunks that bit 12 pairs; 2^15, 2^18: several workgroups
    with a partial last round."""
    x = gaussian(2 ** L, dtype, seed=170 + L)
    ex = resident(x)
    shape = (2,) * L
    ops, coeffs = strings_and_coeffs(L, dtype)
    want = f"pauli_apply_general_kernel<{TAG[dtype]}>" if L < 12 else f"pauli_apply_kernel<{TAG[dtype]}>"
    assert ex.pauli_apply_variant(shape, ops) == runtime.pauli_apply_variant(dtype, shape, ops) == want
    got = ex.pauli_apply_result(shape, ops, coeffs)
    au.check_apply(got, x, shape, ops, coeffs)
    assert ex.download_result().tobytes() == x.tobytes()


def exact_case(dtype):
    L = 16
    rng = np.random.default_rng(1716)
    x = (np.clip(np.round(2 * gaussian(2 ** L, dtype, seed=8)), -4, 4) / 2 + 0.0).astype(dtype)   # (+ 0.0: no negative zeros)
    extra = [{12: "X", 11: "Z"}, {11: "Y", 12: "Y"}, {12: "Y", 13: "Z", 0: "Z"}, {15: "Y", 0: "Y", 12: "X"},
             {1: "X", 2: "Z"}, {0: "X", 1: "X", 5: "Z"}, {15: "X"}, {15: "X", 3: "Z"}, {b: "Z" for b in range(L)}]
    ops = np.concatenate([strings_for(L), np.array([pu.bit_string(L, c) for c in extra], dtype=np.uint8)])
    if np.dtype(dtype).kind != "c":
        ops = ops[(ops == 2).sum(axis=1) % 2 == 0]
    coeffs = rng.integers(-8, 9, size=len(ops)) / 4.0
    coeffs[coeffs == 0] = 0.25
    return x, (2,) * L, ops, coeffs


@pytest.mark.parametrize("dtype", DTYPES)
def test_half_integers_are_exact(dtype):
    """Half-integer amplitudes in [-2, 2], coefficients multiples of 1/4 in [-2, 2], about 40 strings at 2^16 elements
    -- letters inside a 16-byte group, across the 11 | 12 chunk boundary, on the top bit, ny = 1 .. 4, a full-weight Z
    string: every partial sum is a multiple of 1/8 below 2^10 and exact, in fp32 too, so the device equals numpy."""
    x, shape, ops, coeffs = exact_case(dtype)
    assert len(ops) >= (38 if np.dtype(dtype).kind == "c" else 25)
    ex = resident(x)
    assert ex.pauli_apply_variant(shape, ops) == f"pauli_apply_kernel<{TAG[dtype]}>"
    got = ex.pauli_apply_result(shape, ops, coeffs)
    ref = au.pauli_apply_reference(x, shape, ops, coeffs)
    assert np.array_equal(ref.astype(dtype).astype(ref.dtype), ref)       # (the reference fits the plan's dtype)
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, ref.astype(dtype)), int(np.sum(got != ref.astype(dtype)))
    assert np.count_nonzero(got) >= got.size // 4
    assert ex.download_result().tobytes() == x.tobytes()


def device_apply(ex, shape, ops, coeffs, dtype, fill=None):
    """``y`` through ``dev_out``: a torch buffer, downloaded."""
    import torch

    buf = torch.empty(shape, dtype=getattr(torch, dtype), device="cuda")
    if fill is not None:
        buf.fill_(fill)
    assert ex.pauli_apply_result(shape, ops, coeffs, out_ptr=buf.data_ptr()) is None
    return buf.cpu().numpy()


@pytest.mark.parametrize("dtype", ["float32", "float64", "complex64"])
def test_a_dev_out_that_is_not_16_byte_aligned(dtype):
    """``dev_out`` one element into a torch buffer: the power-of-two route stores element by element, the same bytes
    as the 16-byte stores give, and touches neither the element in front nor the one behind."""
    import torch

    L = 13
    n = 2 ** L
    x = gaussian(n, dtype, seed=178)
    shape = (2,) * L
    ops, coeffs = strings_and_coeffs(L, dtype, seed=2)
    ex = resident(x)
    assert ex.pauli_apply_variant(shape, ops) == f"pauli_apply_kernel<{TAG[dtype]}>"
    want = ex.pauli_apply_result(shape, ops, coeffs)
    au.check_apply(want, x, shape, ops, coeffs)
    buf = torch.full((n + 2,), 7.0, dtype=getattr(torch, dtype), device="cuda")
    ptr = buf.data_ptr() + buf.element_size()
    assert buf.data_ptr() % 16 == 0 and ptr % 16 != 0
    assert ex.pauli_apply_result(shape, ops, coeffs, out_ptr=ptr) is None
    got = buf.cpu().numpy()
    assert got[0] == 7.0 and got[-1] == 7.0 and got[1:-1].tobytes() == want.tobytes()
    assert ex.download_result().tobytes() == x.tobytes()


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_the_bits_are_a_function_of_the_arguments_alone(dtype):
    L = 15
    x = gaussian(2 ** L, dtype, seed=175)
    shape = (2,) * L
    ops, coeffs = strings_and_coeffs(L, dtype, seed=1)
    ex = resident(x)
    first = ex.pauli_apply_result(shape, ops, coeffs)
    au.check_apply(first, x, shape, ops, coeffs)
    assert ex.pauli_apply_result(shape, ops, coeffs).tobytes() == first.tobytes()              # the same call twice
    ex.topk_result(7)
    ex.rdm_result(shape, [1, 1] + [0] * (L - 2))
    ex.pauli_result(shape, ops)
    assert ex.pauli_apply_result(shape, ops, coeffs).tobytes() == first.tobytes()              # after other calls in the scratch
    assert resident(x).pauli_apply_result(shape, ops, coeffs).tobytes() == first.tobytes()     # a fresh executor
    assert device_apply(ex, shape, ops, coeffs, dtype, fill=3.0).tobytes() == first.tobytes()  # dev_out against host_out
    assert resident(gaussian(2 ** L, dtype, seed=176)).pauli_apply_result(shape, ops, coeffs).tobytes() != first.tobytes()
    assert ex.download_result().tobytes() == x.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_general_shapes(dtype):
    """Mixed-width and non-power-of-two shapes run on the general route: one below 4096 elements, one above."""
    rng = np.random.default_rng(177)
    for shape in ((2, 3, 2, 5, 2), (2,) * 10 + (3, 2)):
        n = int(np.prod(shape))
        x = gaussian(n, dtype, seed=n)
        rows = [[0] * len(shape)]
        for _ in range(9):
            rows.append([int(rng.integers(0, 4)) if d == 2 else 0 for d in shape])
        ops = np.array(rows, dtype=np.uint8)
        if np.dtype(dtype).kind != "c":
            ops = ops[(ops == 2).sum(axis=1) % 2 == 0]
        coeffs = rng.standard_normal(len(ops))
        ex = resident(x)
        assert ex.pauli_apply_variant(shape, ops) == f"pauli_apply_general_kernel<{TAG[dtype]}>"
        got = ex.pauli_apply_result(shape, ops, coeffs)
        au.check_apply(got, x, shape, ops, coeffs)
        assert device_apply(ex, shape, ops, coeffs, dtype).tobytes() == got.tobytes()
        assert ex.download_result().tobytes() == x.tobytes()
    # a power-of-two count in a shape whose extents are powers of two of mixed width: the fast route
    shape = (4, 2, 8, 2, 16, 2, 2)
    x = gaussian(int(np.prod(shape)), dtype, seed=9)
    ops = np.array([[0, 1, 0, 3, 0, 2, 2], [0, 3, 0, 0, 0, 1, 0], [0, 0, 0, 1, 0, 0, 3]], dtype=np.uint8)
    ex = resident(x)
    assert ex.pauli_apply_variant(shape, ops) == f"pauli_apply_kernel<{TAG[dtype]}>"
    au.check_apply(ex.pauli_apply_result(shape, ops, [0.5, -1.5, 2.0]), x, shape, ops, [0.5, -1.5, 2.0])


@pytest.mark.parametrize("dtype", ["complex64", "float32"])
def test_zero_cases(dtype):
    for shape in ((2,) * 13, (2, 3, 2)):
        n = int(np.prod(shape))
        x = gaussian(n, dtype, seed=5)
        ex = resident(x)
        none = np.zeros((0, len(shape)), np.uint8)
        assert ex.pauli_apply_variant(shape, none) == "none"
        got = ex.pauli_apply_result(shape, none, [])
        assert got.shape == shape and got.dtype == np.dtype(dtype) and not got.any()       # m = 0 writes zeros
        assert not device_apply(ex, shape, none, [], dtype, fill=5.0).any()
        rows = np.array([[1] + [0] * (len(shape) - 1), [3] + [0] * (len(shape) - 2) + [1]], np.uint8)
        zz = resident(np.zeros(n, dtype)).pauli_apply_result(shape, rows, [1.5, -2.0])
        assert zz.shape == shape and not zz.any()                                          # an all-zero tensor
        zc = ex.pauli_apply_result(shape, rows, [0.0, 0.0])
        assert not zc.any()                                                                # all-zero coefficients


def raw_call(ex, rank, ext, m, ops, coeffs, dev, host, handle="own"):
    i64p, u8p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    return runtime.load().ctg_exec_result_pauli_apply(
        ex.handle if handle == "own" else handle, rank, None if ext is None else ext.ctypes.data_as(i64p), m,
        None if ops is None else ops.ctypes.data_as(u8p), None if coeffs is None else coeffs.ctypes.data_as(dp),
        C.c_void_p(dev), C.c_void_p(None if host is None else host.ctypes.data))


def test_refusals_through_the_c_abi():
    import torch

    n = 2 ** 13
    x = gaussian(n, "complex64", seed=13)
    ex = resident(x)
    before = ex.device_bytes()
    ext = np.array([2, 2, 2048], np.int64)
    ops = np.array([[1, 3, 0], [2, 2, 0]], np.uint8)
    cs = np.array([0.5, -1.25])
    dev = torch.full((n,), 7.0 + 7.0j, dtype=torch.complex64, device="cuda")
    host = np.full(n, 7.0 + 7.0j, dtype=np.complex64)
    d = dev.data_ptr()
    big = np.zeros((4097, 3), np.uint8)
    res = ex.result_ptr()
    bad = [
        (3, ext, 2, ops, cs, d, host, None),                                              # a null exec
        (3, None, 2, ops, cs, d, host, "own"), (3, ext, 2, None, cs, d, host, "own"),
        (3, ext, 2, ops, None, d, host, "own"),                                           # null coeffs with m > 0
        (3, ext, 2, ops, cs, None, None, "own"),                                          # both outputs null
        (3, ext, 2, ops, cs, res, host, "own"),                                           # dev_out is the result tensor
        (3, ext, 2, ops, cs, res + 8 * (n - 1), host, "own"),                             # ... overlaps its last element
        (3, ext, 2, ops, cs, res - 8 * (n - 1), host, "own"),                             # ... its first
        (-1, ext, 2, ops, cs, d, host, "own"),                                            # rank < 0
        (3, np.array([2, 2, 2047], np.int64), 2, ops, cs, d, host, "own"),                # a wrong product
        (2, ext, 2, ops, cs, d, host, "own"),
        (3, np.array([2, 2, 0], np.int64), 2, ops, cs, d, host, "own"),
        (3, np.array([2 ** 21, 2 ** 21, 2], np.int64), 2, ops, cs, d, host, "own"),       # past 2^40 elements before the last axis
        (3, ext, -1, ops, cs, d, host, "own"), (3, ext, 4097, big, np.ones(4097), d, host, "own"),
        (3, ext, 2, np.array([[1, 3, 0], [2, 4, 0]], np.uint8), cs, d, host, "own"),      # a code above 3
        (3, ext, 2, np.array([[1, 3, 0], [0, 0, 1]], np.uint8), cs, d, host, "own"),      # a letter on an axis of extent 2048
        (3, ext, 2, ops, np.array([0.5, np.nan]), d, host, "own"),                        # a coefficient that is not finite
        (3, ext, 2, ops, np.array([np.inf, 1.0]), d, host, "own"),
    ]
    for rank, e_, m, o_, c_, dev_, host_, handle in bad:
        assert raw_call(ex, rank, e_, m, o_, c_, dev_, host_, handle) == -1, (rank, m)
        assert runtime.load().ctg_last_error()
        assert np.all(host == 7.0 + 7.0j)
    assert ex.device_bytes() == before                            # (nothing was launched, not even the scratch allocated)
    assert torch.all(dev == 7.0 + 7.0j).item() and ex.download_result().tobytes() == x.tobytes()
    # a real plan: a string with an odd number of Y
    xr = gaussian(n, "float32", seed=14)
    exr = resident(xr)
    devr = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    hostr = np.full(n, 7.0, dtype=np.float32)
    assert raw_call(exr, 3, ext, 2, np.array([[1, 3, 0], [2, 0, 0]], np.uint8), cs, devr.data_ptr(), hostr) == -1
    assert np.all(hostr == 7.0) and torch.all(devr == 7.0).item() and exr.download_result().tobytes() == xr.tobytes()
    assert raw_call(exr, 3, ext, 2, ops, cs, devr.data_ptr(), hostr) == 0                 # (two Y: real)
    au.check_apply(hostr.reshape(2, 2, 2048), xr, (2, 2, 2048), ops, cs)
    assert devr.cpu().numpy().tobytes() == hostr.tobytes()
    # a following valid call is correct, into both outputs
    assert raw_call(ex, 3, ext, 2, ops, cs, d, host) == 0
    au.check_apply(host.reshape(2, 2, 2048), x, (2, 2, 2048), ops, cs)
    assert dev.cpu().numpy().tobytes() == host.tobytes() and ex.download_result().tobytes() == x.tobytes()
    # host_out alone: y is staged in the scratch, which is counted
    host2 = np.zeros(n, dtype=np.complex64)
    assert raw_call(ex, 3, ext, 2, ops, cs, None, host2) == 0 and host2.tobytes() == host.tobytes()
    assert ex.device_bytes() >= before + 8 * n
    # a NaN member: CTG_E_NORM, the buffers untouched
    badx = x.copy()
    badx[4097] = np.nan
    exn = resident(badx)
    host[:] = 7.0 + 7.0j
    assert raw_call(exn, 3, ext, 2, ops, cs, None, host) == -6 and np.all(host == 7.0 + 7.0j)
    with pytest.raises(ValueError):
        exn.pauli_apply_result((2, 2, 2048), ops, cs)


def layered_trees(dtype):
    """A circuit tree sliced by ``target_size`` into at least 4 slices, and one with a sliced output index and a
    sliced inner index."""
    n = 10
    tree, arrays = circuit_tree(n, random_circuit(n, 5, seed=3), dtype)
    inner = tree.slice(target_size=tree.max_size() // 8)
    assert inner.nslices >= 4 and inner.gathered_shape() == (2,) * n
    outer, _ = circuit_tree(n, random_circuit(n, 5, seed=3), dtype)
    big = max((p for p, _, _ in outer.traverse()), key=outer.get_size)
    for ix in [outer.output[2]] + [ix for ix in outer.get_legs(big) if ix not in outer.output][:1]:
        outer.remove_ind_(ix)
    assert outer.nslices > 1 and outer.output[2] in outer.sliced_inds and outer.gathered_shape() == (2,) * n
    return (inner, outer), arrays


TEXTS = ["IIIIIIIIII", "ZIIIIIIIII", "IZZIIIIIII", "XIIIIYIIIZ", "YYIIIIIIXX", "ZZZZZZZZZZ", "IIYIIXIIII", "XXYIIIIIIZ"]
COEFFS = [0.3, 0.5, -1.0, 0.25, 2.0, -0.75, 1.5, -0.6]


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_through_the_layers_on_sliced_trees(dtype):
    trees, arrays = layered_trees(dtype)
    wide = [a.astype("complex128") for a in arrays]
    ops = np.array([pu.codes(t) for t in TEXTS], dtype=np.uint8)
    for tree in trees:
        ref_e, ref_g = au.reference_energy_grads(tree, wide, ops, COEFFS)
        r = tree.contract_energy(arrays, TEXTS, coeffs=COEFFS)
        assert isinstance(r, ca.EnergyResult) and len(r.grads) == tree.N
        exp = tree.contract_expectation(arrays, TEXTS)
        assert r.values.tobytes() == exp.values.tobytes() and r.norm == exp.norm
        assert r.energy == sum(c * v for c, v in zip(COEFFS, exp.values.tolist()))
        x = np.asarray(tree.contract(arrays))
        rel = 1e-10 if dtype == "complex128" else 1e-5
        assert abs(r.energy - ref_e) <= 8 * rel * np.abs(COEFFS).sum()
        # y itself, through the tree layer, and the result stays reusable
        ap = tree.contract_apply_paulis(arrays, TEXTS, coeffs=COEFFS)
        assert isinstance(ap, ca.ApplyResult) and ap.exponent == 0.0 and ap.norm == exp.norm
        au.check_apply(ap.y, x, x.shape, ops, COEFFS)
        assert tree.contract_apply_paulis([], TEXTS, coeffs=COEFFS, reuse=True).y.tobytes() == ap.y.tobytes()
        assert tree.contract_expectation([], TEXTS, reuse=True).values.tobytes() == exp.values.tobytes()
        if dtype == "complex64":
            y = au.pauli_apply_reference(np.asarray(orc_contract(tree, wide)), x.shape, ops, COEFFS)
            plan = compile_vjp(tree, dtype)
            npy = V.split_grads(plan, run_plan(plan, list(arrays) + [np.conj(2.0 * y).astype(dtype)]), [a.shape for a in arrays])
        for i, (g, want) in enumerate(zip(r.grads, ref_g)):
            assert g.dtype == np.dtype(dtype) and g.shape == arrays[i].shape
            gate = 1e-10 if dtype == "complex128" else max(1e-5, 8 * G.relerr(np.conj(npy[i]), want))
            assert G.relerr(g, want) <= gate, (i, G.relerr(g, want), gate)
        _close(tree)


def orc_contract(tree, arrays):
    from oracle import contract_ref as orc

    return np.asarray(orc.contract(tree, arrays)).reshape(tree.gathered_shape())


def test_wrt_a_real_leaf_and_normalize():
    """``wrt`` on a subset gives ``None`` elsewhere; a real leaf in a complex tree gets a real gradient; ``normalize``
    differentiates ``E / N`` on a circuit with a fixed qubit (norm below 1)."""
    n = 9
    tree, arrays = circuit_tree(n, random_circuit(n, 4, seed=5), "complex128", template="??0??????")
    tree = tree.slice(target_size=max(tree.max_size() // 4, 4))
    assert tree.nslices >= 4
    arrays = list(arrays)
    arrays[1] = np.ascontiguousarray(arrays[1].real)
    texts = ["ZIIIIIII", "IXXIIIII", "YIIIIIYZ", "IIIIIIII", "ZZZZZZZZ"]
    coeffs = [0.7, -1.1, 0.4, 0.2, 1.3]
    ops = np.array([pu.codes(t) for t in texts], dtype=np.uint8)
    for normalize in (False, True):
        ref_e, ref_g = au.reference_energy_grads(tree, arrays, ops, coeffs, normalize=normalize)
        r = tree.contract_energy(arrays, texts, coeffs=coeffs, wrt=[1, 2, tree.N - 1], normalize=normalize)
        assert 0 < r.norm < 0.999 and abs(r.energy - ref_e) <= 1e-10 * np.abs(coeffs).sum() / (r.norm if normalize else 1)
        assert [g is None for g in r.grads] == [i not in (1, 2, tree.N - 1) for i in range(tree.N)]
        assert r.grads[1].dtype == np.float64 and r.grads[2].dtype == np.complex128
        for i in (1, 2, tree.N - 1):
            assert G.relerr(r.grads[i], ref_g[i]) <= 1e-10, (normalize, i)
        full = tree.contract_energy(arrays, texts, coeffs=coeffs, normalize=normalize)
        assert full.energy == r.energy and all(g is not None for g in full.grads)
    # a real contraction: a string with an odd number of Y has value and gradient exactly zero and is left out
    real = [np.ascontiguousarray(a.real) for a in arrays]
    rr = tree.contract_energy(real, ["YIIIIIII", "ZIIIIIII", "YIIIIIYZ"], coeffs=[5.0, 0.7, 0.4])
    only = tree.contract_energy(real, ["ZIIIIIII", "YIIIIIYZ"], coeffs=[0.7, 0.4])
    assert rr.values[0] == 0.0 and rr.energy == only.energy
    assert all(a.dtype == np.float64 and a.tobytes() == b.tobytes() for a, b in zip(rr.grads, only.grads))
    ref_e, ref_g = au.reference_energy_grads(tree, real, ops[[0, 2]], [0.7, 0.4])
    assert all(G.relerr(g, w) <= 1e-10 for g, w in zip(only.grads, ref_g))
    _close(tree)


def test_expression_energy():
    rng = np.random.default_rng(71)
    a, b = rng.standard_normal((2, 12, 7)), rng.standard_normal((7, 10, 2))
    expr = ca.einsum_expression("xab,bcy->xacy", a.shape, b.shape)
    tree = expr.fn.tree
    texts = ["XIIZ", "ZIIZ", "YIIY", "IIII"]
    coeffs = [0.5, -1.0, 2.0, 0.1]
    r = expr.energy(a, b, paulis=texts, coeffs=coeffs)
    ref_e, ref_g = au.reference_energy_grads(tree, [a, b], np.array([pu.codes(t) for t in texts]), coeffs)
    assert abs(r.energy - ref_e) <= 1e-10 * abs(ref_e) and all(G.relerr(g, w) <= 1e-10 for g, w in zip(r.grads, ref_g))
    assert r.values.tobytes() == expr.expectation(a, b, paulis=texts).values.tobytes()
    expr.close()
    exs = ca.einsum_expression("xab,bcy->xacy", a.shape, b.shape, strip_exponent=True)
    with pytest.raises(ValueError):
        exs.energy(a, b, paulis=texts, coeffs=coeffs)
    exs.close()


def test_autograd():
    import torch

    n = 8
    tree, arrays = circuit_tree(n, random_circuit(n, 4, seed=11), "complex128")
    tree = tree.slice(target_size=max(tree.max_size() // 4, 4))
    assert tree.nslices >= 4
    texts, coeffs = ["ZIIIIIII", "IXXIIIII", "YIIIIIYZ", "ZZZZZZZZ", "IYIIIIII"], [0.7, -1.1, 0.4, 1.3, -0.2]
    ops = np.array([pu.codes(t) for t in texts], dtype=np.uint8)
    for normalize in (False, True):
        ref_e, ref_g = au.reference_energy_grads(tree, arrays, ops, coeffs, normalize=normalize)
        xs = [torch.tensor(a, device="cuda", requires_grad=True) for a in arrays]
        r = tree.contract_energy(xs, texts, coeffs=coeffs, normalize=normalize)
        E = r.energy
        assert torch.is_tensor(E) and E.is_cuda and E.dtype == torch.float64 and E.ndim == 0 and E.grad_fn is not None
        assert r.grads is None
        plain = tree.contract_energy([torch.tensor(a, device="cuda") for a in arrays], texts, coeffs=coeffs, normalize=normalize)
        assert isinstance(plain.energy, float) and torch.equal(E.detach().cpu(), torch.tensor(plain.energy, dtype=torch.float64))
        assert r.values.tobytes() == plain.values.tobytes()
        (3.0 * E).backward()
        for x, g, want in zip(xs, plain.grads, ref_g):
            assert G.relerr(x.grad.cpu().numpy(), 3.0 * want) <= 1e-10
            assert torch.is_tensor(g) and g.is_cuda and G.relerr(g.cpu().numpy(), want) <= 1e-10
    # a subset that requires grad, a numpy constant among the inputs
    xs = [torch.tensor(a, device="cuda", requires_grad=i in (0, 3)) for i, a in enumerate(arrays)]
    xs[2] = arrays[2]
    tree.contract_energy(xs, texts, coeffs=coeffs).energy.backward()
    ref_e, ref_g = au.reference_energy_grads(tree, arrays, ops, coeffs)
    assert xs[1].grad is None and all(G.relerr(xs[i].grad.cpu().numpy(), ref_g[i]) <= 1e-10 for i in (0, 3))
    _close(tree)


def test_autograd_gradcheck():
    import torch

    n = 5
    tree, arrays = circuit_tree(n, random_circuit(n, 3, seed=2), "complex128")
    big = max((p for p, _, _ in tree.traverse()), key=tree.get_size)
    for ix in [tree.output[1]] + [ix for ix in tree.get_legs(big) if ix not in tree.output][:1]:
        tree.remove_ind_(ix)
    assert tree.nslices == 4 and tree.gathered_shape() == (2,) * n
    reqs = ["IIIII", "XZIIY", "YYIZI", "IZIIX", "ZZZZZ"]
    coeffs = [0.3, 0.9, -0.7, 1.1, 0.5]
    xs = [torch.tensor(a, device="cuda", requires_grad=True) for a in arrays]
    for normalize in (False, True):
        assert torch.autograd.gradcheck(lambda *x: tree.contract_energy(list(x), reqs, coeffs=coeffs, normalize=normalize).energy,
                                        xs, fast_mode=True, atol=1e-8, rtol=1e-6)
    _close(tree)


def test_circuit_energy_gradient():
    """Every rz derivative equals the exact parameter-shift value taken with ``circuits.pauli_expectation``; every fs
    derivative equals CPU autograd through gate tensors built from torch parameters; both within 1e-10 sum |c_s|."""
    import torch

    n = 7
    gates = random_circuit(n, 3, seed=21)
    texts = ["ZIIIIII", "IZZIIII", "XIIIIYI", "YYIIIXX", "ZZZZZZZ", "IIIXIII"]
    coeffs = np.array([0.5, -1.0, 0.25, 2.0, -0.75, 1.2])
    tol = 1e-10 * np.abs(coeffs).sum()
    energy, norm, dparams = circuits.energy_gradient(n, gates, texts, coeffs, dtype="complex128", target_size=64)
    assert len(dparams) == len(gates) and abs(norm - 1) <= 1e-10
    assert abs(energy - circuits.pauli_expectation(n, gates, texts, coeffs=coeffs, dtype="complex128")[2]) <= tol
    rz = [k for k, g in enumerate(gates) if g[0] == "rz"]
    fs = [k for k, g in enumerate(gates) if g[0] == "fs"]
    assert len(rz) >= 3 and len(fs) >= 3
    for k, g in enumerate(gates):
        assert dparams[k].shape == ({"rz": 1, "fs": 2}.get(g[0], 0),) and dparams[k].dtype == np.float64
    for k in rz:
        es = []
        for shift in (np.pi / 2, -np.pi / 2):
            moved = list(gates)
            moved[k] = ("rz", gates[k][1], (gates[k][2][0] + shift,))
            es.append(circuits.pauli_expectation(n, moved, texts, coeffs=coeffs, dtype="complex128")[2])
        assert abs(dparams[k][0] - (es[0] - es[1]) / 2) <= tol, k
    # fs: the gate tensors as functions of torch parameters
    inputs, output, sd, arrays = circuits.circuit_to_network(n, gates, "?" * n, simplify=False, dtype="complex128")
    tree = ca.array_contract_tree(inputs, output, sd)
    params = {k: torch.tensor(gates[k][2], dtype=torch.float64, requires_grad=True) for k in fs}
    xs = [torch.tensor(a) for a in arrays]
    for k, p in params.items():
        c, s = torch.cos(p[0]).to(torch.complex128), torch.sin(p[0]).to(torch.complex128)
        U = torch.zeros(4, 4, dtype=torch.complex128)
        U[0, 0] = 1
        U[1, 1], U[2, 2], U[1, 2], U[2, 1] = c, c, -1j * s, -1j * s
        U[3, 3] = torch.exp(-1j * p[1].to(torch.complex128))
        assert np.abs(U.detach().numpy() - circuits.gate_matrix("fs", gates[k][2])).max() <= 1e-15
        xs[n + k] = U.reshape(2, 2, 2, 2)
    out = tree.contract(xs, implementation=(torch.einsum, torch.tensordot)).reshape((2,) * n)
    ops = np.array([pu.codes(t) for t in texts], dtype=np.uint8)
    E = torch.real(torch.sum(out.conj() * au.torch_apply(out, ops, coeffs))) / torch.real(torch.sum(out.conj() * out))
    grads = torch.autograd.grad(E, [params[k] for k in fs])
    for k, g in zip(fs, grads):
        assert np.abs(dparams[k] - g.numpy()).max() <= tol, (k, dparams[k], g.numpy())
