"""GPU suite: dense local operators applied to the result tensor on the device and what is built on them
(csrc/ctg_op_apply.hip) -- ``Executor.op_apply_result``, ``HipContractor.apply_operators`` /
``operator_expectation`` / ``operator_energy``, the ``ContractionTree`` and ``ContractExpression`` wrappers,
``circuits.operator_expectation`` / ``operator_energy_gradient`` and the torch autograd route.

Data reaches the result tensor bit for bit through a one-tensor tree (``resident`` of tests/test_gpu_result_reduce.py).
Reference and tolerance are in tests/op_apply_util.py, derived from the roundings of the two associations and never
from what the device returns.

The power-of-two route works on output chunks of 4096 elements with grid = min(512, ceil(chunks / 3)): 2^12 elements are
one chunk; 2^13 two chunks on one workgroup, which a term on the top axis pairs; 2^15 elements 8 chunks on 3 workgroups
and 2^18 elements 64 chunks on 22, the last round partial in both.  Flat bit ``b`` of a ``(2,) * L`` tensor is axis ``L
- 1 - b``; a 16-byte group holds 4, 2, 2, 1 elements (float, double, c64, c128), so flat bits 0 and 1 lie inside one
group in single precision and bits 3 and 7 in different groups everywhere.  At 2^12 there is no bit 12: the pair
"straddling bits 11 and 12" is the pair on bits 10 and 11 there."""
import ctypes as C

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import HipContractor
from cotengra_amd.vjp import compile_vjp
from oracle.plan_interp import run_plan

import golden_util as G
import op_apply_util as ou
import pauli_apply_util as au
import pauli_util as pu
import vjp_util as V
from test_gpu_pauli import circuit_tree
from test_gpu_pauli_apply import layered_trees, orc_contract
from test_gpu_result_reduce import resident
from test_gpu_sample import gaussian, random_circuit, statevector

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "complex64", "complex128"]
TAG = {"float32": "float", "float64": "double", "complex64": "c64", "complex128": "c128"}

X = np.array([[0, 1], [1, 0]], dtype=complex)
Y = np.array([[0, -1j], [1j, 0]], dtype=complex)
Z = np.array([[1, 0], [0, -1]], dtype=complex)
HEIS = np.kron(X, X) + np.kron(Y, Y).real + np.kron(Z, Z)      # XX + YY + ZZ: real, block-sparse


def dense(rng, d, dtype):
    m = rng.standard_normal((d, d))
    return m if np.dtype(dtype).kind != "c" else m + 1j * rng.standard_normal((d, d))


def hermitian(rng, d, real=False):
    m = rng.standard_normal((d, d)) + (0 if real else 1j * rng.standard_normal((d, d)))
    return m + m.conj().T


def bits_to_axes(L, *bits):
    return tuple(sorted(L - 1 - b for b in bits))


def route_terms(L, dtype, rng):
    """The terms of the module docstring for ``(2,) * L``, ascending axes."""
    cast = (lambda m: np.real(m)) if np.dtype(dtype).kind != "c" else (lambda m: m)
    if L < 12:
        return [(bits_to_axes(L, 0, 1), dense(rng, 4, dtype)), (bits_to_axes(L, L - 1, L - 2), dense(rng, 4, dtype)),
                (bits_to_axes(L, L - 1), dense(rng, 2, dtype)), (bits_to_axes(L, 2, L - 1), np.diag(np.diag(dense(rng, 4, dtype)))),
                (bits_to_axes(L, 3, L - 1), cast(HEIS)), (bits_to_axes(L, 1, 3, L - 1), dense(rng, 8, dtype)),
                (bits_to_axes(L, 0, 4), dense(rng, 4, dtype)), (bits_to_axes(L, 0, 4), dense(rng, 4, dtype))]
    hi = min(12, L - 1)
    return [(bits_to_axes(L, 0, 1), dense(rng, 4, dtype)),                       # inside one 16-byte group
            (bits_to_axes(L, 3, 7), dense(rng, 4, dtype)),                       # low bits in different groups
            (bits_to_axes(L, hi - 1, hi), dense(rng, 4, dtype)),                 # straddling the chunk boundary
            (bits_to_axes(L, L - 1, L - 2), dense(rng, 4, dtype)),               # the two highest bits
            (bits_to_axes(L, L - 1), dense(rng, 2, dtype)),                      # one axis, the top bit
            (bits_to_axes(L, 5, L - 1), np.diag(np.diag(dense(rng, 4, dtype)))),  # diagonal
            (bits_to_axes(L, 2, L - 1), cast(HEIS)),                             # block-sparse
            (bits_to_axes(L, L - 1, L - 2), cast(HEIS)),                         # block-sparse on high bits: 1 x 1 blocks
            (bits_to_axes(L, 1, 6, L - 1), dense(rng, 8, dtype)),                # three axes
            (bits_to_axes(L, 4, 9), dense(rng, 4, dtype)), (bits_to_axes(L, 4, 9), dense(rng, 4, dtype))]


def _close(tree):
    for fn in tree.contraction_cores.values():
        if isinstance(fn, HipContractor):
            fn.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [6, 12, 13, 15, 18])
def test_routes_and_boundaries(L, dtype):
    x = gaussian(2 ** L, dtype, seed=190 + L)
    ex = resident(x)
    shape = (2,) * L
    terms = route_terms(L, dtype, np.random.default_rng(1900 + L))
    want = f"op_apply_general_kernel<{TAG[dtype]}>" if L < 12 else f"op_apply_kernel<{TAG[dtype]}>"
    assert ex.op_apply_variant(shape, terms) == runtime.op_apply_variant(dtype, shape, terms) == want
    got = ex.op_apply_result(shape, terms)
    ou.check_op_apply(got, x, shape, terms)
    assert ex.download_result().tobytes() == x.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_extents_other_than_two(dtype):
    rng = np.random.default_rng(191)
    cases = [((4, 2, 8, 2, 16, 2, 2), [((0, 2), dense(rng, 32, dtype)), ((4,), dense(rng, 16, dtype))], "op_apply_kernel"),
             ((2, 3, 2, 5, 2), [((1, 3), dense(rng, 15, dtype))], "op_apply_general_kernel"),
             ((2,) * 10 + (3, 2), [((4, 10), dense(rng, 6, dtype))], "op_apply_general_kernel"),
             # D = 64 on six axes that include flat bits 12 and 0 (c128: the block stays in the scratch)
             ((2,) * 13, [((0, 3, 5, 8, 10, 12), dense(rng, 64, dtype))], "op_apply_kernel")]
    for shape, terms, kernel in cases:
        n = int(np.prod(shape))
        x = gaussian(n, dtype, seed=n % 1000)
        ex = resident(x)
        assert ex.op_apply_variant(shape, terms) == runtime.op_apply_variant(dtype, shape, terms) == f"{kernel}<{TAG[dtype]}>"
        got = ex.op_apply_result(shape, terms)
        ou.check_op_apply(got, x, shape, terms)
        assert device_apply(ex, shape, terms, dtype).tobytes() == got.tobytes()
        assert ex.download_result().tobytes() == x.tobytes()


def half_integers(n, dtype, seed):
    x = (np.clip(np.round(2 * gaussian(n, dtype, seed=seed)), -4, 4) / 2 + 0.0).astype(dtype)   # (+ 0.0: no negative zeros)
    return x


def quarters(rng, d, dtype):
    m = rng.integers(-8, 9, size=(d, d)) / 4.0
    return m if np.dtype(dtype).kind != "c" else m + 1j * rng.integers(-8, 9, size=(d, d)) / 4.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_half_integers_are_exact(dtype):
    """Half-integer amplitudes in [-2, 2], matrix entries multiples of 1/4 in [-2, 2], a dozen terms (N = 54) at 2^16
    elements: every product is a multiple of 1/8, a complex component of a term is at most 8 and every partial sum
    stays below 2^9, so each is exact, in fp32 too, and the device equals numpy bit for bit."""
    L = 16
    rng = np.random.default_rng(1916)
    x = half_integers(2 ** L, dtype, seed=8)
    shape = (2,) * L
    real = np.dtype(dtype).kind != "c"
    terms = [(axes, quarters(rng, np.asarray(m).shape[0], dtype)) for axes, m in route_terms(L, dtype, rng)]
    terms[5] = (terms[5][0], np.diag(np.diag(terms[5][1])))
    terms[6] = (terms[6][0], np.real(HEIS) / 4 if real else HEIS / 4)
    terms.append((bits_to_axes(L, 0, 12, 15), quarters(rng, 8, dtype)))
    assert len(terms) == 12
    ex = resident(x)
    assert ex.op_apply_variant(shape, terms) == f"op_apply_kernel<{TAG[dtype]}>"
    got = ex.op_apply_result(shape, terms)
    ref = ou.op_apply_reference(x, shape, terms)
    assert np.array_equal(ref.astype(dtype).astype(ref.dtype), ref)       # (the reference fits the plan's dtype)
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, ref.astype(dtype)), int(np.sum(got != ref.astype(dtype)))
    assert np.count_nonzero(got) >= got.size // 4
    assert ex.download_result().tobytes() == x.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_skipping_zero_blocks_and_entries_changes_no_bit(dtype):
    """A diagonal term and a term with a zero column -- whose zero blocks and columns the kernel skips -- against the
    same operator given as two terms, dense off the diagonal, whose sum it is, nothing skipped: the same bytes on
    half-integer data, where both are exact, and within the sum of both bounds on Gaussian data.  On low bits (one
    block: zero columns), across the chunk boundary and on high bits alone (zero blocks) and on the general route
    (zero entries)."""
    rng = np.random.default_rng(192)
    for L, bits in ((13, (2, 9)), (13, (3, 12)), (14, (12, 13)), (7, (1, 6))):
        shape = (2,) * L
        axes = bits_to_axes(L, *bits)
        x = half_integers(2 ** L, dtype, seed=L)
        g = gaussian(2 ** L, dtype, seed=50 + L)
        ex, exg = resident(x), resident(g)
        diag = np.diag(np.diag(quarters(rng, 4, dtype)))
        colz = quarters(rng, 4, dtype)
        colz[:, 2] = 0
        for sparse in (diag, colz):
            r = quarters(rng, 4, dtype) / 2
            r[r == 0] = 0.25
            a, b = sparse / 2 + r, sparse / 2 - r
            assert np.array_equal(a + b, sparse) and np.all(r != 0)
            one = ex.op_apply_result(shape, [(axes, sparse)])
            two = ex.op_apply_result(shape, [(axes, a), (axes, b)])
            assert one.tobytes() == two.tobytes() and np.array_equal(one, ou.op_apply_reference(x, shape, [(axes, sparse)]).astype(dtype))
            one = exg.op_apply_result(shape, [(axes, sparse)])
            two = exg.op_apply_result(shape, [(axes, a), (axes, b)])
            ou.check_op_apply(one, g, shape, [(axes, sparse)])
            ou.check_op_apply(two, g, shape, [(axes, a), (axes, b)])
            tol = ou.op_apply_tol(g, shape, [(axes, sparse)]) + ou.op_apply_tol(g, shape, [(axes, a), (axes, b)])
            d = pu.widen(two) - pu.widen(one)
            assert np.all(np.maximum(np.abs(d.real), np.abs(d.imag)) <= tol)


def device_apply(ex, shape, terms, dtype, fill=None):
    """``y`` through ``dev_out``: a torch buffer, downloaded."""
    import torch

    buf = torch.empty(shape, dtype=getattr(torch, dtype), device="cuda")
    if fill is not None:
        buf.fill_(fill)
    assert ex.op_apply_result(shape, terms, out_ptr=buf.data_ptr()) is None
    return buf.cpu().numpy()


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_the_bits_are_a_function_of_the_arguments_alone(dtype):
    L = 15
    x = gaussian(2 ** L, dtype, seed=195)
    shape = (2,) * L
    terms = route_terms(L, dtype, np.random.default_rng(1950))
    ex = resident(x)
    first = ex.op_apply_result(shape, terms)
    ou.check_op_apply(first, x, shape, terms)
    assert ex.op_apply_result(shape, terms).tobytes() == first.tobytes()                       # the same call twice
    ex.topk_result(7)
    ex.rdm_result(shape, [1, 1] + [0] * (L - 2))
    ex.pauli_apply_result(shape, [pu.bit_string(L, {0: "X", 13: "Z"})], [0.5])
    assert ex.op_apply_result(shape, terms).tobytes() == first.tobytes()                       # after other calls in the scratch
    assert resident(x).op_apply_result(shape, terms).tobytes() == first.tobytes()              # a fresh executor
    assert device_apply(ex, shape, terms, dtype, fill=3.0).tobytes() == first.tobytes()        # dev_out against host_out
    assert resident(gaussian(2 ** L, dtype, seed=196)).op_apply_result(shape, terms).tobytes() != first.tobytes()
    assert ex.download_result().tobytes() == x.tobytes()


@pytest.mark.parametrize("dtype", ["float32", "float64", "complex64"])
def test_a_dev_out_that_is_not_16_byte_aligned(dtype):
    """``dev_out`` one element into a torch buffer: the power-of-two route stores element by element, the same bytes
    as the 16-byte stores give, and touches neither the element in front nor the one behind."""
    import torch

    L = 13
    n = 2 ** L
    x = gaussian(n, dtype, seed=198)
    shape = (2,) * L
    terms = route_terms(L, dtype, np.random.default_rng(1980))
    ex = resident(x)
    assert ex.op_apply_variant(shape, terms) == f"op_apply_kernel<{TAG[dtype]}>"
    want = ex.op_apply_result(shape, terms)
    ou.check_op_apply(want, x, shape, terms)
    buf = torch.full((n + 2,), 7.0, dtype=getattr(torch, dtype), device="cuda")
    ptr = buf.data_ptr() + buf.element_size()
    assert buf.data_ptr() % 16 == 0 and ptr % 16 != 0
    assert ex.op_apply_result(shape, terms, out_ptr=ptr) is None
    got = buf.cpu().numpy()
    assert got[0] == 7.0 and got[-1] == 7.0 and got[1:-1].tobytes() == want.tobytes()
    assert ex.download_result().tobytes() == x.tobytes()


@pytest.mark.parametrize("dtype", ["complex64", "float32"])
def test_zero_cases(dtype):
    rng = np.random.default_rng(199)
    for shape in ((2,) * 13, (2, 3, 2)):
        n = int(np.prod(shape))
        x = gaussian(n, dtype, seed=5)
        ex = resident(x)
        assert ex.op_apply_variant(shape, []) == "none"
        got = ex.op_apply_result(shape, [])
        assert got.shape == shape and got.dtype == np.dtype(dtype) and not got.any()       # m = 0 writes zeros
        assert not device_apply(ex, shape, [], dtype, fill=5.0).any()
        terms = [((0,), dense(rng, 2, dtype)), ((0, len(shape) - 1), dense(rng, 4, dtype))]
        zz = resident(np.zeros(n, dtype)).op_apply_result(shape, terms)
        assert zz.shape == shape and not zz.any()                                          # an all-zero tensor
        zc = ex.op_apply_result(shape, [(axes, 0 * m) for axes, m in terms])
        assert not zc.any()                                                                # all-zero matrices


def raw_call(ex, rank, ext, m, naxes, axes, mats, dev, host, handle="own"):
    i64p, i32p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    return runtime.load().ctg_exec_result_op_apply(
        ex.handle if handle == "own" else handle, rank, None if ext is None else ext.ctypes.data_as(i64p), m,
        None if naxes is None else naxes.ctypes.data_as(i32p), None if axes is None else axes.ctypes.data_as(i32p),
        None if mats is None else mats.ctypes.data_as(dp), C.c_void_p(dev), C.c_void_p(None if host is None else host.ctypes.data))


def packed(*mats):
    return np.ascontiguousarray(np.concatenate([np.asarray(m, dtype=np.complex128).reshape(-1) for m in mats]).view(np.float64))


def test_refusals_through_the_c_abi():
    import torch

    n = 2 ** 13
    rng = np.random.default_rng(1913)
    x = gaussian(n, "complex64", seed=13)
    ex = resident(x)
    before = ex.device_bytes()
    ext = np.array([2, 2, 2, 1024], np.int64)
    m1, m2 = dense(rng, 4, "complex64"), dense(rng, 2, "complex64")
    na, ax, ms = np.array([2, 1], np.int32), np.array([0, 2, 1], np.int32), packed(m1, m2)
    terms = [((0, 2), m1), ((1,), m2)]
    dev = torch.full((n,), 7.0 + 7.0j, dtype=torch.complex64, device="cuda")
    host = np.full(n, 7.0 + 7.0j, dtype=np.complex64)
    d = dev.data_ptr()
    res = ex.result_ptr()
    nan, inf = ms.copy(), ms.copy()
    nan[5] = np.nan
    inf[-1] = np.inf
    i32 = lambda *v: np.array(v, np.int32)   # noqa: E731
    many = 4097
    bad = [
        (4, ext, 2, na, ax, ms, d, host, None),                                           # a null exec
        (4, None, 2, na, ax, ms, d, host, "own"),
        (4, ext, 2, None, ax, ms, d, host, "own"), (4, ext, 2, na, None, ms, d, host, "own"),   # null naxes, axes, mats
        (4, ext, 2, na, ax, None, d, host, "own"),
        (4, ext, 2, na, ax, ms, None, None, "own"),                                       # both outputs null
        (4, ext, 2, na, ax, ms, res, host, "own"),                                        # dev_out is the result tensor
        (4, ext, 2, na, ax, ms, res + 8 * (n - 1), host, "own"),                          # ... overlaps its last element
        (4, ext, 2, na, ax, ms, res - 8 * (n - 1), host, "own"),                          # ... its first
        (-1, ext, 2, na, ax, ms, d, host, "own"),                                         # rank < 0
        (4, np.array([2, 2, 2, 1023], np.int64), 2, na, ax, ms, d, host, "own"),          # a wrong product
        (3, ext, 2, na, ax, ms, d, host, "own"),
        (4, np.array([2, 2, 2, 0], np.int64), 2, na, ax, ms, d, host, "own"),
        (4, np.array([2 ** 21, 2 ** 21, 2, 2], np.int64), 2, na, ax, ms, d, host, "own"),  # past 2^40 elements before the last axis
        (4, ext, -1, na, ax, ms, d, host, "own"),                                         # m < 0
        (4, ext, many, np.ones(many, np.int32), np.zeros(many, np.int32), np.zeros(8 * many), d, host, "own"),   # too many terms
        (4, ext, 2, i32(2, 0), ax, ms, d, host, "own"),                                   # a term without axes
        (4, ext, 2, na, i32(0, 4, 1), ms, d, host, "own"), (4, ext, 2, na, i32(-1, 2, 1), ms, d, host, "own"),   # out of range
        (4, ext, 2, na, i32(2, 0, 1), ms, d, host, "own"),                                # not ascending
        (4, ext, 2, na, i32(2, 2, 1), ms, d, host, "own"),                                # repeated
        (4, ext, 1, i32(1), i32(3), np.zeros(2 * 1024 * 1024), d, host, "own"),           # D = 1024 > 64
        (4, ext, 2, na, ax, nan, d, host, "own"), (4, ext, 2, na, ax, inf, d, host, "own"),   # not finite
    ]
    for rank, e_, m, n_, a_, m_, dev_, host_, handle in bad:
        assert raw_call(ex, rank, e_, m, n_, a_, m_, dev_, host_, handle) == -1, (rank, m)
        assert runtime.load().ctg_last_error()
        assert np.all(host == 7.0 + 7.0j)
    # more than 2^20 entries: 257 terms of D = 64
    e13 = np.array([2] * 13, np.int64)
    assert raw_call(ex, 13, e13, 257, np.full(257, 6, np.int32), np.tile(np.arange(6, dtype=np.int32), 257),
                    np.zeros(257 * 64 * 64 * 2), d, host) == -1 and np.all(host == 7.0 + 7.0j)
    assert ex.device_bytes() == before                            # (nothing was launched, not even the scratch allocated)
    assert torch.all(dev == 7.0 + 7.0j).item() and ex.download_result().tobytes() == x.tobytes()
    # a real plan: an imaginary entry
    xr = gaussian(n, "float32", seed=14)
    exr = resident(xr)
    devr = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    hostr = np.full(n, 7.0, dtype=np.float32)
    assert raw_call(exr, 4, ext, 2, na, ax, ms, devr.data_ptr(), hostr) == -1
    assert np.all(hostr == 7.0) and torch.all(devr == 7.0).item() and exr.download_result().tobytes() == xr.tobytes()
    real_terms = [((0, 2), m1.real), ((1,), m2.real)]
    assert raw_call(exr, 4, ext, 2, na, ax, packed(m1.real, m2.real), devr.data_ptr(), hostr) == 0
    ou.check_op_apply(hostr.reshape(2, 2, 2, 1024), xr, (2, 2, 2, 1024), real_terms)
    assert devr.cpu().numpy().tobytes() == hostr.tobytes()
    # a following valid call is correct, into both outputs
    assert raw_call(ex, 4, ext, 2, na, ax, ms, d, host) == 0
    ou.check_op_apply(host.reshape(2, 2, 2, 1024), x, (2, 2, 2, 1024), terms)
    assert dev.cpu().numpy().tobytes() == host.tobytes() and ex.download_result().tobytes() == x.tobytes()
    # host_out alone: y is staged in the scratch, which is counted
    host2 = np.zeros(n, dtype=np.complex64)
    assert raw_call(ex, 4, ext, 2, na, ax, ms, None, host2) == 0 and host2.tobytes() == host.tobytes()
    assert ex.device_bytes() >= before + 8 * n
    # a NaN member: CTG_E_NORM, the buffers untouched
    badx = x.copy()
    badx[4097] = np.nan
    exn = resident(badx)
    host[:] = 7.0 + 7.0j
    assert raw_call(exn, 4, ext, 2, na, ax, ms, None, host) == -6 and np.all(host == 7.0 + 7.0j)
    with pytest.raises(ValueError):
        exn.op_apply_result((2, 2, 2, 1024), terms)


PAULI = {"I": np.eye(2, dtype=complex), "X": X, "Y": Y, "Z": Z}


def kron_of(letters):
    m = np.ones((1, 1), dtype=complex)
    for c in letters:
        m = np.kron(m, PAULI[c])
    return m


def test_against_the_pauli_route():
    """13 qubits, complex128: dense matrices of Pauli sums built with ``np.kron`` through ``apply_operators`` /
    ``operator_expectation`` against the same strings through ``apply_paulis`` / ``expectation`` -- kernels that share
    no code."""
    n = 13
    tree, arrays = circuit_tree(n, random_circuit(n, 4, seed=19), "complex128")
    out = list(tree.output)
    sums = [((0, 12), [("XX", 0.5), ("YY", 0.7), ("ZZ", -1.1), ("XZ", 0.25)]),
            ((3,), [("X", 0.3), ("Z", 0.2), ("Y", -0.4)]),
            ((2, 7, 11), [("XYZ", 0.9), ("ZZI", -0.6), ("IYY", 0.35)]),
            ((11, 12), [("ZZ", 1.0), ("ZI", -0.5), ("II", 0.125)])]
    operators, strings, coeffs = [], [], []
    for qs, parts in sums:
        operators.append(([out[q] for q in qs], sum(c * kron_of(t) for t, c in parts)))
        for t, c in parts:
            strings.append({out[q]: letter for q, letter in zip(qs, t)})
            coeffs.append(c)
    x = np.asarray(tree.contract(arrays))
    shape = x.shape
    a = tree.contract_apply_operators(arrays, operators)
    va = tree.contract_operator_expectation([], operators, reuse=True)
    b = tree.contract_apply_paulis(arrays, strings, coeffs=coeffs)
    vb = tree.contract_expectation([], strings, reuse=True)
    requests = [(qs, m) for (qs, _), (_, m) in zip(sums, operators)]
    ops = np.array([[{"I": 0, "X": 1, "Y": 2, "Z": 3}[s.get(ix, "I")] for ix in out] for s in strings], dtype=np.uint8)
    ou.check_op_apply(a.y, x, shape, requests)
    tol = ou.op_apply_tol(x, shape, requests) + au.pauli_apply_tol(x, shape, ops, coeffs)
    d = a.y - b.y
    assert np.all(np.maximum(np.abs(d.real), np.abs(d.imag)) <= tol) and a.norm == b.norm
    k = 0
    for (qs, parts), v in zip(sums, va.values):
        want = sum(c * vb.values[k + i] for i, (_, c) in enumerate(parts))
        assert abs(v - want) <= 1e-12 * sum(abs(c) for _, c in parts) * va.norm, (qs, v, want)
        k += len(parts)
    _close(tree)


def layer_requests(out, rng, real=False):
    """Hermitian requests over the labels ``out`` (10 qubits): labels in non-ascending order and one axis set twice;
    ``(operators by label, requests by axis)``."""
    spec = [((0, 3), 4), ((9,), 2), ((5, 2, 7), 8), ((3, 0), 4), ((8, 9), 4)]
    mats = [hermitian(rng, d, real) for _, d in spec]
    return [([out[q] for q in qs], m) for (qs, _), m in zip(spec, mats)], [(qs, m) for (qs, _), m in zip(spec, mats)]


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_through_the_layers_on_sliced_trees(dtype):
    trees, arrays = layered_trees(dtype)
    wide = [a.astype("complex128") for a in arrays]
    rng = np.random.default_rng(1920)
    for tree in trees:
        operators, requests = layer_requests(list(tree.output), rng)
        scale = sum(np.abs(m).sum() for _, m in requests)
        ref_e, ref_g = ou.reference_energy_grads(tree, wide, requests)
        r = tree.contract_operator_energy(arrays, operators)
        assert isinstance(r, ca.EnergyResult) and len(r.grads) == tree.N and r.values.dtype == np.complex128
        exp = tree.contract_operator_expectation(arrays, operators)
        assert isinstance(exp, ca.ExpectationResult) and r.values.tobytes() == exp.values.tobytes() and r.norm == exp.norm
        assert r.energy == sum(v.real for v in exp.values.tolist())
        x = np.asarray(tree.contract(arrays))
        rel = 1e-10 if dtype == "complex128" else 1e-5
        assert abs(r.energy - ref_e) <= 8 * rel * scale
        # the values against numpy on the downloaded result: rho is exact fp64 up to n roundings per entry
        for v, req in zip(exp.values, requests):
            want = np.vdot(pu.widen(x), ou.op_apply_reference(x, x.shape, [req]))
            assert abs(v - want) <= 4 * x.size * 2.0 ** -53 * np.abs(req[1]).sum() * exp.norm
        # y itself, through the tree layer, and the result stays reusable
        ap = tree.contract_apply_operators(arrays, operators)
        assert isinstance(ap, ca.ApplyResult) and ap.exponent == 0.0 and ap.norm == exp.norm
        ou.check_op_apply(ap.y, x, x.shape, requests)
        assert tree.contract_apply_operators([], operators, reuse=True).y.tobytes() == ap.y.tobytes()
        assert tree.contract_operator_expectation([], operators, reuse=True).values.tobytes() == exp.values.tobytes()
        if dtype == "complex64":
            y = ou.op_apply_reference(np.asarray(orc_contract(tree, wide)), x.shape, requests)
            plan = compile_vjp(tree, dtype)
            npy = V.split_grads(plan, run_plan(plan, list(arrays) + [np.conj(2.0 * y).astype(dtype)]), [a.shape for a in arrays])
        for i, (g, want) in enumerate(zip(r.grads, ref_g)):
            assert g.dtype == np.dtype(dtype) and g.shape == arrays[i].shape
            gate = 1e-10 if dtype == "complex128" else max(1e-5, 8 * G.relerr(np.conj(npy[i]), want))
            assert G.relerr(g, want) <= gate, (i, G.relerr(g, want), gate)
        _close(tree)


def test_wrt_a_real_leaf_and_normalize():
    """``wrt`` on a subset gives ``None`` elsewhere; a real leaf in a complex tree gets a real gradient; ``normalize``
    differentiates ``E / N`` on a circuit with a fixed qubit (norm below 1), with and without a request on axis 0
    to take the identity term."""
    n = 9
    tree, arrays = circuit_tree(n, random_circuit(n, 4, seed=5), "complex128", template="??0??????")
    tree = tree.slice(target_size=max(tree.max_size() // 4, 4))
    assert tree.nslices >= 4
    arrays = list(arrays)
    arrays[1] = np.ascontiguousarray(arrays[1].real)
    out = list(tree.output)
    rng = np.random.default_rng(1921)
    with0 = [((0,), hermitian(rng, 2)), ((1, 2), hermitian(rng, 4)), ((7, 3, 5), hermitian(rng, 8))]
    without0 = with0[1:]
    scale0 = sum(np.abs(m).sum() for _, m in with0)
    for requests in (with0, without0):
        operators = [([out[q] for q in qs], m) for qs, m in requests]
        scale = sum(np.abs(m).sum() for _, m in requests)
        for normalize in (False, True):
            ref_e, ref_g = ou.reference_energy_grads(tree, arrays, requests, normalize=normalize)
            r = tree.contract_operator_energy(arrays, operators, wrt=[1, 2, tree.N - 1], normalize=normalize)
            assert 0 < r.norm < 0.999 and abs(r.energy - ref_e) <= 1e-10 * scale / (r.norm if normalize else 1)
            assert [g is None for g in r.grads] == [i not in (1, 2, tree.N - 1) for i in range(tree.N)]
            assert r.grads[1].dtype == np.float64 and r.grads[2].dtype == np.complex128
            for i in (1, 2, tree.N - 1):
                assert G.relerr(r.grads[i], ref_g[i]) <= 1e-10, (normalize, i)
            full = tree.contract_operator_energy(arrays, operators, normalize=normalize)
            assert full.energy == r.energy and all(g is not None for g in full.grads)
    # a real contraction: the symmetric real part of a Hermitian request is what the energy sees
    real = [np.ascontiguousarray(a.real) for a in arrays]
    sym = [(qs, np.real(m)) for qs, m in with0]
    rr = tree.contract_operator_energy(real, [([out[q] for q in qs], m) for qs, m in with0])
    ref_e, ref_g = ou.reference_energy_grads(tree, real, sym)
    assert abs(rr.energy - ref_e) <= 1e-10 * scale0 and all(g.dtype == np.float64 for g in rr.grads)
    assert all(G.relerr(g, w) <= 1e-10 for g, w in zip(rr.grads, ref_g))
    _close(tree)


def spin_one():
    s = np.sqrt(0.5)
    sx = s * np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=complex)
    sy = s * np.array([[0, -1j, 0], [1j, 0, -1j], [0, 1j, 0]], dtype=complex)
    sz = np.diag([1.0, 0.0, -1.0]).astype(complex)
    return sx, sy, sz


@pytest.mark.parametrize("dtype", ["complex128", "float64"])
def test_spin_one_legs_through_an_expression(dtype):
    """A three-tensor ring with open legs of extent 3 -- the case no Pauli entry point can express: energy and
    gradients of spin-1 Heisenberg bonds and a single-site anisotropy against CPU autograd, the values against numpy,
    ``y`` against the reference; through ``ContractExpression``."""
    rng = np.random.default_rng(1922)
    shapes = [(4, 5, 3), (5, 6, 3), (6, 4, 3)]
    arrays = [gaussian(int(np.prod(s)), dtype, seed=30 + i).reshape(s) / 4 for i, s in enumerate(shapes)]
    expr = ca.einsum_expression("abx,bcy,caz->xyz", *shapes)
    tree = expr.fn.tree
    assert tuple(tree.gathered_shape()) == (3, 3, 3)
    sx, sy, sz = spin_one()
    bond = np.kron(sx, sx) + np.kron(sy, sy).real + np.kron(sz, sz)
    assert np.abs(bond.imag).max() == 0
    bond = bond.real if dtype == "float64" else bond
    aniso = (sz @ sz).real if dtype == "float64" else sz @ sz + 0.3 * sy
    requests = [((0, 1), bond), ((1, 2), 0.5 * bond), ((2,), aniso), ((2, 0), 0.25 * bond)]
    out = list(tree.output)
    operators = [([out[a] for a in axes], m) for axes, m in requests]
    scale = sum(np.abs(m).sum() for _, m in requests)
    x = np.asarray(expr(*arrays))
    ap = expr.apply_operators(*arrays, operators=operators)
    ou.check_op_apply(ap.y, x, x.shape, requests)
    ex = expr.operator_expectation(*arrays, operators=operators)
    for v, req in zip(ex.values, requests):
        want = np.vdot(x, ou.op_apply_reference(x, x.shape, [req]))
        assert abs(v - want) <= 4 * x.size * 2.0 ** -53 * np.abs(req[1]).sum() * ex.norm
    for normalize in (False, True):
        ref_e, ref_g = ou.reference_energy_grads(tree, arrays, requests, normalize=normalize)
        r = expr.operator_energy(*arrays, operators=operators, normalize=normalize)
        assert abs(r.energy - ref_e) <= 1e-10 * scale * (1 if normalize else r.norm)
        for g, want, a in zip(r.grads, ref_g, arrays):
            assert g.dtype == a.dtype and g.shape == a.shape and G.relerr(g, want) <= 1e-10, normalize
    expr.close()
    exs = ca.einsum_expression("abx,bcy,caz->xyz", *shapes, strip_exponent=True)
    with pytest.raises(ValueError):
        exs.operator_energy(*arrays, operators=operators)
    exs.close()


def test_autograd():
    import torch

    n = 8
    tree, arrays = circuit_tree(n, random_circuit(n, 4, seed=11), "complex128")
    tree = tree.slice(target_size=max(tree.max_size() // 4, 4))
    assert tree.nslices >= 4
    out = list(tree.output)
    rng = np.random.default_rng(1923)
    requests = [((0, 1), hermitian(rng, 4)), ((6, 2), hermitian(rng, 4)), ((7,), hermitian(rng, 2)), ((3, 4, 5), hermitian(rng, 8))]
    operators = [([out[q] for q in qs], m) for qs, m in requests]
    for normalize in (False, True):
        ref_e, ref_g = ou.reference_energy_grads(tree, arrays, requests, normalize=normalize)
        xs = [torch.tensor(a, device="cuda", requires_grad=True) for a in arrays]
        r = tree.contract_operator_energy(xs, operators, normalize=normalize)
        E = r.energy
        assert torch.is_tensor(E) and E.is_cuda and E.dtype == torch.float64 and E.ndim == 0 and E.grad_fn is not None
        assert r.grads is None
        plain = tree.contract_operator_energy([torch.tensor(a, device="cuda") for a in arrays], operators, normalize=normalize)
        assert isinstance(plain.energy, float) and torch.equal(E.detach().cpu(), torch.tensor(plain.energy, dtype=torch.float64))
        assert r.values.tobytes() == plain.values.tobytes()
        (3.0 * E).backward()
        for x, g, want in zip(xs, plain.grads, ref_g):
            assert G.relerr(x.grad.cpu().numpy(), 3.0 * want) <= 1e-10
            assert torch.is_tensor(g) and g.is_cuda and G.relerr(g.cpu().numpy(), want) <= 1e-10
    _close(tree)


def test_autograd_gradcheck():
    import torch

    n = 5
    tree, arrays = circuit_tree(n, random_circuit(n, 3, seed=2), "complex128")
    big = max((p for p, _, _ in tree.traverse()), key=tree.get_size)
    for ix in [tree.output[1]] + [ix for ix in tree.get_legs(big) if ix not in tree.output][:1]:
        tree.remove_ind_(ix)
    assert tree.nslices == 4 and tree.gathered_shape() == (2,) * n
    out = list(tree.output)
    rng = np.random.default_rng(1924)
    operators = [([out[1], out[3]], hermitian(rng, 4)), ([out[4]], hermitian(rng, 2)), ([out[2], out[0], out[1]], hermitian(rng, 8))]
    xs = [torch.tensor(a, device="cuda", requires_grad=True) for a in arrays]
    for normalize in (False, True):
        assert torch.autograd.gradcheck(lambda *x: tree.contract_operator_energy(list(x), operators, normalize=normalize).energy,
                                        xs, fast_mode=True, atol=1e-8, rtol=1e-6)
    _close(tree)


def test_circuit_operators():
    """A projector ``|1><1| (x) |1><1|`` and a hopping term ``a^+ b + b^+ a`` on a 7-qubit circuit: the values against
    the numpy statevector, energy and parameter gradient against ``circuits.energy_gradient`` on the Pauli expansion."""
    n = 7
    gates = random_circuit(n, 3, seed=21)
    proj = np.diag([0.0, 0.0, 0.0, 1.0]).astype(complex)
    up = np.array([[0, 0], [1, 0]], dtype=complex)            # |1><0|
    hop = np.kron(up, up.T) + np.kron(up.T, up)
    operators = [((2, 5), proj), ((3, 0), hop)]
    values, norm = circuits.operator_expectation(n, gates, operators, dtype="complex128")
    psi = statevector(n, gates).reshape((2,) * n)
    assert abs(norm - 1) <= 1e-10 and values.dtype == np.complex128
    for v, (qs, m) in zip(values, operators):
        want = np.vdot(psi, ou.op_apply_reference(psi, psi.shape, [(qs, m)]))
        assert abs(v - want) <= 1e-10, (qs, v, want)
    one, _ = circuits.operator_expectation(n, gates, ((2, 5), proj), dtype="complex128")
    assert np.ndim(one) == 0 and one == values[0]
    # |1><1| (x) |1><1| = (II - ZI - IZ + ZZ) / 4;  a^+ b + b^+ a = (XX + YY) / 2
    strings = [{}, {2: "Z"}, {5: "Z"}, {2: "Z", 5: "Z"}, {0: "X", 3: "X"}, {0: "Y", 3: "Y"}]
    coeffs = np.array([0.25, -0.25, -0.25, 0.25, 0.5, 0.5])
    tol = 1e-10 * np.abs(coeffs).sum()
    for normalize in (True, False):
        e1, n1, d1 = circuits.operator_energy_gradient(n, gates, operators, dtype="complex128", target_size=64, normalize=normalize)
        e2, n2, d2 = circuits.energy_gradient(n, gates, strings, coeffs, dtype="complex128", target_size=64, normalize=normalize)
        assert abs(e1 - e2) <= tol and abs(n1 - n2) <= 1e-12 and len(d1) == len(d2) == len(gates)
        assert abs(e1 - sum(values.real)) <= 1e-10
        for a, b in zip(d1, d2):
            assert a.shape == b.shape and a.dtype == np.float64 and (a.size == 0 or np.abs(a - b).max() <= tol)
