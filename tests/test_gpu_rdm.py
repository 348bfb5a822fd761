"""GPU suite: reduced density matrices of the result tensor on the device (csrc/ctg_rdm.hip) --
``Executor.rdm_result``, ``HipContractor.rdm``, ``ContractionTree.contract_rdm``, ``ContractExpression.rdm``,
``circuits.reduced_density_matrix``.

Data reaches the result tensor bit for bit through a one-tensor tree (a single copy step), as in
tests/test_gpu_result_reduce.py.  Reference and tolerance are in tests/rdm_util.py: per real component
``2 (m + 1) 2^-53 sqrt(ref[a,a] ref[b,b])``, derived from the rounding of two summation orders and never from what the
device returns; no entry is excluded.

The power-of-two route (every extent a power of two, at least 4096 elements) works in chunks of 4096 elements: all
rows (16 at least: for D < 16 the lowest bits of r are folded into the row) by the lowest ``c = 12 - log2(max(D, 16))``
remaining bits of r.  Its grid is ``min(512, ceil(chunks / 3))``: 2^15 elements are 8 chunks on 3 workgroups (two take
three chunks, the last round holds two), 2^22 elements 1024 chunks on 342 workgroups (340 take three, the last round
is partial)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import _tree_contractor

import rdm_util as du
import reduce_util as ru
import sample_util as su
from test_gpu_result_reduce import resident
from test_gpu_sample import gaussian, one_tensor_tree, random_circuit, statevector

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "complex64", "complex128"]
HERE = os.path.dirname(os.path.abspath(__file__))


def wide(dtype):
    return np.complex128 if np.dtype(dtype).kind == "c" else np.float64


def bit_cases(L):
    """Kept bits of the flat index of a tensor of 2^L elements (bit b is axis L - 1 - b of the shape (2,) * L)."""
    cases = [()]
    cases += [tuple(range(L - k, L)) for k in range(1, 7)]            # 1 ... 6 kept bits at the top
    cases += [tuple(range(k)) for k in range(1, 7)]                   # ... at the bottom
    cases += [(0, L - 1), (1, 4, L - 2), (0, 1, 2, L - 3, L - 2, L - 1), (2, 3, 7, L - 1)]   # split
    # straddling the chunk boundary: with d kept bits below it the chunk ends above bit 11; D = 4: the bits of r
    # below and above c = 8 + 2 folded (9, 10 of the flat index when the kept bits lie higher), D = 64: c = 6; and
    # the two bits around the 4096-element block
    cases += [(9, 10), (10, 11), (5, 6), (11, 12), (5, 6, 11, 12), (4, 5, 6, 7, 11, 12), (6, 7, 8, 9, 10, 11)]
    out = []
    for c in cases:
        if all(0 <= b < L for b in c) and len(set(c)) == len(c) and tuple(sorted(c)) not in out:
            out.append(tuple(sorted(c)))
    return out


def qubit_request(L, bits):
    """``(shape, keep flags, kept axes in the tensor's order)`` for kept ``bits`` of 2^L elements."""
    axes = sorted(L - 1 - b for b in bits)
    return (2,) * L, [1 if a in axes else 0 for a in range(L)], axes


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [6, 12, 13, 15, 22])
def test_power_of_two_shapes_against_the_reference(L, dtype):
    """2^6: below the fast route's lower bound of 4096 elements (the general route); 2^12: one chunk; 2^13: two chunks
    on one workgroup; 2^15: three workgroups, the last round partial; 2^22: 342 workgroups of three chunks, the last
    round partial."""
    n = 2 ** L
    x = gaussian(n, dtype, seed=100 + L)
    ex = resident(x)
    p = su.probabilities(x)
    for bits in bit_cases(L):
        shape, flags, axes = qubit_request(L, bits)
        got = ex.rdm_result(shape, flags)
        assert got.shape == (2 ** len(bits),) * 2 and got.dtype == wide(dtype)
        if not bits:
            # no axis kept: rho[0, 0] is the norm, within the marginal's tolerance
            assert abs(got[0, 0] - p.sum()) <= ru.marginal_tol(p.sum(), n)
            assert np.imag(got[0, 0]) == 0
        du.check_rdm(got, x, shape, axes)
        assert np.array_equal(got, got.conj().T)
    assert ex.download_result().tobytes() == x.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_axes_kept_is_the_outer_product_bit_for_bit(dtype):
    """n = 64, all six axes kept: t = 1.  The data are float32 values in every dtype, so each product is exactly
    representable in fp64 and an entry is one product (real) or the once-rounded sum of two (complex): the same
    double on the device and in numpy."""
    x = gaussian(64, "complex64" if np.dtype(dtype).kind == "c" else "float32", seed=64).astype(dtype)
    ex = resident(x)
    got = ex.rdm_result((2,) * 6, [1] * 6)
    X = x.astype(wide(dtype)).reshape(64, 1)
    assert np.array_equal(got, X * X.conj().T)
    assert np.array_equal(got, du.rdm_reference(x, (2,) * 6, list(range(6))))
    assert np.array_equal(ex.rdm_result((64,), [1]), got) and np.array_equal(ex.rdm_result((4, 16), [1, 1]), got)


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_power_of_two_axes_of_mixed_width(dtype):
    """Axes of extent 4, 8, 1, 2 ...: the bits of an axis move together; kept extents up to 64."""
    for shape in [(4, 8, 1, 2, 16, 8), (2, 64, 4, 128, 2, 4, 2, 2)]:
        n = int(np.prod(shape))
        x = gaussian(n, dtype, seed=n % 1000)
        ex = resident(x)
        rank = len(shape)
        keeps = [(a,) for a in range(rank)] + [(0, rank - 1), (1, 3), (0, 2, 5), (2, 3)]
        for keep in keeps:
            if int(np.prod([shape[a] for a in keep])) > 64:
                with pytest.raises(ValueError):
                    ex.rdm_result(shape, [1 if a in keep else 0 for a in range(rank)])
                continue
            du.check_rdm(ex.rdm_result(shape, [1 if a in keep else 0 for a in range(rank)]), x, shape, keep)


@pytest.mark.parametrize("dtype", DTYPES)
def test_general_route(dtype):
    cases = [((3, 5, 7, 4), [(0,), (1,), (2,), (3,), (0, 2)]), ((3, 5, 7, 11, 13), [(1, 3)]),
             ((2,) * 11, [(0,), (10,), (2, 9), (0, 1, 2, 8, 9, 10)]),      # a power of two below 4096 elements
             ((2 ** 20 + 3,), [()])]                                       # several chunks of r per pair
    for shape, keeps in cases:
        n = int(np.prod(shape))
        x = gaussian(n, dtype, seed=n % 997)
        ex = resident(x)
        for keep in keeps:
            flags = [1 if a in keep else 0 for a in range(len(shape))]
            assert ex.rdm_variant(shape, flags).startswith("rdm_general_kernel<")
            got = ex.rdm_result(shape, flags)
            du.check_rdm(got, x, shape, keep)
            assert np.array_equal(got, got.conj().T)
    x = gaussian(15015, dtype, seed=3)
    assert resident(x).rdm_result((3, 5, 7, 11, 13), [0, 1, 0, 1, 0]).shape == (55, 55)


@pytest.mark.parametrize("dtype", DTYPES)
def test_half_integers_are_exact(dtype):
    """round(2 gaussian) / 2 at 2^20 elements: every product is a multiple of 1/4 below 2^6 and every partial sum of
    2^21 of them is exact in fp64, so the device must equal numpy whatever the order -- which pins the lane maps of
    the f64 fragments, the folding for D < 16 and the places in LDS harder than any tolerance."""
    L = 20
    x = (np.round(2 * gaussian(2 ** L, dtype, seed=7)) / 2).astype(dtype)
    ex = resident(x)
    for bits in [(18, 19), (0, 1), (0, 19), (5, 12), (14, 15, 16, 17, 18, 19), (0, 1, 2, 3, 4, 5), (0, 1, 2, 17, 18, 19),
                 (1, 5, 6, 11, 12, 18), (3, 9, 16), (2, 4, 11, 13, 19)]:
        shape, flags, axes = qubit_request(L, bits)
        assert ex.rdm_variant(shape, flags).startswith("rdm_chunk_kernel<")
        got = ex.rdm_result(shape, flags)
        ref = du.rdm_reference(x, shape, axes)
        assert np.array_equal(got, ref), (bits, float(np.abs(got - ref).max()))


def structure_case(dtype, D_bits):
    L = 18
    x = gaussian(2 ** L, dtype, seed=33)
    shape = (2 ** D_bits[0], 2 ** (L - D_bits[0] - D_bits[1]), 2 ** D_bits[1])
    tree = ca.ContractionTree(["abc"], "abc", dict(zip("abc", shape)))
    return x.reshape(shape), shape, tree


@pytest.mark.parametrize("dtype", ["complex64", "float64", "complex128"])
@pytest.mark.parametrize("D_bits", [(1, 1), (3, 3), (2, 3)])
def test_hermitian_positive_and_consistent_with_the_marginal(D_bits, dtype):
    x, shape, tree = structure_case(dtype, D_bits)
    r = tree.contract_rdm([x], ["a", "c"])
    rho, D = r.rho, shape[0] * shape[2]
    assert rho.shape == (D, D) and r.dims == (shape[0], shape[2]) and r.exponent == 0.0
    assert np.array_equal(rho, rho.conj().T)                      # the other half is the conjugate, exactly
    assert np.all(np.diag(rho).imag == 0)                         # (for a real plan rho is float64)
    t = x.size // D
    tol = du.rdm_tol(du.rdm_reference(x, shape, [0, 2]), t)
    assert np.linalg.eigvalsh(rho).min() >= -D * tol.max()
    # the diagonal is the marginal: within the sum of the two bounds, on the same result
    m = tree.contract_marginal([], ["a", "c"], reuse=True)
    diag = np.diag(rho).real.reshape(shape[0], shape[2])
    assert np.all(np.abs(diag - m.p) <= np.diag(tol).reshape(diag.shape) + ru.marginal_tol(m.p, t))
    # norm is the one of the statistics passes
    st = _tree_contractor(tree)._reusable[0]
    assert r.norm == m.norm == st["exec"].sample_info()[0]
    assert abs(np.trace(rho).real - r.norm) <= D * tol.max() + ru.marginal_tol(r.norm, x.size)
    # the caller's order
    ca_ = tree.contract_rdm([], ["c", "a"], reuse=True)
    perm = np.arange(D).reshape(shape[0], shape[2]).T.reshape(-1)
    assert ca_.dims == (shape[2], shape[0]) and np.array_equal(ca_.rho, rho[np.ix_(perm, perm)])


def test_deterministic_across_runs_and_executors():
    L = 16
    x, y = gaussian(2 ** L, "complex64", seed=41), gaussian(2 ** L, "complex64", seed=42)
    reqs = [qubit_request(L, b)[:2] for b in [(0, 15), (3, 4, 5, 12, 13, 14), (7,), ()]]
    z = gaussian(3 * 5 * 7 * 11, "complex64", seed=43)

    def answers(ex, gen=False):
        if gen:
            return [ex.rdm_result((3, 5, 7, 11), f).tobytes() for f in ([1, 0, 1, 0], [0, 1, 0, 1])]
        return [ex.rdm_result(s, f).tobytes() for s, f in reqs]

    ex = resident(x)
    first = answers(ex)
    assert answers(ex) == first                                   # a second run
    ex.topk_result(300)
    ex.marginal_result((2 ** L,), [0])
    ex.marginal_result((16, 2 ** 12), [1, 0])
    assert answers(ex) == first                                   # after a top-k and marginals in the same scratch
    assert answers(resident(y)) != first
    assert answers(resident(x)) == first                          # a fresh executor
    g = answers(resident(z), gen=True)
    assert answers(resident(z), gen=True) == g


def test_refusals():
    n = 2 ** 13
    x = gaussian(n, "complex64", seed=13)
    ex = resident(x)
    before = ex.device_bytes()
    # D = 128: refused by the binding, and by the library itself
    with pytest.raises(ValueError):
        ex.rdm_result((128, 64), [1, 0])
    ext, kp = np.array([128, 64], np.int64), np.array([1, 0], np.int32)
    out = np.zeros((128, 128), np.complex128)
    rc = runtime.load().ctg_exec_result_rdm(ex.handle, 2, ext.ctypes.data_as(C.POINTER(C.c_int64)),
                                            kp.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(out.ctypes.data))
    assert rc == -1 and b"CTG_RDM_MAX_DIM" in runtime.load().ctg_last_error() and not out.any()
    for bad_ext, bad_keep in (([n // 2, 3], [1, 0]), ([n], [2]), ([n, 0], [1, 1]), ([n], [-1])):
        with pytest.raises(ValueError):
            ex.rdm_result(bad_ext, bad_keep)
    # extents whose running product passes 2^40 elements before the last axis
    ext, kp = np.array([2 ** 21, 2 ** 21, 2], np.int64), np.array([0, 0, 1], np.int32)
    out = np.full((2, 2), 7.0 + 7.0j, np.complex128)
    rc = runtime.load().ctg_exec_result_rdm(ex.handle, 3, ext.ctypes.data_as(C.POINTER(C.c_int64)),
                                            kp.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(out.ctypes.data))
    assert rc == -1 and runtime.load().ctg_last_error() and np.all(out == 7.0 + 7.0j)
    assert ex.device_bytes() == before                            # (not even the scratch was allocated)
    du.check_rdm(ex.rdm_result((64, 128), [1, 0]), x, (64, 128), [0])
    assert ex.device_bytes() > before
    assert ex.download_result().tobytes() == x.tobytes()
    # a NaN member
    tree = one_tensor_tree(n)
    bad = x.copy()
    bad[4097] = np.nan
    with pytest.raises(ValueError):
        tree.contract_rdm([bad], [])
    # an all-zero tensor: a zero matrix, no error
    for shape, keep in (((64, 128), [1, 0]), ((3, 5), [0, 1])):
        z = resident(np.zeros(int(np.prod(shape)), "complex64")).rdm_result(shape, keep)
        assert z.shape == (shape[0 if keep[0] else 1],) * 2 and not z.any()
    # reuse=True after a call that leaves no result to read
    t2 = ca.ContractionTree.from_path([("a", "b"), ("b", "c")], ("a", "c"), {"a": 32, "b": 7, "c": 24}, path=[(0, 1)])
    rng = np.random.default_rng(51)
    xs = [(rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype("complex64") for s in ((32, 7), (7, 24))]
    fresh = t2.contract_rdm(xs, ["c"])
    assert t2.contract_rdm([], ["c"], reuse=True).rho.tobytes() == fresh.rho.tobytes()
    t2.contract_topk([], 5, reuse=True)
    assert t2.contract_rdm([], ["c"], reuse=True).rho.tobytes() == fresh.rho.tobytes()
    t2.contract_audit(xs)
    with pytest.raises(RuntimeError):
        t2.contract_rdm([], ["c"], reuse=True)


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_through_the_layers_on_a_sliced_tree(dtype):
    from oracle import contract_ref as orc

    tree = ca.tree_from_record(ca.load_network(os.path.join(HERE, "golden", "trees", "sycamore_m10_open8.json")))
    z = np.load(os.path.join(HERE, "golden", "sycamore_m10_open8_arrays.npz"))
    xs = [z[f"t{i}"].astype(dtype) for i in range(tree.N)]
    assert tree.nslices == 8
    amps = np.asarray(tree.contract(xs))                          # (what the result tensor holds)
    oracle = np.asarray(orc.contract(tree, [a.astype("complex128") for a in xs])).reshape(amps.shape)
    rel = 1e-10 if dtype == "complex128" else 1e-5                # the library's promise per amplitude
    out = list(tree.output)
    shape = amps.shape

    def check(rho, axes):
        du.check_rdm(rho, amps, shape, axes)
        ref = du.rdm_reference(oracle, shape, axes)
        d = np.sqrt(np.diag(ref).real)
        assert np.all(np.abs(rho - ref) <= 4 * rel * np.outer(d, d))

    r = tree.contract_rdm(xs, [out[5], out[2]])
    check(r.rho, [5, 2])
    assert r.dims == (2, 2) and abs(np.trace(r.rho).real - r.norm) <= 1e-12 * r.norm
    # every 2-index matrix from one contraction
    pairs = list(itertools.combinations(range(8), 2))
    many = tree.contract_rdm(xs, [[out[i], out[j]] for i, j in pairs])
    for rho, (i, j) in zip(many.rho, pairs):
        check(rho, [i, j])
    six = tree.contract_rdm([], [out[k] for k in (7, 0, 3, 4, 1, 6)], reuse=True)
    check(six.rho, [7, 0, 3, 4, 1, 6])
    # strip_exponent: the mantissa's matrix and the exponent next to it
    s = tree.contract_rdm(xs, [out[1], out[6]], strip_exponent=True)
    ref = du.rdm_reference(amps, shape, [1, 6])
    d = np.sqrt(np.diag(ref).real)
    assert np.all(np.abs(s.rho * 10.0 ** (2 * s.exponent) - ref) <= 4 * rel * np.outer(d, d))
    assert abs(s.norm * 10.0 ** (2 * s.exponent) - r.norm) <= 4 * rel * r.norm


def test_expression_rdm():
    from cotengra_amd import interface

    rng = np.random.default_rng(71)
    a, b = rng.standard_normal((48, 7)), rng.standard_normal((7, 20))
    interface.clear_expression_cache()
    try:
        expr = ca.einsum_expression("ab,bc->ac", a.shape, b.shape, cache_expression=True)
        out = np.asarray(expr(a, b))
        before = expr._bytes
        r = expr.rdm(a, b, keep=[["c"], ["a"], []])
        du.check_rdm(r.rho[0], out, out.shape, [1])
        du.check_rdm(r.rho[1], out, out.shape, [0])
        du.check_rdm(r.rho[2], out, out.shape, [])
        assert r.rho[0].dtype == np.float64 and r.dims == [(20,), (48,), ()]
        assert expr._bytes == expr.device_bytes() > before     # (the scratch is counted)
        exs = ca.einsum_expression("ab,bc->ac", a.shape, b.shape, strip_exponent=True)
        mant, E = exs(a, b)
        rs = exs.rdm(a, b, keep=["c"])
        du.check_rdm(rs.rho, np.asarray(mant), out.shape, [1])
        assert rs.exponent == E
        exs.close()
    finally:
        interface.clear_expression_cache()


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_circuit_reduced_density_matrix(dtype):
    n = 12
    gates = random_circuit(n, 6, seed=7)
    psi = statevector(n, gates)
    rel = 1e-10 if dtype == "complex128" else 1e-5                # the library's promise per amplitude
    for qs in ([4], [9, 2], [0, 3, 5, 6, 8, 11]):
        rho, norm = circuits.reduced_density_matrix(n, gates, qs, dtype=dtype)
        ref = du.rdm_reference(psi, (2,) * n, qs)
        d = np.sqrt(np.diag(ref).real)
        assert rho.shape == (2 ** len(qs),) * 2 and np.all(np.abs(rho - ref) <= 4 * rel * np.outer(d, d))
        assert abs(np.trace(rho).real - 1) <= 1e-12 and abs(norm - 1) <= 4 * rel
        rest = [q for q in range(n) if q not in qs]
        s_ref = circuits.von_neumann_entropy(du.rdm_reference(psi, (2,) * n, rest))
        assert abs(circuits.von_neumann_entropy(rho) - s_ref) <= 1e-6
        if len(rest) <= 6:
            other, _ = circuits.reduced_density_matrix(n, gates, rest, dtype=dtype)
            assert abs(circuits.von_neumann_entropy(rho) - circuits.von_neumann_entropy(other)) <= 1e-6
            assert abs(circuits.purity(rho) - circuits.purity(other)) <= 1e-6
    # a conditional state: two qubits projected
    fixed = {1: 1, 7: 0}
    rho, norm = circuits.reduced_density_matrix(n, gates, [10, 0], fixed=fixed, dtype=dtype)
    sub = np.take(np.take(psi, 1, axis=1), 0, axis=6)             # (qubit 1 = 1; qubit 7 is axis 6 of what is left)
    open_qubits = [q for q in range(n) if q not in fixed]
    ref = du.rdm_reference(sub, sub.shape, [open_qubits.index(10), open_qubits.index(0)])
    p = float(np.trace(ref).real)
    d = np.sqrt(np.diag(ref).real / p)
    assert abs(norm - p) <= 4 * rel * p and np.all(np.abs(rho - ref / p) <= 4 * rel * np.outer(d, d))
