"""GPU suite: reduced density matrices above 64 rows of the result tensor on the device (csrc/ctg_rdm_wide.hip,
DESIGN.md section 20) -- ``Executor.rdm_wide_result``, ``HipContractor.rdm_wide``,
``ContractionTree.contract_rdm_wide``, ``ContractExpression.rdm_wide``, ``circuits.entanglement_spectrum`` /
``entanglement_entropy``.

Data reaches the result tensor bit for bit through a one-tensor tree, as in tests/test_gpu_rdm.py.  Reference and
tolerance are tests/rdm_util.py's ``check_rdm``: per real component ``2 (m + 1) 2^-53 sqrt(ref[a,a] ref[b,b])``, derived
and never tuned; no entry is excluded.

The power-of-two route works on 64-row panels in chunks of 32 values of r; ``splits`` doubles while blocks * splits <
512 and a split keeps 32 chunks.  The shapes below are the smallest at which each piece can go wrong: less than one
chunk of columns (t = 1, 16), one off-diagonal block (D = 128), splits > 1 (t = 8192 at D = 128), many blocks with one
split (D = 1024), kept bits high / low / interleaved, axes of mixed width, and the general route."""
import ctypes as C

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime

import rdm_util as du
import reduce_util as ru
from test_gpu_result_reduce import resident
from test_gpu_sample import gaussian, random_circuit, statevector

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "complex64", "complex128"]


def wide(dtype):
    return np.complex128 if np.dtype(dtype).kind == "c" else np.float64


def bits_request(L, bits):
    """``(shape, keep flags, kept axes in the tensor's order)`` for kept ``bits`` of the flat index of 2^L elements."""
    axes = sorted(L - 1 - b for b in bits)
    return (2,) * L, [1 if a in axes else 0 for a in range(L)], axes


def axes_request(shape, keep):
    return tuple(shape), [1 if a in keep else 0 for a in range(len(shape))], sorted(keep)


def check_case(dtype, shape, flags, axes, seed, route):
    n = int(np.prod(shape))
    x = gaussian(n, dtype, seed=seed)
    ex = resident(x)
    plan = runtime.rdm_wide_plan(dtype, shape, flags)
    assert plan.route == route
    name = ex.rdm_wide_variant(shape, flags)
    assert name == runtime.rdm_wide_variant(dtype, shape, flags)
    assert name.startswith("rdm_wide_kernel<" if route == 0 else "rdm_wide_general_kernel<")
    rho, purity = ex.rdm_wide_result(shape, flags)
    d = plan.dim
    assert rho.shape == (d, d) and rho.dtype == wide(dtype)
    du.check_rdm(rho, x, shape, axes)
    assert np.array_equal(rho, rho.conj().T)                      # exactly Hermitian
    assert np.all(np.diag(rho).imag == 0)
    # the purity: a fixed-order fp64 sum of D^2 squares, each rounded (twice for complex) before it is added
    host = float(np.sum(np.abs(rho) ** 2))
    assert abs(purity - host) <= (d * d + 1) * 2.0 ** -53 * host
    none, again = ex.rdm_wide_result(shape, flags, matrix=False)
    assert none is None and again == purity                       # the same bits without the download
    assert ex.download_result().tobytes() == x.tobytes()
    return plan, x, ex, rho


POW2 = {
    "D128_t32": lambda: bits_request(12, range(5, 12)),                       # t = 32: one chunk; one off-diagonal block
    "D256_interleaved": lambda: bits_request(14, [0, 2, 4, 6, 8, 10, 12, 13]),
    "D128_low": lambda: bits_request(16, range(0, 7)),
    "D512_high": lambda: bits_request(18, range(9, 18)),
    "D128_t8192": lambda: bits_request(20, range(13, 20)),
    "mixed_128": lambda: axes_request((4, 8, 1, 2, 16, 8), (1, 4)),
    "mixed_512": lambda: axes_request((4, 8, 1, 2, 16, 8), (0, 1, 3, 5)),   # t = 16: half a chunk of columns
    "mixed2_128": lambda: axes_request((2, 64, 4, 128, 2, 4, 2, 2), (3,)),
    "mixed2_512": lambda: axes_request((2, 64, 4, 128, 2, 4, 2, 2), (1, 5, 6)),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(POW2))
def test_power_of_two_route(case, dtype):
    shape, flags, axes = POW2[case]()
    plan, _, _, _ = check_case(dtype, shape, flags, axes, seed=len(case) + len(shape), route=0)
    assert plan.edge == 64
    if case == "D128_t8192":
        assert plan.splits > 1
    if case == "D128_t32":
        assert (plan.panels, plan.blocks, plan.chunks, plan.splits) == (2, 3, 1, 1)


def test_all_axes_kept_4096_rows():
    """t = 1: a chunk holds one column of the 32; 2080 blocks."""
    shape, flags, axes = bits_request(12, range(12))
    plan, x, _, rho = check_case("complex64", shape, flags, axes, seed=4096, route=0)
    assert (plan.dim, plan.cols, plan.blocks, plan.splits) == (4096, 1, 2080, 1)
    X = x.astype(np.complex128).reshape(4096, 1)
    assert np.array_equal(rho, X * X.conj().T)                    # one product (two, rounded once) per entry


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_many_blocks_one_split(dtype):
    shape, flags, axes = bits_request(20, range(10, 20))
    plan, _, _, _ = check_case(dtype, shape, flags, axes, seed=1024, route=0)
    assert (plan.dim, plan.blocks, plan.splits) == (1024, 136, 1)


GENERAL = {
    "3^8_keep5": lambda: axes_request((3,) * 8, range(5)),                      # D = 243
    "primes": lambda: axes_request((5, 7, 11, 13), (1, 3)),                     # D = 91
    "2^11_keep7": lambda: bits_request(11, [0, 2, 3, 5, 8, 9, 10]),             # a power of two below 4096 elements
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(GENERAL))
def test_general_route(case, dtype):
    shape, flags, axes = GENERAL[case]()
    check_case(dtype, shape, flags, axes, seed=len(case), route=1)


def test_general_route_2187_rows():
    shape, flags, axes = axes_request((3,) * 8, range(1, 8))
    plan, _, _, _ = check_case("complex64", shape, flags, axes, seed=2187, route=1)
    assert (plan.dim, plan.chunks) == (2187, 1)


def half_integers(n, dtype, seed):
    """values k / 2, |k| <= 8: products are multiples of 1/4 up to 16, every partial sum is exact in fp64"""
    return (np.clip(np.round(2 * gaussian(n, dtype, seed=seed)), -8, 8) / 2).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_half_integers_are_exact(dtype):
    """Bit for bit against numpy, whatever the order: pins the lane maps of the f64 fragments, the places in LDS, the
    block and split bookkeeping (splits = 8 in the first case, four panels in the second) and the mirror."""
    for (shape, flags, axes), route in [(bits_request(20, [0, 3, 4, 9, 13, 18, 19]), 0), (bits_request(16, range(4, 12)), 0),
                                        (axes_request((3,) * 8, (0, 2, 3, 5, 7)), 1)]:
        x = half_integers(int(np.prod(shape)), dtype, seed=len(shape))
        ex = resident(x)
        assert runtime.rdm_wide_plan(dtype, shape, flags).route == route
        rho, purity = ex.rdm_wide_result(shape, flags)
        ref = du.rdm_reference(x, shape, axes)
        assert np.array_equal(rho, ref), (shape, float(np.abs(rho - ref).max()))
    assert runtime.rdm_wide_plan(dtype, *bits_request(20, [0, 3, 4, 9, 13, 18, 19])[:2]).splits == 8


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_diagonal_is_the_marginal_and_a_host_trace_is_the_narrow_matrix(dtype):
    L = 14
    bits = [0, 2, 4, 6, 8, 10, 12, 13]
    shape, flags, axes = bits_request(L, bits)
    x = gaussian(2 ** L, dtype, seed=14)
    ex = resident(x)
    rho, _ = ex.rdm_wide_result(shape, flags)
    ref = du.rdm_reference(x, shape, axes)
    t = 2 ** L // 256
    tol = du.rdm_tol(ref, t)
    marg = ex.marginal_result(shape, flags)
    assert np.all(np.abs(np.diag(rho).real - marg) <= np.diag(tol) + ru.marginal_tol(marg, t))
    # trace the kept axes 1 and 6 (of the eight, in the tensor's order) out on the host: 64 rows are left
    r8 = rho.reshape((2,) * 16)
    traced = np.einsum("abcdefghAbCDEFgH->acdefhACDEFH", r8).reshape(64, 64)
    left = [a for i, a in enumerate(axes) if i not in (1, 6)]
    # (an entry is a sum of four wide entries whose bounds add up to at most the narrow bound by Cauchy-Schwarz, with
    # m four times smaller; the three host additions fit the slack)
    nref = du.check_rdm(traced, x, shape, left)
    narrow = ex.rdm_result(shape, [1 if a in left else 0 for a in range(L)])
    du.check_rdm(narrow, x, shape, left, ref=nref)
    assert np.all(du.rdm_errors(traced, narrow) <= 2 * du.rdm_tol(nref, 2 ** L // 64))


def test_deterministic_across_runs_executors_and_reuse():
    L = 16
    x, y = gaussian(2 ** L, "complex64", seed=61), gaussian(2 ** L, "complex64", seed=62)
    reqs = [bits_request(L, b)[:2] for b in [range(9, 16), [0, 1, 5, 6, 7, 12, 13, 15], range(0, 9)]]
    z = gaussian(3 ** 8, "complex64", seed=63)
    gen = axes_request((3,) * 8, range(5))[:2]

    def answers(ex, requests):
        out = []
        for s, f in requests:
            rho, purity = ex.rdm_wide_result(s, f)
            out.append((rho.tobytes(), purity))
        return out

    ex = resident(x)
    first = answers(ex, reqs)
    assert answers(ex, reqs) == first                             # a second run
    ex.topk_result(300)
    ex.marginal_result((2 ** L,), [0])
    ex.marginal_result((16, 2 ** 12), [1, 0])
    assert answers(ex, reqs) == first                             # after a top-k and marginals in the same scratch
    assert answers(resident(y), reqs) != first
    assert answers(resident(x), reqs) == first                    # a fresh executor
    g = answers(resident(z), [gen])
    assert answers(resident(z), [gen]) == g
    # through reuse=True
    tree = ca.ContractionTree(["abc"], "abc", {"a": 128, "b": 64, "c": 8})
    xs = x.reshape(128, 64, 8)
    fresh = tree.contract_rdm_wide([xs], ["c", "a"])
    again = tree.contract_rdm_wide([], ["c", "a"], reuse=True)
    assert again.rho.tobytes() == fresh.rho.tobytes() and again.purity == fresh.purity and again.norm == fresh.norm
    tree.contract_topk([], 5, reuse=True)
    assert tree.contract_rdm_wide([], ["c", "a"], reuse=True, matrix=False).purity == fresh.purity
    # the caller's order of rows and columns
    du.check_rdm(fresh.rho, xs, (128, 64, 8), [2, 0])
    assert fresh.dims == (8, 128) and fresh.exponent == 0.0
    ac = tree.contract_rdm_wide([], ["a", "c"], reuse=True)
    perm = np.arange(1024).reshape(128, 8).T.reshape(-1)
    assert np.array_equal(fresh.rho, ac.rho[np.ix_(perm, perm)])
    # the narrow matrix can read what the wide call left, and the other way round
    small = tree.contract_rdm([], ["c"], reuse=True)
    du.check_rdm(small.rho, xs, (128, 64, 8), [2])
    assert tree.contract_rdm_wide([], ["c", "a"], reuse=True).rho.tobytes() == fresh.rho.tobytes()


def test_refusals():
    lib = runtime.load()
    n = 2 ** 14
    x = gaussian(n, "complex64", seed=13)
    ex = resident(x)
    before = ex.device_bytes()
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    for shape, words in (((64, 256), (b"CTG_RDM_MAX_DIM", b"ctg_exec_result_rdm")), ((8192, 2), (b"CTG_RDM_WIDE_MAX_DIM",))):
        with pytest.raises(ValueError):
            ex.rdm_wide_result(shape, [1, 0])
        ext, kp = np.array(shape, np.int64), np.array([1, 0], np.int32)
        out = np.full(16, 7.0 + 7.0j, np.complex128)
        pur = C.c_double(-3.0)
        rc = lib.ctg_exec_result_rdm_wide(ex.handle, 2, ext.ctypes.data_as(i64p), kp.ctypes.data_as(i32p),
                                          C.c_void_p(out.ctypes.data), C.byref(pur))
        assert rc == -1 and all(w in lib.ctg_last_error() for w in words)
        assert np.all(out == 7.0 + 7.0j) and pur.value == -3.0
    ext, kp = np.array([128, 128], np.int64), np.array([1, 0], np.int32)
    rc = lib.ctg_exec_result_rdm_wide(ex.handle, 2, ext.ctypes.data_as(i64p), kp.ctypes.data_as(i32p), None, None)
    assert rc == -1 and b"both null" in lib.ctg_last_error()
    for bad_ext, bad_keep in (([n // 2, 3], [1, 0]), ([128, 128], [2, 0]), ([128, 128, 0], [1, 0, 1]), ([128, 128], [-1, 0])):
        with pytest.raises(ValueError):
            ex.rdm_wide_result(bad_ext, bad_keep)
    assert ex.device_bytes() == before                            # (not even the scratch was allocated)
    rho, _ = ex.rdm_wide_result((128, 128), [1, 0])
    du.check_rdm(rho, x, (128, 128), [0])
    assert ex.device_bytes() >= before + runtime.rdm_wide_plan("complex64", (128, 128), [1, 0]).scratch_bytes
    # the narrow entry still refuses what this one takes
    with pytest.raises(ValueError):
        ex.rdm_result((128, 128), [1, 0])
    # a NaN member: CTG_E_NORM
    bad = x.copy()
    bad[4097] = np.nan
    ext = np.array([128, 128], np.int64)
    pur = C.c_double(-3.0)
    rc = lib.ctg_exec_result_rdm_wide(resident(bad).handle, 2, ext.ctypes.data_as(i64p), kp.ctypes.data_as(i32p), None,
                                      C.byref(pur))
    assert rc == -6 and pur.value == -3.0
    with pytest.raises(ValueError):
        ca.ContractionTree(["ab"], "ab", {"a": 128, "b": 128}).contract_rdm_wide([bad.reshape(128, 128)], ["a"])
    # an all-zero tensor: a zero matrix and purity 0, on both routes
    for shape, keep in (((128, 64), [1, 0]), ((81, 27), [1, 0])):
        z, p = resident(np.zeros(int(np.prod(shape)), "complex64")).rdm_wide_result(shape, keep)
        assert z.shape == (shape[0],) * 2 and not z.any() and p == 0.0


def sliced_circuit_tree(n, gates, dtype):
    from cotengra_amd.interface import array_contract_tree

    inputs, output, size_dict, arrays = circuits.circuit_to_network(n, gates, "?" * n, simplify=True, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize="greedy")
    inner = [ix for ix in sorted(size_dict) if ix not in output]
    for ix in inner[:3]:
        tree.remove_ind_(ix)
    return tree, arrays, output


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_through_the_layers_on_a_sliced_tree(dtype):
    n = 12
    gates = random_circuit(n, 6, seed=12)
    psi = statevector(n, gates)
    tree, arrays, output = sliced_circuit_tree(n, gates, dtype)
    assert tree.nslices == 8
    rel = 1e-10 if dtype == "complex128" else 1e-5                # the library's promise per amplitude
    qs = [9, 0, 4, 11, 2, 6, 7]
    r = tree.contract_rdm_wide(arrays, [output[q] for q in qs])
    ref = du.rdm_reference(psi, (2,) * n, qs)
    d = np.sqrt(np.diag(ref).real)
    assert r.rho.shape == (128, 128) and r.dims == (2,) * 7
    assert np.all(np.abs(r.rho - ref) <= 4 * rel * np.outer(d, d))
    assert abs(np.trace(r.rho).real - r.norm) <= 1e-12 * r.norm and abs(r.norm - 1) <= 4 * rel
    # what the result tensor holds, to the derived bound
    amps = np.asarray(tree.contract(arrays))
    again = tree.contract_rdm_wide(arrays, [output[q] for q in qs])
    du.check_rdm(again.rho, amps, amps.shape, qs)
    assert again.rho.tobytes() == r.rho.tobytes() and again.purity == r.purity
    # strip_exponent: the mantissa's matrix and purity, the exponent next to them
    s = tree.contract_rdm_wide(arrays, [output[q] for q in qs], strip_exponent=True)
    assert np.all(np.abs(s.rho * 10.0 ** (2 * s.exponent) - ref) <= 4 * rel * np.outer(d, d))
    assert abs(s.purity * 10.0 ** (4 * s.exponent) - r.purity) <= 16 * rel * r.purity


def test_expression_rdm_wide():
    from cotengra_amd import interface

    rng = np.random.default_rng(72)
    a, b = rng.standard_normal((160, 7)), rng.standard_normal((7, 20))
    interface.clear_expression_cache()
    try:
        expr = ca.einsum_expression("ab,bc->ac", a.shape, b.shape, cache_expression=True)
        out = np.asarray(expr(a, b))
        before = expr._bytes
        r = expr.rdm_wide(a, b, keep=["a"])
        du.check_rdm(r.rho, out, out.shape, [0])
        assert r.rho.dtype == np.float64 and r.dims == (160,)
        assert expr._bytes == expr.device_bytes() > before     # (the scratch is counted)
        with pytest.raises(ValueError):
            expr.rdm_wide(a, b, keep=[["a"], ["c"]])
    finally:
        interface.clear_expression_cache()


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_circuit_entanglement(dtype, monkeypatch):
    calls = []
    narrow, wide_ = runtime.Executor.rdm_result, runtime.Executor.rdm_wide_result
    monkeypatch.setattr(runtime.Executor, "rdm_result",
                        lambda self, e, k: (calls.append(self.rdm_variant(e, k)), narrow(self, e, k))[1])
    monkeypatch.setattr(runtime.Executor, "rdm_wide_result",
                        lambda self, e, k, matrix=True: (calls.append((self.rdm_wide_variant(e, k), matrix)),
                                                         wide_(self, e, k, matrix=matrix))[1])
    n = 14
    gates = random_circuit(n, 6, seed=14)
    psi = statevector(n, gates)
    rel = 1e-10 if dtype == "complex128" else 1e-5                # the library's promise per amplitude
    tag = "c64" if dtype == "complex64" else "c128"
    cut = list(range(7))
    D = 128
    lam_ref = np.linalg.eigvalsh(du.rdm_reference(psi, (2,) * n, cut))[::-1]
    lam, norm = circuits.entanglement_spectrum(n, gates, cut, dtype=dtype)
    assert calls == [(f"rdm_wide_kernel<{tag},64>", True)]
    assert lam.shape == (D,) and np.all(lam[:-1] >= lam[1:]) and lam[-1] >= 0 and abs(lam.sum() - 1) <= 1e-12
    assert abs(norm - 1) <= 4 * rel
    # every entry of rho is within 4 rel sqrt(rho[a,a] rho[b,b]): the Frobenius norm of the difference is at most 4 rel
    # trace, and no eigenvalue moves further (Weyl); rel * D is above that
    assert np.all(np.abs(lam - lam_ref) <= rel * D)
    # Renyi-2 from the device purity alone: the relative error of the purity is at most 2 * 4 rel / sqrt(purity) <=
    # 8 rel sqrt(D), that of norm^2 at most 8 rel
    del calls[:]
    s2, _ = circuits.entanglement_entropy(n, gates, cut, alpha=2, dtype=dtype)
    assert calls == [(f"rdm_wide_kernel<{tag},64>", False)]
    assert abs(s2 - -np.log2(np.sum(lam_ref ** 2))) <= 16 * rel * np.sqrt(D) / np.log(2)
    assert abs(s2 - -np.log2(np.sum(lam ** 2))) <= 16 * rel * np.sqrt(D) / np.log(2)
    # von Neumann: eta(l) = -l log2 l moves by at most eta(delta) when l moves by delta <= 1/2
    s1, _ = circuits.entanglement_entropy(n, gates, cut, dtype=dtype)
    nz = lam_ref[lam_ref > 0]
    eta = lambda v: -v * np.log2(v)   # noqa: E731
    assert abs(s1 - float(np.sum(eta(nz)))) <= 2 * D * eta(4 * rel)
    # the larger side is swapped for the smaller one: the same spectrum from the same kernel
    lam2, _ = circuits.entanglement_spectrum(n, gates, list(range(7, 14)), dtype=dtype)
    assert np.all(np.abs(lam2 - lam_ref) <= rel * D)
    # a 10-qubit state cut 3 | 7 goes through the narrow entry, from either side
    g10 = random_circuit(10, 5, seed=10)
    psi10 = statevector(10, g10)
    ref10 = np.linalg.eigvalsh(du.rdm_reference(psi10, (2,) * 10, [0, 1, 2]))[::-1]
    for side in ([0, 1, 2], list(range(3, 10))):
        del calls[:]
        l10, _ = circuits.entanglement_spectrum(10, g10, side, dtype=dtype)
        assert calls == [f"rdm_general_kernel<{tag}>"]          # (2^10 elements: below the chunk route's 4096)
        assert l10.shape == (8,) and np.all(np.abs(l10 - ref10) <= rel * 8)
