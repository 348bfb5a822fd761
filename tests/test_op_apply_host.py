"""CPU suite: the host side of dense local operators on the result tensor -- the header and the
binding, ``operator_requests`` (label order, merging, every refusal), the kernel names, a numpy mirror of the definition
of the bits against the ``tensordot`` reference of tests/op_apply_util.py, the Hermiticity gate of ``operator_energy``
and the argument errors of every layer, all raised before a device is touched."""
import os
import re

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import _tree_contractor, operator_requests

import op_apply_util as ou
from test_pauli_apply_host import sliced_circuit_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

X = np.array([[0, 1], [1, 0]], dtype=complex)
Y = np.array([[0, -1j], [1j, 0]], dtype=complex)
Z = np.array([[1, 0], [0, -1]], dtype=complex)


def test_header_declares_the_call_and_the_binding_mirrors_it():
    text = open(os.path.join(ROOT, "include", "ctg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = re.sub(r"\s+", " ", code)
    assert ("int ctg_exec_result_op_apply(ctg_exec* exec, int64_t rank, const int64_t* extents, int64_t m, "
            "const int32_t* naxes, const int32_t* axes, const double* mats, void* dev_out, void* host_out);") in flat
    assert re.search(r"#define\s+CTG_ABI_VERSION\s+10\b", code) and runtime.ABI_VERSION == 10
    for name, value in (("CTG_OP_MAX_DIM", 64), ("CTG_OP_MAX_TERMS", 4096)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", code), name
    assert re.search(r"#define\s+CTG_OP_MAX_ENTRIES\s+\(1 << 20\)", code)
    ex = runtime.Executor
    assert (ex.OP_MAX_DIM, ex.OP_MAX_TERMS, ex.OP_MAX_ENTRIES) == (64, 4096, 1 << 20) and ex.OP_MAX_DIM == ex.RDM_MAX_DIM
    assert "ctg_exec_result_op_apply" in runtime.SYMBOLS and hasattr(runtime.load(), "ctg_exec_result_op_apply")
    assert "ctg_op_apply.hip" in __import__("__graft_entry__").SOURCES
    doc = re.sub(r"\s*\n\s*\*\s*", " ", text)
    for phrase in ("No atomics", "function of (dtype, extents, the terms in order, the tensor's bytes) alone",
                   "each rounded once, nothing fused", "m = 0 writes zeros", "never written", "may be skipped"):
        assert phrase in doc, phrase


def test_methods_exist_on_every_layer():
    from cotengra_amd.interface import ContractExpression

    for name in ("op_apply_result", "op_apply_variant"):
        assert hasattr(runtime.Executor, name)
    assert hasattr(runtime, "op_apply_variant") and hasattr(runtime, "op_apply_terms")
    for name in ("apply_operators", "operator_expectation", "operator_energy", "operator_energy_autograd"):
        assert hasattr(ca.HipContractor, name)
    for name in ("contract_apply_operators", "contract_operator_expectation", "contract_operator_energy"):
        assert hasattr(ca.ContractionTree, name)
    for name in ("apply_operators", "operator_expectation", "operator_energy"):
        assert hasattr(ContractExpression, name)
    assert hasattr(circuits, "operator_expectation") and hasattr(circuits, "operator_energy_gradient")
    assert ca.operator_requests is operator_requests


def pair(rng, d=4, real=False):
    m = rng.standard_normal((d, d))
    return m if real else m + 1j * rng.standard_normal((d, d))


def test_kernel_names_for_the_shapes_of_the_gpu_suite():
    rng = np.random.default_rng(190)
    for dtype, tag in (("float32", "float"), ("float64", "double"), ("complex64", "c64"), ("complex128", "c128")):
        real = np.dtype(dtype).kind != "c"
        for L in (6, 12, 13, 15, 18):
            want = f"op_apply_general_kernel<{tag}>" if L < 12 else f"op_apply_kernel<{tag}>"
            assert runtime.op_apply_variant(dtype, (2,) * L, [((0, L - 1), pair(rng, real=real))]) == want
        assert runtime.op_apply_variant(dtype, (4, 2, 8, 2, 16, 2, 2), [((0, 2), pair(rng, 32, real)), ((4,), pair(rng, 16, real))]) \
            == f"op_apply_kernel<{tag}>"
        assert runtime.op_apply_variant(dtype, (2, 3, 2, 5, 2), [((1, 3), pair(rng, 15, real))]) == f"op_apply_general_kernel<{tag}>"
        assert runtime.op_apply_variant(dtype, (2,) * 10 + (3, 2), [((9, 10), pair(rng, 6, real))]) == f"op_apply_general_kernel<{tag}>"
        assert runtime.op_apply_variant(dtype, (2,) * 13, [((0, 1, 5, 7, 11, 12), pair(rng, 64, real))]) == f"op_apply_kernel<{tag}>"
        assert runtime.op_apply_variant(dtype, (2,) * 13, []) == "none"


def test_terms_are_checked_and_packed():
    rng = np.random.default_rng(191)
    a, b = pair(rng), pair(rng, 6)
    ext, naxes, axes, mats = runtime.op_apply_terms("complex64", (2, 3, 2, 2), [((0, 2), a), ((1, 3), b)])
    assert ext == [2, 3, 2, 2] and naxes.dtype == np.int32 and naxes.tolist() == [2, 2] and axes.tolist() == [0, 2, 1, 3]
    assert mats.dtype == np.float64 and mats.shape == (16 + 36, 2)
    assert np.array_equal(mats[:16, 0] + 1j * mats[:16, 1], a.reshape(-1)) and np.array_equal(mats[16:, 0] + 1j * mats[16:, 1], b.reshape(-1))
    nan = a.copy()
    nan[1, 2] = np.nan
    inf = a.copy()
    inf[0, 0] = 1j * np.inf
    bad = [
        ((2, 0, 2), [((0,), X)]),                                   # an extent below 1
        ((2, 2), [((), np.ones((1, 1)))]),                          # no axis
        ((2, 2), [((2,), X)]), ((2, 2), [((-1,), X)]),              # out of range
        ((2, 2), [((1, 0), a)]), ((2, 2), [((0, 0), a)]),           # not ascending, repeated
        ((2, 2), [((0, 1), X)]), ((2, 2), [((0,), a)]),             # a wrong shape
        ((2, 2), [((0,), np.ones((2, 2, 1)))]),
        ((2, 2), [((0, 1), nan)]), ((2, 2), [((0, 1), inf)]),       # not finite
        ((2,) * 7, [(tuple(range(7)), np.eye(128))]),               # D > 64
        ((2, 2), [((0,), X)] * 4097),                               # too many terms
        ((2,) * 6, [(tuple(range(6)), np.eye(64))] * 257),          # too many entries
        ((2, 2), [((0,), np.array([["a", "b"], ["c", "d"]]))]),     # no numbers
        ((2, 2), [(0, X)]), ((2, 2), [X]),                          # no (axes, matrix) pair
    ]
    for extents, terms in bad:
        with pytest.raises(ValueError):
            runtime.op_apply_terms("complex128", extents, terms)
        with pytest.raises(ValueError):
            runtime.op_apply_variant("complex64", extents, terms)
    # the limits themselves are accepted
    runtime.op_apply_terms("complex64", (2,) * 6, [(tuple(range(6)), np.eye(64))] * 256)
    runtime.op_apply_terms("complex64", (2, 2), [((0,), X)] * 4096)
    # a real plan: an imaginary part is refused, an exactly real complex matrix is taken
    with pytest.raises(ValueError):
        runtime.op_apply_terms("float32", (2, 2), [((0,), Y)])
    with pytest.raises(ValueError):
        runtime.op_apply_variant("float64", (2, 2), [((0,), Y)])
    runtime.op_apply_terms("float64", (2, 2), [((0,), X), ((0, 1), np.kron(Y, Y))])
    # the executor binding refuses before it calls
    ex = runtime.Executor.__new__(runtime.Executor)
    ex.plan = type("P", (), {"dtype": "float32"})()
    ex.handle = None
    for extents, terms in (((2, 2), [((0,), Y)]), ((2, 2), [((1, 0), a)]), ((2, 3), [((0, 1), a)])):
        with pytest.raises(ValueError):
            ex.op_apply_result(extents, terms)


class FakeTree:
    """What ``operator_requests`` reads of a tree."""

    def __init__(self, output, shape):
        self.output, self._shape = tuple(output), tuple(shape)

    def gathered_shape(self):
        return self._shape


def test_requests_are_permuted_to_ascending_axes():
    """A matrix given over the labels in any order equals, after the permutation, ``np.einsum`` of its tensor form."""
    rng = np.random.default_rng(192)
    tree = FakeTree("abcde", (2, 3, 2, 5, 2))
    for labels in (["d", "b"], ["b", "d"], ["e", "a", "c"], ["c", "e", "a"], ["b"], "d"):
        pos = [tree.output.index(ix) for ix in labels]
        dims = tuple(tree._shape[a] for a in pos)
        D = int(np.prod(dims))
        mat = rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D))
        for given in (mat, mat.reshape(dims + dims)):
            several, canon, terms = operator_requests(tree, (labels, given))
            assert several is False and len(canon) == len(terms) == 1
            axes, got = canon[0]
            assert list(axes) == sorted(pos) and got.dtype == np.complex128 and got.shape == (D, D)
            assert terms[0][0] == axes and np.array_equal(terms[0][1], got)
            k = len(pos)
            order = np.argsort(pos)
            rows, cols = "abc"[:k], "xyz"[:k]
            want = np.einsum(rows + cols + "->" + "".join(rows[i] for i in order) + "".join(cols[i] for i in order),
                             mat.reshape(dims + dims)).reshape(D, D)
            assert np.array_equal(got, want)
            # the operator itself is the same: apply both to a random tensor
            x = rng.standard_normal(tree._shape) + 1j * rng.standard_normal(tree._shape)
            assert np.allclose(ou.op_apply_reference(x, x.shape, [(pos, mat)]), ou.op_apply_reference(x, x.shape, [(axes, got)]),
                               rtol=0, atol=1e-13 * D)


def test_requests_on_one_axis_set_are_merged_in_order():
    rng = np.random.default_rng(193)
    tree = FakeTree("abcd", (2, 2, 3, 2))
    m1, m2, m3, m4 = pair(rng), pair(rng), pair(rng, 3), pair(rng)
    several, canon, terms = operator_requests(tree, [(["a", "b"], m1), (["c"], m3), (["b", "a"], m2), (["a", "d"], m4)])
    assert several is True and [c[0] for c in canon] == [(0, 1), (2,), (0, 1), (0, 3)]
    assert [t[0] for t in terms] == [(0, 1), (2,), (0, 3)]
    swapped = m2.reshape(2, 2, 2, 2).transpose(1, 0, 3, 2).reshape(4, 4)
    assert np.array_equal(canon[2][1], swapped) and np.array_equal(terms[0][1], m1 + swapped)
    assert np.array_equal(terms[1][1], m3) and np.array_equal(terms[2][1], m4)
    assert operator_requests(tree, []) == (True, [], [])
    assert operator_requests(tree, [(["a"], X)])[0] is True and operator_requests(tree, (["a"], X))[0] is False


def test_requests_are_refused_on_the_host():
    tree = FakeTree("abcdefgh", (2, 2, 2, 2, 2, 2, 2, 3))
    nan = np.eye(2, dtype=complex)
    nan[0, 1] = np.nan
    bad = [
        (["q"], X),                                  # an unknown label
        (["a", "a"], np.eye(4)),                     # repeated
        ([], np.ones((1, 1))),                       # no label
        (["a", "b"], X), (["h"], X), (["a"], np.ones((2, 2, 2))),     # a wrong shape
        (["a"], nan),
        (list("abcdefg"), np.eye(128)),              # D > 64
        (list("abcdeh"), np.eye(96)),
        5, "ab", (["a"], "XX"), (["a"],),
    ]
    for req in bad:
        with pytest.raises(ValueError):
            operator_requests(tree, req)
        with pytest.raises(ValueError):
            operator_requests(tree, [(["a"], X), req])
    # a label that is no output index of a real tree (an inner index)
    real_tree, _ = sliced_circuit_tree()
    inner = next(ix for term in real_tree.inputs for ix in term if ix not in real_tree.output)
    with pytest.raises(ValueError):
        operator_requests(real_tree, ([inner], X))
    # the entry limit: 257 distinct axis sets of D = 64 need 14 axes; the count limit is reached through the runtime
    wide = FakeTree([f"i{k}" for k in range(14)], (2,) * 14)
    import itertools

    sets = list(itertools.islice(itertools.combinations(wide.output, 6), 257))
    with pytest.raises(ValueError, match="entries"):
        operator_requests(wide, [(list(s), np.eye(64)) for s in sets])
    operator_requests(wide, [(list(s), np.eye(64)) for s in sets[:256]])


@pytest.mark.parametrize("dtype", ["float32", "float64", "complex64", "complex128"])
def test_the_definition_of_the_bits_is_exact_on_half_integers(dtype):
    """The numpy mirror of the kernel's arithmetic (``bits_mirror``) on half-integer amplitudes in [-2, 2] and matrix
    entries that are multiples of 1/4 in [-2, 2]: every partial sum is exact, so it equals the ``tensordot`` reference
    bit for bit -- in every shape class of the GPU suite, extents other than 2 included."""
    rng = np.random.default_rng(194)
    cplx = np.dtype(dtype).kind == "c"

    def quarter(d):
        m = rng.integers(-8, 9, size=(d, d)) / 4.0
        return m + 1j * rng.integers(-8, 9, size=(d, d)) / 4.0 if cplx else m

    for shape, terms in (((2,) * 6, [((0, 1), quarter(4)), ((5,), quarter(2)), ((1, 3, 4), quarter(8)), ((0, 1), quarter(4))]),
                         ((2, 3, 2, 5, 2), [((1, 3), quarter(15)), ((0,), quarter(2))]),
                         ((4, 2, 8), [((0, 2), quarter(32)), ((1,), np.diag(np.diag(quarter(2))))])):
        n = int(np.prod(shape))
        x = rng.integers(-4, 5, size=n) / 2.0
        if cplx:
            x = x + 1j * rng.integers(-4, 5, size=n) / 2.0
        x = (x + 0.0).astype(dtype)
        got = ou.bits_mirror(x, shape, terms, dtype)
        ref = ou.op_apply_reference(x, shape, terms)
        assert got.dtype == np.dtype(dtype) and np.array_equal(ref.astype(dtype).astype(ref.dtype), ref)
        assert np.array_equal(got, ref.astype(dtype))
        # and on Gaussian data the mirror stays within the derived bound of the reference
        g = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
        g = g.astype(dtype)
        gterms = [(axes, pair(rng, np.asarray(m).shape[0], real=not cplx)) for axes, m in terms]
        ou.check_op_apply(ou.bits_mirror(g, shape, gterms, dtype), g, shape, gterms)


def test_the_bound_is_not_vacuous():
    """One entry of median size with the wrong sign exceeds the bound by a wide factor."""
    rng = np.random.default_rng(195)
    shape = (2,) * 10
    x = (rng.standard_normal(1024) + 1j * rng.standard_normal(1024)).astype("complex64")
    terms = [((0, 9), pair(rng)), ((3, 4, 5), pair(rng, 8)), ((9,), pair(rng, 2))]
    tol = ou.op_apply_tol(x, shape, terms)
    flipped = 2.0 * float(np.median(np.abs(terms[0][1].real))) * float(np.median(np.abs(x.real)))
    assert flipped > 1e3 * float(tol.max())


def test_operator_energy_takes_hermitian_requests_only(monkeypatch):
    tree, arrays = sliced_circuit_tree()
    fn = _tree_contractor(tree)

    def never(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(fn, "setup", never)
    monkeypatch.setattr(fn, "_reduce_state", never)
    out = list(tree.output)
    rng = np.random.default_rng(196)
    h = pair(rng)
    h = h + h.conj().T
    for call in (fn.operator_energy, fn.operator_energy_autograd):
        with pytest.raises(ValueError, match="Hermitian"):
            call(*arrays, operators=[([out[0], out[2]], h), ([out[1]], X + 1e-9 * Y @ Z)])
        with pytest.raises(ValueError, match="Hermitian"):
            call(*arrays, operators=([out[0], out[2]], pair(rng)))
        with pytest.raises(ValueError):
            call(*arrays, operators=(["nope"], X))
    # within 1e-12 max |O| of Hermitian: taken (the call reaches the device), and its Hermitian part is what is used
    almost = h.copy()
    almost[0, 1] += 1e-13 * np.abs(h).max()
    with pytest.raises(AssertionError):
        fn.operator_energy(*arrays, operators=([out[0], out[2]], almost))
    several, canon, terms = fn._operator_energy_requests([([out[0], out[2]], almost), ([out[2], out[0]], almost)], False)
    assert several and all(np.array_equal(m, m.conj().T) for _, m in canon) and len(terms) == 1
    assert np.array_equal(terms[0][1], terms[0][1].conj().T)
    for bad_wrt in ([-1], [len(arrays)], [0, 99]):
        with pytest.raises((IndexError, ValueError)):
            fn.operator_energy(*arrays, operators=([out[0]], Z), wrt=bad_wrt)
    # apply_operators: a complex matrix in a real contraction is refused before the device; reuse takes no arrays
    real = [np.ascontiguousarray(a.real) for a in arrays]
    with pytest.raises(ValueError):
        fn.apply_operators(*real, operators=([out[0]], Y))
    with pytest.raises(ValueError):
        fn.apply_operators(*arrays, operators=([out[0]], Z), reuse=True)
    with pytest.raises(ValueError):
        fn.operator_expectation(*arrays, operators=([out[0]], np.eye(3)))
    with pytest.raises(AssertionError):
        fn.apply_operators(*real, operators=([out[0]], X))
    fs = ca.HipContractor(tree, strip_exponent=True)
    with pytest.raises(ValueError):
        fs.operator_energy(*arrays, operators=([out[0]], Z))


def test_normalize_with_norm_zero_is_refused():
    tree, arrays = sliced_circuit_tree()
    fn = ca.HipContractor(tree)

    class Ex:
        def rdm_result(self, extents, keep):
            d = 2 ** sum(keep)
            return np.zeros((d, d), dtype=np.complex128)

        def sample_info(self):
            return (0.0, 0.0, 0.0, 0)

        def __getattr__(self, name):
            raise AssertionError(f"the device was touched: {name}")

    fn._reduce_state = lambda *a, **k: ({"exec": Ex()}, False)
    with pytest.raises(ValueError, match="norm zero"):
        fn.operator_energy(*arrays, operators=([tree.output[0]], Z), normalize=True)


def test_expectation_is_the_trace_with_the_reduced_density_matrix():
    """``_operator_values`` on a stand-in executor whose ``rdm_result`` is numpy's: ``<x| O |x>`` of the reference, one
    matrix per distinct axis set."""
    rng = np.random.default_rng(197)
    shape = (2, 3, 2, 4)
    x = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    calls = []

    class Ex:
        def rdm_result(self, extents, keep):
            calls.append(tuple(keep))
            kept = [a for a, f in enumerate(keep) if f]
            rest = [a for a, f in enumerate(keep) if not f]
            m = x.transpose(kept + rest).reshape(int(np.prod([shape[a] for a in kept])), -1)
            return m @ m.conj().T

    canon = [((1, 3), pair(rng, 12)), ((0,), pair(rng, 2)), ((1, 3), pair(rng, 12))]
    values = ca.HipContractor._operator_values(Ex(), shape, canon)
    assert values.dtype == np.complex128 and len(calls) == 2
    for v, (axes, mat) in zip(values, canon):
        want = np.vdot(x, ou.op_apply_reference(x, shape, [(axes, mat)]))
        assert abs(v - want) <= 1e-12 * np.abs(mat).sum() * np.vdot(x, x).real


def test_circuit_argument_errors_need_no_device(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the network was built")

    monkeypatch.setattr(circuits, "circuit_to_network", never)
    gates = [("x_1_2", (0,), ()), ("rz", (1,), (0.3,))]
    proj = np.diag([0.0, 0, 0, 1])
    for call in (circuits.operator_expectation, circuits.operator_energy_gradient):
        for bad in (((0, 3), proj), ((0, 0), proj), ((0, 1), X), ((), np.ones((1, 1))), ((0,), np.array([[np.nan, 0], [0, 1]])),
                    5, "XZ", ((0, 1),), (tuple(range(7)), np.eye(128))):
            with pytest.raises(ValueError):
                call(7 if isinstance(bad, tuple) and len(bad[0]) == 7 else 3, gates, bad)
        with pytest.raises(ValueError, match="fixed"):
            call(3, gates, ((0, 1), proj), fixed={0: 1})
        with pytest.raises(ValueError):
            call(3, gates, ((1, 2), proj), fixed={0: 2})
        with pytest.raises(AssertionError):
            call(3, gates, [((1, 2), proj), (2, Z)], fixed={0: 1})
    with pytest.raises(ValueError, match="Hermitian"):
        circuits.operator_energy_gradient(3, gates, ((0, 1), np.triu(np.ones((4, 4)))))
