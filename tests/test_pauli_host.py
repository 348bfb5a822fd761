"""CPU suite: the host side of Pauli-string expectation values of the result tensor -- the
header and the binding, the reference of tests/pauli_util.py against dense Kronecker products, request parsing and the
argument errors that are raised before a device is touched, the masks and kernel names of the power-of-two route, and a
check that the tolerance of tests/pauli_util.py is not vacuous."""
import os
import re

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import _tree_contractor, pauli_requests

import pauli_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_call_and_the_binding_mirrors_it():
    text = open(os.path.join(ROOT, "include", "ctg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = re.sub(r"\s+", " ", code)
    assert ("int ctg_exec_result_pauli(ctg_exec* exec, int64_t rank, const int64_t* extents, int64_t m, "
            "const uint8_t* ops, double* out);") in flat
    m = re.search(r"#define\s+CTG_PAULI_MAX_STRINGS\s+(\d+)", code)
    assert m and int(m.group(1)) == runtime.Executor.PAULI_MAX_STRINGS == 4096
    assert re.search(r"#define\s+CTG_ABI_VERSION\s+10\b", code) and runtime.ABI_VERSION == 10
    assert "ctg_exec_result_pauli" in runtime.SYMBOLS
    assert code.index("ctg_exec_result_rdm(") < code.index("ctg_exec_result_pauli(")
    assert hasattr(runtime.load(), "ctg_exec_result_pauli")
    doc = re.sub(r"\s*\n\s*\*\s*", " ", text)
    for phrase in ("no floating-point atomics", "function of (dtype, extents, row s of ops, the tensor's bytes) alone",
                   "Every product is formed in fp64", "exactly 0.0 and is written without a launch"):
        assert phrase in doc, phrase


def test_methods_exist_on_every_layer():
    from cotengra_amd.interface import ContractExpression

    assert hasattr(ca.ContractionTree, "contract_expectation")
    assert hasattr(ContractExpression, "expectation") and hasattr(ca.HipContractor, "expectation")
    assert hasattr(runtime.Executor, "pauli_result") and hasattr(runtime.Executor, "pauli_variant")
    assert hasattr(circuits, "pauli_expectation")
    assert ca.ExpectationResult._fields == ("values", "norm", "exponent")


def test_reference_against_dense_kronecker_products():
    rng = np.random.default_rng(16)
    shape = (2,) * 6
    x = (rng.standard_normal(64) + 1j * rng.standard_normal(64)).astype("complex64")
    w = x.astype(np.complex128)
    norm = float(np.vdot(w, w).real)
    ops = rng.integers(0, 4, size=(300, 6))
    ops[0] = 0
    ref = pu.pauli_reference(x, shape, ops)
    for row, v in zip(ops.tolist(), ref):
        dense = np.vdot(w, pu.dense_string(row, shape) @ w)
        assert abs(dense.imag) <= 1e-12 * norm and abs(v - dense.real) <= 1e-12 * norm, row
    assert abs(ref[0] - norm) <= 1e-12 * norm
    # a real tensor: an odd number of Y gives exactly zero, everything else the dense value
    xr = rng.standard_normal(64).astype("float32")
    wr = xr.astype(np.float64)
    for row, v in zip(ops.tolist(), pu.pauli_reference(xr, shape, ops)):
        if row.count(2) % 2:
            assert v == 0.0
        dense = np.vdot(wr, pu.dense_string(row, shape) @ wr)
        assert abs(v - dense.real) <= 1e-12 * float(wr @ wr), row
    # the flat-index form of the definition: S = sum (-1)^popcount(j & zm) conj(x[j ^ xm]) x[j]
    j = np.arange(64)
    for row, v, (xm, zm, ny) in zip(ops.tolist(), ref, runtime.pauli_masks(shape, ops)):
        sign = 1.0 - 2.0 * (np.array([bin(int(t)).count("1") for t in j & zm]) & 1)
        S = np.sum(sign * np.conj(w[j ^ xm]) * w[j])
        want = (-1) ** (ny // 2) * S.real if ny % 2 == 0 else (-1) ** ((ny + 1) // 2) * S.imag
        assert abs(v - want) <= 1e-12 * norm, row
    assert pu.pauli_reference(x, shape, ops[3]).shape == () and pu.pauli_reference(x, shape, ops[3]) == ref[3]


def test_reference_on_a_mixed_shape():
    rng = np.random.default_rng(17)
    shape = (2, 3, 2, 1, 2)
    n = int(np.prod(shape))
    x = (rng.integers(-3, 4, size=n) + 1j * rng.integers(-3, 4, size=n)).astype("complex64")
    w = x.astype(np.complex128)
    for text in ("IIIII", "XIIII", "IIYII", "ZIIIZ", "YIXIZ", "YIYIY", "XIZIY"):
        row = pu.codes(text)
        dense = np.vdot(w, pu.dense_string(row, shape) @ w)
        assert pu.pauli_reference(x, shape, row) == dense.real and dense.imag == 0   # (small integers: exact)
    with pytest.raises(AssertionError):
        pu.pauli_reference(x, shape, pu.codes("IXIII"))


def small_tree():
    return ca.ContractionTree.from_path([("a", "b"), ("b", "c", "d", "e")], ("a", "c", "d", "e"),
                                        {"a": 2, "b": 3, "c": 5, "d": 2, "e": 2}, path=[(0, 1)])


def test_requests_in_three_forms():
    tree = small_tree()
    assert tree.gathered_shape() == (2, 5, 2, 2)
    several, ops = pauli_requests(tree, "xIzY")
    assert several is False and ops.dtype == np.uint8 and ops.tolist() == [[1, 0, 3, 2]]
    for form in ({"a": "X", "d": "z", "e": "Y"}, [("e", "y"), ("a", "x"), ("d", "Z")], (("a", "X"), ("d", "Z"), ("e", "Y")),
                 {"a": "X", "c": "I", "d": "Z", "e": "Y"}):
        s, o = pauli_requests(tree, form)
        assert s is False and np.array_equal(o, ops), form
    several, many = pauli_requests(tree, ["XIZY", {"a": "X", "d": "Z", "e": "Y"}, [("a", "X"), ("d", "Z"), ("e", "Y")], {}, "IIII"])
    assert several is True and many.shape == (5, 4)
    assert np.array_equal(many[:3], np.repeat(ops, 3, axis=0)) and not many[3:].any()
    assert pauli_requests(tree, ["XIZY"])[0] is True and pauli_requests(tree, ["XIZY"])[1].tolist() == ops.tolist()
    several, none = pauli_requests(tree, [])
    assert several is True and none.shape == (0, 4)
    assert pauli_requests(tree, {})[1].tolist() == [[0, 0, 0, 0]]
    # a list of one-pair requests is a list of requests, a list of pairs is one request
    assert pauli_requests(tree, [[("a", "X")], [("d", "Z")]])[1].tolist() == [[1, 0, 0, 0], [0, 0, 3, 0]]
    assert pauli_requests(tree, [("a", "X"), ("d", "Z")])[1].tolist() == [[1, 0, 3, 0]]


def test_argument_errors_need_no_device(monkeypatch):
    tree = small_tree()
    fn = _tree_contractor(tree)

    def never(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(fn, "setup", never)
    xs = [np.ones((2, 3)), np.ones((3, 5, 2, 2))]
    bad_requests = [
        {"q": "X"},                          # an unknown label
        {"b": "Z"},                          # an inner index
        [("a", "X"), ("a", "Z")],            # a repeated label
        {"a": "W"}, "XIQZ", {"a": 1},        # a letter outside IXYZ
        "XIZ", "XIZYI",                      # a string of the wrong length
        {"c": "Z"}, "IXII",                  # a letter on an index of extent 5
        ["IIII", {"c": "Y"}],                # ... in any request of a list
        3, None, [3],
        ["IIII"] * 4097,                     # more than PAULI_MAX_STRINGS
    ]
    for bad in bad_requests:
        with pytest.raises(ValueError):
            fn.expectation(*xs, paulis=bad)
        with pytest.raises(ValueError):
            pauli_requests(tree, bad)
    with pytest.raises(ValueError):
        tree.contract_expectation(xs, "IIIX", reuse=True)      # reuse=True with arrays
    with pytest.raises(RuntimeError):
        tree.contract_expectation([], "IIIX", reuse=True)      # ... before any call
    assert not fn._execs
    assert pauli_requests(tree, ["IIII"] * 4096)[1].shape == (4096, 4)
    # a projected output index has extent 1: only I
    proj = small_tree().remove_ind("d", project=1)
    assert proj.gathered_shape() == (2, 5, 1, 2)
    assert pauli_requests(proj, "XIIZ")[1].tolist() == [[1, 0, 0, 3]]
    with pytest.raises(ValueError):
        pauli_requests(proj, "XIZI")


class StubExecutor:
    """Stands where the executor of a finished contraction would: ``pauli_result`` returns the reference."""

    handle = 1

    def __init__(self, out):
        self.out = np.asarray(out)
        self.calls = []

    def pauli_result(self, extents, ops):
        assert tuple(extents) == self.out.shape
        self.calls.append(np.asarray(ops).tolist())
        return pu.pauli_reference(self.out, self.out.shape, np.asarray(ops).reshape(-1, self.out.ndim))

    def sample_info(self):
        return (float(np.sum(np.abs(self.out) ** 2)), 0.0, 0.0, 0, (0.0, 0.0))

    def result_stats(self):
        return self.sample_info()[:4]

    def get_exponent(self):
        return 0.0, False


def test_single_request_against_list(monkeypatch):
    rng = np.random.default_rng(5)
    tree = small_tree()
    out = rng.standard_normal((2, 5, 2, 2)) + 1j * rng.standard_normal((2, 5, 2, 2))
    fn = _tree_contractor(tree)
    ex = StubExecutor(out)
    monkeypatch.setattr(fn, "_reduce_state", lambda arrays, strip, check, reuse: ({"exec": ex}, False))
    one = fn.expectation(paulis="XIZY")
    assert isinstance(one, ca.ExpectationResult) and np.ndim(one.values) == 0 and one.exponent == 0.0
    assert one.values == pu.pauli_reference(out, out.shape, [1, 0, 3, 2])
    many = fn.expectation(paulis=["XIZY", {}, {"e": "Z"}])
    assert many.values.shape == (3,) and many.values.dtype == np.float64 and many.values[0] == one.values
    assert abs(many.values[1] - many.norm) <= 1e-12 * many.norm
    assert ex.calls == [[[1, 0, 3, 2]], [[1, 0, 3, 2], [0, 0, 0, 0], [0, 0, 0, 3]]]
    empty = fn.expectation(paulis=[])
    assert empty.values.shape == (0,) and empty.norm == many.norm


def test_masks_of_the_power_of_two_route():
    L = 14
    shape = (2,) * L
    rows = [pu.bit_string(L, {}), pu.bit_string(L, {0: "X"}), pu.bit_string(L, {13: "Z"}), pu.bit_string(L, {5: "Y"}),
            pu.bit_string(L, {11: "X", 12: "Y", 13: "Z", 0: "Y"}), pu.bit_string(L, {11: "Z", 12: "Z"}),
            pu.bit_string(L, {12: "X"}), pu.bit_string(L, {b: "Y" for b in range(L)})]
    assert runtime.pauli_masks(shape, rows) == [
        (0, 0, 0), (1, 0, 0), (0, 1 << 13, 0), (32, 32, 1),
        ((1 << 11) | (1 << 12) | 1, (1 << 12) | (1 << 13) | 1, 2),       # straddles bit 12: xm_lo = 2049, xm_hi = 1
        (0, (1 << 11) | (1 << 12), 0), (1 << 12, 0, 0), ((1 << L) - 1, (1 << L) - 1, L)]
    # axes of mixed width: the bit of a qubit is log2 of its stride
    shape = (4, 2, 8, 2, 1, 2)          # strides 64, 32, 4, 2, 2, 1
    assert runtime.pauli_masks(shape, [pu.codes("IXIIII"), pu.codes("IZIYIX"), pu.codes("IYIZIZ"), pu.codes("IIIIII")]) == [
        (32, 0, 0), (2 | 1, 32 | 2, 1), (32, 32 | 2 | 1, 1), (0, 0, 0)]
    for bad_shape, bad_ops in (((4, 2), [[1, 0]]), ((2, 2), [[4, 0]]), ((2, 2), [[1, 0, 0]]), ((2, 0), [[0, 0]]),
                               ((3, 2), [[0, 1]]), ((2, 2), [[-1, 0]]), ((2, 2), [[0.5, 0]])):
        with pytest.raises(ValueError):
            runtime.pauli_masks(bad_shape, bad_ops)
    with pytest.raises(ValueError):
        runtime.pauli_masks((2, 2), np.zeros((4097, 2), np.uint8))


def test_variant_names_follow_the_route():
    z = [pu.bit_string(6, {0: "Z"})]
    assert runtime.pauli_variant("complex64", (2,) * 6, z) == "pauli_general_kernel<c64>"
    assert runtime.pauli_variant("complex64", (2,) * 12, [pu.bit_string(12, {3: "Y"})]) == "pauli_chunk_kernel<c64>"
    assert runtime.pauli_variant("float32", (4, 2, 512), [[0, 3, 0]]) == "pauli_chunk_kernel<float>"
    assert runtime.pauli_variant("complex128", (2, 2048), [[1, 0]]) == "pauli_chunk_kernel<c128>"
    assert runtime.pauli_variant("float64", (2,) * 11, [[0] * 11]) == "pauli_general_kernel<double>"
    assert runtime.pauli_variant("float64", (3, 2, 4096), [[0, 1, 0]]) == "pauli_general_kernel<double>"
    # every string answered without a launch: a real dtype and an odd number of Y in every string; or no string
    odd = [pu.bit_string(12, {3: "Y"}), pu.bit_string(12, {0: "Y", 1: "Y", 7: "Y", 2: "X"})]
    assert runtime.pauli_variant("float32", (2,) * 12, odd) == "none"
    assert runtime.pauli_variant("float64", (2,) * 6, [pu.bit_string(6, {3: "Y"})]) == "none"
    assert runtime.pauli_variant("complex64", (2,) * 12, odd) == "pauli_chunk_kernel<c64>"
    assert runtime.pauli_variant("float32", (2,) * 12, odd + [pu.bit_string(12, {3: "Y", 4: "Y"})]) == "pauli_chunk_kernel<float>"
    assert runtime.pauli_variant("complex64", (2,) * 12, np.zeros((0, 12), np.uint8)) == "none"
    with pytest.raises(ValueError):
        runtime.pauli_variant("complex64", (4, 1024), [[1, 0]])


def test_the_bound_is_not_vacuous():
    """Two numpy summation orders at n = 2^18 -- ``np.vdot`` and a reversed sum of reversed chunks of 512 terms -- must
    differ by less than the bound a device value is held to; and one term of median size with the wrong sign must move
    the value by more than the bound."""
    L = 18
    n = 2 ** L
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype("complex64")
    w = x.astype(np.complex128)
    tol = pu.pauli_tol(x, n)
    for letters in ({}, {0: "X", 13: "Z", 5: "Y"}, {17: "Y", 12: "X", 11: "Z", 3: "Z"}, {b: "Z" for b in range(L)}):
        row = pu.bit_string(L, letters)
        ref = pu.pauli_reference(x, (2,) * L, row)
        terms = np.real(np.conj(w) * pu.apply_string(w, (2,) * L, row).reshape(-1))
        other = 0.0
        for c in reversed(range(0, n, 512)):
            other = other + float(np.sum(terms[c:c + 512][::-1]))
        frac = abs(other - ref) / tol
        flipped = 2.0 * float(np.median(np.abs(terms)))
        print(f"{letters}: two numpy orders use {frac:.3e} of the bound; a flipped median term is {flipped / tol:.1f} bounds")
        assert frac < 1 and flipped > tol


def test_circuit_argument_errors_need_no_device(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the network was built")

    monkeypatch.setattr(circuits, "circuit_to_network", never)
    gates = [("x_1_2", (0,), ())]
    for bad in ("XZ", "XZIQ", {3: "X"}, {-1: "Z"}, {0: "W"}, 5, ["XIZ", {0: "x", 1: 7}], ["III"] * 4097):
        with pytest.raises(ValueError):
            circuits.pauli_expectation(3, gates, bad)
    with pytest.raises(ValueError):
        circuits.pauli_expectation(3, gates, "XII", fixed={0: 1})          # a fixed qubit must be I
    with pytest.raises(ValueError):
        circuits.pauli_expectation(3, gates, [{1: "Z"}, {2: "Y"}], fixed={2: 0})
    with pytest.raises(ValueError):
        circuits.pauli_expectation(3, gates, "IIZ", fixed={1: 2})
    with pytest.raises(ValueError):
        circuits.pauli_expectation(3, gates, "IIZ", fixed={3: 0})
    with pytest.raises(ValueError):
        circuits.pauli_expectation(3, gates, ["IIZ", "ZII"], coeffs=[1.0])
    # (a valid request reaches the network)
    with pytest.raises(AssertionError):
        circuits.pauli_expectation(3, gates, ["IIZ", {0: "x"}], fixed={1: 0}, coeffs=[1.0, -0.5])
