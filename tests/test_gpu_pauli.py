"""GPU suite: expectation values of Pauli strings over the result tensor on the device (csrc/ctg_pauli.hip, DESIGN.md
section 16) -- ``Executor.pauli_result``, ``HipContractor.expectation``, ``ContractionTree.contract_expectation``,
``ContractExpression.expectation``, ``circuits.pauli_expectation``.

Data reaches the result tensor bit for bit through a one-tensor tree (a single copy step), as in
tests/test_gpu_result_reduce.py.  Reference and tolerance are in tests/pauli_util.py: ``2 (m + 1) 2^-53 sum |x|^2``
per value, derived from the rounding of two summation orders and never from what the device returns; no string is
excluded.

The power-of-two route (every extent a power of two, at least 4096 elements) works in chunks of 4096 elements; a string
whose X / Y bits reach bit 12 or higher pairs chunk ``c`` with chunk ``c ^ (xm >> 12)``.  Its grid is ``min(512,
ceil(units / 3))`` with units = chunks or chunk pairs: 2^13 elements are two chunks on one workgroup, or one pair; 2^15
elements 8 chunks on 3 workgroups (the last round partial) or 4 pairs on 2; 2^18 elements 64 chunks on 22 workgroups
(the last round partial) or 32 pairs on 11 (partial as well)."""
import ctypes as C
import os

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import _tree_contractor

import pauli_util as pu
import rdm_util as du
import reduce_util as ru
import sample_util as su
from test_gpu_result_reduce import resident
from test_gpu_sample import gaussian, one_tensor_tree, random_circuit, statevector

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "complex64", "complex128"]
HERE = os.path.dirname(os.path.abspath(__file__))


def strings_for(L, seed=0):
    """Rows of codes over the shape ``(2,) * L`` (bit ``b`` of the flat index is axis ``L - 1 - b``); letters on bits
    the tensor does not have are left out."""
    cases = [{}]
    for b in (0, 1, 11, 12, L - 1):                         # bit 1: inside a 16-byte group; 11 | 12: the chunk boundary
        cases += [{b: "X"}, {b: "Y"}, {b: "Z"}]
    cases += [{11: "X", 12: "X"}, {0: "X", L - 1: "X"}]
    # ny = 1, 2, 3, 4: every phase
    cases += [{0: "Y", 2: "X", 3: "Z"}, {1: "Y", L - 1: "Y", 3: "Z"}, {0: "Y", 2: "Y", L - 1: "Y", 3: "X"},
              {0: "Y", 1: "Y", L - 2: "Y", L - 1: "Y", 2: "Z"}]
    # Z only: bits below 12, above 12, both
    cases += [{0: "Z", 3: "Z", 7: "Z"}, {13: "Z", L - 1: "Z"}, {2: "Z", 11: "Z", 12: "Z", L - 1: "Z"}]
    rows = []
    for c in cases:
        if all(0 <= b < L for b in c):
            row = pu.bit_string(L, c)
            if row not in rows:
                rows.append(row)
    rng = np.random.default_rng(1000 * L + seed)
    rows += rng.integers(1, 4, size=(10, L)).tolist()       # ten strings of full weight
    return np.array(rows, dtype=np.uint8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [6, 12, 13, 15, 18])
def test_power_of_two_shapes_against_the_reference(L, dtype):
    """2^6: below the fast route's lower bound of 4096 elements (the general route); 2^12: one chunk; 2^13: two chunks
    that one X bit pairs; 2^15 and 2^18: several workgroups with a partial last round."""
    n = 2 ** L
    x = gaussian(n, dtype, seed=160 + L)
    ex = resident(x)
    shape = (2,) * L
    ops = strings_for(L)
    want = "pauli_general_kernel<" if L < 12 else "pauli_chunk_kernel<"
    assert ex.pauli_variant(shape, ops).startswith(want)
    got = ex.pauli_result(shape, ops)
    assert got.shape == (len(ops),) and got.dtype == np.float64
    p = su.probabilities(x)
    assert not ops[0].any() and abs(got[0] - p.sum()) <= ru.marginal_tol(p.sum(), n)    # the identity is the norm
    pu.check_pauli(got, x, shape, ops)
    if np.dtype(dtype).kind != "c":
        odd = (ops == 2).sum(axis=1) % 2 == 1
        assert odd.any() and np.all(got[odd] == 0.0) and not np.signbit(got[odd]).any()
    assert ex.download_result().tobytes() == x.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_half_integers_are_exact(dtype):
    """round(2 gaussian) / 2 clipped to [-2, 2] at 2^20 elements: every product is a multiple of 1/4, every term at
    most 8 and every partial sum of 2^20 of them exact in fp64, so the device must equal numpy whatever the order --
    which pins the partner of every element, every sign, the pair doubling and the phases."""
    L = 20
    x = (np.clip(np.round(2 * gaussian(2 ** L, dtype, seed=7)), -4, 4) / 2).astype(dtype)
    ex = resident(x)
    shape = (2,) * L
    extra = [{12: "X", 11: "Z"}, {11: "Y", 12: "Y"}, {12: "Y", 13: "Z", 0: "Z"}, {19: "Y", 0: "Y", 12: "X"},
             {b: "Z" for b in range(L)}]
    ops = np.concatenate([strings_for(L), np.array([pu.bit_string(L, c) for c in extra], dtype=np.uint8)])
    assert len(ops) == 40 and ex.pauli_variant(shape, ops).startswith("pauli_chunk_kernel<")
    got = ex.pauli_result(shape, ops)
    ref = pu.pauli_reference(x, shape, ops)
    assert np.array_equal(got, ref), [(i, got[i], ref[i]) for i in np.flatnonzero(got != ref)]
    assert np.count_nonzero(ref) >= 10


def masked_strings(L, xbits, count, rng):
    """``count`` strings over ``(2,) * L`` whose X / Y letters sit exactly on ``xbits``; Z or I elsewhere."""
    rows = []
    for _ in range(count):
        c = {b: ("X", "Y")[int(rng.integers(0, 2))] for b in xbits}
        for b in range(L):
            if b not in c and rng.integers(0, 3) == 0:
                c[b] = "Z"
        rows.append(pu.bit_string(L, c))
    return rows


def test_a_value_does_not_depend_on_the_batch():
    """70 strings over 2^15 elements with three X masks -- 38 + 2 duplicates on {0, 13} (a pass boundary at 32), 20 with
    no X (Z-type), 10 on {3} -- interleaved: the call, each string alone and the reversed call give the same bits per
    string; so do a repeated call, a call after other work in the same scratch, and another executor."""
    L = 15
    rng = np.random.default_rng(70)
    a, z, c = masked_strings(L, (0, 13), 38, rng), masked_strings(L, (), 20, rng), masked_strings(L, (3,), 10, rng)
    a += [a[5], a[33]]
    rows, pools = [], [a, z, c]
    while any(pools):
        for pool in pools:
            rows += pool[:3]
            del pool[:3]
    ops = np.array(rows, dtype=np.uint8)
    masks = runtime.pauli_masks((2,) * L, ops)
    assert len(ops) == 70 and len({m[0] for m in masks}) == 3 and sum(m[0] == (1 | 1 << 13) for m in masks) == 40
    x = gaussian(2 ** L, "complex64", seed=15)
    ex = resident(x)
    shape = (2,) * L
    whole = ex.pauli_result(shape, ops)
    pu.check_pauli(whole, x, shape, ops)
    alone = np.array([ex.pauli_result(shape, ops[i:i + 1])[0] for i in range(len(ops))])
    assert alone.tobytes() == whole.tobytes()
    assert ex.pauli_result(shape, ops[::-1])[::-1].tobytes() == whole.tobytes()
    assert ex.pauli_result(shape, ops).tobytes() == whole.tobytes()                       # a second run
    ex.topk_result(300)
    ex.rdm_result(shape, [1] * 3 + [0] * (L - 3))
    assert ex.pauli_result(shape, ops).tobytes() == whole.tobytes()                       # after other calls in the same scratch
    assert resident(x).pauli_result(shape, ops).tobytes() == whole.tobytes()              # a fresh executor
    assert resident(gaussian(2 ** L, "complex64", seed=16)).pauli_result(shape, ops).tobytes() != whole.tobytes()
    # the general route
    g = gaussian(2 * 3 * 2 * 5 * 2, "complex64", seed=17)
    gops = np.array([pu.codes(t) for t in ("XIZIY", "IIIII", "YIYIZ", "ZIXIX", "XIZIY")], dtype=np.uint8)
    gw = resident(g).pauli_result((2, 3, 2, 5, 2), gops)
    ga = np.array([resident(g).pauli_result((2, 3, 2, 5, 2), gops[i:i + 1])[0] for i in (4, 3, 2, 1, 0)])[::-1]
    assert gw.tobytes() == ga.tobytes() and gw[0].tobytes() == gw[4].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_width_and_general_shapes(dtype):
    rng = np.random.default_rng(23)
    for shape, want in (((4, 2, 8, 2, 16, 2, 2), "pauli_chunk_kernel<"), ((2, 3, 2, 5, 2), "pauli_general_kernel<"),
                        ((2, 1, 2, 2), "pauli_general_kernel<")):
        n = int(np.prod(shape))
        qubits = [a for a, d in enumerate(shape) if d == 2]
        ops = np.zeros((24, len(shape)), dtype=np.uint8)
        ops[1:, qubits] = rng.integers(0, 4, size=(23, len(qubits)))
        ops[1, qubits] = 2                                   # Y on every qubit
        ops[2, qubits[0]], ops[2, qubits[-1]] = 1, 3
        x = gaussian(n, dtype, seed=n % 1000)
        ex = resident(x)
        assert ex.pauli_variant(shape, ops).startswith(want)
        got = ex.pauli_result(shape, ops)
        pu.check_pauli(got, x, shape, ops)
        assert ex.download_result().tobytes() == x.tobytes()
    # a general shape with several chunks of flat indices per string
    shape = (2, 2 ** 19 + 3, 2)
    x = gaussian(int(np.prod(shape)), dtype, seed=5)
    ops = np.array([pu.codes(t) for t in ("III", "XIZ", "YIY", "ZIX", "YIX")], dtype=np.uint8)
    pu.check_pauli(resident(x).pauli_result(shape, ops), x, shape, ops)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_real_plans(dtype):
    """An odd number of Y on a real tensor: exactly 0.0, written without a launch; even: the reference."""
    L = 13
    shape = (2,) * L
    x = gaussian(2 ** L, dtype, seed=31)
    ex = resident(x)
    odd = np.array([pu.bit_string(L, c) for c in ({0: "Y"}, {12: "Y", 3: "X"}, {1: "Y", 5: "Y", 12: "Y", 2: "Z"})], dtype=np.uint8)
    even = np.array([pu.bit_string(L, c) for c in ({0: "Y", 12: "Y"}, {3: "X", 4: "Z"}, {1: "Y", 2: "Y", 11: "Y", 12: "Y"}, {})],
                    dtype=np.uint8)
    assert ex.pauli_variant(shape, odd) == runtime.pauli_variant(dtype, shape, odd) == "none"
    ex.result_stats()                                                 # (the statistics passes have their own scratch)
    before = ex.device_bytes()
    zeros = ex.pauli_result(shape, odd)
    assert zeros.tobytes() == np.zeros(3).tobytes()
    assert ex.device_bytes() == before                                # (not even the scratch was needed)
    mixed = np.concatenate([odd[:1], even[:2], odd[1:], even[2:]])
    got = ex.pauli_result(shape, mixed)
    pu.check_pauli(got, x, shape, mixed)
    assert np.all(got[[0, 3, 4]] == 0.0) and not np.signbit(got[[0, 3, 4]]).any() and np.all(got[[1, 2, 5, 6]] != 0.0)
    assert got[[1, 2, 5, 6]].tobytes() == ex.pauli_result(shape, even).tobytes()
    # the general route
    g = gaussian(2 * 3 * 2, dtype, seed=32)
    gg = resident(g).pauli_result((2, 3, 2), [pu.codes("YIX"), pu.codes("YIY"), pu.codes("IIY")])
    pu.check_pauli(gg, g, (2, 3, 2), [pu.codes("YIX"), pu.codes("YIY"), pu.codes("IIY")])
    assert gg[0] == 0.0 and gg[2] == 0.0 and gg[1] != 0.0


def circuit_tree(n, gates, dtype, template=None):
    inputs, output, sd, arrays = circuits.circuit_to_network(n, gates, template or "?" * n, simplify=True, dtype=dtype)
    return ca.array_contract_tree(inputs, output, sd), arrays


def test_consistent_with_the_reduced_density_matrix():
    """12 qubits: ``<P>`` of a string supported on up to 6 qubits equals ``trace(P_kept rho_kept)`` of the matrix the
    same result tensor gives (``reuse=True``), within the sum of both bounds."""
    n = 12
    tree, arrays = circuit_tree(n, random_circuit(n, 6, seed=7), "complex64")
    out = list(tree.output)
    x = np.asarray(tree.contract(arrays))
    shape = x.shape
    rng = np.random.default_rng(12)
    for k in (1, 2, 4, 6):
        for _ in range(3):
            qs = [int(q) for q in rng.choice(n, size=k, replace=False)]
            letters = [int(v) for v in rng.integers(1, 4, size=k)]
            r = tree.contract_expectation(arrays, {out[q]: pu.LETTERS[c] for q, c in zip(qs, letters)})
            rho = tree.contract_rdm([], [out[q] for q in qs], reuse=True).rho
            P = pu.dense_string(letters, (2,) * k)
            via_rho = np.trace(P @ rho)
            tol_rho = du.rdm_tol(du.rdm_reference(x, shape, qs), x.size // 2 ** k)
            bound = pu.pauli_tol(x, x.size) + 2.0 * float(np.sum(tol_rho.T[P != 0]))
            assert abs(r.values - via_rho.real) <= bound and abs(via_rho.imag) <= bound, (qs, letters)
            row = [0] * n
            for q, c in zip(qs, letters):
                row[q] = c
            assert abs(r.values - pu.pauli_reference(x, shape, row)) <= pu.pauli_tol(x, x.size)


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_through_the_layers_on_a_sliced_tree(dtype):
    tree = ca.tree_from_record(ca.load_network(os.path.join(HERE, "golden", "trees", "sycamore_m10_open8.json")))
    z = np.load(os.path.join(HERE, "golden", "sycamore_m10_open8_arrays.npz"))
    xs = [z[f"t{i}"].astype(dtype) for i in range(tree.N)]
    assert tree.nslices == 8
    amps = np.asarray(tree.contract(xs))                          # (what the result tensor holds)
    shape, out = amps.shape, list(tree.output)
    n = amps.size
    texts = ["IIIIIIII", "XIZIYIIZ", "ZZZZZZZZ", "YYIIXXZZ", "IIIIIIIX", "YIIIIIII"]
    ref = pu.pauli_reference(amps, shape, [pu.codes(t) for t in texts])
    tol = pu.pauli_tol(amps, n)
    r = tree.contract_expectation([], texts, reuse=True)          # after __call__
    assert isinstance(r, ca.ExpectationResult) and r.values.shape == (6,) and r.exponent == 0.0
    assert np.all(np.abs(r.values - ref) <= tol) and abs(r.norm - ref[0]) <= ru.marginal_tol(ref[0], n)
    fresh = tree.contract_expectation(xs, texts)
    assert np.all(np.abs(fresh.values - ref) <= tol)
    # the three forms of a request, a single one
    fn = _tree_contractor(tree)
    one = fn.expectation(paulis={out[0]: "x", out[2]: "Z", out[4]: "y", out[7]: "Z"}, reuse=True)
    pairs = fn.expectation(paulis=[(out[7], "Z"), (out[4], "Y"), (out[2], "Z"), (out[0], "X")], reuse=True)
    assert np.ndim(one.values) == 0 and one.values == pairs.values == r.values[1]
    tree.contract_topk([], 5, reuse=True)
    assert tree.contract_expectation([], texts[3], reuse=True).values == r.values[3]      # after topk
    # strip_exponent: the mantissa's values and the exponent next to them
    rel = 1e-10 if dtype == "complex128" else 1e-5                # the library's promise per amplitude
    s = tree.contract_expectation(xs, texts, strip_exponent=True)
    assert np.all(np.abs(s.values * 10.0 ** (2 * s.exponent) - ref) <= 4 * rel * ref[0])
    assert abs(s.norm * 10.0 ** (2 * s.exponent) - ref[0]) <= 4 * rel * ref[0]
    # reuse=True after a call that leaves no result to read
    tree.contract_slice(xs, 0)
    with pytest.raises(RuntimeError):
        tree.contract_expectation([], texts, reuse=True)


def test_a_sliced_output_index():
    n = 10
    tree, arrays = circuit_tree(n, random_circuit(n, 5, seed=3), "complex128")
    big = max((p for p, _, _ in tree.traverse()), key=tree.get_size)
    inner = [ix for ix in tree.get_legs(big) if ix not in tree.output][:1]
    for ix in [tree.output[2]] + inner:
        tree.remove_ind_(ix)
    assert tree.nslices > 1 and tree.output[2] in tree.sliced_inds and tree.gathered_shape() == (2,) * n
    x = np.asarray(tree.contract(arrays))
    texts = ["IIZIIIIIII", "XXYIIIIIIZ", "IIYIIXIIII", "ZZZZZZZZZZ"]
    r = tree.contract_expectation(arrays, texts)
    pu.check_pauli(r.values, x, x.shape, [pu.codes(t) for t in texts])


def test_expression_expectation():
    from cotengra_amd import interface

    rng = np.random.default_rng(71)
    a, b = rng.standard_normal((2, 48, 7)), rng.standard_normal((7, 20, 2))
    interface.clear_expression_cache()
    try:
        expr = ca.einsum_expression("xab,bcy->xacy", a.shape, b.shape, cache_expression=True)
        out = np.asarray(expr(a, b))
        before = expr._bytes
        r = expr.expectation(a, b, paulis=["XIIZ", {"y": "X"}, "YIIY", {"x": "Y"}, {}])
        pu.check_pauli(r.values, out, out.shape, [pu.codes(t) for t in ("XIIZ", "IIIX", "YIIY", "YIII", "IIII")])
        assert r.values[3] == 0.0                                 # (a real contraction, one Y)
        assert expr._bytes == expr.device_bytes() > before        # (the scratch is counted)
        with pytest.raises(ValueError):
            expr.expectation(a, b, paulis="IXII")
        exs = ca.einsum_expression("xab,bcy->xacy", a.shape, b.shape, strip_exponent=True)
        mant, E = exs(a, b)
        rs = exs.expectation(a, b, paulis="ZIIX")
        pu.check_pauli(np.array([rs.values]), np.asarray(mant), out.shape, [pu.codes("ZIIX")])
        assert rs.exponent == E
        exs.close()
    finally:
        interface.clear_expression_cache()


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_circuit_pauli_expectation(dtype):
    n = 10
    gates = random_circuit(n, 5, seed=9)
    psi = statevector(n, gates)
    rel = 1e-10 if dtype == "complex128" else 1e-5                # the library's promise per amplitude
    texts = ["ZIIIIIIIII", "IZZIIIIIII", "XIIIIYIIIZ", "YYIIIIIIXX", "ZZZZZZZZZZ", "IIIIIIIIII"]
    ref = pu.pauli_reference(psi, psi.shape, [pu.codes(t) for t in texts])
    coeffs = [0.5, -1.0, 0.25, 2.0, -0.75, 1.0]
    values, norm, energy = circuits.pauli_expectation(n, gates, texts, coeffs=coeffs, dtype=dtype)
    assert values.shape == (6,) and abs(norm - 1) <= 4 * rel and np.all(np.abs(values - ref) <= 8 * rel)
    assert abs(energy - float(np.dot(coeffs, ref))) <= 8 * rel * np.abs(coeffs).sum()
    one, _ = circuits.pauli_expectation(n, gates, {0: "x", 5: "Y", 9: "z"}, dtype=dtype)
    assert np.ndim(one) == 0 and abs(one - ref[2]) <= 8 * rel
    # a conditional state: two qubits projected
    fixed = {1: 1, 7: 0}
    sub = np.take(np.take(psi, 1, axis=1), 0, axis=6)             # (qubit 1 = 1; qubit 7 is axis 6 of what is left)
    p = float(np.sum(np.abs(sub) ** 2))
    reqs = ["ZIIIIIIIII", {0: "X", 9: "Y"}, "IIYZIIIIXI"]
    sub_rows = [pu.codes("ZIIIIIII"), pu.codes("XIIIIIIY"), pu.codes("IYZIIIXI")]
    values, norm = circuits.pauli_expectation(n, gates, reqs, fixed=fixed, dtype=dtype)
    assert abs(norm - p) <= 4 * rel * p
    assert np.all(np.abs(values - pu.pauli_reference(sub, sub.shape, sub_rows) / p) <= 8 * rel)


def raw_call(ex, rank, ext, m, ops, out, handle="own"):
    i64p, u8p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    return runtime.load().ctg_exec_result_pauli(
        ex.handle if handle == "own" else handle, rank, None if ext is None else ext.ctypes.data_as(i64p), m,
        None if ops is None else ops.ctypes.data_as(u8p), None if out is None else out.ctypes.data_as(dp))


def test_refusals_through_the_c_abi():
    n = 2 ** 13
    x = gaussian(n, "complex64", seed=13)
    ex = resident(x)
    before = ex.device_bytes()
    ext = np.array([2, 2, 2048], np.int64)
    ops = np.array([[1, 3, 0], [2, 2, 0]], np.uint8)
    out = np.full(2, 7.0)
    big = np.zeros((4097, 3), np.uint8)
    bad = [
        (3, ext, 2, ops, out, None),                                           # a null exec
        (3, None, 2, ops, out, "own"), (3, ext, 2, None, out, "own"), (3, ext, 2, ops, None, "own"),
        (-1, ext, 2, ops, out, "own"),                                         # rank < 0
        (3, np.array([2, 2, 2047], np.int64), 2, ops, out, "own"),             # a wrong product
        (2, ext, 2, ops, out, "own"),
        (3, np.array([2, 2, 0], np.int64), 2, ops, out, "own"),
        (3, np.array([2 ** 21, 2 ** 21, 2], np.int64), 2, ops, out, "own"),    # past 2^40 elements before the last axis
        (3, ext, -1, ops, out, "own"), (3, ext, 4097, big, np.zeros(4097), "own"),
        (3, ext, 2, np.array([[1, 3, 0], [2, 4, 0]], np.uint8), out, "own"),   # a code above 3
        (3, ext, 2, np.array([[1, 3, 0], [0, 255, 0]], np.uint8), out, "own"),
        (3, ext, 2, np.array([[1, 3, 0], [0, 0, 1]], np.uint8), out, "own"),   # a letter on an axis of extent 2048
        (3, np.array([4, 1, 2048], np.int64), 2, np.array([[0, 3, 0], [0, 0, 0]], np.uint8), out, "own"),   # ... of extent 1
    ]
    for rank, e_, m, o_, out_, handle in bad:
        assert raw_call(ex, rank, e_, m, o_, out_, handle) == -1, (rank, m)
        assert runtime.load().ctg_last_error()
        assert np.all(out == 7.0)
    assert ex.device_bytes() == before                            # (nothing was launched, not even the scratch allocated)
    assert ex.download_result().tobytes() == x.tobytes()
    assert raw_call(ex, 3, ext, 0, ops, out) == 0 and np.all(out == 7.0) and ex.device_bytes() == before   # m = 0 does nothing
    # ... and the binding refuses the same before it calls
    for bad_ext, bad_ops in (([2, 2, 2047], ops), ([2, 2, 2048], [[1, 4, 0]]), ([2, 2, 2048], [[0, 0, 2]]),
                             ([2, 2, 2048], big), ([2, 2, 2048], [[1, 0]])):
        with pytest.raises(ValueError):
            ex.pauli_result(bad_ext, bad_ops)
    # a following valid call is correct
    assert raw_call(ex, 3, ext, 2, ops, out) == 0
    pu.check_pauli(out, x, (2, 2, 2048), ops)
    assert ex.pauli_result((2, 2, 2048), ops).tobytes() == out.tobytes()
    assert ex.device_bytes() > before and ex.download_result().tobytes() == x.tobytes()
    assert ex.pauli_result((2, 2, 2048), np.zeros((0, 3), np.uint8)).shape == (0,)
    # a NaN member: CTG_E_NORM
    badx = x.copy()
    badx[4097] = np.nan
    exn = resident(badx)
    assert raw_call(exn, 3, ext, 2, ops, out) == -6
    with pytest.raises(ValueError):
        exn.pauli_result((2, 2, 2048), ops)
    with pytest.raises(ValueError):
        one_tensor_tree(n).contract_expectation([badx], {})
    # an all-zero tensor: zeros, no error
    for shape, rows in (((2, 2, 2048), ops), ((2, 3, 2), np.array([[1, 0, 3], [2, 0, 2]], np.uint8))):
        zz = resident(np.zeros(int(np.prod(shape)), "complex64")).pauli_result(shape, rows)
        assert zz.shape == (2,) and not zz.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_names(dtype):
    t = {"float32": "float", "float64": "double", "complex64": "c64", "complex128": "c128"}[dtype]
    ex = resident(gaussian(2 ** 12, dtype, seed=1))
    for shape, ops in (((2,) * 12, strings_for(12)), ((4, 2, 512), [[0, 1, 0]]), ((2, 2048), [[3, 0]])):
        assert ex.pauli_variant(shape, ops) == runtime.pauli_variant(dtype, shape, ops) == f"pauli_chunk_kernel<{t}>"
    exg = resident(gaussian(2 ** 6 * 3, dtype, seed=2))
    for shape, ops in (((2,) * 6 + (3,), [[1, 0, 0, 0, 0, 3, 0]]), ((3, 64), [[0, 0]])):
        assert exg.pauli_variant(shape, ops) == runtime.pauli_variant(dtype, shape, ops) == f"pauli_general_kernel<{t}>"
    odd = [pu.bit_string(12, {4: "Y"})]
    assert ex.pauli_variant((2,) * 12, odd) == ("none" if np.dtype(dtype).kind != "c" else f"pauli_chunk_kernel<{t}>")
