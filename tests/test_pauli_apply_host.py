"""CPU suite: the host side of a Pauli sum applied to the result tensor and of the energy gradients built on it
 -- the header and the binding, the methods of every layer, the reference of
tests/pauli_apply_util.py against dense Kronecker products and against the expectation values' reference, the gradient
reference against central finite differences and the VJP convention, a check that the tolerance is not vacuous, and the
argument errors that are raised before a device is touched."""
import os
import re

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import _tree_contractor
from oracle import contract_ref as orc

import pauli_apply_util as au
import pauli_util as pu
import vjp_util as V
from test_circuits import random_circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_call_and_the_binding_mirrors_it():
    text = open(os.path.join(ROOT, "include", "ctg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = re.sub(r"\s+", " ", code)
    assert ("int ctg_exec_result_pauli_apply(ctg_exec* exec, int64_t rank, const int64_t* extents, int64_t m, "
            "const uint8_t* ops, const double* coeffs, void* dev_out, void* host_out);") in flat
    assert re.search(r"#define\s+CTG_ABI_VERSION\s+10\b", code) and runtime.ABI_VERSION == 10
    assert code.index("ctg_exec_result_pauli(") < code.index("ctg_exec_result_pauli_apply(")
    assert "ctg_exec_result_pauli_apply" in runtime.SYMBOLS
    assert hasattr(runtime.load(), "ctg_exec_result_pauli_apply")
    doc = re.sub(r"\s*\n\s*\*\s*", " ", text)
    for phrase in ("No atomics", "function of (dtype, extents, ops in order, coeffs, the tensor's bytes) alone",
                   "each rounded once, nothing fused", "m = 0 writes zeros", "never written"):
        assert phrase in doc, phrase


def test_methods_exist_on_every_layer():
    from cotengra_amd.interface import ContractExpression

    assert hasattr(runtime.Executor, "pauli_apply_result") and hasattr(runtime.Executor, "pauli_apply_variant")
    assert hasattr(runtime, "pauli_apply_variant")
    assert hasattr(ca.HipContractor, "apply_paulis") and hasattr(ca.HipContractor, "energy")
    assert hasattr(ca.ContractionTree, "contract_apply_paulis") and hasattr(ca.ContractionTree, "contract_energy")
    assert hasattr(ContractExpression, "energy") and hasattr(circuits, "energy_gradient")
    assert ca.ApplyResult._fields == ("y", "norm", "exponent")
    assert ca.EnergyResult._fields == ("energy", "values", "norm", "grads")


def test_kernel_names():
    z = [pu.bit_string(6, {0: "Z"})]
    assert runtime.pauli_apply_variant("complex64", (2,) * 6, z) == "pauli_apply_general_kernel<c64>"
    assert runtime.pauli_apply_variant("complex64", (2,) * 12, [pu.bit_string(12, {3: "Y"})]) == "pauli_apply_kernel<c64>"
    assert runtime.pauli_apply_variant("float32", (4, 2, 512), [[0, 3, 0]]) == "pauli_apply_kernel<float>"
    assert runtime.pauli_apply_variant("complex128", (2, 2048), [[1, 0]]) == "pauli_apply_kernel<c128>"
    assert runtime.pauli_apply_variant("float64", (2,) * 10 + (3, 2), [[0] * 12]) == "pauli_apply_general_kernel<double>"
    assert runtime.pauli_apply_variant("complex64", (2,) * 12, np.zeros((0, 12), np.uint8)) == "none"
    with pytest.raises(ValueError):
        runtime.pauli_apply_variant("float32", (2,) * 12, [pu.bit_string(12, {3: "Y"})])   # P x is not real
    with pytest.raises(ValueError):
        runtime.pauli_apply_variant("complex64", (4, 1024), [[1, 0]])


def some_strings(L, rng, m=9):
    rows = [[0] * L, pu.bit_string(L, {0: "X"}), pu.bit_string(L, {1: "Y"}), pu.bit_string(L, {L - 1: "Z", 0: "Y", 2: "Y"}),
            pu.bit_string(L, {0: "Y", 1: "Y", 2: "Y", 3: "X"})]
    rows += rng.integers(0, 4, size=(m - len(rows), L)).tolist()
    return np.array(rows, dtype=np.uint8)


def test_reference_against_dense_kronecker_products():
    rng = np.random.default_rng(17)
    L = 6
    shape = (2,) * L
    x = rng.standard_normal(2 ** L) + 1j * rng.standard_normal(2 ** L)
    ops = some_strings(L, rng)
    coeffs = rng.standard_normal(len(ops))
    ref = au.pauli_apply_reference(x, shape, ops, coeffs).reshape(-1)
    dense = sum(c * pu.dense_string(row, shape) @ x for row, c in zip(ops.tolist(), coeffs))
    assert np.abs(ref - dense).max() <= 1e-13 * np.abs(coeffs).sum() * np.abs(x).max()
    # the formula of the header: (P x)[j] = i^ny (-1)^popcount((j ^ xm) & zm) x[j ^ xm]
    j = np.arange(2 ** L)
    for row, (xm, zm, ny) in zip(ops.tolist(), runtime.pauli_masks(shape, ops)):
        sign = np.array([(-1.0) ** bin((int(k) ^ xm) & zm).count("1") for k in j])
        assert np.allclose((1j) ** ny * sign * x[j ^ xm], pu.dense_string(row, shape) @ x, rtol=0, atol=1e-14)
    # a real tensor, even numbers of Y only
    xr = rng.standard_normal(2 ** L)
    even = ops[(ops == 2).sum(axis=1) % 2 == 0]
    rr = au.pauli_apply_reference(xr, shape, even, coeffs[:len(even)])
    assert rr.dtype == np.float64
    dr = sum(c * pu.dense_string(row, shape) @ xr for row, c in zip(even.tolist(), coeffs))
    assert np.abs(dr.imag).max() == 0 and np.abs(rr.reshape(-1) - dr.real).max() <= 1e-13 * np.abs(coeffs).sum() * np.abs(xr).max()


def test_energy_of_the_reference_equals_the_expectation_values():
    rng = np.random.default_rng(18)
    L = 10
    shape = (2,) * L
    x = (rng.standard_normal(2 ** L) + 1j * rng.standard_normal(2 ** L)).astype("complex64")
    ops = some_strings(L, rng, m=12)
    coeffs = rng.standard_normal(len(ops))
    y = au.pauli_apply_reference(x, shape, ops, coeffs)
    lhs = float(np.real(np.vdot(pu.widen(x), y.reshape(-1))))
    rhs = float(np.dot(coeffs, pu.pauli_reference(x, shape, ops)))
    tol_y = au.pauli_apply_tol(x, shape, ops, coeffs, ref=y)
    bound = float(np.sum(2.0 * np.abs(pu.widen(x)).reshape(shape) * tol_y)) + np.abs(coeffs).sum() * pu.pauli_tol(x, x.size)
    assert abs(lhs - rhs) <= bound


def sliced_circuit_tree(n=5, depth=3, seed=4, template=None, out_slice=True):
    inputs, output, sd, arrays = circuits.circuit_to_network(n, random_circuit(n, depth, seed=seed), template or "?" * n,
                                                             simplify=True, dtype="complex128")
    tree = ca.array_contract_tree(inputs, output, sd)
    big = max((p for p, _, _ in tree.traverse()), key=tree.get_size)
    inner = [ix for ix in tree.get_legs(big) if ix not in tree.output][:1]
    for ix in ([tree.output[1]] if out_slice else []) + inner:
        tree.remove_ind_(ix)
    assert tree.nslices > 1
    return tree, arrays


def test_gradient_reference_against_finite_differences_and_the_vjp_convention():
    """A tiny tree sliced on an output and an inner index, complex128: torch's gradient of ``E = Re vdot(O, H O)`` equals
    central differences of the numpy oracle's energy along random directions, and ``conj(reference_vjp(h = conj(2 y)))``
    -- what ``HipContractor.energy`` computes."""
    tree, arrays = sliced_circuit_tree()
    rng = np.random.default_rng(19)
    L = len(tree.output)
    ops = some_strings(L, rng, m=8)
    coeffs = rng.standard_normal(len(ops))
    for normalize in (False, True):
        if normalize:
            arrays = [a * 1.3 for a in arrays]   # (a norm other than 1)
        energy, grads = au.reference_energy_grads(tree, arrays, ops, coeffs, normalize=normalize)
        out = np.asarray(orc.contract(tree, arrays)).reshape(tree.gathered_shape())
        assert abs(energy - au.energy_numpy(out, ops, coeffs, normalize)) <= 1e-12 * np.abs(coeffs).sum()
        for i in (0, len(arrays) // 2, len(arrays) - 1):
            d = rng.standard_normal(arrays[i].shape) + 1j * rng.standard_normal(arrays[i].shape)
            h = 1e-5
            es = []
            for sgn in (1, -1):
                moved = list(arrays)
                moved[i] = arrays[i] + sgn * h * d
                o = np.asarray(orc.contract(tree, moved)).reshape(tree.gathered_shape())
                es.append(au.energy_numpy(o, ops, coeffs, normalize))
            fd = (es[0] - es[1]) / (2 * h)
            an = float(np.sum(grads[i].real * d.real + grads[i].imag * d.imag))
            assert abs(fd - an) <= 1e-7 * max(1.0, abs(an)), (normalize, i, fd, an)
        if not normalize:
            y = au.pauli_apply_reference(out, out.shape, ops, coeffs)
            vj = V.reference_vjp(tree, arrays, np.conj(2.0 * y))
            for g, v in zip(grads, vj):
                assert np.abs(g - 2.0 * np.conj(v) / 2.0).max() <= 1e-12 * max(1.0, np.abs(g).max())


def test_the_bound_is_not_vacuous():
    """Two numpy associations at n = 2^14 and 24 strings -- string after string, and the weights of a group summed
    first (the device's) -- must differ by less than the bound; one term of median size with the wrong sign must exceed
    it by a wide factor."""
    L = 14
    shape = (2,) * L
    rng = np.random.default_rng(20)
    x = (rng.standard_normal(2 ** L) + 1j * rng.standard_normal(2 ** L)).astype("complex64")
    zs = [pu.bit_string(L, {int(b): "Z" for b in rng.choice(L, size=3, replace=False)}) for _ in range(12)]
    xs = [pu.bit_string(L, {0: "X", 13: "Y", int(b): "Z"}) for b in rng.choice(np.arange(1, 13), size=12, replace=False)]
    ops = np.array(zs + xs, dtype=np.uint8)
    coeffs = rng.standard_normal(len(ops))
    ref = au.pauli_apply_reference(x, shape, ops, coeffs)
    tol = au.pauli_apply_tol(x, shape, ops, coeffs, ref=ref)
    w = pu.widen(x).reshape(shape)
    other = np.zeros(shape, dtype=np.complex128)
    for group in (range(0, 12), range(12, 24)):
        weight = np.zeros(shape, dtype=np.complex128)
        unit = np.ones(shape, dtype=np.complex128)
        flip = [a for a, op in enumerate(ops[group[0]]) if op in (1, 2)]
        for s in group:
            # P_s x = weight_s(j) x[j ^ xm]: apply the string to the all-ones tensor
            weight = weight + coeffs[s] * pu.apply_string(unit, shape, ops[s].tolist())
        other = other + weight * (np.flip(w, axis=flip) if flip else w)
    err = np.maximum(np.abs((other - ref).real), np.abs((other - ref).imag))
    frac = float((err / tol).max())
    terms = np.abs(coeffs[:, None]) * np.abs(w.real).reshape(1, -1)
    flipped = 2.0 * float(np.median(terms))
    print(f"two numpy associations use {frac:.3e} of the bound; a flipped median term is {flipped / float(np.median(tol)):.3e} bounds")
    assert frac < 1 and flipped > 1e3 * float(np.median(tol)) and flipped > 1e3 * float(tol.max())


def test_argument_errors_need_no_device(monkeypatch):
    tree, arrays = sliced_circuit_tree()
    fn = _tree_contractor(tree)

    def never(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(fn, "setup", never)
    monkeypatch.setattr(fn, "_reduce_state", never)
    L = len(tree.output)
    good = ["Z" + "I" * (L - 1), "X" * L]
    for call in (fn.energy, fn.apply_paulis):
        for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, float("nan")], [float("inf"), 0.0], [1.0, 1j], ["a", "b"]):
            with pytest.raises(ValueError):
                call(*arrays, paulis=good, coeffs=bad)
        with pytest.raises(ValueError):
            call(*arrays, paulis=["Q" + "I" * (L - 1)])
    for bad_wrt in ([-1], [len(arrays)], [0, 99]):
        with pytest.raises((IndexError, ValueError)):
            fn.energy(*arrays, paulis=good, wrt=bad_wrt)
    with pytest.raises((IndexError, ValueError)):
        tree.contract_energy(arrays, good, wrt=[len(arrays)])
    # a real contraction: a string with an odd number of Y is refused by apply_paulis before the device
    real = [np.ascontiguousarray(a.real) for a in arrays]
    with pytest.raises(ValueError):
        fn.apply_paulis(*real, paulis=["Y" + "I" * (L - 1)])
    # (a valid request reaches the device)
    with pytest.raises(AssertionError):
        fn.energy(*arrays, paulis=good, coeffs=[0.5, -1.0])
    # normalize adds an identity term: 4096 strings without an identity among them leave no room for it
    full = ["Z" + "I" * (L - 1)] * 4096
    for call in (fn.energy, fn.energy_autograd):
        with pytest.raises(ValueError, match="identity"):
            call(*arrays, paulis=full, normalize=True)
    with pytest.raises(AssertionError):
        fn.energy(*arrays, paulis=full)                                    # (without normalize it reaches the device)
    with pytest.raises(AssertionError):
        fn.energy(*arrays, paulis=full[:-1] + ["I" * L], normalize=True)   # (the identity string takes the term)
    # strip_exponent is refused, as vjp refuses it
    fs = ca.HipContractor(tree, strip_exponent=True)
    with pytest.raises(ValueError):
        fs.energy(*arrays, paulis=good)
    # the executor binding refuses before it calls
    ex = runtime.Executor.__new__(runtime.Executor)
    ex.plan = type("P", (), {"dtype": "float32"})()
    ex.handle = None
    for ext, ops, cs in (((2, 2), [[1, 0]], [1.0, 2.0]), ((2, 2), [[1, 0]], [float("nan")]), ((2, 2), [[2, 0]], [1.0]),
                         ((2, 3), [[0, 1]], [1.0])):
        with pytest.raises(ValueError):
            ex.pauli_apply_result(ext, ops, cs)


def test_normalize_with_norm_zero_is_refused():
    """``normalize=True`` on a result of norm zero: ``ValueError`` from the host check on the statistics, before the
    apply call or the VJP plan exist."""
    tree, arrays = sliced_circuit_tree()
    fn = ca.HipContractor(tree)

    class Ex:
        def pauli_result(self, extents, ops):
            return np.zeros(len(ops))

        def sample_info(self):
            return (0.0, 0.0, 0.0, 0)

        def __getattr__(self, name):
            raise AssertionError(f"the device was touched: {name}")

    fn._reduce_state = lambda *a, **k: ({"exec": Ex()}, False)
    with pytest.raises(ValueError, match="norm zero"):
        fn.energy(*arrays, paulis=["Z" + "I" * (len(tree.output) - 1)], normalize=True)


def test_circuit_argument_errors_need_no_device(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the network was built")

    monkeypatch.setattr(circuits, "circuit_to_network", never)
    gates = [("x_1_2", (0,), ()), ("rz", (1,), (0.3,))]
    for bad in ("XZ", "XZIQ", {3: "X"}, {0: "W"}, 5):
        with pytest.raises(ValueError):
            circuits.energy_gradient(3, gates, bad, [1.0])
    with pytest.raises(ValueError):
        circuits.energy_gradient(3, gates, "XII", [1.0], fixed={0: 1})
    with pytest.raises(ValueError):
        circuits.energy_gradient(3, gates, ["IIZ", "ZII"], [1.0])
    with pytest.raises(ValueError):
        circuits.energy_gradient(3, gates, ["IIZ", "ZII"], [1.0, float("nan")])
    with pytest.raises(ValueError):
        circuits.energy_gradient(3, gates, ["IIZ", "ZII"], None)
    with pytest.raises(AssertionError):
        circuits.energy_gradient(3, gates, ["IIZ", {0: "x"}], [1.0, -0.5], fixed={1: 0})


def test_gate_derivatives_are_the_derivatives():
    for name, ps in (("rz", (0.37,)), ("fs", (1.1, -0.6)), ("x_1_2", ())):
        ds = circuits.gate_derivatives(name, ps)
        assert len(ds) == len(ps)
        for k, d in enumerate(ds):
            h = 1e-6
            up, dn = list(ps), list(ps)
            up[k] += h
            dn[k] -= h
            fd = (circuits.gate_matrix(name, up) - circuits.gate_matrix(name, dn)) / (2 * h)
            assert np.abs(fd - d).max() <= 1e-9
