"""CPU suite: the host side of reduced density matrices of the result tensor -- the header and
the binding, ``keep`` parsing and the argument errors that are raised before a device is touched, the permutation from
the tensor's order of the kept axes to the caller's, the spectrum helpers, and a check that the tolerance of
tests/rdm_util.py is not vacuous."""
import os
import re

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import _tree_contractor

import rdm_util as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_call_and_the_binding_mirrors_it():
    text = open(os.path.join(ROOT, "include", "ctg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = re.sub(r"\s+", " ", code)
    assert ("int ctg_exec_result_rdm(ctg_exec* exec, int64_t rank, const int64_t* extents, const int32_t* keep, "
            "void* out);") in flat
    m = re.search(r"#define\s+CTG_RDM_MAX_DIM\s+(\d+)", code)
    assert m and int(m.group(1)) == runtime.Executor.RDM_MAX_DIM == 64
    assert re.search(r"#define\s+CTG_ABI_VERSION\s+10\b", code) and runtime.ABI_VERSION == 10
    assert "ctg_exec_result_rdm" in runtime.SYMBOLS
    assert code.index("ctg_exec_result_marginal(") < code.index("ctg_exec_result_rdm(")
    lib = runtime.load()
    assert hasattr(lib, "ctg_exec_result_rdm")
    # the properties the header promises
    doc = re.sub(r"\s*\n\s*\*\s*", " ", text)
    for phrase in ("exactly Hermitian", "Im rho[a, a] is exactly 0.0", "No floating-point atomics",
                   "function of (extents, keep) alone", "Every product is formed in fp64"):
        assert phrase in doc, phrase


def test_methods_exist_on_every_layer():
    from cotengra_amd.interface import ContractExpression

    assert hasattr(ca.ContractionTree, "contract_rdm")
    assert hasattr(ContractExpression, "rdm") and hasattr(ca.HipContractor, "rdm")
    assert hasattr(runtime.Executor, "rdm_result")
    for name in ("reduced_density_matrix", "purity", "von_neumann_entropy"):
        assert hasattr(circuits, name)
    assert ca.RdmResult._fields == ("rho", "dims", "norm", "exponent")


def test_variant_names_follow_the_route():
    assert runtime.rdm_variant("complex64", (2,) * 12, [1] * 6 + [0] * 6) == "rdm_chunk_kernel<c64,4>"
    assert runtime.rdm_variant("float32", (4, 1024), [1, 0]) == "rdm_chunk_kernel<float,1>"
    assert runtime.rdm_variant("complex128", (32, 128), [1, 0]) == "rdm_chunk_kernel<c128,2>"
    assert runtime.rdm_variant("float64", (2,) * 12, [0] * 12) == "rdm_chunk_kernel<double,1>"
    assert runtime.rdm_variant("complex64", (2,) * 11, [1] + [0] * 10) == "rdm_general_kernel<c64>"
    assert runtime.rdm_variant("float64", (3, 4096), [1, 0]) == "rdm_general_kernel<double>"
    with pytest.raises(ValueError):
        runtime.rdm_variant("complex64", (128, 64), [1, 0])


def small_tree():
    return ca.ContractionTree.from_path([("a", "b"), ("b", "c", "d")], ("a", "c", "d"), {"a": 6, "b": 3, "c": 5, "d": 4},
                                        path=[(0, 1)])


def test_argument_errors_need_no_device(monkeypatch):
    tree = small_tree()
    fn = _tree_contractor(tree)

    def never(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(fn, "setup", never)
    xs = [np.ones((6, 3)), np.ones((3, 5, 4))]
    for bad in (["z"], ["a", "a"], ["b"], [["a"], ["b"]], "ac", 3):
        with pytest.raises(ValueError):
            fn.rdm(*xs, keep=bad)
    with pytest.raises(ValueError):
        tree.contract_rdm(xs, ["c", "c"])
    with pytest.raises(ValueError):
        fn.rdm(*xs, keep=["a", "c", "d"])              # D = 120 > 64
    with pytest.raises(ValueError):
        fn.rdm(*xs, keep=[["a"], ["d", "c", "a"]])     # ... in any request of a list
    with pytest.raises(ValueError):
        fn.rdm(*xs, keep=["a"], reuse=True)            # reuse=True with arrays
    with pytest.raises(RuntimeError):
        fn.rdm(keep=["a"], reuse=True)                 # ... before any call
    assert not fn._execs
    gates = [("x_1_2", (0,), ())]
    for bad in ([], [0, 0], [3], [-1]):
        with pytest.raises(ValueError):
            circuits.reduced_density_matrix(3, gates, bad)
    with pytest.raises(ValueError):
        circuits.reduced_density_matrix(3, gates, [0], fixed={0: 1})
    with pytest.raises(ValueError):
        circuits.reduced_density_matrix(3, gates, [0], fixed={1: 2})
    with pytest.raises(ValueError):
        circuits.reduced_density_matrix(8, gates, list(range(7)))   # D = 128


class StubExecutor:
    """Stands where the executor of a finished contraction would: ``rdm_result`` returns the reference in the
    tensor's own order of the kept axes."""

    handle = 1

    def __init__(self, out):
        self.out = np.asarray(out)
        self.calls = []

    def rdm_result(self, extents, keep):
        assert tuple(extents) == self.out.shape
        self.calls.append(tuple(keep))
        return du.rdm_reference(self.out, self.out.shape, [a for a, f in enumerate(keep) if f])

    def sample_info(self):
        return (float(np.sum(np.abs(self.out) ** 2)), 0.0, 0.0, 0, (0.0, 0.0))

    def get_exponent(self):
        return 0.0, False


def stubbed(tree, out, monkeypatch):
    fn = _tree_contractor(tree)
    ex = StubExecutor(out)
    monkeypatch.setattr(fn, "_reduce_state", lambda arrays, strip, check, reuse: ({"exec": ex}, False))
    return fn, ex


def test_rows_and_columns_in_the_callers_order(monkeypatch):
    rng = np.random.default_rng(5)
    tree = small_tree()
    out = rng.standard_normal((6, 5, 4)) + 1j * rng.standard_normal((6, 5, 4))
    fn, ex = stubbed(tree, out, monkeypatch)
    ad = fn.rdm(keep=["a", "d"])
    assert ad.rho.shape == (24, 24) and ad.dims == (6, 4) and ex.calls == [(1, 0, 1)]
    assert np.array_equal(ad.rho, du.rdm_reference(out, out.shape, [0, 2]))
    da = fn.rdm(keep=["d", "a"])
    assert da.dims == (4, 6)
    assert np.array_equal(da.rho, du.rdm_reference(out, out.shape, [2, 0]))
    assert not np.array_equal(da.rho, ad.rho)
    assert abs(np.trace(ad.rho).real - ad.norm) <= 1e-12 * ad.norm and ad.exponent == 0.0
    # a list of requests: a list of matrices from one contraction
    many = fn.rdm(keep=[["c"], [], ["d", "c"], ["c", "d"]])
    assert isinstance(many.rho, list) and [r.shape for r in many.rho] == [(5, 5), (1, 1), (20, 20), (20, 20)]
    assert many.dims == [(5,), (), (4, 5), (5, 4)]
    for rho, axes in zip(many.rho, ([1], [], [2, 1], [1, 2])):
        assert np.array_equal(rho, du.rdm_reference(out, out.shape, axes))
    assert abs(many.rho[1][0, 0].real - many.norm) <= 1e-12 * many.norm


def test_an_output_index_projected_to_size_one(monkeypatch):
    rng = np.random.default_rng(6)
    tree = small_tree().remove_ind("c", project=2)
    assert tree.gathered_shape() == (6, 1, 4)
    out = rng.standard_normal((6, 1, 4))
    fn, ex = stubbed(tree, out, monkeypatch)
    r = fn.rdm(keep=[["d", "c"], ["c"], ["c", "a"]])
    assert [x.shape for x in r.rho] == [(4, 4), (1, 1), (6, 6)] and r.dims == [(4, 1), (1,), (1, 6)]
    assert r.rho[0].dtype == np.float64
    assert np.array_equal(r.rho[0], du.rdm_reference(out, out.shape, [2, 1]))
    assert np.array_equal(r.rho[2], du.rdm_reference(out, out.shape, [1, 0]))
    assert ex.calls == [(0, 1, 1), (0, 1, 0), (1, 1, 0)]


def test_purity_and_entropy_of_a_bell_pair_and_a_product_state():
    bell = np.zeros((2, 2), complex)
    bell[0, 0] = bell[1, 1] = 2 ** -0.5
    one = du.rdm_reference(bell, (2, 2), [0])
    assert abs(circuits.von_neumann_entropy(one) - 1.0) <= 1e-12 and abs(circuits.purity(one) - 0.5) <= 1e-12
    assert abs(circuits.von_neumann_entropy(one, base=np.e) - np.log(2)) <= 1e-12
    both = du.rdm_reference(bell, (2, 2), [0, 1])
    assert abs(circuits.von_neumann_entropy(both)) <= 1e-12 and abs(circuits.purity(both) - 1.0) <= 1e-12
    # a product state, not normalised: every subsystem is pure
    rng = np.random.default_rng(8)
    u, v = rng.standard_normal(4) + 1j * rng.standard_normal(4), rng.standard_normal(8) + 1j * rng.standard_normal(8)
    prod = np.outer(u, v)
    for axes in ([0], [1]):
        rho = du.rdm_reference(prod, prod.shape, axes)
        assert abs(circuits.von_neumann_entropy(rho)) <= 1e-9 and abs(circuits.purity(rho) - 1.0) <= 1e-12
    # the maximally mixed state of dimension 8, and a negative eigenvalue from rounding is clipped
    assert abs(circuits.von_neumann_entropy(np.eye(8)) - 3.0) <= 1e-12 and abs(circuits.purity(np.eye(8)) - 0.125) <= 1e-12
    assert circuits.von_neumann_entropy(np.diag([1.0, -1e-17])) == 0.0
    with pytest.raises(ValueError):
        circuits.purity(np.zeros((2, 2)))


def test_reference_against_brute_force():
    rng = np.random.default_rng(2)
    shape = (2, 3, 1, 4)
    x = (rng.integers(-3, 4, size=shape) + 1j * rng.integers(-3, 4, size=shape)).astype("complex64")
    for axes in ([], [0], [3, 1], [1, 3], [0, 1, 2, 3]):
        ref = du.rdm_reference(x, shape, axes)
        dims = [shape[a] for a in axes]
        brute = np.zeros((int(np.prod(dims)),) * 2, complex)
        for pa in np.ndindex(*shape):
            for pb in np.ndindex(*shape):
                if all(pa[k] == pb[k] for k in range(4) if k not in axes):
                    ia = int(np.ravel_multi_index([pa[k] for k in axes], dims)) if axes else 0
                    ib = int(np.ravel_multi_index([pb[k] for k in axes], dims)) if axes else 0
                    brute[ia, ib] += complex(x[pa]) * np.conj(complex(x[pb]))
        assert ref.dtype == np.complex128 and np.array_equal(ref, brute)     # (small integers: exact in any order)
        du.check_rdm(ref, x, shape, axes)
    with pytest.raises(AssertionError):
        ref = du.rdm_reference(x, shape, [0])
        du.check_rdm(ref * (1 + 1e-9), x, shape, [0])
    assert du.rdm_reference(x.real, shape, [1]).dtype == np.float64


def test_the_bound_is_not_vacuous():
    """Two numpy summation orders -- ``@`` and a reversed sum of chunks of 512 columns -- at t = 2^18, D = 8: their
    difference must lie within the bound a device result is held to, and the fraction of it they use is printed."""
    t, d = 2 ** 18, 8
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((d, t)) + 1j * rng.standard_normal((d, t))).astype("complex64")
    X = du.rdm_matrix(x, (d, t), [0])
    ref = X @ X.conj().T
    other = np.zeros((d, d), complex)
    for c in reversed(range(0, t, 512)):
        blk = X[:, c:c + 512][:, ::-1]
        other = other + np.einsum("ak,bk->ab", blk, blk.conj())
    err, tol = du.rdm_errors(other, ref), du.rdm_tol(ref, t)
    frac = float(np.max(err / tol))
    print(f"two numpy orders at t=2^18: max |difference| / bound = {frac:.3e}")
    assert np.all(err <= tol) and 0 < frac < 1
