"""CPU suite: the host side of top-k and marginals of the result tensor -- the header and the
binding, the references of tests/reduce_util.py against brute force, and the argument errors that are raised from
Python before a device is touched."""
import itertools
import os
import re

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import _tree_contractor

import reduce_util as ru
import sample_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    return open(os.path.join(ROOT, "include", "ctg_hip.h")).read()


def test_header_declares_the_calls_without_an_abi_bump():
    text = header_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = re.sub(r"\s+", " ", code)
    assert "int ctg_exec_result_topk(ctg_exec* exec, int64_t k, int64_t* idx, void* elems, double* p);" in flat
    assert ("int ctg_exec_result_marginal(ctg_exec* exec, int64_t rank, const int64_t* extents, const int32_t* keep, "
            "double* out);") in flat
    assert re.search(r"#define\s+CTG_TOPK_MAX\s+\(1 << 20\)", code)
    assert re.search(r"#define\s+CTG_ABI_VERSION\s+10\b", code)
    assert runtime.ABI_VERSION == 10
    assert "ctg_exec_result_topk" in runtime.SYMBOLS and "ctg_exec_result_marginal" in runtime.SYMBOLS
    assert runtime.Executor.TOPK_MAX == 1 << 20
    # the calls come after the ABI-10 block, and the header says that they were added without a bump
    assert code.index("ctg_exec_range_audit(") < code.index("ctg_exec_result_topk(") < code.index("ctg_exec_result_marginal(")
    assert "WITHOUT a bump" in text


def test_methods_exist_on_every_layer():
    from cotengra_amd.interface import ContractExpression

    for name in ("contract_topk", "contract_marginal"):
        assert hasattr(ca.ContractionTree, name)
    for cls in (ContractExpression, ca.HipContractor):
        assert hasattr(cls, "topk") and hasattr(cls, "marginal")
    assert hasattr(runtime.Executor, "topk_result") and hasattr(runtime.Executor, "marginal_result")
    assert hasattr(circuits, "top_chaotic")
    assert ca.TopKResult._fields == ("indices", "coords", "amplitudes", "p", "norm", "sum_p2", "exponent")
    assert ca.MarginalResult._fields == ("p", "norm", "exponent")


def brute_topk(p, k):
    order = sorted(range(len(p)), key=lambda i: (-p[i], i))
    return order[:k]


def test_topk_reference_against_brute_force():
    rng = np.random.default_rng(1)
    cases = [rng.standard_normal(17), np.round(2 * rng.standard_normal(40)) / 2, np.ones(9), np.zeros(5),
             np.array([-0.0, 0.0, 1.0, -1.0, 0.5]), (rng.standard_normal(11) + 1j * rng.standard_normal(11)).astype("complex64")]
    for x in cases:
        p = su.probabilities(x)
        for k in (1, 2, len(x) // 2, len(x)):
            idx, pk = ru.topk_reference(x, k)
            assert idx.dtype == np.int64 and list(idx) == brute_topk(list(p), k)
            assert pk.tobytes() == p[idx].tobytes()
    idx, _ = ru.topk_reference(np.ones(9), 4)
    assert list(idx) == [0, 1, 2, 3]
    idx, _ = ru.topk_reference(np.array([1.0, 2.0, -2.0, 1.0, 2.0]), 4)
    assert list(idx) == [1, 2, 4, 0]


def test_marginal_reference_against_brute_force():
    rng = np.random.default_rng(2)
    shape = (2, 3, 1, 4)
    x = (rng.integers(-3, 4, size=shape) + 1j * rng.integers(-3, 4, size=shape)).astype("complex128")
    p = su.probabilities(x).reshape(shape)
    for r in range(len(shape) + 1):
        for keep in itertools.combinations(range(len(shape)), r):
            ref = ru.marginal_reference(x, shape, keep)
            assert ref.shape == tuple(shape[a] for a in keep)
            brute = np.zeros(ref.shape)
            for pos in itertools.product(*[range(d) for d in shape]):
                brute[tuple(pos[a] for a in keep)] += p[pos]
            assert np.array_equal(ref, brute)   # (small integers: exact in any order)
            ru.check_marginal(ref, x, shape, keep)
    assert np.array_equal(ru.marginal_tol(np.array([1.0, 4.0]), 8), 2.0 * 8 * 2.0 ** -53 * np.array([1.0, 4.0]))
    with pytest.raises(AssertionError):
        ru.check_marginal(ru.marginal_reference(x, shape, (0,)) * (1 + 1e-9), x, shape, (0,))


def test_argument_errors_need_no_device():
    tree = ca.ContractionTree.from_path([("a", "b"), ("b", "c")], ("a", "c"), {"a": 4, "b": 3, "c": 5}, path=[(0, 1)])
    fn = _tree_contractor(tree)
    a, b = np.ones((4, 3)), np.ones((3, 5))
    for bad in (0, -1):
        with pytest.raises(ValueError):
            fn.topk(a, b, k=bad)
        with pytest.raises(ValueError):
            tree.contract_topk([a, b], bad)
    for bad in (1.5, "3", None, True):
        with pytest.raises(TypeError):
            fn.topk(a, b, k=bad)
    with pytest.raises(ValueError):
        fn.topk(a, b, k=21)                      # (the result has 20 elements)
    for bad in (["z"], ["a", "a"], ["b"], [["a"], ["b"]], "ac", 3):
        with pytest.raises(ValueError):
            fn.marginal(a, b, keep=bad)
    with pytest.raises(ValueError):
        tree.contract_marginal([a, b], ["c", "c"])
    with pytest.raises(ValueError):
        fn.topk(a, b, k=1, reuse=True)           # reuse=True with arrays
    with pytest.raises(ValueError):
        fn.marginal(a, b, keep=["a"], reuse=True)
    with pytest.raises(RuntimeError):
        fn.topk(k=1, reuse=True)                 # ... before any call
    with pytest.raises(RuntimeError):
        fn.marginal(keep=["a"], reuse=True)
    assert not fn._execs                         # nothing was created on a device
    with pytest.raises(ValueError):
        circuits.top_chaotic(3, [("x_1_2", (0,), ())], [0, 1], top=5)
    with pytest.raises(ValueError):
        circuits.top_chaotic(3, [("x_1_2", (0,), ())], [0, 1], top=0)
