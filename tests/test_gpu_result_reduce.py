"""GPU suite: the k most probable members, and marginals, of the result tensor on the device (csrc/ctg_reduce.hip,
DESIGN.md section 12) -- ``HipContractor.topk`` / ``.marginal``, ``ContractionTree.contract_topk`` /
``.contract_marginal``, ``ContractExpression.topk`` / ``.marginal``, ``circuits.top_chaotic``.

Data reaches the result tensor bit for bit through a one-tensor tree (a single copy step), as in
tests/test_gpu_sample.py.  The references and the tolerance of a marginal are in tests/reduce_util.py: top-k is
compared exactly, a marginal within ``2 t 2^-53`` of the reference per output (t elements per output), which is
derived from the error of two summation orders and never from what the device returns."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import _tree_contractor

import reduce_util as ru
import sample_util as su
from test_gpu_sample import gaussian, one_tensor_tree, random_circuit, statevector

pytestmark = pytest.mark.gpu

B = 4096             # kSampleBlock
COMPACT = 1 << 16    # kTopkCompact of csrc/ctg_reduce.hip: the select finishes on a list once this few keys survive
TOPK_MAX = 1 << 20   # CTG_TOPK_MAX
DTYPES = ["float32", "float64", "complex64", "complex128"]
HERE = os.path.dirname(os.path.abspath(__file__))


def check_topk(res, x, k):
    """``res`` (a TopKResult or an ``(idx, elems, p)`` triple) is the reference, index for index and bit for bit."""
    idx, amps, p = (res.indices, res.amplitudes, res.p) if hasattr(res, "indices") else res
    ridx, rp = ru.topk_reference(x, k)
    # (what the result tensor holds: the executor adds the slice into a zeroed result, so a -0.0 of the input is
    # held as +0.0 and every other value bit for bit)
    flat = np.asarray(x).reshape(-1) + 0
    assert idx.dtype == np.int64 and idx.shape == (k,)
    assert np.array_equal(idx, ridx), (k, idx[:8], ridx[:8], int(np.flatnonzero(idx != ridx)[0]))
    assert amps.dtype == flat.dtype and amps.tobytes() == flat[ridx].tobytes()
    assert p.dtype == np.float64 and p.tobytes() == rp.tobytes()


def topk_many(x, ks):
    """Contract once, then every k of ``ks`` on the result left there."""
    tree = one_tensor_tree(x.size)
    out = {}
    for i, k in enumerate(ks):
        out[k] = tree.contract_topk([x], k) if i == 0 else tree.contract_topk([], k, reuse=True)
    return out


def resident(x):
    """The executor of the one-tensor tree with ``x`` in its result tensor."""
    ex = _tree_contractor(one_tensor_tree(x.size)).setup(x)["exec"]
    ex.zero_result()
    ex.run_slices()
    return ex


# ---- top-k ---------------------------------------------------------------------------------------------------- #


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 17, 2 ** 20 + 3])
def test_topk_exact_against_the_reference(n, dtype):
    x = gaussian(n, dtype, seed=n)
    ks = sorted({k for k in (1, 2, 64, 65, min(n, 4097), n) if k <= n})
    too_many = [k for k in ks if k > TOPK_MAX]
    res = topk_many(x, [k for k in ks if k <= TOPK_MAX])
    p = su.probabilities(x)
    for k, r in res.items():
        check_topk(r, x, k)
        assert r.coords.shape == (k, 1) and np.array_equal(r.coords[:, 0], r.indices)
        assert abs(r.norm - p.sum()) <= su.default_tol(p, np.array([p.sum()])) and r.exponent == 0.0
    # (k = n above CTG_TOPK_MAX: the call refuses it, as the header says)
    for k in too_many:
        with pytest.raises(ValueError):
            one_tensor_tree(n).contract_topk([x], k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_topk_half_integers_have_thousands_of_ties(dtype):
    n = 3 * B + 17
    x = (np.round(2 * gaussian(n, dtype, seed=7)) / 2).astype(dtype)
    assert np.unique(su.probabilities(x)).size < 200
    for k, r in topk_many(x, [1, 64, 1000, B + 5, n]).items():
        check_topk(r, x, k)


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_topk_all_equal_and_all_zero_take_the_lowest_indices(dtype):
    n, k = 3 * B + 17, B + 5
    r = one_tensor_tree(n).contract_topk([np.ones(n, dtype)], k)
    assert np.array_equal(r.indices, np.arange(k)) and np.all(r.p == 1.0) and np.all(r.amplitudes == 1)
    z = one_tensor_tree(n).contract_topk([np.zeros(n, dtype)], k)      # (no error: unlike sampling)
    assert np.array_equal(z.indices, np.arange(k)) and np.all(z.p == 0.0) and z.norm == 0.0
    check_topk(z, np.zeros(n, dtype), k)


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_topk_threshold_class_straddles_waves_and_blocks(dtype):
    """Two members above, the class of the threshold at 63, 64, B - 1, B, 2B + 1, everything else below: every k
    that cuts inside the class takes its members in index order; the larger k go on into the class of the rest."""
    n = 3 * B + 17
    cls = [63, 64, B - 1, B, 2 * B + 1]
    x = np.ones(n, dtype)
    x[cls] = -2
    x[[B + 7, 10]] = 3
    for k, r in topk_many(x, [1, 2, 3, 4, 5, 6, 7, 8, 70, B + 9]).items():
        check_topk(r, x, k)
        if 2 < k <= 7:
            assert list(r.indices) == [10, B + 7] + cls[:k - 2]


def test_topk_all_equal_above_the_compact_bound_never_compacts():
    """The class never shrinks below kTopkCompact: all six digit passes read the tensor."""
    n = COMPACT + B + 3
    x = np.full(n, 0.75, "complex64")
    for k, r in topk_many(x, [1, COMPACT + 77, n]).items():
        assert np.array_equal(r.indices, np.arange(k)) and np.all(r.p == 0.5625)
    # ... and a class that stays above the bound for three passes, then splits: digit passes over the tensor first,
    # the compact list afterwards
    n = 3 * COMPACT + 5
    y = gaussian(n, "float64", seed=3)
    y[::2] = 1.0 + (np.arange(y[::2].size) % 4096) * 2.0 ** -40
    for k, r in topk_many(y, [COMPACT // 4, n // 2 + 9]).items():
        check_topk(r, y, k)


def test_topk_range_of_36_decades_and_subnormal_p():
    n = 3 * B + 17
    rng = np.random.default_rng(21)
    mod = 10.0 ** rng.uniform(-18, 0, n)
    x = (mod * np.exp(2j * np.pi * rng.random(n))).astype("complex64")
    for k, r in topk_many(x, [1, 64, 4097, n]).items():
        check_topk(r, x, k)
    y = gaussian(n, "float64", seed=23) * 1e-160
    y[5::7] = -0.0
    y[6::11] = 0.0
    p = su.probabilities(y)
    assert 0 < p.max() < np.finfo(np.float64).tiny and np.any(np.signbit(y) & (y == 0))
    for k, r in topk_many(y, [1, 65, n - 2000, n]).items():
        check_topk(r, y, k)


def test_topk_bad_k_raises_and_launches_nothing():
    n = 2 ** 20 + 3
    x = gaussian(n, "complex64", seed=9)
    ex = resident(x)
    before = ex.device_bytes()
    for bad in (0, n + 1, TOPK_MAX + 1):
        with pytest.raises(ValueError):
            ex.topk_result(bad)
    assert ex.device_bytes() == before                      # (not even the scratch was allocated)
    assert ex.download_result().tobytes() == x.tobytes()
    check_topk(ex.topk_result(3), x, 3)
    assert ex.device_bytes() > before
    assert ex.download_result().tobytes() == x.tobytes()


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_nan_is_an_error_return(dtype):
    n = 3 * B + 17
    x = gaussian(n, dtype, seed=13)
    x[B + 1] = np.nan
    tree = one_tensor_tree(n)
    with pytest.raises(ValueError):
        tree.contract_sample([x], 1, uniforms=np.array([0.5]))
    with pytest.raises(ValueError):
        tree.contract_topk([x], 5)
    with pytest.raises(ValueError):
        tree.contract_marginal([x], ["a"])
    x[B + 1] = 1.0
    check_topk(tree.contract_topk([x], 5), x, 5)            # (the executor is as good as before)


# ---- marginals -------------------------------------------------------------------------------------------------- #


def flags(rank, keep):
    return [1 if a in keep else 0 for a in range(rank)]


QUBIT_KEEPS = [(), (0,), (19,), (3, 17), (0, 1, 18, 19), tuple(range(8, 20)), tuple(range(20))]


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_marginals_of_twenty_qubits(dtype):
    shape = (2,) * 20
    x = gaussian(2 ** 20, dtype, seed=17)
    ex = resident(x)
    for keep in QUBIT_KEEPS:
        got = ex.marginal_result(shape, flags(20, keep)).reshape([2] * len(keep))
        ru.check_marginal(got, x, shape, keep)
    assert ex.marginal_result(shape, [1] * 20).tobytes() == su.probabilities(x).tobytes()
    # small integers: every partial sum is exact, whatever the order
    rng = np.random.default_rng(18)
    y = rng.integers(-7, 8, 2 ** 20).astype(dtype)
    if np.dtype(dtype).kind == "c":
        y = y + 1j * rng.integers(-7, 8, 2 ** 20).astype(dtype)
    ex = resident(y)
    for keep in QUBIT_KEEPS:
        got = ex.marginal_result(shape, flags(20, keep)).reshape([2] * len(keep))
        assert np.array_equal(got, ru.marginal_reference(y, shape, keep))


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_marginals_of_power_of_two_axes_of_mixed_width(dtype):
    """Axes of extent 4, 8, 1, 2 ...: the bits of an axis move together.  2^13 elements: one slab of two blocks; 2^21:
    several chunks of blocks per output; 2^24 with the 12 low bits kept (complex64 only): 16 slabs, whose results
    are stored or added according to the kept bits of the slab number."""
    shapes = [(4, 8, 1, 2, 16, 8), (2, 64, 4, 128, 2, 4, 2, 2)] + ([(4, 4, 16, 16, 4096)] if dtype == "complex64" else [])
    for shape in shapes:
        n = int(np.prod(shape))
        x = gaussian(n, dtype, seed=n % 1000)
        ex = resident(x)
        rank = len(shape)
        keeps = [()] + [(a,) for a in range(rank)] + [(0, rank - 1), (1, 3), tuple(range(rank))]
        if n == 2 ** 24:
            keeps = [(4,), (0, 4), (1, 4), (1, 3, 4), (2, 4)]
        for keep in keeps:
            got = ex.marginal_result(shape, flags(rank, keep)).reshape([shape[a] for a in keep])
            ru.check_marginal(got, x, shape, keep)


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
@pytest.mark.parametrize("shape", [(3, 5, 7, 11), (4, 3, 4, 3, 4), (2 ** 20 + 3,), (1, 6, 1, 5)])
def test_marginals_of_any_shape(shape, dtype):
    n = int(np.prod(shape))
    x = gaussian(n, dtype, seed=n % 1000 + 1)
    ex = resident(x)
    rank = len(shape)
    keeps = [()] + [(a,) for a in range(rank)] + list(itertools.combinations(range(rank), 2)) + [tuple(range(rank))]
    for keep in dict.fromkeys(keeps):
        got = ex.marginal_result(shape, flags(rank, keep)).reshape([shape[a] for a in keep])
        ru.check_marginal(got, x, shape, keep)
    assert ex.marginal_result(shape, [1] * rank).tobytes() == su.probabilities(x).tobytes()
    # rank 0: the whole tensor as one dropped axis
    tot = ex.marginal_result([], [])
    assert tot.shape == (1,) and abs(tot[0] - su.probabilities(x).sum()) <= ru.marginal_tol(su.probabilities(x).sum(), n)


def test_marginal_labels_in_the_callers_order():
    rng = np.random.default_rng(27)
    tree = ca.ContractionTree.from_path([("a", "b"), ("b", "c", "d")], ("a", "c", "d"), {"a": 6, "b": 3, "c": 5, "d": 4},
                                        path=[(0, 1)])
    xs = [rng.standard_normal((6, 3)), rng.standard_normal((3, 5, 4))]
    out = np.asarray(tree.contract(xs))
    shape = out.shape
    ad = tree.contract_marginal(xs, ["a", "d"])
    ru.check_marginal(ad.p, out, shape, (0, 2))
    da = tree.contract_marginal([], ["d", "a"], reuse=True)
    assert da.p.shape == (4, 6) and np.array_equal(da.p, ad.p.T)
    many = tree.contract_marginal([], [["c"], [], ["d", "c", "a"]], reuse=True)
    assert isinstance(many.p, list) and [m.shape for m in many.p] == [(5,), (), (4, 5, 6)]
    ru.check_marginal(many.p[0], out, shape, (1,))
    ru.check_marginal(many.p[1], out, shape, ())
    ru.check_marginal(many.p[2].transpose(2, 1, 0), out, shape, (0, 1, 2))
    assert many.norm == ad.norm and abs(many.p[1] - ad.norm) <= ru.marginal_tol(ad.norm, out.size)


def test_marginal_bad_arguments_raise():
    x = gaussian(B + 5, "complex64", seed=3)
    ex = resident(x)
    for ext, keep in (([B, 5], [1, 0]), ([B + 5], [2]), ([B + 5, 0], [1, 1]), ([B + 5], [-1])):
        with pytest.raises(ValueError):
            ex.marginal_result(ext, keep)
    # extents whose running product passes 2^40 elements before the last axis: refused by the library itself
    before = ex.device_bytes()
    ext, kp = np.array([2 ** 21, 2 ** 21, 2], np.int64), np.array([0, 0, 1], np.int32)
    out = np.full(2, 7.0)
    rc = runtime.load().ctg_exec_result_marginal(ex.handle, 3, ext.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 kp.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == -1 and runtime.load().ctg_last_error() and np.all(out == 7.0) and ex.device_bytes() == before
    assert ex.download_result().tobytes() == x.tobytes()


# ---- both calls --------------------------------------------------------------------------------------------------- #


def answers(tree, x):
    t = tree.contract_topk([x], 300)
    m = tree.contract_marginal([], [[], ["a"]], reuse=True)
    return t, m


def same_answers(a, b):
    (ta, ma), (tb, mb) = a, b
    assert np.array_equal(ta.indices, tb.indices) and ta.amplitudes.tobytes() == tb.amplitudes.tobytes()
    assert ta.p.tobytes() == tb.p.tobytes() and (ta.norm, ta.sum_p2) == (tb.norm, tb.sum_p2)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(ma.p, mb.p)) and ma.norm == mb.norm


def test_deterministic_across_runs_and_executors():
    n = 2 ** 15
    x, y = gaussian(n, "complex64", seed=41), gaussian(n, "complex64", seed=42)
    tree = one_tensor_tree(n)
    first = answers(tree, x)
    same_answers(first, answers(tree, x))
    other = answers(tree, y)
    assert not np.array_equal(other[0].indices, first[0].indices)
    same_answers(first, answers(tree, x))
    same_answers(first, answers(one_tensor_tree(n), x))
    # the power-of-two route and the general one (n = 2^15 as one axis / as 2^15 - 1 + 1 elements of another tree)
    z = gaussian(n - 1, "complex64", seed=43)
    t2 = one_tensor_tree(n - 1)
    same_answers(answers(t2, z), answers(one_tensor_tree(n - 1), z))


def test_reuse_reads_the_result_of_the_call_before():
    rng = np.random.default_rng(51)
    tree = ca.ContractionTree.from_path([("a", "b"), ("b", "c")], ("a", "c"), {"a": 96, "b": 7, "c": 80}, path=[(0, 1)])
    xs = [(rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype("complex64") for s in ((96, 7), (7, 80))]
    fresh_t, fresh_m = tree.contract_topk(xs, 65), tree.contract_marginal(xs, ["c"])
    out = np.asarray(tree.contract(xs))
    t = tree.contract_topk([], 65, reuse=True)
    m = tree.contract_marginal([], ["c"], reuse=True)
    check_topk(t, out, 65)
    assert np.array_equal(t.indices, fresh_t.indices) and t.p.tobytes() == fresh_t.p.tobytes()
    assert m.p.tobytes() == fresh_m.p.tobytes() and m.norm == fresh_m.norm
    tree.contract_sample(xs, 4, seed=1)
    assert np.array_equal(tree.contract_topk([], 65, reuse=True).indices, fresh_t.indices)
    tree.contract_audit(xs)
    with pytest.raises(RuntimeError):
        tree.contract_topk([], 65, reuse=True)
    with pytest.raises(RuntimeError):
        tree.contract_marginal([], ["c"], reuse=True)
    check_topk(tree.contract_topk(xs, 65), out, 65)


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_torch_inputs_read_the_torch_owned_result(dtype):
    import torch

    n = 3 * B + 17
    x = gaussian(n, dtype, seed=81)
    tree = one_tensor_tree(n)
    ref_t, ref_m = tree.contract_topk([x], 129), tree.contract_marginal([x], [[], ["a"]])
    tree2 = one_tensor_tree(n)
    xt = torch.tensor(x, device="cuda")
    t = tree2.contract_topk([xt], 129)
    check_topk(t, x, 129)
    m = tree2.contract_marginal([xt], [[], ["a"]])
    assert all(p.tobytes() == q.tobytes() for p, q in zip(m.p, ref_m.p))
    assert any("result" in st for st in _tree_contractor(tree2)._execs.values())   # (torch owns the result)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ts = tree2.contract_topk([xt], 129)
        ms = tree2.contract_marginal([xt], [[], ["a"]])
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(ts.indices, ref_t.indices) and ts.p.tobytes() == ref_t.p.tobytes()
    assert all(p.tobytes() == q.tobytes() for p, q in zip(ms.p, ref_m.p))


def test_expression_topk_marginal_and_cache_bytes():
    from cotengra_amd import interface

    rng = np.random.default_rng(71)
    a, b = rng.standard_normal((96, 7)), rng.standard_normal((7, 80))
    interface.clear_expression_cache()
    try:
        expr = ca.einsum_expression("ab,bc->ac", a.shape, b.shape, cache_expression=True)
        assert expr._cached
        out = np.asarray(expr(a, b))
        before = expr._bytes
        assert before == expr.device_bytes() > 0
        t = expr.topk(a, b, k=100)
        check_topk(t, out, 100)
        assert np.array_equal(np.ravel_multi_index(tuple(t.coords.T), out.shape), t.indices)
        grown = expr._bytes
        assert grown == expr.device_bytes() > before
        m = expr.marginal(a, b, keep=[["c"], ["c", "a"]])
        ru.check_marginal(m.p[0], out, out.shape, (1,))
        ru.check_marginal(m.p[1].T, out, out.shape, (0, 1))
        assert expr._bytes == expr.device_bytes() >= grown
        # an expression built with strip_exponent answers about its mantissa, the exponent next to it
        exs = ca.einsum_expression("ab,bc->ac", a.shape, b.shape, strip_exponent=True)
        mant, E = exs(a, b)
        ts = exs.topk(a, b, k=100)
        check_topk(ts, np.asarray(mant), 100)
        ms = exs.marginal(a, b, keep=["a"])
        ru.check_marginal(ms.p, np.asarray(mant), out.shape, (0,))
        assert ts.exponent == E and ms.exponent == E
        exs.close()
    finally:
        interface.clear_expression_cache()


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_golden_batch_m10_open8(dtype):
    tree = ca.tree_from_record(ca.load_network(os.path.join(HERE, "golden", "trees", "sycamore_m10_open8.json")))
    z = np.load(os.path.join(HERE, "golden", "sycamore_m10_open8_arrays.npz"))
    golden = np.load(os.path.join(HERE, "golden", "sycamore_m10_open8_expected.npz"))["amplitudes"]
    xs = [z[f"t{i}"].astype(dtype) for i in range(tree.N)]
    assert tree.nslices == 8 and golden.size == 256
    amps = np.asarray(tree.contract(xs))
    t = tree.contract_topk(xs, 16)
    check_topk(t, amps, 16)
    assert t.coords.shape == (16, 8) and np.array_equal(np.ravel_multi_index(tuple(t.coords.T), amps.shape), t.indices)
    out = list(tree.output)
    reqs = [[out[0]], [out[7]], [out[2], out[5]], []]
    m = tree.contract_marginal(xs, reqs)
    for got, keep in zip(m.p, [(0,), (7,), (2, 5), ()]):
        ru.check_marginal(got, amps, amps.shape, keep)
    if dtype == "complex128":
        ref = float(np.sum(su.probabilities(golden)))
        assert abs(float(m.p[3]) - ref) <= 1e-10 * ref


def test_top_chaotic_end_to_end():
    """The circuit of test_sample_chaotic_end_to_end: per bunch the three heaviest members of the sub-block of the
    dense state vector."""
    n, qs, seed = 12, [1, 3, 5, 6, 9], 61
    gates = random_circuit(n, 6, seed=7)
    psi = statevector(n, gates)
    out = circuits.top_chaotic(n, gates, qs, bunches=4, top=3, seed=seed, dtype="complex128")
    templates, _ = circuits.chaotic_prefixes(n, qs, 4, seed)
    assert out["prefixes"] == templates and len(out["bitstrings"]) == 12
    assert set(out) == {"bitstrings", "amplitudes", "p", "bunch", "prefixes", "norms", "sum_p2"}
    for b, template in enumerate(templates):
        sel = tuple(slice(None) if ch == "?" else int(ch) for ch in template)
        sub = psi[sel].reshape(-1)
        p = su.probabilities(sub)
        order = np.argsort(-p)
        srt = p[order]
        assert np.all(srt[:-1] - srt[1:] > 1e-12 * srt[:-1])          # (no ties in the sub-block)
        mine = slice(3 * b, 3 * b + 3)
        assert np.all(out["bunch"][mine] == b)
        want = []
        for i in order[:3]:
            bits = list(template)
            for q, c in zip(qs, np.unravel_index(i, (2,) * len(qs))):
                bits[q] = str(int(c))
            want.append("".join(bits))
        assert out["bitstrings"][mine] == want
        assert np.abs(out["amplitudes"][mine] - sub[order[:3]]).max() <= 1e-10
        assert abs(out["norms"][b] - p.sum()) <= 1e-10 * p.sum()
    drawn = circuits.sample_chaotic(n, gates, 256, qs, bunches=4, seed=seed, dtype="complex128")
    xeb_top = circuits.linear_xeb(len(qs), out["p"] / np.repeat(out["norms"], 3))
    xeb_drawn = circuits.linear_xeb(len(qs), drawn["p"] / np.repeat(drawn["norms"], 64))
    assert xeb_top > xeb_drawn
