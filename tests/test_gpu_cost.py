"""GPU suite: the distribution of a classical cost under the output distribution on the device (csrc/ctg_cost.hip,
DESIGN.md section 22) -- ``Executor.cost_result``, ``HipContractor.cost``, ``ContractionTree.contract_cost``,
``ContractExpression.cost``, ``circuits.cost_statistics``.

Data reaches the result tensor bit for bit through a one-tensor tree, as in tests/test_gpu_result_reduce.py.  What the
device reports as integers or as the bits of doubles -- the cost vector, ``s``, ``W``, per level ``A``, the threshold,
the masses below and at it, the histogram, the extremes with their indices and masses -- must EQUAL the models of
tests/cost_util.py; the fp64 sums (moments, tails, CVaR) meet the bounds derived there.  Every tensor is scaled so that
``sum p`` lies in [0.7, 0.8] (checked on the CPU in tests/test_cost_host.py): the ``s`` the call reports must equal the
model's, it is never read from the device.

Shapes: the tile pass transforms bits 0 .. 11 of a chunk of 4096 entries, a strided pass up to 8 further bits.  L = 0, 1,
5, 12: a tile, partial bits; 13: a strided pass of one bit; 16, 20: one strided pass; 21: two.  The select always runs six
digit passes; 3 * 5 * 7 * 11 elements exercise the general extents and the grid tails; 2^22 elements are 1024 chunks on
512 workgroups, so a workgroup takes more than one chunk."""
import ctypes as C
import functools

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import _tree_contractor

import cost_util as cu
import pauli_util as pu
import spectrum_util as spu
from test_gpu_result_reduce import resident
from test_gpu_sample import gaussian, one_tensor_tree, statevector

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "complex64", "complex128"]
LEVELS = (2.0 ** -10, 0.1, 0.5, 1.0)
# (L, dtype) of every Gaussian tensor of this suite
TENSORS = [(L, "complex64") for L in (0, 1, 5, 12, 13, 16, 20, 21, 22)] + [(13, dt) for dt in DTYPES if dt != "complex64"]
VALUES_SHAPE = (3, 5, 7, 11)


@functools.lru_cache(maxsize=None)
def tensor(L, dtype):
    x = cu.scaled(gaussian(2 ** L, dtype, seed=200 + L), dtype)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def values_tensor():
    x = cu.scaled(gaussian(int(np.prod(VALUES_SHAPE)), "complex128", seed=77), "complex128")
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def zero_optimum_tensor():
    """L = 13, amplitude zero at both minima of the ring cost (0 and n - 1) and at its first maximum."""
    L = 13
    x = np.array(gaussian(2 ** L, "complex64", seed=91))
    Cv = ring_cost(L)
    x[[0, 2 ** L - 1, int(np.argmax(Cv))]] = 0
    x = cu.scaled(x, "complex64")
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=4)
def on_device(L, dtype):
    return resident(tensor(L, dtype))


def masks_for(L, m, seed):
    """``m`` term masks over ``L`` bits: the identity, the bottom and the top bit first, then random ones with duplicates."""
    rng = np.random.default_rng(seed)
    first = [0, 1, 1 << max(L - 1, 0), (1 << L) - 1][:m]
    rest = rng.integers(0, 1 << L, size=max(m - len(first), 0)).tolist()
    out = [int(v) for v in first + rest]
    if m >= 7:
        out[5] = out[4]                                     # a mask twice, and the identity twice
        out[6] = 0
    return out


def ops_of(L, masks):
    return np.array([[(mk >> (L - 1 - a)) & 1 for a in range(L)] for mk in masks], dtype=np.uint8).reshape(len(masks), L) * 3


@functools.lru_cache(maxsize=None)
def ring_cost(L):
    terms, coeffs = cu.ring_terms(L)
    return cu.cost_model(cu.term_masks(L, terms), coeffs, L)


def ring_ops(L):
    terms, coeffs = cu.ring_terms(L)
    return cu.term_ops(L, terms), np.asarray(coeffs)


@functools.lru_cache(maxsize=None)
def gaussian_terms(L, m=300):
    masks = masks_for(L, m, seed=300 + L)
    coeffs = np.random.default_rng(400 + L).standard_normal(m)
    return masks, coeffs, cu.cost_model(masks, coeffs, L)


def words_of(words):
    """The words of a call as a dict, the double words as floats."""
    f = words.view(np.float64)
    nl = int(words[14])
    lv = [dict(A=int(words[24 + 5 * l]), t=float(f[25 + 5 * l]), below=int(words[26 + 5 * l]), at=int(words[27 + 5 * l]),
               tail=float(f[28 + 5 * l])) for l in range(nl)]
    return dict(s=int(words[0]), W=int(words[1]), m1=float(f[2]), m2=float(f[3]), min=float(f[4]), argmin=int(words[5]), max=float(f[6]),
                argmax=int(words[7]), smin=float(f[8]), sargmin=int(words[9]), mmin=int(words[10]), smax=float(f[11]),
                sargmax=int(words[12]), mmax=int(words[13]), nl=nl, tail=int(words[15]), S=float(f[16]), levels=lv)


def check_statistics(got, x, Cv, tail, levels, what):
    """Everything ``words_of`` holds against the models: integers and thresholds exactly, fp64 sums within their bounds."""
    Cv = np.asarray(Cv, dtype=np.float64).reshape(-1)
    p = cu.probabilities(x)
    S, s, w = cu.weights(x)
    W = int(w.sum(dtype=np.uint64))
    assert (got["s"], got["W"], got["nl"], got["tail"]) == (s, W, len(levels), tail), (what, got["s"], s, got["W"], W)
    assert abs(got["S"] - S) <= x.size * 2.0 ** -53 * S
    for k, key in ((1, "m1"), (2, "m2")):
        ref, tol = float(np.sum(p * Cv ** k)), cu.moment_tol(x, Cv, k)
        print(f"{what}: moment {k}: got {got[key]!r} ref {ref!r} err {abs(got[key] - ref):.2e} bound {tol:.2e}")
        assert abs(got[key] - ref) <= tol
    assert (got["min"], got["argmin"], got["max"], got["argmax"]) == (Cv.min(), int(np.argmin(Cv)), Cv.max(), int(np.argmax(Cv))), what
    sup = w > 0
    smin, smax = Cv[sup].min(), Cv[sup].max()
    assert (got["smin"], got["sargmin"], got["mmin"]) == (smin, int(np.flatnonzero(sup & (Cv == smin))[0]),
                                                       int(w[Cv == smin].sum(dtype=np.uint64))), what
    assert (got["smax"], got["sargmax"], got["mmax"]) == (smax, int(np.flatnonzero(sup & (Cv == smax))[0]),
                                                       int(w[Cv == smax].sum(dtype=np.uint64))), what
    unit = 2.0 ** -s
    for alpha, lv in zip(levels, got["levels"]):
        ref = cu.select_model(Cv, w, alpha, tail)
        assert (lv["A"], lv["below"], lv["at"]) == (ref["A"], ref["below"], ref["at"]), (what, alpha, lv, ref)
        assert np.float64(lv["t"]).view(np.uint64) == np.float64(ref["t"]).view(np.uint64), (what, alpha, lv["t"], ref["t"])
        cvar_ref, tail_ref = cu.cvar_reference(x, Cv, ref["t"], alpha, tail)
        tol = cu.moment_tol(x, Cv, 1)
        assert abs(lv["tail"] - tail_ref) <= tol, (what, alpha, lv["tail"], tail_ref, tol)
        cvar = (lv["tail"] + ((lv["A"] - lv["below"]) * unit) * lv["t"]) / (lv["A"] * unit)
        ctol = cu.cvar_tol(x, Cv, s, alpha)
        print(f"{what}: alpha {alpha:g} tail {tail:+d}: t {lv['t']!r} cvar {cvar!r} ref {cvar_ref!r} err {abs(cvar - cvar_ref):.2e} bound {ctol:.2e}")
        assert abs(cvar - cvar_ref) <= ctol


# ---- the cost vector ------------------------------------------------------------------------------------------ #


@pytest.mark.parametrize("L,m", [(0, 1), (1, 7), (5, 1), (5, 7), (12, 1), (12, 7), (12, 300), (13, 300), (16, 7), (20, 300), (21, 7)])
def test_the_cost_vector_bit_for_bit_against_the_model(L, m):
    import torch

    shape = (2,) * L
    masks = [mk & ((1 << L) - 1) for mk in masks_for(L, m, seed=10 * L + m)]
    coeffs = np.random.default_rng(L + m).standard_normal(len(masks))
    ex = on_device(L, "complex64")
    plan = ex.cost_plan(shape, "terms")
    assert (plan.bits, plan.tile_bits, sum(plan.pass_bits), plan.passes) == (L, min(L, 12), max(L - 12, 0), 0 if L <= 12 else (L - 12 + 7) // 8)
    buf = torch.full((2 ** L,), 7.0, dtype=torch.float64, device="cuda")
    words, hist = ex.cost_result(shape, ops=ops_of(L, masks), coeffs=coeffs, dev_cost_out=buf.data_ptr())
    torch.cuda.synchronize()
    model = cu.cost_model(masks, coeffs, L)
    spu.assert_same_bits(buf.cpu().numpy(), model, f"L={L} m={m}")
    assert hist is None and words[14] == 0
    got = words_of(words)
    assert (got["min"], got["argmin"], got["max"], got["argmax"]) == (model.min(), int(np.argmin(model)), model.max(), int(np.argmax(model)))
    assert ex.download_result().tobytes() == tensor(L, "complex64").tobytes()


def test_the_cost_vector_with_axes_of_extent_one():
    import torch

    shape = (2, 1, 2, 2, 1, 2, 2)
    ex = on_device(5, "complex64")
    ops = np.array([[0, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 3], [0, 0, 3, 3, 0, 0, 0], [3, 0, 3, 3, 0, 3, 3]], dtype=np.uint8)
    coeffs = np.array([0.25, -1.5, 0.75, 3.0])
    masks = runtime.cost_masks(shape, ops).tolist()
    assert masks == [0, 0b10001, 0b01100, 0b11111]
    buf = torch.zeros((32,), dtype=torch.float64, device="cuda")
    ex.cost_result(shape, ops=ops, coeffs=coeffs, dev_cost_out=buf.data_ptr())
    torch.cuda.synchronize()
    spu.assert_same_bits(buf.cpu().numpy(), cu.cost_model(masks, coeffs, 5), "extent-1 axes")
    with pytest.raises(ValueError):
        ex.cost_result(shape, ops=np.array([[0, 3, 0, 0, 0, 0, 0]], dtype=np.uint8), coeffs=[1.0])


# ---- the select, the moments, the tails ----------------------------------------------------------------------- #


@pytest.mark.parametrize("tail", [-1, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_select_on_integer_ring_costs_with_heavy_ties(dtype, tail):
    L = 13
    ops, coeffs = ring_ops(L)
    Cv = ring_cost(L)
    assert len(set(Cv.tolist())) == 7
    words, _ = on_device(L, dtype).cost_result((2,) * L, ops=ops, coeffs=coeffs, tail=tail, levels=LEVELS)
    check_statistics(words_of(words), tensor(L, dtype), Cv, tail, LEVELS, f"ring {dtype}")


@pytest.mark.parametrize("tail", [-1, 1])
def test_select_on_distinct_gaussian_costs_runs_down_to_one_element(tail):
    L = 13
    masks, coeffs, Cv = gaussian_terms(L)
    assert len(set(Cv.tolist())) == 2 ** L                 # all values distinct: the last digit holds one element
    words, _ = on_device(L, "complex64").cost_result((2,) * L, ops=ops_of(L, masks), coeffs=coeffs, tail=tail, levels=LEVELS)
    got = words_of(words)
    check_statistics(got, tensor(L, "complex64"), Cv, tail, LEVELS, "gaussian")
    _, _, w = cu.weights(tensor(L, "complex64"))
    for lv in got["levels"]:
        assert lv["at"] == int(w[Cv == lv["t"]][0])


@pytest.mark.parametrize("tail", [-1, 1])
def test_select_on_a_constant_cost(tail):
    L = 13
    ops = np.zeros((1, L), dtype=np.uint8)
    words, _ = on_device(L, "complex64").cost_result((2,) * L, ops=ops, coeffs=[2.5], tail=tail, levels=LEVELS)
    got = words_of(words)
    check_statistics(got, tensor(L, "complex64"), np.full(2 ** L, 2.5), tail, LEVELS, "constant")
    assert all(lv["t"] == 2.5 and lv["below"] == 0 and lv["at"] == got["W"] and lv["tail"] == 0.0 for lv in got["levels"])


@functools.lru_cache(maxsize=None)
def general_values():
    rng = np.random.default_rng(5)
    n = int(np.prod(VALUES_SHAPE))
    v = rng.integers(-3, 4, size=n).astype(np.float64)
    v[::7] = rng.standard_normal(len(v[::7]))
    v[3] = -0.0
    assert (v < 0).any() and (v == 0).any() and (v > 0).any()
    return v


@pytest.mark.parametrize("tail", [-1, 1])
def test_select_on_values_with_general_extents(tail):
    import torch

    x = values_tensor()
    ex = resident(x)
    v = general_values()
    dev = torch.as_tensor(v, device="cuda")
    out = torch.full((v.size,), 7.0, dtype=torch.float64, device="cuda")
    plan = ex.cost_plan(VALUES_SHAPE, "values", len(LEVELS))
    assert plan.kernels[0] == "cost_check_kernel" and plan.chunks == 1 and plan.bits == -1
    words, hist = ex.cost_result(VALUES_SHAPE, dev_cost=dev.data_ptr(), tail=tail, levels=LEVELS, edges=[-1.0, 0.0, 1.0],
                                 dev_cost_out=out.data_ptr())
    torch.cuda.synchronize()
    check_statistics(words_of(words), x, v, tail, LEVELS, "values")
    _, _, w = cu.weights(x)
    assert hist.tolist() == cu.hist_model(v + 0.0, w, [-1.0, 0.0, 1.0]).tolist()
    assert out.cpu().numpy().tobytes() == v.tobytes() and dev.cpu().numpy().tobytes() == v.tobytes()      # C copied, never written
    assert ex.download_result().tobytes() == x.tobytes()


def test_select_where_a_workgroup_takes_more_than_one_chunk():
    L = 22
    ex = on_device(L, "complex64")
    plan = ex.cost_plan((2,) * L, "terms", 4)
    assert (plan.chunks, plan.grid, plan.passes) == (1024, 512, 2)
    ops, coeffs = ring_ops(L)
    words, _ = ex.cost_result((2,) * L, ops=ops, coeffs=coeffs, tail=-1, levels=LEVELS)
    check_statistics(words_of(words), tensor(L, "complex64"), ring_cost(L), -1, LEVELS, "ring 2^22")


# ---- the histogram -------------------------------------------------------------------------------------------- #


@pytest.mark.parametrize("kind", ["two", "many"])
@pytest.mark.parametrize("cost", ["ring", "gaussian"])
def test_the_histogram_is_exact(cost, kind):
    L = 13
    x = tensor(L, "complex64")
    if cost == "ring":
        (ops, coeffs), Cv = ring_ops(L), ring_cost(L)
    else:
        masks, coeffs, Cv = gaussian_terms(L)
        ops = ops_of(L, masks)
    # 2 edges, both equal to a cost of the ring; 4097 edges of step 1 / 256, every integer among them
    edges = np.array([2.0, 6.0]) if kind == "two" else np.linspace(-1.0, 15.0, 4097)
    assert kind == "two" or (len(edges) == runtime.COST_MAX_EDGES and 2.0 in edges.tolist())
    words, hist = on_device(L, "complex64").cost_result((2,) * L, ops=ops, coeffs=coeffs, edges=edges)
    _, _, w = cu.weights(x)
    ref = cu.hist_model(Cv, w, edges)
    assert hist.shape == (len(edges) + 1,) and hist.tolist() == ref.tolist()
    assert int(hist.sum()) == int(words[1]) == int(w.sum(dtype=np.uint64))


# ---- against section 16 --------------------------------------------------------------------------------------- #


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_mean_is_the_sum_of_the_terms_expectations(dtype):
    L = 13
    x = tensor(L, dtype)
    ex = on_device(L, dtype)
    masks, coeffs, Cv = gaussian_terms(L, 40)
    ops = ops_of(L, masks)
    words, _ = ex.cost_result((2,) * L, ops=ops, coeffs=coeffs)
    each = ex.pauli_result((2,) * L, ops)
    ref = float(np.dot(coeffs, each))
    # ours within moment_tol of the exact sum over z; the terms' sum within sum |c_s| pauli_tol plus the dot's own roundings,
    # and the model's C within n 2^-53 sum |c| of the exact cost
    sum_c = float(np.sum(np.abs(coeffs)))
    tol = cu.moment_tol(x, Cv, 1) + sum_c * pu.pauli_tol(x, x.size) + (x.size + len(coeffs)) * 2.0 ** -53 * sum_c * 0.8
    got = words_of(words)["m1"]
    print(f"mean {dtype}: cost {got!r} terms {ref!r} err {abs(got - ref):.2e} bound {tol:.2e}")
    assert abs(got - ref) <= tol


# ---- the extremes --------------------------------------------------------------------------------------------- #


def test_the_optimum_where_its_amplitude_is_zero():
    L = 13
    n = 2 ** L
    x = zero_optimum_tensor()
    Cv = ring_cost(L)
    first_max = int(np.argmax(Cv))
    ops, coeffs = ring_ops(L)
    ex = resident(x)
    words, _ = ex.cost_result((2,) * L, ops=ops, coeffs=coeffs, levels=[1.0])
    got = words_of(words)
    check_statistics(got, x, Cv, -1, [1.0], "zero optimum")
    _, s, w = cu.weights(x)
    assert (got["min"], got["argmin"]) == (0.0, 0) and (got["max"], got["argmax"]) == (12.0, first_max)
    assert got["smin"] == 2.0 and got["sargmin"] == int(np.flatnonzero(Cv == 2.0)[0]) and got["mmin"] == int(w[Cv == 2.0].sum(dtype=np.uint64))
    assert got["smax"] == 12.0 and got["sargmax"] == int(np.flatnonzero(Cv == 12.0)[1]) and got["sargmax"] != got["argmax"]
    assert got["mmax"] == int(w[Cv == 12.0].sum(dtype=np.uint64))


# ---- no side effect, reuse ------------------------------------------------------------------------------------ #


def test_the_result_tensor_is_not_written_and_reuse_reads_it():
    x = values_tensor().reshape(-1)
    v = general_values()
    tree = one_tensor_tree(x.size)
    fn = _tree_contractor(tree)
    fresh = fn.cost(x, values=v, levels=LEVELS, edges=[-1.0, 0.0, 1.0], keep_values=True)
    assert isinstance(fresh, ca.CostResult) and fresh.exponent == 0.0
    held = fn._reusable[0]["exec"].download_result()
    assert held.tobytes() == x.tobytes()
    again = fn.cost(values=v, levels=LEVELS, edges=[-1.0, 0.0, 1.0], reuse=True)
    assert fn._reusable[0]["exec"].download_result().tobytes() == x.tobytes()
    assert again.raw["W"] == fresh.raw["W"] and again.raw["A"] == fresh.raw["A"] and again.raw["below"] == fresh.raw["below"]
    assert again.mean == fresh.mean and again.variance == fresh.variance and np.array_equal(again.cvar, fresh.cvar)
    assert np.array_equal(again.hist, fresh.hist) and again.values is None
    assert isinstance(fresh.values, np.ndarray) and fresh.values.tobytes() == v.tobytes()      # (a copy of the caller's, -0.0 included)
    # the normalised quantities against numpy
    p = cu.probabilities(x)
    S, s, w = cu.weights(x)
    assert fresh.raw["s"] == s and abs(fresh.norm - S) <= x.size * 2.0 ** -53 * S
    assert abs(fresh.mean - float(np.sum(p * v)) / S) <= 2 * cu.moment_tol(x, v, 1) / S
    ref_hist = cu.hist_model(v, w, [-1.0, 0.0, 1.0])[1:-1] * 2.0 ** -s / fresh.norm
    assert np.allclose(fresh.hist, ref_hist, rtol=1e-15, atol=0)
    assert fresh.minimum == v.min() and fresh.argmin == (int(np.argmin(v)),) and fresh.p_min > 0
    top = fn.topk(k=1, reuse=True)                         # another reader of the same result still finds it
    assert top.indices[0] == int(np.argmax(p))


# ---- refusals ------------------------------------------------------------------------------------------------- #


def raw_call(ex, rank, ext, m, ops, coeffs, dev_cost, tail, nl, levels, ne, edges, words, hist, dev_out, handle="own"):
    i64p, dp, u8p = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)   # noqa: E731
    return runtime.load().ctg_exec_result_cost(
        ex.handle if handle == "own" else handle, rank, ptr(ext, i64p), m, ptr(ops, u8p), ptr(coeffs, dp), C.c_void_p(dev_cost), tail, nl,
        ptr(levels, dp), ne, ptr(edges, dp), ptr(words, i64p), ptr(hist, i64p), C.c_void_p(dev_out))


def test_refusals_through_the_c_abi():
    import torch

    L = 13
    n = 2 ** L
    x = tensor(L, "complex64")
    ex = resident(x)
    before = ex.device_bytes()
    ext = np.full(L, 2, np.int64)
    ops, coeffs = ring_ops(L)
    ops = np.ascontiguousarray(ops)
    m = len(coeffs)
    levels = np.array([0.25, 1.0])
    edges = np.array([0.0, 4.0, 8.0])
    words = np.full(runtime.COST_WORDS, 7, np.int64)
    hist = np.full(len(edges) + 1, 7, np.int64)
    buf = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    vals = torch.zeros((n,), dtype=torch.float64, device="cuda")
    dev, res = buf.data_ptr(), ex.result_ptr()

    def with_(a, i, v):
        b = a.copy()
        b.reshape(-1)[i] = v
        return b

    wide = np.array([2] * 12 + [1, 2], np.int64)
    zwide = np.zeros((1, 14), np.uint8)
    zwide[0, 12] = 3
    bad = [
        dict(handle=None), dict(ext=None), dict(words=None),                            # null arguments
        dict(rank=-1), dict(rank=L - 1), dict(ext=with_(ext, 3, 0)), dict(ext=with_(ext, 3, 1)),
        dict(rank=2, ext=np.array([4, 2048], np.int64), ops=np.zeros((m, 2), np.uint8)),   # an extent above 2 with terms
        dict(ops=with_(ops, 5, 1)), dict(ops=with_(ops, 5, 2)), dict(ops=with_(ops, 5, 4)),   # a code other than 0 and 3
        dict(rank=14, ext=wide, ops=zwide, coeffs=np.ones(1), m=1),                     # Z on an axis of extent 1
        dict(m=-1), dict(m=(1 << 20) + 1), dict(nl=-1), dict(nl=9, levels=np.full(9, 0.5)), dict(ne=1), dict(ne=4098, edges=np.arange(4098.0)),
        dict(levels=np.array([0.0, 1.0])), dict(levels=np.array([0.5, 1.5])), dict(levels=np.array([np.nan, 1.0])), dict(levels=None),
        dict(edges=np.array([0.0, 0.0, 8.0])), dict(edges=np.array([0.0, 9.0, 8.0])), dict(edges=np.array([0.0, np.inf, 8.0])),
        dict(edges=np.array([np.nan, 4.0, 8.0])), dict(edges=None), dict(hist=None),
        dict(coeffs=with_(coeffs, 2, np.inf)), dict(coeffs=with_(coeffs, 2, np.nan)), dict(coeffs=np.full(m, 1.7e308)),
        dict(dev_cost=vals.data_ptr()),                                                 # both sources
        dict(ops=None, coeffs=None), dict(ops=None), dict(coeffs=None),                 # neither source; half a source
        dict(tail=0), dict(tail=2),
        dict(dev_out=res), dict(dev_out=res + 8 * n - 8), dict(dev_out=res - 8 * n + 8), dict(dev_out=dev + 4),
        dict(ops=None, coeffs=None, dev_cost=vals.data_ptr() + 4),                      # a misaligned dev_cost
        dict(ops=None, coeffs=None, dev_cost=dev),                                      # dev_cost_out overlaps dev_cost
    ]
    for row in bad:
        a = dict(rank=L, ext=ext, m=m, ops=ops, coeffs=coeffs, dev_cost=None, tail=-1, nl=2, levels=levels, ne=3, edges=edges, words=words,
                 hist=hist, dev_out=dev, handle="own")
        a.update(row)
        rc = raw_call(ex, a["rank"], a["ext"], a["m"], a["ops"], a["coeffs"], a["dev_cost"], a["tail"], a["nl"], a["levels"], a["ne"],
                      a["edges"], a["words"], a["hist"], a["dev_out"], a["handle"])
        assert rc == -1, row
        assert runtime.load().ctg_last_error()
        assert np.all(words == 7) and np.all(hist == 7)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    assert ex.device_bytes() == before                    # (nothing was launched, not even the scratch reserved)
    assert ex.download_result().tobytes() == x.tobytes()
    # a value that is not finite: refused by the first pass, every output untouched
    for poison in (np.nan, np.inf, -np.inf):
        vals.zero_()
        vals[4097] = poison
        torch.cuda.synchronize()
        assert raw_call(ex, L, ext, 0, None, None, vals.data_ptr(), -1, 2, levels, 3, edges, words, hist, dev) == -1
        torch.cuda.synchronize()
        assert np.all(words == 7) and np.all(hist == 7) and bool((buf == 7.0).all())
    # ... and the binding raises ValueError
    for kw in (dict(ops=with_(ops, 5, 1), coeffs=coeffs), dict(ops=ops, coeffs=coeffs[:-1]), dict(ops=ops, coeffs=coeffs, levels=[0.0]),
               dict(ops=ops, coeffs=coeffs, edges=[1.0]), dict(ops=ops, coeffs=coeffs, tail=0), dict(), dict(ops=ops),
               dict(dev_cost=vals.data_ptr()), dict(ops=ops, coeffs=coeffs, dev_cost=vals.data_ptr())):
        with pytest.raises(ValueError):
            ex.cost_result(ext, **kw)
    # a following valid call is correct, to every output
    assert raw_call(ex, L, ext, m, ops, coeffs, None, -1, 2, levels, 3, edges, words, hist, dev) == 0
    torch.cuda.synchronize()
    Cv = ring_cost(L)
    spu.assert_same_bits(buf.cpu().numpy(), Cv, "dev_cost_out")
    check_statistics(words_of(words), x, Cv, -1, levels.tolist(), "after the refusals")
    assert hist.tolist() == cu.hist_model(Cv, cu.weights(x)[2], edges).tolist()
    # a NaN member: CTG_E_NORM, through every layer
    badx = np.array(x)
    badx[4097] = np.nan
    exn = resident(badx)
    words[:] = 7
    assert raw_call(exn, L, ext, m, ops, coeffs, None, -1, 2, levels, 0, None, words, None, None) == -6 and np.all(words == 7)
    with pytest.raises(ValueError):
        exn.cost_result(ext, ops=ops, coeffs=coeffs)
    # an all-zero tensor: zero masses, NaN-free statistics
    wz, hz = resident(np.zeros(n, "complex64")).cost_result(ext, ops=ops, coeffs=coeffs, levels=levels, edges=edges)
    z = words_of(wz)
    assert (z["s"], z["W"], z["m1"], z["m2"], z["S"]) == (0, 0, 0.0, 0.0, 0.0) and not hz.any()
    assert (z["min"], z["argmin"], z["max"]) == (0.0, 0, 12.0) and (z["smin"], z["sargmin"], z["mmin"]) == (0.0, -1, 0)
    assert all(lv == dict(A=0, t=0.0, below=0, at=0, tail=0.0) for lv in z["levels"])
    tree = one_tensor_tree(n)
    r = tree.contract_cost([np.zeros(n, "complex64")], values=np.arange(float(n)), levels=[0.5], edges=[0.0, 1.0])
    assert (r.mean, r.variance, r.p_min, r.p_max, r.norm) == (0.0, 0.0, 0.0, 0.0, 0.0) and r.cvar.tolist() == [0.0] and r.hist.tolist() == [0.0]
    assert (r.minimum, r.maximum, r.argmin, r.argmax) == (0.0, float(n - 1), (0,), (n - 1,))


# ---- the layers ----------------------------------------------------------------------------------------------- #


def qaoa_circuit(n, edges, layers, seed):
    """QAOA-shaped, from the gates of ``circuits``: a layer of half rotations, then per layer an fSim gate on every edge of
    the ring (the cost layer's place) and an rz and a half rotation on every qubit (the mixer's)."""
    rng = np.random.default_rng(seed)
    gates = [("hz_1_2", (q,), ()) for q in range(n)]
    for _ in range(layers):
        for i, j in edges:
            if abs(i - j) == 1:
                gates.append(("fs", (min(i, j), max(i, j)), (float(rng.normal()), float(rng.normal()))))
        for q in range(n):
            gates.append(("rz", (q,), (float(rng.normal()),)))
            gates.append(("x_1_2", (q,), ()))
    return gates


def circuit_tree(n, gates, dtype):
    from cotengra_amd.interface import array_contract_tree

    inputs, output, size_dict, arrays = circuits.circuit_to_network(n, gates, "?" * n, simplify=True, dtype=dtype)
    return array_contract_tree(inputs, output, size_dict, optimize="greedy"), arrays


def check_result(r, x, Cv, levels, tail, edges, what):
    """A ``CostResult`` against the tensor ``x`` its contraction holds (``tree.contract``) plus numpy.  The circuit's norm
    is about 1, on the edge of a binade, so here -- and only here -- the weights are formed with the ``s`` the call reports."""
    x = np.asarray(x).reshape(-1)
    Cv = np.asarray(Cv, dtype=np.float64).reshape(-1)
    p = cu.probabilities(x)
    S = float(np.sum(p))
    s = r.raw["s"]
    assert s in (61, 62) and abs(r.norm - S) <= x.size * 2.0 ** -53 * S
    w = np.rint(np.ldexp(p, s)).astype(np.uint64)
    assert r.raw["W"] == int(w.sum(dtype=np.uint64))
    assert abs(r.mean - float(np.sum(p * Cv)) / S) <= 2 * cu.moment_tol(x, Cv, 1) / S, what
    var = float(np.sum(p * Cv * Cv)) / S - (float(np.sum(p * Cv)) / S) ** 2
    assert abs(r.variance - var) <= 2 * cu.moment_tol(x, Cv, 2) / S + 4 * float(np.max(np.abs(Cv))) * cu.moment_tol(x, Cv, 1) / S, what
    assert r.minimum == Cv.min() and r.maximum == Cv.max()
    assert r.raw["argmin_flat"] == int(np.argmin(Cv)) and r.raw["argmax_flat"] == int(np.argmax(Cv))
    for l, alpha in enumerate(levels):
        ref = cu.select_model(Cv, w, alpha, tail)
        assert (r.raw["A"][l], r.raw["below"][l], r.raw["at"][l], r.thresholds[l]) == (ref["A"], ref["below"], ref["at"], ref["t"]), (what, alpha)
        cref, _ = cu.cvar_reference(x, Cv, ref["t"], alpha, tail)
        assert abs(r.cvar[l] - cref) <= cu.cvar_tol(x, Cv, s, alpha), (what, alpha, r.cvar[l], cref)
    if edges is not None:
        assert r.raw["hist"].tolist() == cu.hist_model(Cv, w, edges).tolist()
        assert np.allclose(r.hist, r.raw["hist"][1:-1] * 2.0 ** -s / r.norm, rtol=1e-15, atol=0)
    sup = w > 0
    assert r.support_min == Cv[sup].min() and r.p_min == int(w[Cv == r.support_min].sum(dtype=np.uint64)) * 2.0 ** -s / r.norm


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_through_the_layers_on_a_qaoa_shaped_circuit(dtype):
    n = 10
    edges = [(q, (q + 1) % n) for q in range(n)]
    gates = qaoa_circuit(n, edges, 2, seed=4)
    terms_q, coeffs = circuits.maxcut_terms(edges)
    Cv = cu.cost_model(cu.term_masks(n, [tuple(t) for t in terms_q]), coeffs, n)
    levels, grid = (0.05, 0.25, 1.0), np.arange(0.0, 12.0, 2.0)
    tree, arrays = circuit_tree(n, gates, dtype)
    out = list(tree.output)
    terms = [{out[q]: "Z" for q in t} for t in terms_q]
    x = np.asarray(tree.contract(arrays))                 # (what the result tensor holds)
    assert x.shape == (2,) * n
    r = tree.contract_cost([], terms=terms, coeffs=coeffs, levels=levels, edges=grid, keep_values=True, reuse=True)   # after __call__
    assert isinstance(r, ca.CostResult) and r.exponent == 0.0 and r.values.shape == (2,) * n
    spu.assert_same_bits(np.asarray(r.values), Cv.reshape((2,) * n), "values")
    check_result(r, x, Cv, levels, -1, grid, f"tree {dtype}")
    assert r.argmin == (0,) * n and r.minimum == 0.0 and r.maximum == 10.0
    up = tree.contract_cost(arrays, terms=terms, coeffs=coeffs, levels=levels, tail="upper")
    check_result(up, x, Cv, levels, 1, None, f"upper {dtype}")
    assert up.hist is None and up.values is None and up.cvar[0] >= up.cvar[1] >= up.cvar[2] and abs(up.cvar[2] - up.mean) <= 1e-9
    # the same cost as a vector of values
    vals = tree.contract_cost([], values=Cv.reshape((2,) * n), levels=levels, edges=grid, reuse=True)
    assert vals.raw["A"] == r.raw["A"] and vals.raw["below"] == r.raw["below"] and vals.raw["hist"].tolist() == r.raw["hist"].tolist()
    assert vals.mean == r.mean and np.array_equal(vals.cvar, r.cvar)
    # sliced, an output index among the sliced ones
    tree2, arrays2 = circuit_tree(n, gates, dtype)
    big = max((p for p, _, _ in tree2.traverse()), key=tree2.get_size)
    inner = [ix for ix in tree2.get_legs(big) if ix not in tree2.output][:1]
    for ix in [tree2.output[4]] + inner:
        tree2.remove_ind_(ix)
    assert tree2.nslices > 1 and tree2.gathered_shape() == (2,) * n and list(tree2.output) == out
    x2 = np.asarray(tree2.contract(arrays2))
    r2 = tree2.contract_cost([], terms=terms, coeffs=coeffs, levels=levels, edges=grid, reuse=True)
    check_result(r2, x2, Cv, levels, -1, grid, f"sliced {dtype}")
    rel = 1e-10 if dtype == "complex128" else 1e-5
    assert abs(r2.mean - r.mean) <= 8 * rel * 10
    # the expression
    expr = ca.array_contract_expression(tree.inputs, tree.output, shapes=[a.shape for a in arrays], optimize="greedy")
    assert list(expr.tree.output) == out
    xe = np.asarray(expr(*arrays))
    check_result(expr.cost(*arrays, terms=terms, coeffs=coeffs, levels=levels), xe, Cv, levels, -1, None, f"expression {dtype}")
    assert expr.device_bytes() >= runtime.cost_plan(dtype, (2,) * n, "terms", len(levels)).scratch_bytes - 8 * 2 ** n   # (the scratch is counted)
    # the circuit entry against the state vector
    psi = statevector(n, gates).reshape(-1)
    pp = np.abs(psi) ** 2
    cs = circuits.cost_statistics(n, gates, terms_q, coeffs, levels=levels, edges=grid, dtype=dtype)
    assert abs(cs.norm - 1) <= 4 * rel and abs(cs.mean - float(np.sum(pp * Cv))) <= 8 * rel * 10
    assert cs.minimum == 0.0 and cs.argmin == (0,) * n and abs(cs.p_min - (pp[0] + pp[-1])) <= 8 * rel
    assert np.all(np.abs(cs.hist - np.array([pp[(Cv >= a) & (Cv < a + 2)].sum() for a in grid[:-1]])) <= 8 * rel)
    # two qubits projected: the cost over the others
    fixed = {1: 1, 7: 0}
    sub_terms, sub_co = circuits.maxcut_terms([(0, 2), (2, 3), (3, 4), (8, 9)], [1.0, 2.0, 0.5, 1.5])
    cf = circuits.cost_statistics(n, gates, sub_terms, sub_co, fixed=fixed, levels=[0.5], dtype=dtype)
    sub = np.take(np.take(statevector(n, gates), 1, axis=1), 0, axis=6)
    ps = (np.abs(sub) ** 2).reshape(-1)
    ax = {0: 0, 2: 1, 3: 2, 4: 3, 8: 6, 9: 7}
    Cs = cu.cost_model(cu.term_masks(8, [tuple(ax[q] for q in t) for t in sub_terms]), sub_co, 8)
    assert abs(cf.norm - ps.sum()) <= 4 * rel and abs(cf.mean - float(np.sum(ps * Cs)) / ps.sum()) <= 8 * rel * 5 / ps.sum()
    assert cf.maximum == 5.0 and len(cf.argmax) == 8
