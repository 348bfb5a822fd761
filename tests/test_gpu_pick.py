"""Chosen members of the output on the device: ``pair_pick_kernel`` in every width and both
gather forms against ``np.einsum`` of the whole output, pick plans of whole trees, bit-for-bit determinism, the
k-reduction route, ``strip_exponent``, and the public entry points.

Tolerance: the one the full tensor is held to, per picked element -- ``ref`` the whole output in double precision
by ``np.einsum``; single precision ``golden_util.single_gate(ref, numpy's single-precision run) * max|ref|``, double
precision ``1e-12 * max|ref|``."""
import os

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits
from cotengra_amd.contractor import _tree_contractor
from cotengra_amd.plan import KERNEL_PICK, pick_route

import golden_util as G
from test_gpu_sample import random_circuit, statevector

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = ["float32", "float64", "complex64", "complex128"]
WIDE = {"float32": "float64", "float64": "float64", "complex64": "complex128", "complex128": "complex128"}
KS = [1, 2, 3, 4, 8, 16, 27, 32, 63, 64, 65, 128, 243, 1024, 4096]   # (8, 16, 32: every segment width in both forms)
MS = [1, 2, 63, 64, 65, 257, 5000]
SIDE = 64


def k_indices(K):
    """The contracted indices of a root with contraction ``K``: extent-3 indices for the powers of three (the
    fast level of the k tables is then no power of two), one index otherwise."""
    if K in (27, 243):
        n = {27: 3, 243: 5}[K]
        return [f"k{i}" for i in range(n)], {f"k{i}": 3 for i in range(n)}
    return ["k0"], {"k0": K}


def shape_tree(K, layout, R=SIDE, N=SIDE):
    """``A[a, k..] B[k.., c] -> (a, c)``: two inputs (``leaf``), or -- ``arena`` -- each side the product of two
    inputs, so that the root's children are intermediates."""
    ks, sizes = k_indices(K)
    sizes.update(a=R, c=N, x=2, y=2)
    if layout == "leaf":
        return ca.ContractionTree.from_path([("a", *ks), (*ks, "c")], ("a", "c"), sizes, path=[(0, 1)])
    return ca.ContractionTree.from_path([("a", "x"), ("x", *ks), (*ks, "y"), ("y", "c")], ("a", "c"), sizes,
                                        ssa_path=[(0, 1), (2, 3), (4, 5)])


def data(rng, shape, dtype):
    x = rng.standard_normal(shape)
    if dtype.startswith("complex"):
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dtype)


def einsum_of(tree, arrays, dtype):
    ids = {}
    sym = lambda t: [ids.setdefault(ix, len(ids)) for ix in t]  # noqa: E731
    args = []
    for x, term in zip(arrays, tree.inputs):
        args += [np.asarray(x).astype(dtype), sym(term)]
    return np.einsum(*args, sym(tree.output), optimize=True)


def bound_of(tree, arrays, dtype):
    """``(ref, absolute bound)`` for results of ``dtype``."""
    ref = einsum_of(tree, arrays, WIDE[dtype])
    scale = float(np.abs(ref).max())
    if dtype in ("float64", "complex128"):
        return ref, 1e-12 * scale
    return ref, G.single_gate(ref, einsum_of(tree, arrays, dtype)) * scale


def requests(shape, M, seed, dup=True):
    rng = np.random.default_rng(seed)
    coords = np.stack([rng.integers(0, d, M) for d in shape], axis=1).astype(np.int64)
    if dup and M > 2:
        coords[M // 2:M // 2 + M // 4 + 1] = coords[:M // 4 + 1]   # duplicates, apart from each other
    return coords


def pick_state(tree):
    """``(contractor, executor state, index of the sparse step)`` of the pick contractor cached on ``tree``."""
    fns = [f for k, f in tree.contraction_cores.items() if isinstance(k, tuple) and k[0] == "hip-pick"]
    assert len(fns) == 1, list(tree.contraction_cores)
    (st,) = fns[0]._execs.values()
    (i,) = [i for i, s in enumerate(st["plan"].steps) if s.kernel == KERNEL_PICK]
    return fns[0], st, i


def pick_name(tree):
    _, st, i = pick_state(tree)
    return st["exec"].step_kernels()[i]


def parse(name):
    assert name.startswith("pair_pick_kernel<") and name.endswith(">"), name
    t, vec, seg = name[len("pair_pick_kernel<"):-1].split(",")
    return t, int(vec), int(seg)


def seg_of(K, vec):
    slots, seg = -(-K // vec), 1
    while seg < 64 and seg < slots:
        seg *= 2
    return seg


T_NAME = {"float32": "float", "float64": "double", "complex64": "c64", "complex128": "c128"}

_CASES = {}


def shape_case(K, layout, dtype):
    """Tree, arrays, reference and bound of a shape (built once)."""
    key = (K, layout, dtype)
    if key not in _CASES:
        tree = shape_tree(K, layout)
        rng = np.random.default_rng(100 + K)
        arrays = [data(rng, s, dtype) for s in tree.get_shapes()]
        _CASES[key] = (tree, arrays) + bound_of(tree, arrays, dtype)
    return _CASES[key]


# ---- the kernel in every width, both gather forms, all four dtypes ------------------------------------------------- #

@pytest.mark.parametrize("layout", ["leaf", "arena"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes(dtype, K, layout):
    tree, arrays, ref, bound = shape_case(K, layout, dtype)
    vec = 2 if (layout == "arena" and K % 2 == 0) else 1
    for M in MS:
        coords = requests(ref.shape, M, seed=M)
        got = tree.contract_pick(arrays, coords=coords)
        assert got.shape == (M,) and got.dtype == np.dtype(dtype)
        assert parse(pick_name(tree)) == (T_NAME[dtype], vec, seg_of(K, vec)), (pick_name(tree), K, layout)
        err = float(np.abs(got - ref[tuple(coords.T)]).max())
        print(f"{dtype} K={K} {layout} M={M}: {pick_name(tree)} err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (dtype, K, layout, M, err, bound)


def test_every_segment_width_is_met():
    met = set()
    for K in KS:
        for layout in ("leaf", "arena"):
            tree, arrays, ref, bound = shape_case(K, layout, "complex64")
            coords = requests(ref.shape, 65, seed=1)
            got = tree.contract_pick(arrays, coords=coords)
            assert np.abs(got - ref[tuple(coords.T)]).max() <= bound
            t, vec, seg = parse(pick_name(tree))
            assert vec == (2 if layout == "arena" and K % 2 == 0 else 1), (K, layout, vec)
            met.add((vec, seg))
    assert {s for _, s in met} == {1, 2, 4, 8, 16, 32, 64}, met
    assert {s for v, s in met if v == 2} == {1, 2, 4, 8, 16, 32, 64}, met
    assert {s for v, s in met if v == 1} == {1, 2, 4, 8, 16, 32, 64}, met


@pytest.mark.parametrize("layout", ["leaf", "arena"])
@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
@pytest.mark.parametrize("K", [4, 64, 65, 128, 243, 512, 1024])
def test_tables_that_share_a_row(K, dtype, layout):
    """All requests in one A row (the row stays in registers where it fits), and all in one B row.  In the long
    table a segment walks four requests; the kept row is one round at K = 64, two to four rounds -- the last one
    with slots past the end of the row at 65 and 243 -- at K = 65, 128, 243 and 512, and too long to keep at 1024."""
    tree, arrays, ref, bound = shape_case(K, layout, dtype)
    for fixed in (0, 1):
        coords = requests(ref.shape, 300, seed=fixed)
        coords[:, fixed] = 17
        got = tree.contract_pick(arrays, coords=coords)
        assert np.abs(got - ref[tuple(coords.T)]).max() <= bound
        # the same requests among others that do not share the row: the same bits
        mixed = np.concatenate([requests(ref.shape, 200, seed=9), coords])
        assert tree.contract_pick(arrays, coords=mixed)[200:].tobytes() == got.tobytes()
        # and in a table long enough that a segment walks several requests and keeps an A row in registers
        # (csrc/ctg_pick.hip: pick_shape): the same bits again
        long = np.concatenate([coords, requests(ref.shape, 70000, seed=10)[:, :]])
        long[300:, 0] //= 16   # (few A rows: consecutive requests of the sorted table share them)
        out = tree.contract_pick(arrays, coords=long)
        assert out[:300].tobytes() == got.tobytes()
        assert np.abs(out - ref[tuple(long.T)]).max() <= bound


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_few_requests_under_a_long_contraction_take_the_k_reduction(dtype):
    K = 1 << 17
    tree = ca.ContractionTree.from_path([("a", "k"), ("k", "c")], ("a", "c"), dict(a=4, k=K, c=4), path=[(0, 1)])
    rng = np.random.default_rng(3)
    arrays = [data(rng, s, dtype) for s in tree.get_shapes()]
    ref, bound = bound_of(tree, arrays, dtype)
    coords = np.array([[3, 1], [0, 0], [3, 1], [2, 3], [1, 2]])
    assert pick_route(len(coords), K) == "kred"
    got = tree.contract_pick(arrays, coords=coords)
    name = pick_name(tree)
    assert name.startswith("pair_kred_kernel + pair_kred_finish_kernel<"), name
    assert np.abs(got - ref[tuple(coords.T)]).max() <= bound
    # the other side of the rule: the same tree with many requests runs the pick kernel
    many = requests(ref.shape, 513, seed=2)
    assert pick_route(len(many), K) == "pick"
    got = tree.contract_pick(arrays, coords=many)
    assert parse(pick_name(tree)) == (T_NAME[dtype], 1, 64)
    assert np.abs(got - ref[tuple(many.T)]).max() <= bound


# ---- through a tree ------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize("dtype", ["complex64", "float64"])
@pytest.mark.parametrize("R,N", [(32, 32), (32, 96), (96, 32), (96, 96)])
def test_chain_trees(R, N, dtype):
    """a[R, x] b[x, K] . c[K, y] d[y, N]: both children of the root are intermediates."""
    tree = ca.ContractionTree.from_path([("a", "x"), ("x", "k"), ("k", "y"), ("y", "c")], ("c", "a"),
                                        dict(a=R, x=24, k=96, y=40, c=N), ssa_path=[(0, 1), (2, 3), (4, 5)])
    rng = np.random.default_rng(R + N)
    arrays = [data(rng, s, dtype) for s in tree.get_shapes()]
    ref, bound = bound_of(tree, arrays, dtype)
    coords = requests(ref.shape, 777, seed=4)
    got = tree.contract_pick(arrays, coords=coords)
    assert parse(pick_name(tree)) == (T_NAME[dtype], 2, 64)
    assert np.abs(got - ref[tuple(coords.T)]).max() <= bound
    idx = np.ravel_multi_index(tuple(coords.T), ref.shape)
    assert tree.contract_pick(arrays, indices=idx).tobytes() == got.tobytes()


def m10():
    tree = ca.tree_from_record(ca.load_network(os.path.join(HERE, "golden", "trees", "sycamore_m10_open8.json")))
    z = np.load(os.path.join(HERE, "golden", "sycamore_m10_open8_arrays.npz"))
    golden = np.load(os.path.join(HERE, "golden", "sycamore_m10_open8_expected.npz"))["amplitudes"]
    assert tree.nslices == 8 and golden.size == 256
    return tree, z, golden


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_sycamore_m10_open8(dtype):
    from oracle import contract_ref as orc

    tree, z, golden = m10()
    xs = [z[f"t{i}"].astype(dtype) for i in range(tree.N)]
    ref = golden.reshape(tree.gathered_shape())
    scale = float(np.abs(ref).max())
    tol = 1e-12 if dtype == "complex128" else G.single_gate(ref, np.asarray(orc.contract(tree, xs)).reshape(ref.shape))
    idx = np.random.default_rng(5).permutation(256)
    full = np.asarray(tree.contract(xs))
    got = tree.contract_pick(xs, indices=idx)
    assert np.abs(got - ref.reshape(-1)[idx]).max() <= tol * scale
    assert np.abs(full - ref).max() <= tol * scale
    assert np.abs(got - full.reshape(-1)[idx]).max() <= tol * scale
    # the ordinary contractor is still there and still returns the whole tensor
    assert np.asarray(tree.contract(xs)).tobytes() == full.tobytes()


def test_hyper_index_golden_tree():
    case = next(c for c in G.cases("tree") if c["name"] == "rand_s666_r3_o2_hi2_ho2")
    for dtype in ("complex64", "complex128"):
        tree = G.tree_of(case)
        assert len(tree.output) >= 2 and not tree.sliced_inds
        arrays = G.arrays_of(case, dtype, tree)
        ref, bound = bound_of(tree, arrays, dtype)
        coords = requests(ref.shape, 100, seed=6)
        got = tree.contract_pick(arrays, coords=coords)
        assert np.abs(got - ref[tuple(coords.T)]).max() <= bound


def test_single_input_tree():
    tree = ca.ContractionTree([("a", "b", "b", "k")], ("b", "a"), dict(a=30, b=40, k=50))
    rng = np.random.default_rng(8)
    arrays = [data(rng, s, "complex64") for s in tree.get_shapes()]
    ref, bound = bound_of(tree, arrays, "complex64")
    coords = requests(ref.shape, 500, seed=7)
    got = tree.contract_pick(arrays, coords=coords)
    assert np.abs(got - ref[tuple(coords.T)]).max() <= bound


# ---- determinism, bit for bit -------------------------------------------------------------------------------------- #

@pytest.mark.parametrize("K,layout", [(3, "leaf"), (64, "arena"), (243, "leaf"), (1024, "arena"), (4096, "leaf")])
def test_bits_do_not_depend_on_the_table(K, layout):
    tree, arrays, ref, _ = shape_case(K, layout, "complex64")
    coords = requests(ref.shape, 5000, seed=11)
    a = tree.contract_pick(arrays, coords=coords)
    assert tree.contract_pick(arrays, coords=coords).tobytes() == a.tobytes()
    perm = np.random.default_rng(12).permutation(len(coords))
    b = tree.contract_pick(arrays, coords=coords[perm])
    assert b[np.argsort(perm)].tobytes() == a.tobytes()
    sub = np.sort(np.random.default_rng(13).choice(len(coords), 333, replace=False))
    assert tree.contract_pick(arrays, coords=coords[sub]).tobytes() == a[sub].tobytes()
    # after an unrelated ordinary call on the same tree
    tree.contract(arrays)
    assert tree.contract_pick(arrays, coords=coords).tobytes() == a.tobytes()


def test_bits_do_not_depend_on_the_slice_batch(monkeypatch):
    outs = []
    for cap in ("1", "4"):
        monkeypatch.setenv("CTG_SLICE_BATCH", cap)
        tree, z, _ = m10()
        xs = [z[f"t{i}"].astype("complex64") for i in range(tree.N)]
        idx = np.random.default_rng(5).permutation(256)
        outs.append(tree.contract_pick(xs, indices=idx))
        _, st, _ = pick_state(tree)
        print("slice batch", cap, st["exec"].batch)
        assert int(st["exec"].batch) == int(cap)
    assert outs[0].tobytes() == outs[1].tobytes()


# ---- strip_exponent ------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_strip_exponent(dtype):
    tree, arrays, ref, bound = shape_case(64, "arena", dtype)
    coords = requests(ref.shape, 257, seed=14)
    plain = tree.contract_pick(arrays, coords=coords)
    mant, e = tree.contract_pick(arrays, coords=coords, strip_exponent=True)
    assert np.abs(np.asarray(mant) * 10.0 ** e - plain).max() <= bound
    assert np.abs(np.asarray(mant) * 10.0 ** e - ref[tuple(coords.T)]).max() <= bound
    zeros = [np.zeros_like(arrays[0])] + list(arrays[1:])
    mant, e = tree.contract_pick(zeros, coords=coords, strip_exponent=True, check_zero=True)
    vals = np.asarray(mant) * (0.0 if e == float("-inf") else 10.0 ** e)
    assert not np.any(np.isnan(vals)) and np.all(vals == 0)


# ---- entry points -------------------------------------------------------------------------------------------------- #

def test_round_trip_with_sample():
    tree, arrays, ref, bound = shape_case(128, "arena", "complex64")
    res = tree.contract_sample(arrays, 64, seed=1)
    a = tree.contract_pick(arrays, indices=res.indices)
    assert np.abs(a - res.amplitudes).max() <= bound
    assert np.abs(a - ref.reshape(-1)[res.indices]).max() <= bound
    assert tree.contract_pick(arrays, coords=res.coords).tobytes() == a.tobytes()


def test_expression_pick_and_torch_inputs():
    import torch

    tree, arrays, ref, bound = shape_case(64, "leaf", "complex64")
    coords = requests(ref.shape, 100, seed=15)
    from cotengra_amd.interface import ContractExpression

    expr = ContractExpression(tree)
    a = expr.pick(*arrays, coords=coords)
    assert np.abs(a - ref[tuple(coords.T)]).max() <= bound
    ts = [torch.tensor(x, device="cuda", requires_grad=(i == 0)) for i, x in enumerate(arrays)]
    b = expr.pick(*ts, coords=coords)
    assert isinstance(b, torch.Tensor) and b.is_cuda and not b.requires_grad
    assert b.cpu().numpy().tobytes() == a.tobytes()


def test_later_calls_on_the_same_tree():
    tree, arrays, ref, bound = shape_case(27, "arena", "complex64")
    full = np.asarray(tree.contract(arrays))
    top = tree.contract_topk((), 4, reuse=True)
    tree.contract_pick(arrays, coords=requests(ref.shape, 10, seed=16))
    with pytest.raises(RuntimeError):
        tree.contract_topk((), 4, reuse=True)
    assert np.asarray(tree.contract(arrays)).tobytes() == full.tobytes()
    assert np.array_equal(tree.contract_topk((), 4, reuse=True).indices, top.indices)
    # one pick contractor at a time: a new table replaces the one before
    tree.contract_pick(arrays, coords=requests(ref.shape, 11, seed=17))
    assert sum(1 for k in tree.contraction_cores if k[0] == "hip-pick") == 1
    assert _tree_contractor(tree)._execs


def test_amplitudes_of():
    n = 10
    gates = random_circuit(n, 6, seed=21)
    psi = statevector(n, gates)
    rng = np.random.default_rng(22)
    bits = rng.integers(0, 2, size=(200, n))
    fixed = {2: 1, 5: 0, 8: 1}
    for q, v in fixed.items():
        bits[:, q] = v
    strings = ["".join(str(int(b)) for b in row) for row in bits]
    out = circuits.amplitudes_of(n, gates, strings, dtype="complex64")
    assert out["open_qubits"] == [q for q in range(n) if q not in fixed]
    assert out["bitstrings"] == strings and out["amplitudes"].shape == (200,)
    sel = tuple(fixed.get(q, slice(None)) for q in range(n))
    ref = psi[sel]
    inputs, output, sd, arrays = circuits.circuit_to_network(
        n, gates, "".join(str(fixed[q]) if q in fixed else "?" for q in range(n)), simplify=True, dtype="complex64")
    tree = ca.array_contract_tree(inputs, output, sd)
    from oracle import contract_ref as orc

    tol = G.single_gate(ref, np.asarray(orc.contract(tree, arrays)).reshape(ref.shape)) * float(np.abs(ref).max())
    exact = np.array([psi[tuple(row)] for row in bits])
    assert np.abs(out["amplitudes"] - exact).max() <= tol
    assert np.allclose(out["p"], np.abs(out["amplitudes"]).astype(np.float64) ** 2)
    assert np.isfinite(circuits.linear_xeb(n, out["p"]))
