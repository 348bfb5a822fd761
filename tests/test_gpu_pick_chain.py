"""The requests of a pick carried down the tree on the device: ``pair_pick_rows_kernel`` in
both forms and both load widths against ``np.einsum`` of the whole output, a sparse node that reads a sparse child,
bit-for-bit determinism, ``chain=True`` against ``chain=False``, ``strip_exponent`` and the public entry points.

Tolerance: that of ``test_gpu_pick`` (``bound_of``): per picked element ``1e-12 * max|ref|`` in double precision and
``golden_util.single_gate(ref, numpy's single-precision run) * max|ref|`` in single, ``ref`` the whole output in
double precision by ``np.einsum``."""
import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits
from cotengra_amd import plan as P
from cotengra_amd.circuits import circuit_to_network

import golden_util as G
from test_gpu_pick import DTYPES, T_NAME, bound_of, data
from test_gpu_sample import random_circuit, statevector

pytestmark = pytest.mark.gpu

MS = [1, 63, 64, 65, 257]
# (row_lo, N, K) of the sparse step: every row_lo of {1, 2, 3, 31, 32, 33, 96}, every N of {1, 2, 7, 8, 9, 32, 33},
# every K of {1, 2, 3, 8, 9, 64, 65}, both sides of row_lo >= 32, N >= 8 and K >= 8 with the other two conditions
# met.  (row_lo >= N: the child with more kept elements supplies the rows.)
SHAPES = [
    (1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 1, 8), (1, 1, 9), (1, 1, 64), (1, 1, 65),
    (2, 1, 8), (2, 2, 2), (2, 2, 65), (3, 1, 3), (3, 2, 9), (3, 2, 64),
    (31, 1, 64), (31, 7, 8), (31, 8, 8), (31, 9, 9), (31, 8, 65),
    (32, 1, 8), (32, 2, 64), (32, 7, 8), (32, 7, 64), (32, 8, 3), (32, 8, 8), (32, 8, 9), (32, 9, 64), (32, 32, 8),
    (32, 32, 65),
    (33, 2, 1), (33, 7, 9), (33, 8, 2), (33, 8, 8), (33, 9, 65), (33, 32, 64), (33, 33, 8), (33, 33, 3),
    (96, 1, 65), (96, 8, 8), (96, 9, 1), (96, 32, 9), (96, 33, 64), (96, 33, 65),
]
assert {s[0] for s in SHAPES} == {1, 2, 3, 31, 32, 33, 96} and {s[1] for s in SHAPES} == {1, 2, 7, 8, 9, 32, 33}
assert {s[2] for s in SHAPES} == {1, 2, 3, 8, 9, 64, 65}

NAMES_MET = set()


def chain_tree(row_lo, N, K, layout, o=8, o3=2, sliced=False):
    """``x[o1,a,k] y[o2,k,b] -> p``, ``p z[o3,a,b] -> (o1,o2,o3)`` with ``a = row_lo``, ``b = N``, ``k = K``: two
    leaves under ``p`` (``leaf``), or -- ``arena`` -- ``x`` and ``y`` each the product of two inputs."""
    sizes = dict(o1=o, o2=o, o3=o3, a=row_lo, b=N, k=K, u=4 if sliced else 2, v=2)
    if layout == "leaf":
        tree = ca.ContractionTree.from_path([("o1", "a", "k"), ("o2", "k", "b"), ("o3", "a", "b")], ("o1", "o2", "o3"),
                                            sizes, ssa_path=[(0, 1), (3, 2)])
    else:
        tree = ca.ContractionTree.from_path(
            [("o1", "a", "u"), ("u", "k"), ("o2", "v", "b"), ("v", "k"), ("o3", "a", "b")], ("o1", "o2", "o3"), sizes,
            ssa_path=[(0, 1), (2, 3), (5, 6), (7, 4)])
    if sliced:
        tree.remove_ind_("u")
    return tree


def table(M, o=8, o3=2, n_pairs=None, seed=0):
    """``M`` requests with duplicates over at most ``o * o / 2`` distinct ``(o1, o2)``: ``p`` is sparse."""
    rng = np.random.default_rng(seed + M)
    n_pairs = min(M, o * o // 2) if n_pairs is None else n_pairs
    pairs = rng.permutation(o * o)[:n_pairs]
    which = np.concatenate([np.arange(n_pairs), rng.integers(0, n_pairs, M - n_pairs)])
    rng.shuffle(which)
    coords = np.stack([pairs[which] // o, pairs[which] % o, rng.integers(0, o3, M)], axis=1).astype(np.int64)
    if M > 2:
        coords[M // 2:M // 2 + M // 4 + 1] = coords[:M // 4 + 1]   # whole requests twice, apart from each other
    return coords


def chain_state(tree):
    """``(plan, executor, indices of the KERNEL_PICK_ROWS steps)`` of the pick contractor cached on ``tree``."""
    fns = [f for k, f in tree.contraction_cores.items() if isinstance(k, tuple) and k[0] == "hip-pick"]
    assert len(fns) == 1, list(tree.contraction_cores)
    (st,) = fns[0]._execs.values()
    idx = [i for i, s in enumerate(st["plan"].steps) if s.kernel == P.KERNEL_PICK_ROWS]
    return st["plan"], st["exec"], idx


def rows_names(tree):
    plan, ex, idx = chain_state(tree)
    names = ex.step_kernels()
    return [(plan.steps[i], names[i]) for i in idx]


def expected_name(step, dtype, vec):
    if P.pick_rows_route(step.row_lo, step.K, step.N, dtype) == "mfma":
        return "pair_pick_rows_mfma_kernel<c64>"
    return f"pair_pick_rows_kernel<{T_NAME[dtype]},{vec}>"


_CASES = {}


def shape_case(shape, layout, dtype):
    key = (shape, layout, dtype)
    if key not in _CASES:
        tree = chain_tree(*shape, layout)
        rng = np.random.default_rng(sum(shape))
        arrays = [data(rng, s, dtype) for s in tree.get_shapes()]
        _CASES[key] = (tree, arrays) + bound_of(tree, arrays, dtype)
    return _CASES[key]


# ---- the kernel over its shapes, both layouts, all four dtypes ------------------------------------------------------ #

@pytest.mark.parametrize("layout", ["leaf", "arena"])
@pytest.mark.parametrize("shape", SHAPES, ids=["i%d-n%d-k%d" % s for s in SHAPES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes(dtype, shape, layout):
    row_lo, N, K = shape
    tree, arrays, ref, bound = shape_case(shape, layout, dtype)
    # two adjacent k per load: both children contiguous along an even k (intermediates are laid out so; of the
    # leaves y[o2, k, b] is only when b = 1)
    vec = 2 if K % 2 == 0 and (layout == "arena" or N == 1) else 1
    for M in MS:
        coords = table(M)
        got = tree.contract_pick(arrays, coords=coords, chain=1)
        assert got.shape == (M,) and got.dtype == np.dtype(dtype)
        ((step, name),) = rows_names(tree)
        assert (step.row_lo, step.N, step.K) == shape and step.R == len(np.unique(coords[:, :2], axis=0)) * row_lo
        NAMES_MET.add(name)
        err = float(np.abs(got - ref[tuple(coords.T)]).max())
        print(f"{dtype} i={row_lo} n={N} k={K} {layout} M={M}: {name} err {err:.3e} bound {bound:.3e}")
        assert name == expected_name(step, dtype, vec), (name, shape, layout)
        assert err <= bound, (dtype, shape, layout, M, err, bound)


def test_both_forms_and_both_widths_are_met():
    met = set()
    for shape in [(1, 1, 64), (33, 8, 8), (33, 8, 2), (33, 33, 3), (96, 33, 64), (32, 7, 64)]:
        for layout in ("leaf", "arena"):
            tree, arrays, ref, bound = shape_case(shape, layout, "complex64")
            coords = table(65)
            got = tree.contract_pick(arrays, coords=coords, chain=1)
            assert np.abs(got - ref[tuple(coords.T)]).max() <= bound
            ((_, name),) = rows_names(tree)
            met.add(name)
    print("instantiations met:", sorted(met | NAMES_MET))
    assert {"pair_pick_rows_mfma_kernel<c64>", "pair_pick_rows_kernel<c64,1>", "pair_pick_rows_kernel<c64,2>"} <= met


# ---- two levels: a sparse node reads a sparse child ----------------------------------------------------------------- #

@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_two_levels(dtype):
    sizes = dict(o1=8, o2=8, o3=4, o4=3, a=33, b=9, c=8, k=12)
    tree = ca.ContractionTree.from_path(
        [("o1", "a", "k"), ("o2", "k", "b"), ("o3", "b", "c"), ("o4", "a", "c")], ("o1", "o2", "o3", "o4"), sizes,
        ssa_path=[(0, 1), (4, 2), (5, 3)])
    rng = np.random.default_rng(3)
    arrays = [data(rng, s, dtype) for s in tree.get_shapes()]
    ref, bound = bound_of(tree, arrays, dtype)
    coords = np.stack([rng.integers(0, d, 40) for d in ref.shape], axis=1).astype(np.int64)
    coords[:, :2] = coords[:, :2] % 5   # (at most 25 distinct (o1, o2))
    nodes = P.pick_chain_nodes(tree, coords, True)
    assert len(nodes) == 2
    got = tree.contract_pick(arrays, coords=coords, chain=True)
    found = rows_names(tree)
    assert len(found) == 2 and any(P.is_rows_axis(ix) for s, _ in found for ix in s.a.inds + s.b.inds)
    print([n for _, n in found])
    assert np.abs(got - ref[tuple(coords.T)]).max() <= bound
    one = tree.contract_pick(arrays, coords=coords, chain=1)
    assert len(rows_names(tree)) == 1
    assert np.abs(one - ref[tuple(coords.T)]).max() <= bound


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_a_hyper_leg_kept_dense_on_both_children(dtype):
    """``h`` is on both children of the sparse node and on its result: B moves with the position inside a row, so
    the step has no matrix-core form whatever its extents (here 96 x 8 over k = 8) and takes the vector form."""
    tree = ca.ContractionTree.from_path(
        [("o1", "h", "a", "k"), ("o1", "o2", "h", "k", "b"), ("o3", "h", "a", "b")], ("o1", "o2", "o3"),
        dict(o1=8, o2=8, o3=2, h=3, a=32, b=8, k=8), ssa_path=[(0, 1), (3, 2)])
    rng = np.random.default_rng(9)
    arrays = [data(rng, s, dtype) for s in tree.get_shapes()]
    ref, bound = bound_of(tree, arrays, dtype)
    coords = table(65)
    got = tree.contract_pick(arrays, coords=coords, chain=True)
    ((step, name),) = rows_names(tree)
    assert (step.row_lo, step.N, step.K) == (96, 8, 8) and np.any(step.rows["B"][1] != 0)
    assert P.pick_rows_route(96, 8, 8, dtype) == ("mfma" if dtype == "complex64" else "vector")
    assert name == f"pair_pick_rows_kernel<{T_NAME[dtype]},1>", name
    assert np.abs(got - ref[tuple(coords.T)]).max() <= bound


def test_hyper_index_golden_tree_chained():
    case = next(c for c in G.cases("tree") if c["name"] == "rand_s666_r3_o2_hi2_ho2")
    tree = G.tree_of(case)
    arrays = G.arrays_of(case, "complex64", tree)
    ref, bound = bound_of(tree, arrays, "complex64")
    rng = np.random.default_rng(6)
    few = np.stack([rng.integers(0, d, 2) for d in ref.shape], axis=1).astype(np.int64)
    coords = few[rng.integers(0, 2, 30)]   # (two distinct requests: whatever can be sparse is)
    got = tree.contract_pick(arrays, coords=coords, chain=True)
    assert len(chain_state(tree)[2]) == len(P.pick_chain_nodes(tree, coords, True))
    print("sparse nodes", P.pick_chain_nodes(tree, coords, True))
    assert np.abs(got - ref[tuple(coords.T)]).max() <= bound


# ---- determinism, bit for bit --------------------------------------------------------------------------------------- #

@pytest.mark.parametrize("shape,layout", [((33, 8, 9), "leaf"), ((96, 33, 64), "arena"), ((3, 2, 64), "arena"),
                                          ((1, 1, 65), "leaf")])
def test_bits_do_not_depend_on_the_table(shape, layout):
    tree, arrays, ref, _ = shape_case(shape, layout, "complex64")
    coords = table(257)
    a = tree.contract_pick(arrays, coords=coords, chain=1)
    assert tree.contract_pick(arrays, coords=coords, chain=1).tobytes() == a.tobytes()
    perm = np.random.default_rng(12).permutation(len(coords))
    b = tree.contract_pick(arrays, coords=coords[perm], chain=1)
    assert b[np.argsort(perm)].tobytes() == a.tobytes()
    dup = np.concatenate([coords, coords[::5], coords[:9]])
    c = tree.contract_pick(arrays, coords=dup, chain=1)
    assert c[:len(coords)].tobytes() == a.tobytes() and c[len(coords):].tobytes() == np.concatenate([a[::5], a[:9]]).tobytes()
    # after an unrelated ordinary call on the same tree
    tree.contract(arrays)
    assert tree.contract_pick(arrays, coords=coords, chain=1).tobytes() == a.tobytes()


def test_bits_do_not_depend_on_the_slice_batch(monkeypatch):
    outs = []
    for cap in ("1", "4"):
        monkeypatch.setenv("CTG_SLICE_BATCH", cap)
        tree = chain_tree(33, 8, 16, "arena", sliced=True)
        assert tree.nslices == 4
        rng = np.random.default_rng(4)
        arrays = [data(rng, s, "complex64") for s in tree.get_shapes()]
        outs.append(tree.contract_pick(arrays, coords=table(65), chain=1))
        plan, ex, idx = chain_state(tree)
        print("slice batch", cap, ex.batch)
        assert len(idx) == 1 and int(ex.batch) == int(cap)
    ref, bound = bound_of(tree, arrays, "complex64")
    assert np.abs(outs[0] - ref[tuple(table(65).T)]).max() <= bound
    assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("dtype,K", [("complex64", 4), ("complex64", 8), ("complex128", 4)])
def test_a_row_that_reuses_a_and_the_same_row_first_in_its_run(dtype, K):
    """Enough rows that a lane group walks four of them and keeps the A values of rows with one ``rowA.hi``
    (csrc/ctg_pick_rows.hip: pick_rows_shape): with the first row of the sorted table taken away every other row
    moves one place in its run -- a row that reused A now loads it, and the other way round."""
    o = 256
    tree = chain_tree(8, 8, K, "arena", o=o)
    rng = np.random.default_rng(6)
    arrays = [data(rng, s, dtype) for s in tree.get_shapes()]
    ref, bound = bound_of(tree, arrays, dtype)
    pairs = np.sort(rng.permutation(o * o)[:o * o // 2])
    coords = np.stack([pairs // o, pairs % o, rng.integers(0, 2, len(pairs))], axis=1).astype(np.int64)
    a = tree.contract_pick(arrays, coords=coords, chain=1)
    ((step, name),) = rows_names(tree)
    assert step.R // step.row_lo == len(pairs) >= 4 * 4096 and name.startswith("pair_pick_rows_kernel<")
    assert np.abs(a - ref[tuple(coords.T)]).max() <= bound
    for drop in (1, 2, 3):
        b = tree.contract_pick(arrays, coords=coords[drop:], chain=1)
        assert b.tobytes() == a[drop:].tobytes()
    # few rows: nothing is walked, nothing reused
    few = coords[::997]
    assert tree.contract_pick(arrays, coords=few, chain=1).tobytes() == a[::997].tobytes()


# ---- chain=True against chain=False --------------------------------------------------------------------------------- #

_CIRCUIT = {}


def circuit12(dtype):
    if dtype not in _CIRCUIT:
        n = 12
        inputs, output, sd, arrays = circuit_to_network(n, random_circuit(n, 8, 3), "?" * n, simplify=True, dtype=dtype)
        tree = ca.array_contract_tree(inputs, output, sd)
        coords = np.random.default_rng(5).integers(0, 2, (50, n)).astype(np.int64)
        # (more indices than np.einsum has letters for: the pairwise numpy reference, the recipe of bound_of)
        from oracle import contract_ref as orc

        ref = np.asarray(orc.contract(tree, [x.astype("complex128") for x in arrays])).reshape(tree.gathered_shape())
        scale = float(np.abs(ref).max())
        if dtype == "complex128":
            bound = 1e-12 * scale
        else:
            bound = G.single_gate(ref, np.asarray(orc.contract(tree, arrays)).reshape(ref.shape)) * scale
        _CIRCUIT[dtype] = (tree, arrays, coords, ref, bound)
    return _CIRCUIT[dtype]


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_chained_against_unchained(dtype):
    tree, arrays, coords, ref, bound = circuit12(dtype)
    plain = tree.contract_pick(arrays, coords=coords)
    assert not chain_state(tree)[2]
    chained = tree.contract_pick(arrays, coords=coords, chain=True)
    plan, _, idx = chain_state(tree)
    print("sparse steps", [plan.steps[i].label for i in idx], [n for _, n in rows_names(tree)])
    assert idx, "no node below the root is sparse"
    assert np.abs(chained - plain).max() <= bound
    assert np.abs(chained - ref[tuple(coords.T)]).max() <= bound
    assert np.abs(plain - ref[tuple(coords.T)]).max() <= bound


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_strip_exponent(dtype):
    tree, arrays, coords, ref, bound = circuit12(dtype)
    plain = tree.contract_pick(arrays, coords=coords, chain=True)
    mant, e = tree.contract_pick(arrays, coords=coords, chain=True, strip_exponent=True)
    assert chain_state(tree)[2]
    assert np.abs(np.asarray(mant) * 10.0 ** e - plain).max() <= bound
    assert np.abs(np.asarray(mant) * 10.0 ** e - ref[tuple(coords.T)]).max() <= bound


# ---- entry points --------------------------------------------------------------------------------------------------- #

def test_amplitudes_of_chained():
    n = 12
    gates = random_circuit(n, 6, seed=21)
    psi = statevector(n, gates)
    bits = np.random.default_rng(22).integers(0, 2, size=(60, n))
    strings = ["".join(str(int(b)) for b in row) for row in bits]
    out = circuits.amplitudes_of(n, gates, strings, dtype="complex64", chain=True)
    assert out["open_qubits"] == list(range(n)) and out["amplitudes"].shape == (60,)
    inputs, output, sd, arrays = circuit_to_network(n, gates, "?" * n, simplify=True, dtype="complex64")
    tree = ca.array_contract_tree(inputs, output, sd)
    assert P.pick_chain_nodes(tree, bits, True), "no node below the root is sparse"
    from oracle import contract_ref as orc

    tol = G.single_gate(psi, np.asarray(orc.contract(tree, arrays)).reshape(psi.shape)) * float(np.abs(psi).max())
    exact = np.array([psi[tuple(row)] for row in bits])
    assert np.abs(out["amplitudes"] - exact).max() <= tol
    plain = circuits.amplitudes_of(n, gates, strings, dtype="complex64")
    assert np.abs(out["amplitudes"] - plain["amplitudes"]).max() <= tol


def test_expression_pick_chained_with_torch_inputs():
    import torch
    from cotengra_amd.interface import ContractExpression

    tree, arrays, ref, bound = shape_case((33, 8, 8), "arena", "complex64")
    coords = table(65)
    expr = ContractExpression(tree)
    a = expr.pick(*arrays, coords=coords, chain=1)
    assert len(chain_state(tree)[2]) == 1
    assert np.abs(a - ref[tuple(coords.T)]).max() <= bound
    ts = [torch.tensor(x, device="cuda") for x in arrays]
    b = expr.pick(*ts, coords=coords, chain=1)
    assert isinstance(b, torch.Tensor) and b.is_cuda
    assert b.cpu().numpy().tobytes() == a.tobytes()
