"""The requests of a pick plan carried down the tree as row-sparse intermediates, checked
without a device: the default plan is unchanged, the rule that makes a node sparse, the form of its step, the arena
it saves, the values through the numpy plan interpreter against ``np.einsum`` of the whole network, independence
of the table's order and duplicates, the library's plan validator, and the route between the kernel's two forms."""
import os
import re

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import plan as P
from cotengra_amd import runtime
from cotengra_amd.circuits import circuit_to_network
from cotengra_amd.plan import KERNEL_PICK, KIND_ACCUM, KIND_PAIR, KIND_SINGLE, KIND_STEM2, compile_tree
from oracle import plan_interp

import test_pick_host as H
from test_circuits import random_circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_TREES = H.ALL_TREES


# ---- trees and tables -------------------------------------------------------------------------------------------- #

def chain3(a=3, b=5, k=6, o3=4):
    """``x[o1,a,k] y[o2,k,b] -> p``, ``p z[o3,a,b] -> (o1,o2,o3)``; ``spine(tree) == [p]``."""
    return ca.ContractionTree.from_path(
        [("o1", "a", "k"), ("o2", "k", "b"), ("o3", "a", "b")], ("o1", "o2", "o3"),
        dict(o1=8, o2=8, o3=o3, a=a, b=b, k=k), ssa_path=[(0, 1), (3, 2)])


def chain4():
    """``x y -> p``, ``p z[o3,b,c] -> q``, ``q u[o4,a,c] -> (o1,o2,o3,o4)``; ``spine(tree) == [q, p]``."""
    return ca.ContractionTree.from_path(
        [("o1", "a", "k"), ("o2", "k", "b"), ("o3", "b", "c"), ("o4", "a", "c")], ("o1", "o2", "o3", "o4"),
        dict(o1=8, o2=8, o3=4, o4=3, a=3, b=5, c=2, k=6), ssa_path=[(0, 1), (4, 2), (5, 3)])


def spine(tree):
    """The intermediates on the way down from the root (the non-leaf child of each), top first."""
    out, node = [], tree.root
    while True:
        kids = [c for c in tree.children[node] if not tree.is_leaf(c)]
        if not kids:
            return out
        (node,) = kids
        out.append(node)


def table3(n_pairs, M=None, seed=0, o3=4):
    """``M`` requests of ``chain3`` with exactly ``n_pairs`` distinct ``(o1, o2)``."""
    rng = np.random.default_rng(seed)
    pairs = rng.permutation(64)[:n_pairs]
    M = n_pairs + 7 if M is None else M
    which = np.concatenate([np.arange(n_pairs), rng.integers(0, n_pairs, M - n_pairs)])
    rng.shuffle(which)
    return np.stack([pairs[which] // 8, pairs[which] % 8, rng.integers(0, o3, M)], axis=1).astype(np.int64)


def table4(M=20, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, d, M) for d in (8, 8, 4, 3)], axis=1).astype(np.int64)


_CIRCUIT = {}


def circuit12():
    """``random_circuit(12, 8, seed=3)`` with all qubits open and 50 random requests: tree, arrays, coords."""
    if not _CIRCUIT:
        n = 12
        inputs, output, sd, arrays = circuit_to_network(n, random_circuit(n, 8, 3), "?" * n, simplify=True)
        tree = ca.array_contract_tree(inputs, output, sd)
        coords = np.random.default_rng(5).integers(0, 2, (50, n)).astype(np.int64)
        _CIRCUIT["v"] = (tree, arrays, coords)
        _FULL_BY_ORACLE(tree, arrays)   # (the whole state once, for the sliced twin as well)
    return _CIRCUIT["v"]


def einsum_at(tree, arrays, coords):
    """The whole output in complex128 at the requests, and its largest modulus: ``np.einsum`` of the network, or
    -- more indices than ``np.einsum`` has letters for -- the pairwise numpy reference of the unsliced tree."""
    ids = {}
    sym = lambda t: [ids.setdefault(ix, len(ids)) for ix in t]  # noqa: E731
    args = []
    for x, term in zip(arrays, tree.inputs):
        args += [np.asarray(x, dtype="complex128"), sym(term)]
    if len(ids) <= 52:
        full = np.einsum(*args, sym(tree.output), optimize=True)
    else:
        full = np.asarray(_FULL_BY_ORACLE(tree, arrays))
    return full[tuple(coords.T)], float(np.abs(full).max())


def _FULL_BY_ORACLE(tree, arrays):
    key = id(arrays)
    if key not in _ORACLE:
        from oracle import contract_ref as orc

        assert not tree.sliced_inds
        _ORACLE[key] = np.asarray(orc.contract(tree, [np.asarray(x, dtype="complex128") for x in arrays])).reshape(
            tree.gathered_shape())
    return _ORACLE[key]


_ORACLE = {}


def rows_steps(plan):
    return [s for s in plan.steps if s.kernel == P.KERNEL_PICK_ROWS]


def same_plan(a, b):
    sa, sb = a.serialise(), b.serialise()
    return sa.keys() == sb.keys() and all(np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])) for k in sa)


# ---- the default is the plan of before --------------------------------------------------------------------------- #

@pytest.mark.parametrize("name,tree", ALL_TREES, ids=[n for n, _ in ALL_TREES])
def test_default_unchanged(name, tree):
    coords = H.tables_of(tree)["dup"]
    for dtype in ("complex128", "complex64"):
        a = compile_tree(tree, dtype, pick=coords)
        b = compile_tree(tree, dtype, pick=coords, pick_chain=False)
        assert same_plan(a, b)
        assert not rows_steps(a) and not rows_steps(b)


def test_chain_needs_a_table():
    with pytest.raises(ValueError, match="pick_chain"):
        compile_tree(chain3(), "complex128", pick_chain=True)


# ---- the rule ---------------------------------------------------------------------------------------------------- #

def test_rule_at_both_sides_of_the_gain():
    assert P.PICK_CHAIN_GAIN == 2
    tree = chain3()
    (p,) = spine(tree)
    t32, t33 = table3(32), table3(33)
    assert P.pick_chain_nodes(tree, t32, True) == [(p, 32, 64, 3 * 5)]
    assert P.pick_chain_nodes(tree, t33, True) == []
    assert P.pick_chain_nodes(tree, t32, False) == [] and P.pick_chain_nodes(tree, t32, 0) == []
    plan = compile_tree(tree, "complex128", pick=t32, pick_chain=True)
    assert [s.node for s in rows_steps(plan)] == [p]
    plan = compile_tree(tree, "complex128", pick=t33, pick_chain=True)
    assert not rows_steps(plan) and same_plan(plan, compile_tree(tree, "complex128", pick=t33))


def test_levels():
    tree, coords = chain4(), table4()
    q, p = spine(tree)
    m_q = len(np.unique(coords[:, :3], axis=0))
    m_p = len(np.unique(coords[:, :2], axis=0))
    assert P.pick_chain_nodes(tree, coords, True) == [(q, m_q, 8 * 8 * 4, 3 * 2), (p, m_p, 64, 3 * 5)]
    assert P.pick_chain_nodes(tree, coords, 2) == P.pick_chain_nodes(tree, coords, True)
    assert P.pick_chain_nodes(tree, coords, 1) == [(q, m_q, 8 * 8 * 4, 3 * 2)]
    assert [s.node for s in rows_steps(compile_tree(tree, "complex128", pick=coords, pick_chain=True))] == [p, q]
    assert [s.node for s in rows_steps(compile_tree(tree, "complex128", pick=coords, pick_chain=1))] == [q]


def test_a_leaf_and_a_node_without_output_legs_are_never_sparse():
    # (ab.bc) carries no output leg; the leaves x and z do
    tree = ca.ContractionTree.from_path([("o1", "a"), ("a", "b"), ("b", "c"), ("c", "o2")], ("o1", "o2"),
                                        dict(o1=16, o2=16, a=2, b=3, c=2), ssa_path=[(1, 2), (0, 4), (5, 3)])
    coords = np.array([[1, 2], [3, 4], [1, 4]])
    (top,) = [c for c in tree.children[tree.root] if not tree.is_leaf(c)]
    assert [n for n, _, _, _ in P.pick_chain_nodes(tree, coords, True)] == [top]


# ---- the form of a sparse node's step ---------------------------------------------------------------------------- #

@pytest.mark.parametrize("case", ["chain3", "chain4", "circuit"])
def test_form(case):
    tree, coords = {"chain3": lambda: (chain3(), table3(20)), "chain4": lambda: (chain4(), table4()),
                    "circuit": lambda: (circuit12()[0], circuit12()[2])}[case]()
    nodes = P.pick_chain_nodes(tree, coords, True)
    assert nodes
    plan = compile_tree(tree, "complex64", pick=coords, pick_chain=True)
    assert [s.kernel for s in plan.steps].count(KERNEL_PICK) == 1
    for node, M_c, O_c, D_c in nodes:
        (step,) = [s for s in plan.steps if s.node == node]
        assert (step.kind, step.kernel, step.Bt) == (KIND_PAIR, P.KERNEL_PICK_ROWS, 1)
        assert step.R == M_c * step.row_lo and step.row_lo * step.N == D_c and step.c.size == M_c * D_c
        for key in "ABC":
            hi, lo = step.rows[key]
            assert len(hi) == M_c and len(lo) == step.row_lo
        for key in "AB":
            hi, lo = step.k_tabs[key]
            assert len(hi) * len(lo) == step.K and len(lo) == step.k_lo
        assert len(step.n_tabs["B"]) == step.N and len(step.n_tabs["C"]) == step.N
        # rows sorted by (A, B); the result's rows a permutation of the canonical positions
        key = np.stack([step.rows["A"][0], step.rows["B"][0]], axis=1)
        assert np.array_equal(key[np.lexsort((key[:, 1], key[:, 0]))], key)
        assert sorted(step.rows["C"][0].tolist()) == [j * D_c for j in range(M_c)]
        assert step.label == f"pick rows m{M_c} i{step.row_lo} k{step.K} n{step.N}"
        assert step.lds_comp == -1
    sparse = {n for n, _, _, _ in nodes}
    assert all(s.node not in sparse for s in plan.steps if s.kind == KIND_STEM2)
    for run in plan.lds_runs:
        assert all(plan.steps[i].node not in sparse for i in run["members"])
    assert "pick_rows" in {row["kernel"] for row in plan.describe_steps()}


def test_sparse_nodes_leave_the_lds_component_they_would_join():
    """The golden trees whose root step joins an LDS-resident subtree in the ordinary plan, one level down: a
    child of the root that the ordinary pick plan keeps in a component is in none once it is sparse."""
    left = 0
    for name, tree in H.GOLDEN:
        coords = np.repeat(H.random_coords(tree, 1, seed=2), 5, axis=0)   # (one distinct request: M_c = 1 everywhere)
        sparse = {n for n, _, _, _ in P.pick_chain_nodes(tree, coords, True)}
        plain = compile_tree(tree, "complex128", pick=coords)
        plan = compile_tree(tree, "complex128", pick=coords, pick_chain=True)
        left += sum(1 for s in plain.steps if s.node in sparse and s.lds_comp >= 0)
        for s in plan.steps:
            if s.node in sparse:
                assert s.kernel == P.KERNEL_PICK_ROWS and s.lds_comp == -1
        for run in plan.lds_runs:
            assert all(plan.steps[i].node not in sparse for i in run["members"])
    assert left >= 1, "no golden tree exercises the exclusion"


def test_sparse_nodes_leave_the_fused_stem_steps(monkeypatch):
    H.G.fuse_whatever_fits(monkeypatch)
    tree = H.G.stem_network(*H.G.STEM_CASES[0], seed=0)
    coords = np.repeat(H.random_coords(tree, 2, seed=3), 3, axis=0)
    sparse = {n for n, _, _, _ in P.pick_chain_nodes(tree, coords, True)}
    assert sparse
    plan = compile_tree(tree, "complex64", fuse_min_elems=1, pick=coords, pick_chain=True)
    assert all(s.node not in sparse and s.node != tree.root for s in plan.steps if s.kind == KIND_STEM2)
    assert sorted(s.node for s in rows_steps(plan)) == sorted(sparse)


# ---- layout ------------------------------------------------------------------------------------------------------ #

def test_arena_of_the_chained_plan_is_smaller():
    tree, _, coords = circuit12()
    plain = compile_tree(tree, "complex64", pick=coords)
    chained = compile_tree(tree, "complex64", pick=coords, pick_chain=True)
    print("arena elements", plain.arena_elems, "->", chained.arena_elems)
    assert chained.arena_elems < plain.arena_elems


def test_children_of_a_sparse_node_are_laid_out_for_its_step():
    """A sparse child and a dense intermediate under a sparse node: both k tables of that node's step unit-stride."""
    tree, coords = chain4(), table4()
    plan = compile_tree(tree, "complex128", pick=coords, pick_chain=True)
    for step in [s for s in plan.steps if s.kernel in (KERNEL_PICK, P.KERNEL_PICK_ROWS) and s.a.leaf < 0 and s.b.leaf < 0]:
        for key in "AB":
            hi, lo = step.k_tabs[key]
            assert np.array_equal(lo, np.arange(step.k_lo))


# ---- values through the plan interpreter ------------------------------------------------------------------------- #

def check_values(tree, arrays, coords, chain=True, need_sparse=False):
    ref, scale = einsum_at(tree, arrays, coords)
    plan = compile_tree(tree, "complex128", pick=coords, pick_chain=chain)
    if need_sparse:
        assert rows_steps(plan), "no node below the root is sparse"
    for lds in (False, True):
        got = plan_interp.run_plan(plan, arrays, lds=lds)
        assert got.shape == (len(coords),)
        assert np.abs(got - ref).max() <= 1e-12 * scale, (np.abs(got - ref).max(), scale)
    return plan


@pytest.mark.parametrize("name,tree", ALL_TREES, ids=[n for n, _ in ALL_TREES])
def test_values_all_trees(name, tree):
    arrays = H.arrays_of(tree)
    for label, coords in H.tables_of(tree).items():
        check_values(tree, arrays, coords)


@pytest.mark.parametrize("case", ["chain3-32", "chain3-33", "chain3-1", "chain4", "chain4-1level", "hyper"])
def test_values_hand_built_chains(case):
    chain = True
    if case.startswith("chain3"):
        n = int(case.split("-")[1])
        tree, coords = chain3(), table3(n)
    elif case.startswith("chain4"):
        tree, coords, chain = chain4(), table4(), (1 if case.endswith("1level") else True)
    else:
        # a hyper leg h kept dense on both children of the sparse node, and an output leg on both
        tree = ca.ContractionTree.from_path(
            [("o1", "h", "a", "k"), ("o1", "o2", "h", "k", "b"), ("o3", "h", "a", "b")], ("o1", "o2", "o3"),
            dict(o1=8, o2=8, o3=4, h=3, a=2, b=5, k=4), ssa_path=[(0, 1), (3, 2)])
        coords = table3(12)
    rng = np.random.default_rng(2)
    arrays = [rng.standard_normal(s) + 1j * rng.standard_normal(s) for s in tree.get_shapes()]
    check_values(tree, arrays, coords, chain, need_sparse=case not in ("chain3-33",))


def test_values_circuit_all_qubits_open():
    tree, arrays, coords = circuit12()
    plan = check_values(tree, arrays, coords, need_sparse=True)
    nodes = P.pick_chain_nodes(tree, coords, True)
    print("sparse nodes (node, M_c, O_c, D_c):", nodes, "sparse elements", sum(m * d for _, m, _, d in nodes),
          "dense", sum(o * d for _, _, o, d in nodes))
    assert len(rows_steps(plan)) == len(nodes) >= 1


def test_values_sliced_circuit():
    tree, arrays, coords = circuit12()
    sliced = tree.slice(target_size=max(tree.max_size() // 4, 2), allow_outer=False)
    assert sliced.nslices > 1
    check_values(sliced, arrays, coords, need_sparse=True)


# ---- the table's order and duplicates ---------------------------------------------------------------------------- #

def test_permuted_and_duplicated_tables():
    tree, arrays, coords = circuit12()
    base = plan_interp.run_plan(compile_tree(tree, "complex128", pick=coords, pick_chain=True), arrays)
    nodes = P.pick_chain_nodes(tree, coords, True)
    perm = np.random.default_rng(8).permutation(len(coords))
    dup = np.concatenate([coords, coords[::3], coords[:7]])
    for table, back in ((coords[perm], np.argsort(perm)), (dup, np.arange(len(coords)))):
        assert P.pick_chain_nodes(tree, table, True) == nodes
        got = plan_interp.run_plan(compile_tree(tree, "complex128", pick=table, pick_chain=True), arrays)
        assert np.array_equal(got[back], base)
    got = plan_interp.run_plan(compile_tree(tree, "complex128", pick=dup, pick_chain=True), arrays)
    assert np.array_equal(got[len(coords):], np.concatenate([base[::3], base[:7]]))


# ---- the library's validator ------------------------------------------------------------------------------------- #

def validator_plan():
    """A chained plan with a SINGLE record (a repeated index on a leaf) and slices."""
    tree = ca.ContractionTree.from_path(
        [("o1", "a", "a", "k"), ("o2", "k", "b", "s"), ("o3", "a", "b", "s")], ("o1", "o2", "o3"),
        dict(o1=8, o2=8, o3=4, a=3, b=5, k=6, s=2), ssa_path=[(0, 1), (3, 2)])
    tree.remove_ind_("s")
    plan = compile_tree(tree, "complex64", pick=table3(16), pick_chain=True)
    (step,) = rows_steps(plan)
    return plan, plan.steps.index(step)


def test_validator_accepts_a_chained_plan():
    plan, i = validator_plan()
    dp = runtime.DevicePlan(plan)
    assert dp.nslices == 2
    dp.close()
    tree, _, coords = circuit12()
    runtime.DevicePlan(compile_tree(tree, "complex64", pick=coords, pick_chain=True)).close()
    assert runtime.load().ctg_abi_version() == 10


def _on_kind(kind):
    def make(i):
        def edit(recs):
            (j,) = [j for j in range(len(recs)) if recs[j, 0] == kind][:1]
            recs[i, 1], recs[j, 1] = 0, P.KERNEL_PICK_ROWS
        return edit
    return make


def _bt_two(i):
    def edit(recs):
        recs[i, 12] = 2
    return edit


@pytest.mark.parametrize("make", [_on_kind(KIND_SINGLE), _on_kind(KIND_ACCUM), _bt_two],
                         ids=["on-single", "on-accumulate", "Bt=2"])
def test_validator_rejects_the_kernel_code_anywhere_else(make):
    plan, i = validator_plan()
    with pytest.raises(ValueError, match="the pick rows kernel executes pair steps with Bt = 1 only"):
        runtime.DevicePlan(H.serialised_with(plan, make(i)))


@pytest.mark.parametrize("table", H.PICK_TABLES)
def test_validator_rejects_a_step_with_an_absent_table(table):
    text = open(os.path.join(ROOT, "cotengra_amd", "csrc", "ctg_common.h")).read()
    word = int(re.search(r"\b%s\s*=\s*(\d+)" % table, text).group(1))
    plan, i = validator_plan()

    def edit(recs):
        assert recs[i, word] >= 0
        recs[i, word] = -1

    with pytest.raises(ValueError, match="the pick rows kernel needs every row, k and n table"):
        runtime.DevicePlan(H.serialised_with(plan, edit))


def test_validator_checks_the_row_tables():
    """A per-row offset past the operand is refused like any table entry."""
    plan, i = validator_plan()
    plan.steps[i].rows["A"][0][-1] += plan.steps[i].a.size
    with pytest.raises(runtime.CtgError, match="outside its space"):
        runtime.DevicePlan(plan)


# ---- the route --------------------------------------------------------------------------------------------------- #

def test_route_is_pinned_at_both_sides_of_its_thresholds():
    assert P.pick_rows_route(32, 8, 8, "complex64") == "mfma"
    assert P.pick_rows_route(31, 8, 8, "complex64") == "vector"
    assert P.pick_rows_route(32, 7, 8, "complex64") == "vector"
    assert P.pick_rows_route(32, 8, 7, "complex64") == "vector"
    for dtype in ("float32", "float64", "complex128"):
        assert P.pick_rows_route(96, 64, 32, dtype) == "vector"


def test_route_constants_are_the_launchers():
    text = open(os.path.join(ROOT, "cotengra_amd", "csrc", "ctg_common.h")).read()
    m = re.search(r"kPickRowsMfmaMinRowLo\s*=\s*(\d+)\s*,\s*kPickRowsMfmaMinN\s*=\s*(\d+)\s*,\s*kPickRowsMfmaMinK\s*=\s*(\d+)\s*;", text)
    assert m, "the launcher's rule has moved"
    assert tuple(int(g) for g in m.groups()) == (P.PICK_ROWS_MFMA_MIN_ROW_LO, P.PICK_ROWS_MFMA_MIN_N, P.PICK_ROWS_MFMA_MIN_K)
    assert "dtype == 2 && row_lo >= kPickRowsMfmaMinRowLo && N >= kPickRowsMfmaMinN && K >= kPickRowsMfmaMinK" in text
    assert re.search(r"KERNEL_PICK_ROWS\s*=\s*%d\b" % P.KERNEL_PICK_ROWS, text)


# ---- the pick contractor's cache key -------------------------------------------------------------------------------- #

def test_chain_is_part_of_the_cache_key():
    from cotengra_amd.contractor import _tree_contractor, pick_requests

    tree = chain4()
    fn = _tree_contractor(tree)
    req = pick_requests(tree, table4(), None)
    plain = fn._pick_contractor(req)
    assert fn._pick_contractor(req, False) is plain and fn._pick_contractor(req, 0) is plain
    assert plain._pick_chain in (False, 0)
    one = fn._pick_contractor(req, 1)
    assert one is not plain and one._pick_chain == 1 and one._pick_chain is not True
    full = fn._pick_contractor(req, True)     # (True == 1 as a key, and is another plan)
    assert full is not one and full._pick_chain is True
    assert len(rows_steps(full.host_plan("complex64"))) == 2 and len(rows_steps(one.host_plan("complex64"))) == 1
    fn.close()
