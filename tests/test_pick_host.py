"""Chosen members of the output through a sparse root step, checked without a device: the
public entry points' argument checks, the form of the plans ``compile_tree(pick=...)`` emits, their values through
the numpy plan interpreter against ``np.einsum`` of the whole network, the library's plan validator, and the rule
that routes the step to its own kernel or to the k-reduction kernels."""
import os
import re

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import contractor as CT
from cotengra_amd import plan as P
from cotengra_amd import runtime
from cotengra_amd.plan import KERNEL_PICK, KIND_ACCUM, KIND_PAIR, KIND_SINGLE, KIND_STEM2, compile_tree
from oracle import plan_interp

import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- trees ------------------------------------------------------------------------------------------------------- #

def tree_batch():
    """abk,kbc->abc: a batch index on both operands, extents 2 and 3 mixed."""
    return ca.ContractionTree.from_path([("a", "b", "k"), ("k", "b", "c")], ("a", "b", "c"),
                                        dict(a=3, b=2, k=3, c=2), path=[(0, 1)])


def tree_preproc_leaf():
    """aak,kc->ac: a root child that is a leaf with preprocessing (a repeated index)."""
    return ca.ContractionTree.from_path([("a", "a", "k"), ("k", "c")], ("a", "c"), dict(a=3, k=4, c=3), path=[(0, 1)])


def tree_sliced():
    """Three tensors, two inner indices sliced: 4 slices."""
    tree = ca.ContractionTree.from_path([("a", "b", "c"), ("b", "c", "d", "e"), ("d", "e", "f")], ("f", "a"),
                                        dict(a=3, b=2, c=3, d=2, e=3, f=4), path=[(0, 1), (0, 1)])
    tree.remove_ind_("b")
    tree.remove_ind_("d")
    assert tree.nslices == 4
    return tree


def tree_single():
    """One input: a diagonal and a sum."""
    return ca.ContractionTree([("a", "b", "b", "k")], ("b", "a"), dict(a=3, b=4, k=5))


def golden_trees():
    """Three golden trees with at least two output indices, none of them sliced."""
    out = []
    for case in G.cases("tree"):
        tree = G.tree_of(case)
        if tree.N > 3 and len(tree.output) >= 2 and not any(ix in tree.sliced_inds for ix in tree.output) \
                and tree.nslices <= 16:
            out.append((case["name"], tree))
    picked = [t for t in out if t[1].nslices > 1][:1] + [t for t in out if t[1].nslices == 1][:2]
    assert len(picked) == 3, [n for n, _ in out]
    return picked


TREES = {"batch": tree_batch, "preproc_leaf": tree_preproc_leaf, "sliced": tree_sliced, "single": tree_single}
GOLDEN = golden_trees()
ALL_TREES = [(k, f()) for k, f in TREES.items()] + GOLDEN

_FULL = {}


def arrays_of(tree):
    rng = np.random.default_rng(7)
    return [rng.standard_normal(s) + 1j * rng.standard_normal(s) for s in tree.get_shapes()]


def full_of(name, tree):
    """``np.einsum`` of the whole network in complex128 (computed once per tree)."""
    if name not in _FULL:
        ids = {}
        sym = lambda t: [ids.setdefault(ix, len(ids)) for ix in t]  # noqa: E731
        arrays = arrays_of(tree)
        args = []
        for x, term in zip(arrays, tree.inputs):
            args += [x, sym(term)]
        _FULL[name] = np.einsum(*args, sym(tree.output))
    return _FULL[name]


def random_coords(tree, M, seed=0):
    rng = np.random.default_rng(seed)
    shape = tree.gathered_shape()
    return np.stack([rng.integers(0, d, M) for d in shape], axis=1).astype(np.int64)


def tables_of(tree):
    """Request tables: random with duplicates, all requests in one A row, and M = 1."""
    base = random_coords(tree, 23, seed=3)
    dup = np.concatenate([base, base[::-1][:9], base[:5]])
    plan = compile_tree(tree, "complex128", pick=random_coords(tree, 40, seed=4))
    step = pick_step(plan)
    # (requests that agree on every output index of A: take the first request's values on those columns)
    one_row = random_coords(tree, 17, seed=5)
    on_a = [j for j, ix in enumerate(tree.output) if step.a.stride_of(ix) != 0]
    one_row[:, on_a] = one_row[0, on_a]
    return {"dup": dup, "one_a_row": one_row, "m1": random_coords(tree, 1, seed=6)}


def pick_step(plan):
    if len(plan.input_sizes) == 1:
        steps = [s for s in plan.steps if s.kind == KIND_SINGLE]
    else:
        steps = [s for s in plan.steps if s.kernel == KERNEL_PICK]
    assert len(steps) == 1, steps
    return steps[0]


# ---- argument checks: ValueError before the device is touched ---------------------------------------------------- #

def fresh_contractor(tree):
    return CT.HipContractor(tree, handle_slicing=True)


def test_exactly_one_of_coords_and_indices():
    tree = tree_batch()
    fn, arrays = fresh_contractor(tree), arrays_of(tree)
    with pytest.raises(ValueError, match="exactly one"):
        fn.pick(*arrays)
    with pytest.raises(ValueError, match="exactly one"):
        fn.pick(*arrays, coords=np.zeros((1, 3), np.int64), indices=np.zeros(1, np.int64))
    assert not fn._execs


@pytest.mark.parametrize("kw", [
    dict(coords=np.zeros((2, 2), np.int64)),            # wrong width
    dict(coords=np.zeros(3, np.int64)),                 # wrong dimension
    dict(indices=np.zeros((2, 1), np.int64)),           # wrong dimension
    dict(coords=np.zeros((2, 3), np.float64)),          # not integers
    dict(indices=np.zeros(2, np.float32)),
    dict(coords=np.array([[0, 0, 2]])),                 # c has extent 2
    dict(coords=np.array([[-1, 0, 0]])),
    dict(indices=np.array([12])),                       # 3 * 2 * 2 elements
    dict(indices=np.array([-1])),
], ids=["width", "coords-1d", "indices-2d", "float-coords", "float-indices", "coord-high", "coord-negative",
        "index-high", "index-negative"])
def test_bad_requests_are_refused(kw):
    tree = tree_batch()
    fn = fresh_contractor(tree)
    with pytest.raises(ValueError, match="pick"):
        fn.pick(*arrays_of(tree), **kw)
    with pytest.raises(ValueError, match="pick"):
        tree.contract_pick(arrays_of(tree), **kw)
    assert not fn._execs and all(not f._execs for f in tree.contraction_cores.values())


def test_too_many_requests(monkeypatch):
    assert P.PICK_MAX == 1 << 24 and CT.PICK_MAX == P.PICK_MAX
    monkeypatch.setattr(CT, "PICK_MAX", 8)
    tree = tree_batch()
    with pytest.raises(ValueError, match="at most 8"):
        fresh_contractor(tree).pick(*arrays_of(tree), indices=np.zeros(9, np.int64))


@pytest.mark.parametrize("project", [None, 1])
def test_sliced_output_index_is_refused(project):
    tree = tree_batch()
    tree.remove_ind_("c", project=project)
    fn = fresh_contractor(tree)
    with pytest.raises(ValueError, match=r"sliced.*") as ei:
        fn.pick(*arrays_of(tree), coords=np.zeros((1, 3), np.int64))
    assert "'c'" in str(ei.value)
    with pytest.raises(ValueError, match="sliced"):
        compile_tree(tree, "complex64", pick=np.zeros((1, 3), np.int64))
    assert not fn._execs


def test_no_request_returns_an_empty_array_and_creates_nothing():
    tree = tree_batch()
    fn = fresh_contractor(tree)
    arrays = [x.astype("complex64") for x in arrays_of(tree)]
    for kw in (dict(coords=np.zeros((0, 3), np.int64)), dict(indices=np.zeros(0, np.int64)), dict(indices=[])):
        out = fn.pick(*arrays, **kw)
        assert isinstance(out, np.ndarray) and out.shape == (0,) and out.dtype == np.complex64
    assert not fn._execs and not fn._plans and not tree.contraction_cores


def test_expression_and_tree_entry_points_exist():
    assert callable(ca.ContractionTree.contract_pick)
    from cotengra_amd.interface import ContractExpression

    assert callable(ContractExpression.pick)
    from cotengra_amd import circuits

    assert callable(circuits.amplitudes_of) and "linear_xeb" in circuits.amplitudes_of.__doc__


def test_requests_from_indices_are_the_unravelled_coords():
    tree = tree_batch()
    shape = tree.gathered_shape()
    idx = np.array([0, 11, 5, 5, 7])
    req = CT.pick_requests(tree, indices=idx)
    assert req.dtype == np.int64 and np.array_equal(np.ravel_multi_index(tuple(req.T), shape), idx)
    assert np.array_equal(CT.pick_requests(tree, coords=req.astype(np.int32)), req)


# ---- the form of the plan ---------------------------------------------------------------------------------------- #

@pytest.mark.parametrize("name,tree", ALL_TREES, ids=[n for n, _ in ALL_TREES])
def test_plan_form(name, tree):
    coords = tables_of(tree)["dup"]
    M = len(coords)
    plan = compile_tree(tree, "complex128", pick=coords)
    assert plan.result_elems == M and tuple(plan.result_shape) == (M,)
    step = pick_step(plan)
    if tree.N > 1:
        assert [s.kernel for s in plan.steps].count(KERNEL_PICK) == 1
        assert (step.kind, step.R, step.N, step.Bt, step.row_lo) == (KIND_PAIR, M, 1, 1, 1)
        key = np.stack([step.rows["A"][0], step.rows["B"][0]], axis=1)
        order = np.lexsort((key[:, 1], key[:, 0]))
        assert np.array_equal(key[order], key), "requests are not sorted by (A row, B row)"
        for k in "ABC":
            assert np.array_equal(step.rows[k][1], [0])
        assert np.array_equal(step.n_tabs["B"], [0]) and np.array_equal(step.n_tabs["C"], [0])
    else:
        assert all(s.kernel != KERNEL_PICK for s in plan.steps)
        assert (step.R, step.row_lo) == (M, 1)
        assert np.all(np.diff(step.rows["A"][0]) >= 0)
    assert step.node == tree.root and step.c.size == M
    assert sorted(step.rows["C"][0].tolist()) == list(range(M))
    # the root belongs to no stem step and to no LDS-resident subtree
    root_index = plan.steps.index(step)
    assert all(s.node != tree.root for s in plan.steps if s.kind == KIND_STEM2)
    assert step.lds_comp == -1 and all(root_index not in run["members"] for run in plan.lds_runs)
    acc = plan.steps[-1]
    assert acc.kind == KIND_ACCUM and acc.R == M and acc.c.size == M


def test_root_leaves_the_lds_component_it_would_join():
    """In the ordinary plans of the small golden trees the root step is a member of an LDS-resident subtree;
    in their pick plans it is not, and its children may still be."""
    joined = 0
    for name, tree in GOLDEN:
        default = compile_tree(tree, "complex128")
        root_default = [s for s in default.steps if s.node == tree.root and s.kind == KIND_PAIR][0]
        joined += root_default.lds_comp >= 0
        plan = compile_tree(tree, "complex128", pick=random_coords(tree, 5))
        assert pick_step(plan).lds_comp == -1
    assert joined >= 1, "no golden tree exercises the exclusion"


def test_root_leaves_the_fused_stem_step_it_would_close(monkeypatch):
    """A stem whose last pair the ordinary plan fuses: the pick plan keeps the root out of it."""
    G.fuse_whatever_fits(monkeypatch)
    tree = G.stem_network(*G.STEM_CASES[0], seed=0)
    default = compile_tree(tree, "complex64", fuse_min_elems=1)
    assert any(s.kind == KIND_STEM2 and s.node == tree.root for s in default.steps)
    plan = compile_tree(tree, "complex64", fuse_min_elems=1, pick=random_coords(tree, 9))
    assert all(s.node != tree.root for s in plan.steps if s.kind == KIND_STEM2)
    assert [s.kernel for s in plan.steps].count(KERNEL_PICK) == 1


def test_children_that_are_intermediates_are_laid_out_for_the_step():
    """Both k tables unit-stride, every request offset a multiple of K, when both children are arena tensors."""
    # (ab.bc) and (cd.de) meet at the root over c
    tree4 = ca.ContractionTree.from_path([("a", "b"), ("b", "c"), ("c", "d"), ("d", "e")], ("e", "a"),
                                         dict(a=4, b=3, c=6, d=3, e=5), ssa_path=[(0, 1), (2, 3), (4, 5)])
    plan = compile_tree(tree4, "complex128", pick=random_coords(tree4, 11))
    step = pick_step(plan)
    K = step.K
    assert K == 6
    for key in "AB":
        hi, lo = step.k_tabs[key]
        assert np.array_equal(hi[:, None] + lo[None, :], np.arange(K).reshape(len(hi), -1))
        assert np.all(step.rows[key][0] % K == 0)


@pytest.mark.parametrize("name,tree", ALL_TREES, ids=[n for n, _ in ALL_TREES])
def test_default_plans_hold_no_pick_step(name, tree):
    plan = compile_tree(tree, "complex128")
    assert all(s.kernel != KERNEL_PICK for s in plan.steps)
    assert tuple(plan.result_shape) == tuple(tree.gathered_shape())


# ---- values through the plan interpreter ------------------------------------------------------------------------- #

@pytest.mark.parametrize("lds", [False, True], ids=["steps", "lds"])
@pytest.mark.parametrize("name,tree", ALL_TREES, ids=[n for n, _ in ALL_TREES])
def test_values_against_einsum(name, tree, lds):
    full = full_of(name, tree)
    arrays = arrays_of(tree)
    bound = 1e-12 * np.abs(full).max()
    for label, coords in tables_of(tree).items():
        plan = compile_tree(tree, "complex128", pick=coords)
        got = plan_interp.run_plan(plan, arrays, lds=lds)
        ref = full[tuple(coords.T)]
        assert got.shape == (len(coords),)
        assert np.abs(got - ref).max() <= bound, (name, label, np.abs(got - ref).max(), bound)


def test_default_layout_of_the_children_gives_the_same_values():
    name, tree = GOLDEN[1]
    coords = tables_of(tree)["dup"]
    plan = compile_tree(tree, "complex128", pick=coords, _pick_relayout=False)
    got = plan_interp.run_plan(plan, arrays_of(tree))
    full = full_of(name, tree)
    assert np.abs(got - full[tuple(coords.T)]).max() <= 1e-12 * np.abs(full).max()


# ---- the library's validator ------------------------------------------------------------------------------------- #

def serialised_with(plan, edit):
    ser = plan.serialise

    def edited():
        s = ser()
        recs = s["steps"].copy().reshape(-1, P.STEP_WORDS)
        edit(recs)
        s["steps"] = recs.reshape(-1)
        return s

    plan.serialise = edited
    return plan


def validator_plan():
    tree = tree_sliced()
    plan = compile_tree(tree, "complex64", pick=random_coords(tree, 10))
    i = plan.steps.index(pick_step(plan))
    return plan, i


def test_validator_accepts_a_pick_plan():
    plan, i = validator_plan()
    dp = runtime.DevicePlan(plan)
    assert dp.nslices == 4
    assert dp.workspace_bytes()["result"] == 10 * 8
    dp.close()
    assert runtime.load().ctg_abi_version() == 10


def _n_two(i):
    def edit(recs):
        recs[i, 14] = 2
    return edit


def _row_lo_two(i):
    def edit(recs):
        assert recs[i, 16] % 2 == 0
        recs[i, 15], recs[i, 16] = 2, recs[i, 16] // 2
    return edit


def _on_accum(i):
    def edit(recs):
        acc = [j for j in range(len(recs)) if recs[j, 0] == KIND_ACCUM]
        recs[i, 1], recs[acc[0], 1] = 0, KERNEL_PICK
    return edit


@pytest.mark.parametrize("make", [_n_two, _row_lo_two, _on_accum], ids=["N=2", "row_lo=2", "on-accumulate"])
def test_validator_rejects_the_kernel_code_anywhere_else(make):
    plan, i = validator_plan()
    with pytest.raises(ValueError, match="the pick kernel executes pair steps"):
        runtime.DevicePlan(serialised_with(plan, make(i)))


PICK_TABLES = ["W_ROWA_HI", "W_ROWA_LO", "W_ROWB_HI", "W_ROWB_LO", "W_ROWC_HI", "W_ROWC_LO", "W_KA_HI", "W_KA", "W_KB_HI",
               "W_KB", "W_NB", "W_NC"]


@pytest.mark.parametrize("table", PICK_TABLES)
def test_validator_rejects_a_pick_step_with_an_absent_table(table):
    """An offset of -1 stands for an absent table elsewhere; the pick kernel and the host's choice of its load
    width read every one."""
    text = open(os.path.join(ROOT, "cotengra_amd", "csrc", "ctg_common.h")).read()
    word = int(re.search(r"\b%s\s*=\s*(\d+)" % table, text).group(1))
    plan, i = validator_plan()

    def edit(recs):
        assert recs[i, word] >= 0
        recs[i, word] = -1

    with pytest.raises(ValueError, match="the pick kernel needs every row, k and n table"):
        runtime.DevicePlan(serialised_with(plan, edit))


# ---- the route ---------------------------------------------------------------------------------------------------- #

def test_route_is_pinned_at_both_sides_of_its_threshold():
    assert P.pick_route(512, 1 << 15) == "kred"
    assert P.pick_route(513, 1 << 15) == "pick"
    assert P.pick_route(512, (1 << 15) - 1) == "pick"
    assert P.pick_route(1, 1 << 17) == "kred" and P.pick_route(4, 1 << 17) == "kred"
    assert P.pick_route(1, 4096) == "pick" and P.pick_route(1 << 20, 1 << 17) == "pick"
    # whatever goes to the k-reduction route must be taken by it there (csrc/ctg_kernels_valu.hip: valu_route)
    assert P.PICK_KRED_MIN_K >= 256 and P.PICK_KRED_MAX_M <= 1 << 15


def test_route_constants_are_the_launchers():
    text = open(os.path.join(ROOT, "cotengra_amd", "csrc", "ctg_common.h")).read()
    m = re.search(r"kPickKredMinK\s*=\s*1\s*<<\s*(\d+)\s*,\s*kPickKredMaxM\s*=\s*(\d+)\s*;", text)
    assert m, "the launcher's rule has moved"
    assert (1 << int(m.group(1)), int(m.group(2))) == (P.PICK_KRED_MIN_K, P.PICK_KRED_MAX_M)
    assert "K >= kPickKredMinK && M <= kPickKredMaxM" in text


# ---- the pick contractor's lifetime ---------------------------------------------------------------------------------- #

def test_pick_contractor_is_closed_with_the_contractor_that_built_it():
    from cotengra_amd.contractor import _tree_contractor

    tree = tree_sliced()
    fn = _tree_contractor(tree)
    picks = lambda: [v for k, v in tree.contraction_cores.items() if isinstance(k, tuple) and k[0] == "hip-pick"]  # noqa: E731
    first = fn._pick_contractor(CT.pick_requests(tree, random_coords(tree, 5), None))
    assert picks() == [first] and fn._pick_contractor(first._pick) is first
    second = fn._pick_contractor(CT.pick_requests(tree, random_coords(tree, 6), None))
    assert picks() == [second] and second is not first   # (one at a time: the first was replaced and closed)
    fn.close()
    assert picks() == [] and fn._picker is None
    assert any(v is fn for v in tree.contraction_cores.values())   # (the ordinary contractor stays cached)
