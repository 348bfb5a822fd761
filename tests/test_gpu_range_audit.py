"""GPU suite: the range audit (csrc/ctg_range.hip, ctg_exec_range_audit, cotengra_amd/rangeaudit.py, DESIGN.md section
11) -- exponent histogram, zero count and sum of squares of every tensor of a slice, and the opt-in arithmetic choice
``HipContractor(stem_bf16x3="auto", crest_limit=L)`` built on it.

The reference is numpy on the very bytes the device holds (tests/range_util.py): counts must be EQUAL, the sum of
squares within ``n 2^-53 sumsq`` (two summation orders; derived there).  kRangeChunk = 16384 components is the pass's
unit: a tensor below it takes the tail path alone, one above it the register path and the tail, and one above
2048 chunks gives a workgroup several chunks."""
import os

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import plan as P
from cotengra_amd import rangeaudit as RA
from cotengra_amd.contractor import HipContractor
from oracle import contract_ref as orc

import golden_util as G
import range_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384        # kRangeChunk of csrc/ctg_range.hip
MAX_BLOCKS = 2048    # kRangeMaxBlocks
SIZES = [1, 3, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17]
ARITHS = ["fp32", "bf16x3", "fp16x2"]


@pytest.fixture
def any_arith(monkeypatch):
    G.fuse_whatever_fits(monkeypatch, h2_all=True)


def _column_tree(R):
    """a[R, 1] . b[1, 1]: one pair step whose result is a copy of ``a`` times ``b``."""
    return ca.ContractionTree.from_path([("r", "k"), ("k", "n")], ("r", "n"), dict(r=R, k=1, n=1), path=[(0, 1)])


def _pool(kind):
    """``full``: 2^k for k = -149 ... 127, +-0, inf, NaN, both signs.  ``window``: the finite part whose largest
    member stays inside the upload window -- the kernels see these very values."""
    top = 127 if kind == "full" else 31
    mags = [np.float32(2.0) ** np.float32(k) if k > -127 else np.float32(np.ldexp(1.0, k)) for k in range(-149, top + 1)]
    vals = []
    for i, m in enumerate(mags):
        vals += [m, -m] if i % 3 == 0 else [m if i % 2 else -m]
    vals += [np.float32(0.0), np.float32(-0.0)]
    if kind == "full":
        vals += [np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)]
    return np.asarray(vals, dtype=np.float32)


def _column(R, dtype, kind, seed):
    rng = np.random.default_rng(seed)
    pool = _pool(kind)
    n = R * (2 if dtype == "complex64" else 1)
    # (every member of the pool where there is room, then random ones)
    f = np.concatenate([pool, rng.choice(pool, size=max(n - pool.size, 0))])[:n] if n >= pool.size else rng.choice(pool, size=n)
    f = rng.permutation(f).astype(np.float32)
    a = f.view(np.complex64) if dtype == "complex64" else f
    return a.reshape(R, 1)


def _audit_column(a, dtype):
    R = a.shape[0]
    fn = HipContractor(_column_tree(R))
    try:
        st = fn.setup(a, np.ones((1, 1), dtype=dtype))
        ex, plan = st["exec"], st["plan"]
        ex.zero_result()
        rows, sumsq = ex.range_audit(0)
        (s,) = [i for i, t in enumerate(plan.steps) if t.kind == P.KIND_PAIR]
        c = plan.steps[s].c
        assert c.space == P.SPACE_ARENA
        stored = np.asarray(ex.download_arena(c.offset, c.size)).copy()
        n_in = len(plan.input_sizes)
        assert rows.shape == (n_in + len(plan.steps), 260) and sumsq.shape == (n_in + len(plan.steps),)
        return rows, sumsq, n_in, s, stored, plan
    finally:
        fn.close()


@pytest.mark.parametrize("kind", ["full", "window"])
@pytest.mark.parametrize("dtype", ["float32", "complex64"])
@pytest.mark.parametrize("R", SIZES)
def test_exact_counts_on_the_stored_bytes(R, dtype, kind):
    a = _column(R, dtype, kind, seed=R)
    rows, sumsq, n_in, s, stored, plan = _audit_column(a, dtype)
    assert stored.size == R
    U.check_row(rows[n_in + s], sumsq[n_in + s], stored)
    # the accumulate step is not materialised in the arena; b = 1 is a leaf of one element
    acc = [i for i, t in enumerate(plan.steps) if t.kind == P.KIND_ACCUM]
    assert acc and all(not rows[n_in + i].any() and sumsq[n_in + i] == 0.0 for i in acc)
    U.check_row(rows[1], sumsq[1], np.ones(1, dtype=dtype))
    if kind == "window" and 2.0 ** -32 <= np.abs(U.components(a)).max() < 2.0 ** 32:
        # the upload leaves this input alone (its largest member lies inside the window: every size but the
        # smallest ones) and b = 1: the stored bytes hold the pool (not a tensor of NaN)
        U.check_row(rows[0], sumsq[0], a)
        assert np.count_nonzero(rows[n_in + s][4:]) >= min(20, R // 4)


def test_a_workgroup_takes_several_chunks():
    """More chunks than workgroups (2048): a workgroup adds several chunks into one row, 32-bit counts per workgroup,
    64-bit ones in the sum; no multiple of the chunk, so the tail path runs in the last workgroup's turn."""
    R = MAX_BLOCKS * CHUNK + 3 * CHUNK + 5
    rng = np.random.default_rng(5)
    a = rng.standard_normal(R, dtype=np.float32).reshape(R, 1)
    a[::1000] = 0.0
    rows, sumsq, n_in, s, stored, _ = _audit_column(a, "float32")
    U.check_row(rows[n_in + s], sumsq[n_in + s], stored)
    # the leaf holds the same bytes (b = 1, nothing rescaled) at another address: the same 258 numbers, bit for bit
    assert np.array_equal(stored, a.reshape(-1))
    assert np.array_equal(rows[0], rows[n_in + s]) and sumsq[:1].view(np.uint64)[0] == sumsq[n_in + s:n_in + s + 1].view(np.uint64)[0]


@pytest.mark.parametrize("dtype", ["float32", "complex64"])
@pytest.mark.parametrize("values", [(1.5,), (1.5, -3.0)])
def test_hot_bins(values, dtype):
    """Every component in one bin (or two): the full count, whichever path counted it (float32: 12305 components,
    the tail path; complex64: 24610, one chunk in registers and a tail)."""
    R = 3 * 4096 + 17
    n = R * (2 if dtype == "complex64" else 1)
    f = np.resize(np.asarray(values, dtype=np.float32), n)
    a = (f.view(np.complex64) if dtype == "complex64" else f).reshape(R, 1)
    rows, sumsq, n_in, s, stored, _ = _audit_column(a, dtype)
    row = rows[n_in + s]
    assert np.array_equal(components_of(stored), f)
    U.check_row(row, sumsq[n_in + s], stored)
    if len(values) == 1:
        assert row[4 + 127] == n and np.count_nonzero(row[4:]) == 1
    else:
        assert row[4 + 127] == (n + 1) // 2 and row[4 + 128] == n // 2 and np.count_nonzero(row[4:]) == 2
    assert row[2] == 0 and sumsq[n_in + s] == float(np.sum(f.astype(np.float64) ** 2))


def components_of(x):
    return U.components(x)


# ---------------------------------------------------------------------- #
# every step of a multi-step tree
# ---------------------------------------------------------------------- #


def _stem_tree(case, sliced=0):
    nq, gates = G.STEM_CASES[case]
    return G.stem_network(nq, gates, 100 * case, sliced=sliced)


_TREES = {"stem0": lambda: _stem_tree(0), "chain": lambda: G.chain_tree(8192, 64, 64, 64)}
_NODE_CACHE = {}


def _exact_case(name):
    """(tree, inputs in {0, +-1/2, +-1, +-2}, every node's reference row) -- computed once, never modified."""
    if name not in _NODE_CACHE:
        tree = _TREES[name]()
        xs = U.small_exact_arrays(tree, seed=3)
        nodes = U.node_tensors(tree, xs)
        for v in nodes.values():   # exact in fp32: the float64 einsum holds fp32 values
            assert np.array_equal(v.astype("complex64").astype("complex128"), v)
        _NODE_CACHE[name] = (tree, xs, {k: U.reference_row(v.astype("complex64")) for k, v in nodes.items()})
    return _NODE_CACHE[name]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", sorted(_TREES))
def test_every_step_of_a_tree(name, arith, any_arith):
    tree, xs, ref = _exact_case(name)
    fn = HipContractor(tree, fuse=True, fuse_min_elems=1 << 10, stem_bf16x3=arith)
    try:
        st = fn.setup(*xs)
        ex, plan = st["exec"], st["plan"]
        names = ex.step_kernels()
        ex.zero_result()
        rows, sumsq = ex.range_audit(0)
        got = np.asarray(ex.download_result()).copy()
        recs = fn.audit(*xs)
    finally:
        fn.close()
    n_in = len(plan.input_sizes)
    leaves = list(tree.gen_leaves())
    for i, leaf in enumerate(leaves):
        U.check_row(rows[i], sumsq[i], xs[i])
    audited = 0
    for s, step in enumerate(plan.steps):
        row = rows[n_in + s]
        if step.kind == P.KIND_ACCUM:
            assert row[0] == 0
            continue
        assert row[0] == 1, (s, names[s])
        audited += 1
        want, want_sq = ref[step.node]
        assert row[1] == want[1] and row[2] == want[2], (s, names[s], row[:4], want[:4])
        shift = U.shifted_equal(row[4:], want[4:])
        assert shift is not None, (s, names[s])
        assert abs(sumsq[n_in + s] - want_sq * 4.0 ** shift) <= U.sumsq_tol(want[1], want_sq * 4.0 ** shift)
    fused = [s for s, step in enumerate(plan.steps) if step.kind == P.KIND_STEM2]
    if name == "stem0":
        assert fused and all(rows[n_in + s][0] == 1 for s in fused)
        assert any(n.startswith("stem2h_kernel") for n in names) == (arith == "fp16x2")
    assert audited >= 2
    # the slice went into the result as a run would have put it there, and the values are exact
    assert np.array_equal(got, np.asarray(orc.contract(tree, [x.astype("complex128") for x in xs])).astype("complex64"))
    kap = [r["kappa"] for r in recs if r["kappa"] is not None]
    assert len(kap) == audited and all(k >= 1 - 1e-6 for k in kap), kap
    for r in recs:
        want = ("a", "b", "b2") if r["kernel"].startswith("stem2h_kernel") else \
            ("a", "b") if r["kernel"].startswith("pair_mfma_h2_kernel") else ()
        assert r["scaled"] == tuple(k for k in want if k in r["operands"])


def test_leaf_rows_of_gaussian_inputs(any_arith):
    tree = _stem_tree(0, sliced=2)
    xs = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=0, dtype="complex64")
    for x in xs:
        G.assert_in_upload_window(x)
    fn = HipContractor(tree, fuse=True, fuse_min_elems=1 << 10)
    try:
        ex = fn.setup(*xs)["exec"]
        ex.zero_result()
        rows, sumsq = ex.range_audit(tree.nslices - 1)
    finally:
        fn.close()
    for i, x in enumerate(xs):
        U.check_row(rows[i], sumsq[i], x)


def _sycamore_m10():
    tree = ca.tree_from_record(ca.load_network(os.path.join(ROOT, "tests/golden/trees/sycamore_m10.json")))
    z = np.load(os.path.join(ROOT, "tests/golden/sycamore_m10_arrays.npz"))
    return tree, [z[f"t{i}"].astype("complex64") for i in range(tree.N)]


def test_lds_subtrees_are_not_audited(monkeypatch):
    for k in G.ARITH_ENV:
        monkeypatch.delenv(k, raising=False)
    tree, xs = _sycamore_m10()
    fn = HipContractor(tree)
    try:
        st = fn.setup(*xs)
        ex, plan = st["exec"], st["plan"]
        names = ex.step_kernels()
        ex.zero_result()
        rows, sumsq = ex.range_audit(0)
        recs = fn.audit(*xs, slices=(0, tree.nslices - 1))
    finally:
        fn.close()
    n_in = len(plan.input_sizes)
    members = [s for s, n in enumerate(names) if n.startswith("lds_run_kernel") and not plan.steps[s].invariant]
    assert plan.lds_runs and members
    assert all(not rows[n_in + s].any() for s in members)
    live = [t for t in range(rows.shape[0]) if rows[t][0] == 1]
    assert len(live) > n_in
    for t in live:
        assert rows[t][4:].sum() == rows[t][1] and rows[t][3] == 0 and 0 <= rows[t][2] <= rows[t][4]
    for t in range(rows.shape[0]):
        if rows[t][0] == 0:
            assert not rows[t].any() and sumsq[t] == 0.0
    kap = [r["kappa"] for r in recs if r["kappa"] is not None]
    assert kap and all(k >= 1 - 1e-6 for k in kap), min(kap)
    assert all(r["c"] is None for r in recs if r["step"] in members)


# ---------------------------------------------------------------------- #
# executor history
# ---------------------------------------------------------------------- #


def test_executor_history(any_arith):
    tree = _stem_tree(0, sliced=2)
    xs = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=0, dtype="complex64")
    kw = dict(fuse=True, fuse_min_elems=1 << 10, stem_bf16x3="fp16x2")
    fn, fresh = HipContractor(tree, **kw), HipContractor(tree, **kw)
    try:
        ex = fn.setup(*xs)["exec"]
        assert any(n.startswith("stem2h_kernel") for n in ex.step_kernels())
        ex.zero_result()
        r1, q1 = ex.range_audit(1)
        by_audit = np.asarray(ex.download_result()).copy()
        ex.zero_result()
        r2, q2 = ex.range_audit(1)
        assert np.array_equal(r1, r2) and np.array_equal(q1.view(np.uint64), q2.view(np.uint64))
        fx = fresh.setup(*xs)["exec"]
        fx.zero_result()
        fx.run_slices(1, 1, 1)
        by_run = np.asarray(fx.download_result()).copy()
        assert np.array_equal(by_audit.view(np.uint32), by_run.view(np.uint32))
        # another slice's audit, then the whole contraction: what a fresh contractor returns
        fn.audit(*xs, slices=(2, 0))
        assert not np.asarray(fn.setup(*xs)["exec"].download_result()).any()   # the audit leaves the result zeroed
        after = np.asarray(fn(*xs)).copy()
        plain = np.asarray(fresh(*xs)).copy()
        assert np.array_equal(after.view(np.uint32), plain.view(np.uint32))
        # and an audit on the executor that has just run everything gives the first audit's numbers
        ex.zero_result()
        r3, q3 = ex.range_audit(1)
        assert np.array_equal(r1, r3) and np.array_equal(q1.view(np.uint64), q3.view(np.uint64))
    finally:
        fn.close()
        fresh.close()
    ref = np.asarray(orc.contract(tree, [x.astype("complex128") for x in xs]))
    assert G.relerr(plain, ref) <= G.single_gate(ref, orc.contract(tree, xs))


def test_errors():
    tree = _stem_tree(0, sliced=1)
    xs = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=0, dtype="complex64")
    fn = HipContractor(tree)
    try:
        ex = fn.setup(*xs)["exec"]
        for bad in (-1, tree.nslices):
            with pytest.raises(ValueError):
                ex.range_audit(bad)
        ex.set_strip_exponent(True, False)
        with pytest.raises(ValueError):
            ex.range_audit(0)
        ex.set_strip_exponent(False, False)
        ex.zero_result()
        rows, _ = ex.range_audit(0)
        assert rows[0][0] == 1
        ex128 = fn.setup(*[x.astype("complex128") for x in xs])["exec"]
        with pytest.raises(ValueError):
            ex128.range_audit(0)
    finally:
        fn.close()


# ---------------------------------------------------------------------- #
# the opt-in choice of arithmetic
# ---------------------------------------------------------------------- #

CREST_LIMIT = 32.0   # L: see _auto_data


def _auto_data():
    """Stem case 10.  G: Gaussian inputs.  O: G with one element of the big state x 2^12.  From numpy alone: every
    tensor of G has crest_up <= L / 2, and some tensor that a fused pair takes as an operand has crest_up >= 2 L in
    O (measured on the CPU when the test was written: 11.2 at most in G; 446, 101 and 39 for the three big operands
    of O) -- so the device's own rounding cannot move either data set across L."""
    nq, gates = G.STEM_CASES[10]
    tree = G.stem_network(nq, gates, 1000)
    g = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=10, dtype="complex64")
    o = [a.copy() for a in g]
    o[0].reshape(-1)[12345] *= np.float32(2.0 ** 12)
    return tree, g, o


def _crests(tree, xs, plan):
    nodes = U.node_tensors(tree, xs)
    leaves = list(tree.gen_leaves())
    n_in = len(leaves)
    crest = {i: RA.summarise(*U.reference_row(nodes[l].astype("complex64"))).crest_up for i, l in enumerate(leaves)}
    for s, step in enumerate(plan.steps):
        if step.kind in (P.KIND_PAIR, P.KIND_STEM2):
            crest[n_in + s] = RA.summarise(*U.reference_row(nodes[step.node].astype("complex64"))).crest_up
    joins = RA.join_operands(plan)
    scaled = {joins[s][k] for s, step in enumerate(plan.steps) if step.kind == P.KIND_STEM2
              for k in ("a", "b", "b2") if joins[s][k] is not None}
    return crest, scaled


def test_auto_arithmetic(any_arith, monkeypatch):
    tree, g, o = _auto_data()
    kw = dict(fuse=True, fuse_min_elems=1 << 10)
    auto = HipContractor(tree, stem_bf16x3="auto", crest_limit=CREST_LIMIT, **kw)
    h2 = HipContractor(tree, stem_bf16x3="fp16x2", **kw)
    b3 = HipContractor(tree, stem_bf16x3="bf16x3", **kw)
    try:
        plan = auto.host_plan("complex64")
        crest_g, scaled = _crests(tree, g, plan)
        crest_o, _ = _crests(tree, o, plan)
        assert scaled and max(crest_g.values()) <= CREST_LIMIT / 2, max(crest_g.values())
        assert max(crest_o[t] for t in scaled) >= 2 * CREST_LIMIT

        got = np.asarray(auto(*g)).copy()
        assert auto.arithmetic_chosen == "fp16x2"
        names = auto.setup(*g)["exec"].step_kernels()
        assert any(n.startswith("stem2h_kernel") for n in names)
        assert len(auto.last_audit) == len(plan.steps)
        seen = max(r[k].crest_up for r in auto.last_audit for k in r["operands"] if r[k] is not None)
        assert seen <= CREST_LIMIT
        assert np.array_equal(got.view(np.uint32), np.asarray(h2(*g)).view(np.uint32))

        got = np.asarray(auto(*o)).copy()
        assert auto.arithmetic_chosen == "bf16x3"
        names = auto.setup(*o)["exec"].step_kernels()
        assert not any(n.startswith("stem2h_kernel") for n in names)
        assert np.array_equal(got.view(np.uint32), np.asarray(b3(*o)).view(np.uint32))

        # and back: the choice is made per call
        got = np.asarray(auto(*g)).copy()
        assert auto.arithmetic_chosen == "fp16x2"
        assert np.array_equal(got.view(np.uint32), np.asarray(h2(*g)).view(np.uint32))
    finally:
        for fn in (auto, h2, b3):
            fn.close()
    monkeypatch.setenv("CTG_STEM_ARITH", "fp32")
    env = HipContractor(tree, stem_bf16x3="auto", crest_limit=CREST_LIMIT, **kw)
    f32 = HipContractor(tree, stem_bf16x3="fp32", **kw)
    try:
        got = np.asarray(env(*o)).copy()
        assert env.arithmetic_chosen == "environment" and env.last_audit is None
        assert np.array_equal(got.view(np.uint32), np.asarray(f32(*o)).view(np.uint32))
    finally:
        env.close()
        f32.close()
