"""What an executor returns for (inputs uploaded, arithmetic and options set, slices asked for) is THE SAME BITS as a
fresh executor of the same plan would return for them, whatever was uploaded, run or set on it before.

An executor carries state that one run writes and a later run reads: above all the record of the largest |component|
per step (``ctg_exec::smax_slot``) that producers raise with ``atomicMax`` and the fp16 x 2 kernels (``stem2h_kernel``,
``pair_mfma_h2_kernel``) split their operand under -- a record must be zero before its producer runs again --, and
``d_fac`` under ``strip_exponent``, the input scale, the wide sum, ``stem_h2_ran``, ``group_key``, a captured graph.
``HipContractor`` caches its executor, so every second call of the public API meets that state.

Every result is checked twice: (a) against a plain complex128 reference (the oracle, or numpy ``@`` for the GEMM
chains) under the suite's own gates -- ``G.single_gate`` for stems and trees, the norm-wise 2e-6 of the tiled chains --
and (b) bit for bit against a fresh ``HipContractor`` that only ever saw that input.  (a) is what fails if both
executors are wrong in the same way.

Every scale here is an exact power of two that leaves each input's largest |component| inside the upload window
[2^-32, 2^32) (``G.scaled_in_window`` asserts it): outside it the upload normalises the scale away and no kernel sees
it.  An INTERMEDIATE moves by 2^-40 ... 2^-60 through several inputs of 2^-15 ... 2^-30 each.

This module runs in the default arithmetic (it is not one of conftest's bf16 x 3 modules): that is the point."""
import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd.contractor import HipContractor
from cotengra_amd.plan import compile_tree
from oracle import contract_ref as orc

import exec_history_util as H
import golden_util as G

pytestmark = pytest.mark.gpu

CHAIN_GATE = 2e-6     # (test_chained_tiled_steps_take_the_producers_record: norm-wise)
ARITH = {0: "fp32", 1: "bf16x3", 2: "fp16x2"}


def _exec(fn):
    """The contractor's one cached executor, without another upload."""
    (st,) = fn._execs.values()
    return st["exec"]


def _whole(ex):
    ex.zero_result()
    ex.run_share(0, 1)
    return np.asarray(ex.download_result()).copy()


def _some(ex, ids):
    ex.zero_result()
    ex.run_slice_list(ids)
    return np.asarray(ex.download_result()).copy()


def _one(ex, i):
    ex.zero_result()
    ex.run_slices(i, 1, 1)
    return np.asarray(ex.download_result()).copy()


def _fresh(tree, xs, job, **kw):
    """``job(executor)`` on a new contractor that sees ``xs`` and nothing else."""
    fn = HipContractor(tree, **kw)
    try:
        return job(fn.setup(*xs)["exec"])
    finally:
        fn.close()


def _gate(tree, xs, ref):
    return G.single_gate(ref, orc.contract(tree, xs))


# ---------------------------------------------------------------------- #
# A. unsliced chain of tiled steps, one contractor, four uploads
# ---------------------------------------------------------------------- #


def test_unsliced_tiled_chain_four_uploads(monkeypatch):
    """Two pair_mfma_h2_kernel steps, the second one reading the first one's record; X, then a and b each x 2^-25 (the
    intermediate 2^-50 lower), then a and b each x 2^12, then X again -- through the public call."""
    H.default_arithmetic(monkeypatch)
    tree = G.chain_tree(*H.CHAIN)
    R, K, N, N2 = H.CHAIN
    rng = np.random.default_rng(5)
    a, b, c = G.cplx(rng, R, K), G.cplx(rng, K, N), G.cplx(rng, N, N2)
    G.assert_in_upload_window(c)
    uploads = [("X", 0), ("X_small", -25), ("X_big", 12), ("X again", 0)]
    fn = HipContractor(tree)
    outs = []
    for label, lg in uploads:
        xs = (G.scaled_in_window(a, lg), G.scaled_in_window(b, lg), c)
        got = np.asarray(fn(*xs)).copy()
        ex = _exec(fn)
        H.chain_plan_checks(ex.plan)
        names = ex.step_kernels()
        assert names[0].startswith("pair_mfma_h2_kernel") and names[1].startswith("pair_mfma_h2_kernel"), names
        ref = (xs[0].astype("complex128") @ xs[1].astype("complex128")) @ c.astype("complex128")
        err = G.relerr(got, ref)
        print(f"A {label}: relerr {err:.3e}")
        assert err <= CHAIN_GATE, (label, err)                                          # (a)
        f2 = HipContractor(tree)
        fresh = np.asarray(f2(*xs)).copy()
        f2.close()
        assert np.array_equal(got, fresh), label                                        # (b)
        outs.append(got)
    fn.close()
    assert np.array_equal(outs[0], outs[3])


# ---------------------------------------------------------------------- #
# B. unsliced stem, default rule
# ---------------------------------------------------------------------- #


STEM_B_LOG2 = {0: -20, 1: -13, 2: -13, 3: -14}
assert set(STEM_B_LOG2) == H.STEM_B_FIRST_LEAVES


def _stem_b_uploads(tree):
    arrays = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=10, dtype="complex64")
    for x in arrays:
        G.assert_in_upload_window(x)
    # (the state is normalised: its largest |component| is 2^-7, and x 2^-30 would leave the upload window -- it takes
    # 2^-20, the three gate tensors under the first, recording stem launch 2^-13, 2^-13 and 2^-14: 2^-60 in all)
    small = [G.scaled_in_window(x, STEM_B_LOG2.get(i, 0)) for i, x in enumerate(arrays)]
    return [("plain", arrays), ("small", small), ("plain again", arrays)]


def test_unsliced_stem_default_rule(monkeypatch):
    """The first pair of the stem runs bf16 x 3 and records, the later pairs run fp16 x 2 on their producer's record;
    no CTG_STEM_H2_ALL, so no max-abs pass hides a stale record.  Plain, then the first launch's result 2^-60 lower,
    then plain."""
    G.fuse_whatever_fits(monkeypatch, h2_all=False)
    tree = H.stem_b()
    fn = HipContractor(tree, **H.STEM_OPTS)
    for label, xs in _stem_b_uploads(tree):
        got = np.asarray(fn(*xs)).copy()
        ex = _exec(fn)
        stems = H.stem_b_plan_checks(ex.plan)
        names = ex.step_kernels()
        assert names[stems[0]].startswith("stem2_kernel<"), names            # bf16 x 3, records
        assert all(names[i].startswith("stem2h_kernel<") for i in stems[1:]), names
        ref = np.asarray(orc.contract(tree, H.wide(xs)))
        err, gate = G.relerr(got, ref), _gate(tree, xs, ref)
        print(f"B {label}: relerr {err:.3e} gate {gate:.1e}")
        assert err <= gate, (label, err, gate)                                            # (a)
        f2 = HipContractor(tree, **H.STEM_OPTS)
        fresh = np.asarray(f2(*xs)).copy()
        f2.close()
        assert np.array_equal(got, fresh), label                                          # (b)
    fn.close()


# ---------------------------------------------------------------------- #
# C. sliced tree, slice-invariant tiled producer
# ---------------------------------------------------------------------- #


def test_sliced_tree_invariant_tiled_producer(monkeypatch):
    """(a b)[slice-invariant] (s c d)[slice s]: both steps run pair_mfma_h2_kernel at the sizes of the issue (a = 16384,
    b = c = d = 256, four slices), the per-slice one reading the invariant one's record.  Plain, then a and b each
    x 2^-25, then plain: whole contractions and single slices."""
    H.default_arithmetic(monkeypatch)
    tree = H.sliced_chain()
    rng = np.random.default_rng(9)
    a, b, c = G.cplx(rng, 16384, 256), G.cplx(rng, 256, 256), G.cplx(rng, 4, 256, 256)
    G.assert_in_upload_window(c)
    jobs = [("whole", _whole)] + [(f"slice {i}", (lambda ex, i=i: _one(ex, i))) for i in range(4)]
    fn = HipContractor(tree)
    for label, lg in [("plain", 0), ("small", -25), ("plain again", 0)]:
        xs = (G.scaled_in_window(a, lg), G.scaled_in_window(b, lg), c)
        ab = xs[0].astype("complex128") @ xs[1].astype("complex128")
        per = [ab @ c[i].astype("complex128") for i in range(4)]
        refs = [sum(per)] + per
        ex = fn.setup(*xs)["exec"]
        H.sliced_chain_plan_checks(ex.plan)
        for (what, job), ref in zip(jobs, refs):
            got = job(ex)
            names = ex.step_kernels()
            assert names[0].startswith("pair_mfma_h2_kernel") and names[1].startswith("pair_mfma_h2_kernel"), names
            err = G.relerr(got, ref)
            print(f"C {label} {what}: relerr {err:.3e}")
            assert err <= CHAIN_GATE, (label, what, err)                                  # (a)
            assert np.array_equal(got, _fresh(tree, xs, job)), (label, what)              # (b)
    fn.close()


# ---------------------------------------------------------------------- #
# D. sliced stem: invariant stem -> group-shared stem -> per-slice stem
# ---------------------------------------------------------------------- #

D_SEED = 6            # (g3_5 and g3_6 stay open in this tree's output: every key writes its own chunk of the result)
D_KEY_LOG2 = {(0, 0): 0, (0, 1): -10, (1, 0): -20, (1, 1): -30}


@pytest.fixture
def stem_d(monkeypatch):
    G.fuse_whatever_fits(monkeypatch, h2_all=False)
    G.groups_everywhere(monkeypatch)
    tree = H.stem_d(D_SEED)
    assert all(ix in tree.output for ix in H.STEM_D_KEY)
    arrays = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=D_SEED, dtype="complex64")
    for x in arrays:
        G.assert_in_upload_window(x)
    return tree, arrays


def _stem_d_checks(ex):
    H.stem_d_plan_checks(ex.plan)
    names = ex.step_kernels()
    assert names[1].startswith(("stem2_kernel<", "stem2h_kernel<")), names     # the invariant producer records
    assert names[2].startswith("stem2h_kernel<") and names[3].startswith("stem2h_kernel<"), names


def test_sliced_stem_reupload(stem_d):
    """D1: plain, then the leaves under the slice-invariant stem step (the state and gates 0-2) x 2^-15 each -- its
    result 2^-60 lower --, then plain; whole contractions."""
    tree, arrays = stem_d
    small = [G.scaled_in_window(x, -15) if i in H.STEM_D_INVARIANT_LEAVES else x for i, x in enumerate(arrays)]
    fn = HipContractor(tree, **H.STEM_OPTS)
    for label, xs in [("plain", arrays), ("small", small), ("plain again", arrays)]:
        ex = fn.setup(*xs)["exec"]
        got = _whole(ex)
        _stem_d_checks(ex)
        ref = np.asarray(orc.contract(tree, H.wide(xs)))
        err, gate = G.relerr(got, ref), _gate(tree, xs, ref)
        print(f"D1 {label}: relerr {err:.3e} gate {gate:.1e}")
        assert err <= gate, (label, err, gate)                                            # (a)
        assert np.array_equal(got, _fresh(tree, xs, _whole, **H.STEM_OPTS)), label        # (b)
    fn.close()


def _groups_by_size(tree, plan):
    """Group numbers from the largest block of the gate-3 tensor to the smallest, with their slice ids."""
    out = []
    for g in range(plan.nslices // plan.group_size):
        ids = plan.group_ids(g)
        key = orc.slice_key(tree, ids[0])
        out.append((D_KEY_LOG2[(key["g3_5"], key["g3_6"])], g, ids))
    assert sorted(lg for lg, _, _ in out) == sorted(D_KEY_LOG2.values())
    return [(g, ids) for _, g, ids in sorted(out, reverse=True)]


def test_sliced_stem_group_order(stem_d):
    """D2: the blocks of the gate-3 tensor along the key indices scaled by 2^0, 2^-10, 2^-20, 2^-30 -- what a group
    shares differs by those powers from group to group.  Every group against the oracle's sum of its slices, the same
    bits on a fresh executor and whatever the visiting order; and all 16 slices in one call (the executor sorts them by
    key: the largest group runs first), every key's block of the result against the oracle's block."""
    tree, plain = stem_d
    xs = H.stem_d_key_blocks(tree, plain, D_KEY_LOG2)
    x128 = H.wide(xs)
    fn = HipContractor(tree, **H.STEM_OPTS)
    ex = fn.setup(*xs)["exec"]
    groups = _groups_by_size(tree, ex.plan)
    down = {}
    for g, ids in groups:                          # largest first: a stale record is too LARGE for the next group
        got = _some(ex, ids)
        _stem_d_checks(ex)
        ref = H.slices_ref(tree, x128, ids)
        err, gate = G.relerr(got, ref), G.single_gate(ref, H.slices_ref(tree, xs, ids))
        print(f"D2 group {g} after larger ones: relerr {err:.3e} gate {gate:.1e}")
        assert err <= gate, (g, err, gate)                                                # (a)
        assert np.array_equal(got, _fresh(tree, xs, lambda e: _some(e, ids), **H.STEM_OPTS)), g     # (b)
        down[g] = got
    for g, ids in groups[::-1]:                    # ... and the other way round
        assert np.array_equal(_some(ex, ids), down[g]), g
    # all slices in one call
    whole = _whole(ex)
    fn.close()
    ref = np.asarray(orc.contract(tree, x128))
    npy = np.asarray(orc.contract(tree, xs))
    ax = [tree.output.index(ix) for ix in H.STEM_D_KEY]
    for (v5, v6), lg in D_KEY_LOG2.items():
        sel = [slice(None)] * len(tree.output)
        sel[ax[0]], sel[ax[1]] = v5, v6
        sel = tuple(sel)
        err, gate = G.relerr(whole[sel], ref[sel]), G.single_gate(ref[sel], npy[sel])
        print(f"D2 one call, block 2^{lg}: relerr {err:.3e} gate {gate:.1e}")
        assert err <= gate, (lg, err, gate)                                               # (a) per block

    def one_call_each_smallest_first(e):
        e.zero_result()
        for _, ids in groups[::-1]:
            e.run_slice_list(ids)
        return np.asarray(e.download_result()).copy()

    assert np.array_equal(whole, _fresh(tree, xs, one_call_each_smallest_first, **H.STEM_OPTS))    # (b)


def test_sliced_stem_shares(stem_d):
    """D3: the shares of two ranks, each on a fresh executor, and one after the other on one executor: the same bits
    per share (a rank's share is whole groups; what ran before on the executor is another rank's)."""
    tree, plain = stem_d
    xs = H.stem_d_key_blocks(tree, plain, D_KEY_LOG2)
    x128 = H.wide(xs)

    def share(rank):
        def job(e):
            e.zero_result()
            e.run_share(rank, 2)
            return np.asarray(e.download_result()).copy()
        return job

    fn = HipContractor(tree, **H.STEM_OPTS)
    ex = fn.setup(*xs)["exec"]
    for rank in (0, 1):
        got = share(rank)(ex)
        _stem_d_checks(ex)
        assert np.array_equal(got, _fresh(tree, xs, share(rank), **H.STEM_OPTS)), rank     # (b)
        # (a), per group of the share: the groups of a share differ by up to 2^20
        for g in range(rank, ex.plan.nslices // ex.plan.group_size, 2):
            ids = ex.plan.group_ids(g)
            ref = H.slices_ref(tree, x128, ids)
            mask = ref != 0
            err, gate = G.relerr(got[mask], ref[mask]), G.single_gate(ref, H.slices_ref(tree, xs, ids))
            print(f"D3 rank {rank} group {g}: relerr {err:.3e} gate {gate:.1e}")
            assert err <= gate, (rank, g, err, gate)
    fn.close()


# ---------------------------------------------------------------------- #
# E. sweep: every small golden tree, two uploads (and the first one again)
# ---------------------------------------------------------------------- #

SWEEP_TREES = sorted(set(G.LDS_TREES) | set(G.GROUP_CASES))
SINGLE = {"complex64": "complex128", "float32": "float64"}
# A single-precision result must stay inside the float32 range: the scales of the second upload (every third leaf
# x 2^-20, the others x 2^5 -- 2^-10 per three leaves) go to the first 18 leaves there (2^-60 in all); trees of 64 and
# 200 leaves would otherwise put the value itself below 2^-200, where no float32 result can follow.  Double precision
# and strip_exponent (mantissa and exponent) take the scales on every leaf.
SINGLE_SCALED_LEAVES = 18


def _case(name):
    return next(c for c in G.cases("tree") if c["name"] == name)


def _sweep_uploads(case, tree, wide_dtype, scaled_leaves):
    plain = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=1, dtype=wide_dtype,
                                       rescale=case.get("rescale", False))
    scaled = [G.scaled_in_window(x, (-20 if i % 3 == 0 else 5)) if i < scaled_leaves else x for i, x in enumerate(plain)]
    return [("seed 1", plain), ("scaled", scaled), ("seed 1 again", plain)]


def _sweep_ids(tree):
    """What is run: the whole tree, or -- C5_hyper200 has 4e9 slices -- its first six."""
    return None if tree.nslices <= 256 else list(range(6))


def _strip_close(m, e, m_ref, e_ref, tol):
    """(mantissa, exponent) against the oracle's as test_raw_inputs_under_strip_exponent_at_sycamore_depth compares
    them -- log10 of the largest |element| plus the exponent, and the mantissa normalised by it -- element-wise norm for
    tensors."""
    m, m_ref = np.asarray(m).astype("complex128"), np.asarray(m_ref).astype("complex128")
    top, top_ref = np.abs(m).max(), np.abs(m_ref).max()
    assert top > 0 and top_ref > 0
    lg, lg_ref = np.log10(top) + e, np.log10(top_ref) + e_ref
    assert abs(lg - lg_ref) <= max(tol, 1e-12) / np.log(10.0) * 1.5 + 1e-12, (lg, lg_ref)
    assert np.abs(m / top - m_ref / top_ref).max() <= 1.5 * tol, (np.abs(m / top - m_ref / top_ref).max(), tol)


def _sweep_dtypes(mode):
    if mode == "default":
        return ["complex64", "float32", "complex128", "float64"]
    return ["complex64", "complex128"] if mode == "strip" else ["complex64"]


@pytest.mark.parametrize("mode", ["default", "strip", "graph", "groups"])
@pytest.mark.parametrize("name", SWEEP_TREES)
def test_sweep_golden_trees_two_uploads(name, mode, monkeypatch):
    """Every small golden tree (the LDS-resident-subtree trees and the slice-group trees): seed 1, the same arrays with
    every third leaf x 2^-20 and the others x 2^5, seed 1 again, on one contractor -- in every dtype, under
    strip_exponent, through a captured slice graph (CTG_GRAPH=1 CTG_SLICE_BATCH=1) and with slice groups forced on."""
    H.default_arithmetic(monkeypatch)
    case = _case(name)
    if mode == "graph":
        monkeypatch.setenv("CTG_GRAPH", "1")
        monkeypatch.setenv("CTG_SLICE_BATCH", "1")
    if mode == "groups":
        G.groups_everywhere(monkeypatch)
        tree = G.tree_of(case)
        if tree.multiplicity < 4:
            pytest.skip("fewer than four slices")
        if compile_tree(tree, "complex64").group_size < 2:
            pytest.skip("no step is independent of a sliced index")
    for dtype in _sweep_dtypes(mode):
        tree = G.tree_of(case)
        wide_dtype = SINGLE.get(dtype, dtype)
        single = dtype in SINGLE
        ids = _sweep_ids(tree)
        strip = mode == "strip"
        uploads = _sweep_uploads(case, tree, wide_dtype, SINGLE_SCALED_LEAVES if single and not strip else tree.N)

        def job(ex):
            ex.set_strip_exponent(strip, False)
            ex.zero_result()
            if ids is None:
                ex.run_share(0, 1)
            else:
                ex.run_slice_list(ids)
            out, e, _ = ex.get_state()
            return np.asarray(out).copy(), (e if strip else 0.0)

        fn = HipContractor(tree)
        for label, ws in uploads:
            xs = [a.astype(dtype) for a in ws]
            got, e = job(fn.setup(*xs)["exec"])
            if mode == "groups":
                assert fn.get_plan(dtype)[0].group_size >= 2
            what = (name, mode, dtype, label)
            if strip:
                stripped = ((lambda a: orc.contract(tree, a, strip_exponent=True)) if ids is None else
                            (lambda a: H.slices_ref_stripped(tree, a, ids)))
                m_ref, e_ref = stripped(ws)
                tol = 1e-10
                if single:
                    m_np, e_np = stripped(xs)
                    m_ref_ = np.asarray(m_ref).astype("complex128")
                    tol = max(1e-5, 8.0 * G.relerr(np.asarray(m_np).astype("complex128") * 10.0 ** (e_np - e_ref), m_ref_))
                _strip_close(got.reshape(np.shape(m_ref)), e, m_ref, e_ref, tol)          # (a)
            else:
                ref = np.asarray(orc.contract(tree, ws)) if ids is None else H.slices_ref(tree, ws, ids)
                tol = 1e-10
                if single:
                    tol = G.single_gate(ref, orc.contract(tree, xs) if ids is None else H.slices_ref(tree, xs, ids))
                err = G.relerr(got.reshape(np.shape(ref)), ref)
                assert err <= tol, (what, err, tol)                                       # (a)
            fresh, e_fresh = _fresh(tree, xs, job)
            assert np.array_equal(got, fresh) and e == e_fresh, what                      # (b)
        fn.close()


# ---------------------------------------------------------------------- #
# F. options changed mid-life
# ---------------------------------------------------------------------- #


@pytest.mark.parametrize("which", ["B", "D"])
def test_arithmetic_and_strip_exponent_changed_mid_life(which, monkeypatch):
    """set_stem_arithmetic 1, 2, 0, 2 on one executor, a run after each: the bits of a fresh executor created in that
    arithmetic.  The same for strip_exponent on -> off."""
    G.fuse_whatever_fits(monkeypatch, h2_all=False)
    if which == "B":
        tree = H.stem_b()
        xs = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=10, dtype="complex64")
    else:
        G.groups_everywhere(monkeypatch)
        tree = H.stem_d(D_SEED)
        plain = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=D_SEED, dtype="complex64")
        xs = H.stem_d_key_blocks(tree, plain, D_KEY_LOG2)
    ref = np.asarray(orc.contract(tree, H.wide(xs)))
    fn = HipContractor(tree, **H.STEM_OPTS)
    ex = fn.setup(*xs)["exec"]
    seen = {}
    for arith in (1, 2, 0, 2):
        ex.set_stem_arithmetic(arith)
        got = _whole(ex)
        fresh = _fresh(tree, xs, _whole, stem_bf16x3=ARITH[arith], **H.STEM_OPTS)
        assert np.array_equal(got, fresh), arith
        seen[arith] = got
    assert not np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[0], seen[2])   # (they are three arithmetics)
    if which == "B":
        assert G.relerr(seen[2], ref) <= _gate(tree, xs, ref)
    else:   # (the blocks of the result differ by up to 2^30: every key's block against the oracle's)
        npy = np.asarray(orc.contract(tree, xs))
        ax = [tree.output.index(ix) for ix in H.STEM_D_KEY]
        for v5, v6 in D_KEY_LOG2:
            sel = [slice(None)] * len(tree.output)
            sel[ax[0]], sel[ax[1]] = v5, v6
            sel = tuple(sel)
            assert G.relerr(seen[2][sel], ref[sel]) <= G.single_gate(ref[sel], npy[sel]), (v5, v6)

    def stripped(e):
        e.set_strip_exponent(True, False)
        e.zero_result()
        e.run_share(0, 1)
        out, exp, _ = e.get_state()
        return np.asarray(out).copy(), exp

    m, e10 = stripped(ex)
    m_f, e_f = _fresh(tree, xs, stripped, **H.STEM_OPTS)
    assert np.array_equal(m, m_f) and e10 == e_f
    ex.set_strip_exponent(False, False)
    assert np.array_equal(_whole(ex), seen[2])
    fn.close()
