"""Shared loader for the committed golden fixtures (tests/golden/)."""
import json
import os

import numpy as np

import cotengra_amd as ca

HERE = os.path.dirname(os.path.abspath(__file__))
_CASES = None
_EXPECTED = None


def load():
    global _CASES, _EXPECTED
    if _CASES is None:
        with open(os.path.join(HERE, "golden", "golden_cases.json"), encoding="utf-8") as f:
            _CASES = json.load(f)["cases"]
        _EXPECTED = np.load(os.path.join(HERE, "golden", "golden_expected.npz"))
    return _CASES, _EXPECTED


_R2 = None


def load_r2():
    """Round-2 fixtures (tests/golden/gen/make_golden_r2.py): projected output
    indices."""
    global _R2
    if _R2 is None:
        with open(os.path.join(HERE, "golden", "golden_r2_cases.json"), encoding="utf-8") as f:
            cs = json.load(f)["cases"]
        _R2 = (cs, np.load(os.path.join(HERE, "golden", "golden_r2_expected.npz")))
    return _R2


def cases(kind=None):
    cs, _ = load()
    return [c for c in cs if kind is None or c["kind"] == kind]


def expected(key):
    _, ex = load()
    return ex[key]


def tree_of(case):
    inputs = [tuple(t) for t in case["inputs"]]
    output = tuple(case["output"])
    if len(inputs) > 1:
        tree = ca.ContractionTree.from_path(inputs, output, case["size_dict"], path=case["path"])
    else:
        tree = ca.ContractionTree(inputs, output, case["size_dict"])
    for ind, project in case["sliced"]:
        tree.remove_ind_(ind, project=project)
    return tree


def arrays_of(case, dtype, tree=None):
    inputs = [tuple(t) for t in case["inputs"]] if tree is None else tree.inputs
    return ca.make_arrays_from_inputs(
        inputs, case["size_dict"], seed=case["seed"], dtype=dtype, rescale=case.get("rescale", False)
    )


def eq_tree_and_arrays(case, dtype):
    inputs, output = ca.eq_to_inputs_output(case["eq"])
    tree = ca.array_contract_tree(inputs, output, case["size_dict"],
                                  optimize=case["path"] if len(inputs) > 1 else "greedy")
    arrays = ca.make_arrays_from_inputs(inputs, case["size_dict"], seed=case["seed"], dtype=dtype)
    return tree, arrays


def relerr(x, ref):
    x, ref = np.asarray(x), np.asarray(ref)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    scale = max(float(np.abs(ref).max()) if ref.size else 0.0, 1e-300)
    return float(np.abs(x - ref).max() / scale) if ref.size else 0.0


NORTH_STAR = 1e-5


def single_gate(ref, numpy_single):
    """Tolerance (relative to max|ref|) of a single-precision device result:
    the north-star 1e-5, or -- where numpy itself, running the same contraction
    in the same single precision, is further than 1.25e-6 from the double
    precision reference -- eight times numpy's own error.  One rule for every
    single-precision comparison in the GPU suite (tree level since round 2,
    kernel-shape tests since round 3)."""
    if numpy_single is None:
        return NORTH_STAR
    return max(NORTH_STAR, 8.0 * relerr(np.asarray(numpy_single), ref))


def stem_flags(name):
    """Template arguments of a ``stem2_kernel<...>`` instantiation as the executor spells them
    (csrc/ctg_stem.hip: stem2_kernel_name): chunks and items known at compile time (0: the
    run-time-count variant), B2 in registers, bf16 x 3 products, row-interleaved step 2, single step,
    and -- three-step tiles only -- the middle stage's items per wave and whether it has 16 columns."""
    a = [x.strip() for x in name[name.index("<") + 1 : name.rindex(">")].split(",")]
    t = [x == "true" for x in a]
    return {"pack1": t[0], "pack2": t[1], "rt1": int(a[2]), "cs1": int(a[3]), "nch": int(a[4]), "it2": int(a[5]),
            "br1": t[6], "k2q": int(a[7]), "vec": t[8], "bf3": t[9], "ri2": t[10], "one": t[11],
            "itm": int(a[12]) if len(a) > 12 else 0, "packm": t[13] if len(t) > 13 else False,
            # round 5: two-accumulator real parts / the intermediate as bf16 limbs
            "xm": t[14] if len(t) > 14 else False, "lm": t[15] if len(t) > 15 else False,
            "ws": t[16] if len(t) > 16 else False}   # (specialised waves)


def pair_flags(name):
    """What the executor says of a pair step in float32, float64 or complex128, or of a step of any type that does
    not run on the matrix cores (include/ctg_hip.h: ctg_exec_step_kernel; complex64 on the matrix-core route:
    pair_flags_c64): ``kernel``, the name without template
    arguments, and -- matrix-core kernels -- ``dtype`` ("float", "double" or "c128"), the MFMA tiles per wave
    ``tm``, ``tn`` and ``vec``, the 16-byte gathers (None in complex128); -- long contractions -- ``no``, the
    outputs a wave computes together (0: pair_kred_kernel, a wave per output), and ``finish_wave``, whether a
    wavefront per output adds the partial sums."""
    parts = [x.strip() for x in name.split(" + ")]

    def args(s):
        return [x.strip() for x in s[s.index("<") + 1 : s.rindex(">")].split(",")] if "<" in s else []

    head = parts[0]
    out = {"kernel": head.split("<")[0], "dtype": None, "tm": 0, "tn": 0, "vec": None, "no": 0, "finish_wave": None}
    a = args(head)
    if out["kernel"] == "pair_mfma_c128_kernel":
        out.update(dtype="c128", tm=int(a[0]), tn=int(a[1]))
    elif out["kernel"] == "pair_mfma_real_kernel":
        assert a[0] in ("float", "double") and a[3] in ("true", "false"), name
        out.update(dtype=a[0], tm=int(a[1]), tn=int(a[2]), vec=a[3] == "true")
    elif out["kernel"] == "pair_kred_multi_kernel":
        out["no"] = int(a[0])
    else:
        assert out["kernel"] in ("pair_valu_kernel", "pair_kred_kernel") and not a, name
    if out["kernel"].startswith("pair_kred"):
        assert len(parts) == 2 and parts[1].startswith("pair_kred_finish_kernel<"), name
        (w,) = args(parts[1])
        assert w in ("true", "false"), name
        out["finish_wave"] = w == "true"
    else:
        assert len(parts) == 1, name
    return out


C64_TILED = ("pair_mfma_c64_kernel", "pair_mfma_fast_kernel", "pair_mfma_bf3_kernel", "pair_mfma_h2_kernel")
C64_KERNELS = C64_TILED + ("pair_mfma_stream_kernel", "pair_mfma_kstream_kernel", "pair_skinny_kernel", "pair_rowwise_kernel")


def pair_flags_c64(name):
    """What the executor says of a complex64 pair step on the matrix-core route (include/ctg_hip.h:
    ctg_exec_step_kernel): ``kernel``, the name without template arguments; ``args``, its template arguments as a tuple
    of ints and bools -- (FN, VEC, ADD, SHORTK, NV) streaming, (FN, VEC) k-streaming, (K, N) skinny, (NN, TS) row-wise,
    (128, BN, 16) tiled --; ``vec``, the 16-byte gathers of a tiled kernel (written behind its tile, None elsewhere);
    ``splits``, the slabs of partial sums that splitk_reduce_kernel adds per output (1: no such pass)."""
    parts = [x.strip() for x in name.split(" + ")]
    head = parts[0]
    kernel = head.split("<")[0]
    assert kernel in C64_KERNELS and "<" in head, name
    inner, tail = head[head.index("<") + 1 : head.rindex(">")], head[head.rindex(">") + 1 :]
    conv = {"true": True, "false": False}
    args = tuple(conv[x.strip()] if x.strip() in conv else int(x) for x in inner.split(","))
    out = {"kernel": kernel, "args": args, "vec": None, "splits": 1}
    if kernel in C64_TILED:
        assert tail in (",true", ",false") and len(args) == 3, name
        out["vec"] = tail == ",true"
    else:
        assert tail == "", name
        assert len(args) == (5 if kernel == "pair_mfma_stream_kernel" else 2), name
    if len(parts) == 2:
        assert kernel in C64_TILED[:3] + ("pair_mfma_kstream_kernel",), name
        assert parts[1].startswith("splitk_reduce_kernel[") and parts[1].endswith("]"), name
        out["splits"] = int(parts[1][len("splitk_reduce_kernel[") : -1])
        assert out["splits"] > 1, name
    else:
        assert len(parts) == 1 and kernel != "pair_mfma_kstream_kernel", name
    return out


def lds_form(name):
    """What the executor says of one shadow record of an LDS-resident subtree (include/ctg_hip.h: ctg_exec_lds_form,
    ``Executor.lds_forms()``): ``kernel``, "load", "pair" or "pair_mfma"; ``arg``, "gather" | "sum", the columns per
    lane 1 | 2 | 4, or "cols" | "rows"; ``wave``, the wave the record is dealt to or -1 when the workgroup shares it;
    ``rot``, the start rotation of a shared matrix-core record (None elsewhere); ``magic``, whether rows are divided by
    the multiply-high (False: a shift)."""
    parts = name.split(" ")
    head, div = parts[0], parts[-1]
    kernel, arg = head[:-1].split("<")
    assert head.endswith(">") and div in ("shift", "magic"), name
    assert (kernel, arg) in [("load", "gather"), ("load", "sum"), ("pair", "1"), ("pair", "2"), ("pair", "4"),
                             ("pair_mfma", "cols"), ("pair_mfma", "rows")], name
    out = {"kernel": kernel, "arg": int(arg) if kernel == "pair" else arg, "wave": -1, "rot": None, "magic": div == "magic"}
    deal = parts[1:-1]
    if deal[0] == "all":
        if kernel == "pair_mfma":
            assert len(deal) == 2 and deal[1].startswith("rot="), name
            out["rot"] = int(deal[1][4:])
            assert 0 <= out["rot"] < 16, name
        else:
            assert len(deal) == 1, name
    else:
        assert len(deal) == 1 and deal[0].startswith("wave="), name
        out["wave"] = int(deal[0][5:])
        assert 0 <= out["wave"] < 16, name
    return out


def stem_network(nq, gates, seed, sliced=0):
    """A small 'stem': one tensor of ``nq`` binary indices to which tensors are
    applied one after the other, gate ``(k, n)`` contracting ``k`` randomly chosen
    indices of the running tensor and adding ``n`` fresh ones (the structure of a
    sliced Sycamore contraction).  Returns ``(tree, inputs)``
    with the tree contracting the chain in order and ``sliced`` of the first
    tensor's indices sliced."""
    rng = np.random.default_rng(seed)
    cur = [f"a{i}" for i in range(nq)]
    inputs = [tuple(cur)]
    for g, (kin, nout) in enumerate(gates):
        sel = sorted(int(i) for i in rng.choice(len(cur), size=kin, replace=False))
        new = [f"g{g}_{j}" for j in range(nout)]
        inputs.append(tuple(cur[i] for i in rng.permutation(sel)) + tuple(new))
        cur = [c for i, c in enumerate(cur) if i not in sel] + new
    # the open indices in a scrambled order: the root's layout is the caller's
    output = tuple(cur[i] for i in rng.permutation(len(cur)))
    size_dict = {ix: 2 for t in inputs for ix in t}
    ssa, cur_id, nxt = [], 0, len(inputs)
    for i in range(1, len(inputs)):
        ssa.append((cur_id, i))
        cur_id, nxt = nxt, nxt + 1
    tree = ca.ContractionTree.from_path(inputs, output, size_dict, ssa_path=ssa)
    for ix in inputs[0][:sliced]:
        tree.remove_ind_(ix)
    return tree


# (nq, gates): single stem steps -- a large step no pair takes runs on the stem kernel's first half
ONE_CASES = [
    (17, [(3, 3), (5, 5)]),                       # k32 n32
    (17, [(3, 3), (7, 5)]),                       # k128 n32
    (17, [(3, 3), (6, 6)]),                       # k64 n64: two waves per row tile
    (18, [(3, 3), (7, 7)]),                       # k128 n128: four waves per row tile
    (17, [(3, 3), (4, 5)]),                       # k16 n32: 512-row tiles
    (17, [(3, 3), (5, 6)]),                       # k32 n64
    (17, [(3, 3), (5, 5), (6, 6), (5, 5)]),       # a chain of odd length: a pair and a step left over
]


def random_stem(seed):
    """A random stem for the fused-pair tests: 3 to 6 gates of 4 to 7 contracted and 4 to 7 new
    indices on a tensor of 15 to 18 binary indices, up to two indices sliced."""
    rng = np.random.default_rng(1000 + seed)
    nq = int(rng.integers(15, 19))
    gates, cur = [(3, 3)], nq
    for _ in range(int(rng.integers(3, 7))):
        kin = int(rng.integers(4, 8))
        nout = int(np.clip(kin + rng.integers(-2, 3), 4, 7))
        if kin > cur - 6 or cur - kin + nout > 19:
            continue
        gates.append((kin, nout))
        cur += nout - kin
    return stem_network(nq, gates, seed, sliced=int(rng.integers(0, 3)))


# (nq, gates): the families of the fused kernel -- 16 / 32 columns on either step, 256 and 512 tile rows, K up to 128,
# N2 up to 128 -- and chains with leftovers.  NOT every instantiation: these stems (with 0 and 2 indices sliced), ONE_CASES
# and random_stem(0..47) together reach 19 of the 47 static fp32 pairs and 20 of the 38 16-bit geometries; one row per
# instantiation, asserted by name, is tests/stem_variant_cases.py (run by tests/test_gpu_stem_variants.py)
STEM_CASES = [
    (16, [(3, 3), (5, 5), (5, 5)]),                    # k32 n32 | k32 n32
    (16, [(3, 3), (4, 4), (5, 5)]),                    # k16 n16 | k32 n32: 16 columns first, 512 rows
    (16, [(3, 3), (5, 5), (4, 4)]),                    # k32 n32 | k16 n16: 16 columns last
    (16, [(3, 3), (4, 4), (4, 4)]),                    # k16 n16 | k16 n16
    (17, [(3, 3), (5, 5), (6, 6)]),                    # k32 n32 | k64 n64
    (17, [(3, 3), (7, 5), (5, 5)]),                    # k128 n32 | k32 n32
    (17, [(3, 3), (5, 5), (5, 6)]),                    # k32 n32 | k32 n64
    (17, [(3, 3), (6, 5), (6, 6)]),                    # k64 n32 | k64 n64
    (17, [(3, 3), (4, 5), (5, 7)]),                    # k16 n32 | k32 n128
    (18, [(3, 3), (6, 4), (5, 4)]),                    # k64 n16 | k32 n16
    (17, [(3, 3), (5, 5), (5, 5), (4, 4), (5, 5), (6, 6), (5, 5)]),   # a longer stem: pairs + leftovers
    (17, [(3, 3), (6, 6), (5, 5)]),                    # k64 n64 | k32 n32: two waves per row tile
    (17, [(3, 3), (6, 6), (4, 4)]),                    # k64 n64 | k16 n16
    (18, [(3, 3), (4, 6), (6, 6)]),                    # k16 n64 | k64 n64
    (17, [(3, 3), (5, 7), (5, 5)]),                    # k32 n128 | k32 n32: four waves per row tile
    (18, [(3, 3), (4, 7), (5, 4)]),                    # k16 n128 | k32 n16
]


# ---------------------------------------------------------------------- #
# helpers shared by the GPU modules (tests/test_gpu_round4.py, test_gpu_round6.py, test_gpu_exec_history.py)
# ---------------------------------------------------------------------- #

# the small golden trees in which the planner finds LDS-resident subtrees, and the sliced ones for the slice groups
LDS_TREES = ["C1_rand10_d4", "C2_lattice8x8_d4", "lattice8x8_sliced", "lattice4x4_sliced", "preproc_s0_a", "preproc_s1",
             "rand_s42_r3_o2_hi1_ho2", "rand_s666_r3_o2_hi2_ho2_sliced", "rand_s42_r2_o2_hi0_ho2_outsliced",
             "project_1", "C5_hyper200"]
GROUP_CASES = [c["name"] for c in cases("tree")
               if c["name"] in ("lattice4x4_sliced", "lattice8x8_sliced", "preproc_s0_ac", "preproc_s1_ac")
               or (c["name"].startswith("rand_") and c["name"].endswith("sliced"))]


def chain_tree(R, K, N, N2=None):
    """a[R, K] b[K, N] (c[N, N2]): one long tiled step, or two of them in a chain (the second one's big operand
    produced -- and its largest element recorded -- by the first)."""
    if N2 is None:
        return ca.ContractionTree.from_path([("a", "b"), ("b", "c")], ("a", "c"), dict(a=R, b=K, c=N), path=[(0, 1)])
    return ca.ContractionTree.from_path([("a", "b"), ("b", "c"), ("c", "d")], ("a", "d"), dict(a=R, b=K, c=N, d=N2),
                                        path=[(0, 1), (0, 1)])


def cplx(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype("complex64")


# what the library reads from the environment to pick an arithmetic, a slice batch, a captured graph or slice groups
ARITH_ENV = ("CTG_STEM_ARITH", "CTG_STEM_BF16X3", "CTG_STEM_H2", "CTG_STEM_H2_ALL", "CTG_PAIR_BF16X3", "CTG_PAIR_H2",
             "CTG_NO_PAIR_RECORD", "CTG_GRAPH", "CTG_SLICE_BATCH", "CTG_SLICE_GROUPS", "CTG_NO_BATCHED_GROUPS")


def fuse_whatever_fits(monkeypatch, h2_all=True):
    """The pairing model takes every stem pair the kernel can run, and nothing in the environment names an arithmetic.
    By default the FIRST pair of a stem -- its big operand comes from a kernel that records no maximum -- is multiplied
    in bf16 x 3; ``h2_all`` gives every capable pair fp16 x 2 (a max-abs pass supplies the scale)."""
    from cotengra_amd import stem
    monkeypatch.setattr(stem, "gather_rate", lambda run_bytes: 5.4e12)
    for k in ARITH_ENV:
        monkeypatch.delenv(k, raising=False)
    if h2_all:
        monkeypatch.setenv("CTG_STEM_H2_ALL", "1")


def groups_everywhere(monkeypatch):
    """Slice groups wherever a step is independent of a sliced index, whatever the model says they save."""
    from cotengra_amd import plan as P

    monkeypatch.delenv("CTG_SLICE_GROUPS", raising=False)
    monkeypatch.setattr(P, "GROUP_MIN_WIDTH", 1)
    monkeypatch.setattr(P, "GROUP_MIN_SAVING", 0.0)


# An input whose largest |component| lies outside [2^-32, 2^32) is brought back to the edge of that window at upload
# (prescale_inputs_kernel): a scale that leaves the window never reaches a kernel.
UPLOAD_WINDOW_LOG2 = 32


def assert_in_upload_window(x):
    x = np.asarray(x)
    top = float(max(np.abs(x.real).max(), np.abs(x.imag).max())) if np.iscomplexobj(x) else float(np.abs(x).max())
    assert 2.0 ** -UPLOAD_WINDOW_LOG2 <= top < 2.0 ** UPLOAD_WINDOW_LOG2, ("the upload would normalise this scale away", top)


def scaled_in_window(x, log2):
    """``x * 2^log2`` (an exact power of two, the dtype kept), its largest |component| asserted to stay inside the
    upload window -- the kernels see the scale."""
    assert int(log2) == log2
    y = (np.asarray(x) * np.asarray(2.0 ** int(log2), dtype=np.asarray(x).real.dtype)).astype(np.asarray(x).dtype)
    assert_in_upload_window(y)
    return y
