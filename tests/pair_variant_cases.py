"""The pair-kernel variants of float32, float64 and complex128, one table per dispatcher
(csrc/ctg_pair_mfma_f64.hip: launch_pair_mfma_c128, launch_pair_mfma_real; csrc/ctg_kernels_valu.hip:
launch_pair_valu_t).  tests/test_pair_variant_plans.py checks on the host that the planner gives every row
the step this table records; tests/test_gpu_pair_variants.py runs the rows, asserts the kernel the executor
names and compares the numbers with numpy.

The tiles are what the dispatchers choose for the recorded ``(R, Bt, K, N)``; they are asserted on the device
through the kernel's name and nowhere computed in Python."""
import numpy as np

import cotengra_amd as ca

DTYPES = ("complex128", "float32", "float64")
ALL_DTYPES = ("complex64",) + DTYPES


class Case:
    def __init__(self, ident, eq, sizes, step, tiles=None, vec=None, seed=0):
        self.id, self.eq, self.sizes, self.step, self.seed = ident, eq, dict(sizes), tuple(step), seed
        self.tiles = dict(zip(DTYPES, tiles)) if tiles else None   # dtype -> (TM, TN)
        self.vec = dict(zip(("float32", "float64"), vec)) if vec else None   # dtype -> VEC, the 16-byte gathers
        (self.ta, self.tb), self.out = ca.eq_to_inputs_output(eq)

    def tree(self, sliced=()):
        tree = ca.ContractionTree.from_path([self.ta, self.tb], self.out, self.sizes, path=[(0, 1)])
        for ix in sliced:
            tree.remove_ind_(ix)
        return tree

    def arrays(self, dtype):
        """Standard normal operands, seeded by the case."""
        rng = np.random.default_rng(self.seed)
        out = []
        for t in (self.ta, self.tb):
            shape = [self.sizes[i] for i in t]
            x = rng.standard_normal(shape)
            if "complex" in dtype:
                x = x + 1j * rng.standard_normal(shape)
            out.append(x.astype(dtype))
        return out

    def __repr__(self):
        return self.id


def _t(*tiles):
    return [(t // 10, t % 10) for t in tiles]


# id, equation, extents, the planner's (R, Bt, K, N), the tile in complex128 / float32 / float64.
# Tile counts: complex128 <4,2> at ceil(R/128) ceil(N/32) Bt >= 1024; real <4,2> at ceil(R/128) ceil(N/64) Bt >=
# 1024; float <4,4> at ceil(R/128) ceil(N/128) Bt >= 1024 and N >= 96 (the dispatchers' rules, quoted for the
# reader: a test asserts the tile by the kernel's name only).
TILE_CASES = [
    # ragged in R, K and N, just over the planner's threshold for the matrix cores
    Case("T1", "ab,bc->ac", dict(a=257, b=65, c=257), (257, 1, 65, 257), _t(22, 22, 22), seed=1),
    # both operands transposed (the operand with more kept elements supplies the rows: c)
    Case("T2", "ba,cb->ca", dict(a=257, b=67, c=259), (259, 1, 67, 257), _t(22, 22, 22), seed=2),
    # T3 / T4: one row apart, on either side of the complex128 threshold (127 x 8 = 1016 / 128 x 8 = 1024 tiles);
    # the last row tile of T4 holds one row
    Case("T3", "ab,bc->ac", dict(a=16256, b=20, c=256), (16256, 1, 20, 256), _t(22, 22, 22), seed=3),
    Case("T4", "ab,bc->ac", dict(a=16257, b=20, c=256), (16257, 1, 20, 256), _t(42, 22, 22), seed=4),
    Case("T5", "ba,cb->ca", dict(a=16257, b=18, c=250), (16257, 1, 18, 250), _t(42, 22, 22), seed=5),
    # the threshold reached through the batch index
    Case("T6", "xab,xbc->xac", dict(x=4, a=4096, b=12, c=256), (4096, 4, 12, 256), _t(42, 22, 22), seed=6),
    # T7 / T8: the same boundary for the real kernels
    Case("T7", "ab,bc->ac", dict(a=16256, b=20, c=512), (16256, 1, 20, 512), _t(42, 22, 22), seed=7),
    Case("T8", "ab,bc->ac", dict(a=16257, b=20, c=512), (16257, 1, 20, 512), _t(42, 42, 42), seed=8),
    Case("T9", "ba,cb->ca", dict(a=16257, b=18, c=449), (16257, 1, 18, 449), _t(42, 42, 42), seed=9),
    # two column tiles, the second with one column
    Case("T10", "ab,bc->ac", dict(a=65537, b=20, c=65), (65537, 1, 20, 65), _t(42, 42, 42), seed=10),
    # the 4 x 4 tile with 96 of 128 columns
    Case("T11", "ab,bc->ac", dict(a=131072, b=20, c=96), (131072, 1, 20, 96), _t(42, 44, 42), seed=11),
    # N < 96: the wide tile is refused and the tall one is taken
    Case("T12", "ab,bc->ac", dict(a=130945, b=20, c=95), (130945, 1, 20, 95), _t(42, 42, 42), seed=12),
    Case("T13", "ab,bc->ac", dict(a=16257, b=20, c=1024), (16257, 1, 20, 1024), _t(42, 44, 42), seed=13),
    # K = 52 is four k-steps: the three-slot ring of k offsets wraps.  Transposed.
    Case("T14", "ba,cb->ca", dict(a=16260, b=52, c=900), (16260, 1, 52, 900), _t(42, 44, 42), seed=14),
    # odd K and N on the large tiles: the 4 x 4 tile with the element-wise gather (T11, T13 and T14 gather in pieces)
    Case("T15", "ab,bc->ac", dict(a=16257, b=21, c=1023), (16257, 1, 21, 1023), _t(42, 44, 42), vec=(False, False),
         seed=15),
]

# The 16-byte gathers of the real kernels (VEC), all on the <2,2> tile: VEC in float32 / float64.
# V8: the row group (a, b) and the column group (c, d) are each contiguous in their operand, all extents are
# multiples of four and k is a multiple of four: real_vec_ok (csrc/ctg_runtime.hip) says yes for both operands in
# both types -- A in pieces along k, B along its columns.
GATHER_CASES = [
    Case("V1", "ab,bc->ac", dict(a=512, b=128, c=192), (512, 1, 128, 192), vec=(True, True), seed=21),
    Case("V2", "ab,cb->ac", dict(a=512, b=128, c=192), (512, 1, 128, 192), vec=(True, True), seed=22),
    Case("V3", "ba,bc->ac", dict(a=512, b=128, c=192), (512, 1, 128, 192), vec=(True, True), seed=23),
    Case("V4", "ba,cb->ca", dict(a=384, b=256, c=256), (384, 1, 256, 256), vec=(True, True), seed=24),
    # extents that are multiples of 2 only: double yes, float no
    Case("V5", "ab,bc->ac", dict(a=514, b=66, c=130), (514, 1, 66, 130), vec=(False, True), seed=25),
    # odd extents: the element-wise gather
    Case("V6", "ab,bc->ac", dict(a=513, b=65, c=131), (513, 1, 65, 131), vec=(False, False), seed=26),
    Case("V7", "xab,xbc->xac", dict(x=3, a=256, b=64, c=256), (256, 3, 64, 256), vec=(True, True), seed=27),
    Case("V8", "abk,kcd->abcd", dict(a=32, b=16, k=64, c=8, d=16), (512, 1, 64, 128), vec=(True, True), seed=28),
    # K a multiple of 4 but not of 16: the last k-step is half empty, in whole pieces
    Case("V9", "ab,bc->ac", dict(a=512, b=52, c=192), (512, 1, 52, 192), vec=(True, True), seed=29),
]
for _c in GATHER_CASES:
    _c.tiles = dict(zip(DTYPES, _t(22, 22, 22)))


def split_contracted(case, fast):
    """``case`` with its contracted index written as two, (s, k') -- or (k', s) when ``fast`` -- and s, the smallest
    prime factor of the extent, meant to be sliced (``tree(sliced=("s",))``).  The operands are reshaped views of
    the unsliced case's, the sum over the slices is its result; the step keeps a contraction of K / s, so it stays
    on the matrix cores and the slice strides enter the host's check of the 16-byte gathers: k' (slow) or 1
    (``fast``: every other slice of an operand whose fastest index is the contracted one starts at an odd element)."""
    k = next(ix for ix in case.ta if ix in case.tb and ix not in case.out)
    ext = case.sizes[k]
    p = next(q for q in range(2, ext + 1) if ext % q == 0)
    eq = case.eq.replace(k, k + "s" if fast else "s" + k)
    R, Bt, K, N = case.step
    new = Case(case.id + ("f" if fast else "s"), eq, dict(case.sizes, **{"s": p, k: ext // p}), (R, Bt, K // p, N),
               tiles=[case.tiles[d] for d in DTYPES] if case.tiles else None, seed=case.seed)
    new.split = k
    return new


# The tall and wide tiles with a launch of several slices (gridDim.y = nz): the row index of T4 / T8 / T13 as
# (s, a) with s = 4 sliced, in the types where the unsliced case is tall or wide.  dtype -> rows per slice, the
# fewest that still give ONE slice the tile's 1024 blocks with a last row tile of one row (asserted by name).
SLICED_ROWS = {
    "T4": {"complex128": 16257},
    "T8": {"complex128": 8065, "float32": 16257, "float64": 16257},
    "T13": {"complex128": 3969, "float32": 16257, "float64": 8065},
}


def sliced_case(ident, dtype):
    base = next(c for c in TILE_CASES if c.id == ident)
    rows = SLICED_ROWS[ident][dtype]
    sizes = dict(base.sizes, s=4, a=rows)
    return Case(f"{ident}s", "sab,bc->sac", sizes, (rows, 1, base.step[2], base.step[3]),
                tiles=[base.tiles[d] for d in DTYPES], seed=100 + base.seed)


# Long contractions under few outputs (launch_pair_valu_t: K >= 256 and R N <= 2^15 put the lanes along k): the
# cases of tests/test_gpu_pairwise.py that are meant for these kernels, by their index in its CASES, and the kernel
# each takes in all four types -- one wave per output and k-chunk, or (two to four outputs) one wave per k-chunk
# for all of them.
KRED_PAIRWISE = [
    # index, equation (for the reader; the test reads CASES), kernel, outputs per wave
    (5, "ak,kb->ab", "pair_kred_multi_kernel", 4),    # 2 x 2 outputs, K = 2^18
    (6, "k,k->", "pair_kred_kernel", 0),              # the dot product
    (-4, "ak,k->a", "pair_kred_multi_kernel", 3),
    (-3, "xk,xk->x", "pair_kred_multi_kernel", 3),    # (the batch index of a VALU step counts as rows)
    (-2, "ka,kb->ab", "pair_kred_multi_kernel", 4),
    (-1, "akl,lk->a", "pair_kred_multi_kernel", 2),
]

# ... and two that must stay on the thread-per-output kernel, pair_valu_kernel, in all four types
THREAD_PAIRWISE = [(10, "ab,cd->abcd"), (11, "ab,ab->ab")]   # outer product, Hadamard product

# One shape per branch of the finish pass.  launch_pair_valu_t cuts K into G chunks -- 512 k per chunk up to 64
# outputs, 2048 above, never more than 256 chunks nor than 2^14 / outputs, chunks rounded up to 64 k -- and adds the
# G partial sums of an output with a wavefront (pair_kred_finish_kernel<true>) when outputs <= 4096 and G >= 16, with
# one thread otherwise (<false>).  id, equation, extents, (R, Bt, K, N), kernel, outputs per wave, wave finish.
FINISH_CASES = [
    # 7 outputs, K = 40000: 79 chunks of 512 -> the wave form
    (Case("F1", "ak,k->a", dict(a=7, k=40000), (7, 1, 40000, 1), seed=31), "pair_kred_kernel", 0, True),
    # 5 outputs, K = 2000: 4 chunks, fewer than 16 -> the other form
    (Case("F2", "ak,k->a", dict(a=5, k=2000), (5, 1, 2000, 1), seed=32), "pair_kred_kernel", 0, False),
    # 1400 x 4 = 5600 outputs, more than 4096 (2 chunks of 2048 k) -> the other form
    (Case("F3", "ak,kb->ab", dict(a=1400, k=4000, b=4), (1400, 1, 4000, 4), seed=33), "pair_kred_kernel", 0, False),
    # 3 outputs, K = 1000: the multi-output kernel with 2 chunks -> the other form (the cases of KRED_PAIRWISE have
    # K >= 65537, 128 or more chunks: the wave form)
    (Case("F4", "ak,k->a", dict(a=3, k=1000), (3, 1, 1000, 1), seed=34), "pair_kred_multi_kernel", 3, False),
]
