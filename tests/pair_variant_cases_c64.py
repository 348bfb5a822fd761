"""The pair-kernel variants of complex64, one table per dispatcher of csrc/ctg_pair_mfma.hip (launch_pair_mfma: the
streaming, k-streaming, tiled, skinny and row-wise kernels).  tests/test_pair_variant_plans.py checks on the host that
the planner gives every row the step this table records; tests/test_gpu_pair_variants_c64.py runs the rows, asserts
the kernel the executor names (tests/golden_util.py: pair_flags_c64) and compares the numbers with numpy.

The template arguments are what the executor's hints (csrc/ctg_runtime.hip: build_hints_into) and the launchers choose
for the recorded ``(R, Bt, K, N)`` and the layout of the equation; they are asserted on the device through the
kernel's name and nowhere computed in Python.  Every row uses the smallest extents that still take its kernel: the
streaming kernels need R >= 8192, the skinny kernel R >= 65536, the k-streaming kernel K >= 65536, and a tiled row
needs 512 blocks of its tile (the narrowing rule of build_hints_into halves the tile below that)."""
from pair_variant_cases import Case, split_contracted  # noqa: F401  (split_contracted: used with these rows)

T, F = True, False

STREAM, KSTREAM, SKINNY_K, ROWWISE = ("pair_mfma_stream_kernel", "pair_mfma_kstream_kernel", "pair_skinny_kernel",
                                      "pair_rowwise_kernel")
C64, FAST, BF3, H2 = "pair_mfma_c64_kernel", "pair_mfma_fast_kernel", "pair_mfma_bf3_kernel", "pair_mfma_h2_kernel"


class Row(Case):
    """A case, the kernel and template arguments expected of its step, and -- tiled kernels -- the 16-byte gathers
    and whether the step is cut along k (``ksplit``: True, more than one slab per output; False, none).  ``kernel``
    None: either tiled fp32 kernel; ``args`` (): not asserted.  ``env``:
    what the environment must say for the row to take its kernel; ``sliced``: indices to slice."""

    def __init__(self, ident, eq, sizes, step, kernel, args, vec=None, ksplit=False, env=None, sliced=(), seed=0):
        super().__init__(ident, eq, sizes, step, seed=seed)
        self.kernel, self.args, self.vec, self.ksplit = kernel, tuple(args), vec, ksplit
        self.env, self.sliced = dict(env or {}), tuple(sliced)

    def like(self, ident, eq, sizes, step, sliced=()):
        return Row(ident, eq, sizes, step, self.kernel, self.args, self.vec, self.ksplit, self.env, sliced,
                   seed=self.seed + 1000)


def _seeded(rows, first):
    for i, r in enumerate(rows):
        r.seed = first + i
    return rows


# ---------------------------------------------------------------------------------------------------------------- #
# pair_mfma_stream_kernel<FN,VEC,ADD,SHORTK,NV>: FN = ceil(N / 16) rounded to 1, 2, 4; ADD, the 32 rows of a group
# are base + constant (extents that are powers of two); VEC, 16-byte gathers (ADD, K even and contiguous); SHORTK,
# K < 16, with NV = 2, 4, 8 gather slots per lane for K <= 4, <= 8, < 16.
# ---------------------------------------------------------------------------------------------------------------- #
_P2 = dict(a=128, b=64)    # R = 8192: 256 groups
_RG = dict(a=91, b=91)     # R = 8281: rows not 32-additive, the last of 259 groups holds 25 rows


def _s(ident, k, n, args, rows=_P2, eq="abk,kn->abn"):
    sizes = dict(rows, k=k, n=n)
    return Row(ident, eq, sizes, (sizes["a"] * sizes.get("b", 1), 1, k, n), STREAM, args)


STREAM_CASES = _seeded([
    _s("S1ttt2", 4, 16, (1, T, T, T, 2)), _s("S1ttt4", 8, 16, (1, T, T, T, 4)), _s("S1ttt8", 12, 16, (1, T, T, T, 8)),
    _s("S1ttf8", 16, 16, (1, T, T, F, 8)),
    # odd K, or K no multiple of 16: the element-wise gather
    _s("S1ftt2", 3, 16, (1, F, T, T, 2)), _s("S1ftt4", 7, 12, (1, F, T, T, 4)), _s("S1ftt8", 13, 9, (1, F, T, T, 8)),
    _s("S1ftf8", 24, 16, (1, F, T, F, 8)),
    # two chunks, the second holds one k; N is ragged inside a 16-column fragment
    _s("S1fff8", 17, 10, (1, F, F, F, 8), rows=_RG),
    # eight chunks: more than 48 KB of LDS, the kernel opts in; k is not the fastest index of A
    _s("S1ttf8_k128", 128, 16, (1, T, T, F, 8), eq="akb,kn->abn"),
    _s("S2ttt2", 2, 32, (2, T, T, T, 2)), _s("S2ttt4", 6, 17, (2, T, T, T, 4)), _s("S2ttt8", 14, 24, (2, T, T, T, 8)),
    _s("S2ttf8", 64, 32, (2, T, T, F, 8), eq="kab,nk->abn"),
    _s("S2ftt2", 3, 32, (2, F, T, T, 2)), _s("S2ftt4", 5, 20, (2, F, T, T, 4)), _s("S2ftt8", 15, 24, (2, F, T, T, 8)),
    _s("S2ftf8", 40, 32, (2, F, T, F, 8)),
    _s("S2fff8", 48, 31, (2, F, F, F, 8), rows=_RG),
    _s("S4ttt2", 4, 64, (4, T, T, T, 2)), _s("S4ttt4", 8, 64, (4, T, T, T, 4)), _s("S4ttt8", 12, 48, (4, T, T, T, 8)),
    _s("S4ttf8", 32, 64, (4, T, T, F, 8)),
    _s("S4ftt2", 3, 40, (4, F, T, T, 2)), _s("S4ftt4", 5, 48, (4, F, T, T, 4)), _s("S4ftt8", 15, 40, (4, F, T, T, 8)),
    _s("S4ftf8", 24, 64, (4, F, T, F, 8)),
    # rows that are not additive stay on this kernel only above 32 columns or from K = 16 on (the row-wise kernel
    # takes the others): all four SHORTK forms exist at FN = 4 only
    _s("S4fft2", 4, 33, (4, F, F, T, 2), rows=_RG), _s("S4fft4", 8, 64, (4, F, F, T, 4), rows=_RG),
    _s("S4fft8", 15, 40, (4, F, F, T, 8), rows=_RG), _s("S4fff8", 32, 64, (4, F, F, F, 8), rows=_RG),
    # 257 groups, the last with 8 rows; 256 blocks of four waves: three waves of the last block get no group
    _s("S1fff8_tail", 16, 16, (1, F, F, F, 8), rows=dict(a=8200), eq="ak,kn->an"),
    # K = 32: with half of the contraction sliced (split_contracted) the step is S1ttf8's
    _s("S1ttf8_k32", 32, 16, (1, T, T, F, 8)),
], 200)

# <1|2,false,false,true,2|4|8>: a step with rows that are not additive, K < 16 and N <= 32 goes to the row-wise kernel
# (build_hints_into: `!h.additive32 && K < MFMA_BK` under `K <= 32 && N <= 32`) -- instantiated, never launched.
STREAM_UNREACHABLE = [(fn, F, F, T, nv) for fn in (1, 2) for nv in (2, 4, 8)]

# The same kernels with the loop over tasks going round: a task is one 16-deep chunk of one 32-row group, a wave keeps
# DEPTH = 16 / NV tasks in flight (2 for NV = 8) and owns every n_waves-th group.  The launcher caps the grid at 256
# CUs x the resident blocks of four waves (hipOccupancyMaxActiveBlocksPerMultiprocessor).  The launch bounds promise
# 4 blocks for FN = 1 and 2 for FN = 4; the registers the compiler takes allow (hipcc -Rpass-analysis=
# kernel-resource-usage, gfx950) 5 for <1,t,t,t,2> (93 VGPRs), 4 for <1,f,f,f,8> (110), 3 for <4,f,f,t,4> (166) and
# 2 for <4,t,t,f,8> (231): W = 5120, 4096, 3072 and 2048 waves.  G = q W + 1 groups give every wave q groups =
# q ceil(K / 16) tasks, more than 2 DEPTH, and wave 0 one group more (on fewer waves: more tasks each); on the
# ADD = false rows the last group is ragged.
#   D1ttt2: DEPTH 8, G = 17 * 5120 + 1 -> 17 tasks a wave (18: wave 0)    D1fff8: DEPTH 2, G = 3 * 4096 + 1 -> 6 (8)
#   D4fft4: DEPTH 4, G = 9 * 3072 + 1 -> 9 (10)                           D4ttf8: DEPTH 2, G = 5 * 2048 + 1 -> 10 (12)
# (D4ttf8 has full columns and whole chunks: the unrolled loop of the VEC && ADD form, two chunks per pass.)
# Operands and result: 446, 87, 510 and 252 MB.
DEEP_CASES = _seeded([
    _s("D1ttt2", 4, 16, (1, T, T, T, 2), rows=dict(a=17 * 5120 + 1, b=32)),
    # 23131 x 17 = 393227 rows: 12289 groups, the last with 11 rows
    _s("D1fff8", 17, 10, (1, F, F, F, 8), rows=dict(a=23131, b=17)),
    # 30509 x 29 = 884761 rows: 27649 groups, the last with 25 rows
    _s("D4fft4", 8, 64, (4, F, F, T, 4), rows=dict(a=30509, b=29)),
    _s("D4ttf8", 32, 64, (4, T, T, F, 8), rows=dict(a=5 * 2048 + 1, b=32)),
], 300)


# ---------------------------------------------------------------------------------------------------------------- #
# pair_mfma_kstream_kernel<FN,VEC>: R, N <= 32 under K >= 2^16; every wave's partial tile is a slab of the reduction.
# ---------------------------------------------------------------------------------------------------------------- #
def _k(ident, eq, a, k, b, args):
    return Row(ident, eq, dict(a=a, k=k, b=b), (a, 1, k, b), KSTREAM, args, ksplit=True)


KSTREAM_CASES = _seeded([
    _k("K1t", "ka,bk->ab", 32, 1 << 16, 16, (1, T)),
    _k("K2t", "ak,kb->ab", 32, 1 << 16, 32, (2, T)),
    _k("K1f", "ak,kb->ab", 20, 1 << 16, 16, (1, F)),
    _k("K2f", "ak,kb->ab", 31, 1 << 16, 17, (2, F)),
], 400)

# K = 2^16 + 16: the planner's low k table is not a power of two long, the k-streaming kernel refuses (kstream_ok) and
# the tiled kernel cuts the contraction
KSTREAM_REFUSED = Row("K_refused", "ak,kb->ab", dict(a=32, k=(1 << 16) + 16, b=32), (32, 1, (1 << 16) + 16, 32), None,
                      (), ksplit=True, seed=405)


# ---------------------------------------------------------------------------------------------------------------- #
# The tiled kernels, "<128,BN,16>,VEC": pair_mfma_fast_kernel on full tiles with tile-additive offsets,
# pair_mfma_c64_kernel otherwise; from K >= 64 on full 64-column tiles the 16-bit pipe.
# ---------------------------------------------------------------------------------------------------------------- #
def _t(ident, a, k, n, kernel, bn, vec, ksplit=False, x=0, env=None):
    """``ak,kn->an``, or -- ``x`` -- its batch-fastest form ``akx,knx->anx``: the pairs of A are not contiguous."""
    if x:
        return Row(ident, "akx,knx->anx", dict(a=a, k=k, n=n, x=x), (a, x, k, n), kernel, (128, bn, 16), vec, ksplit, env)
    return Row(ident, "ak,kn->an", dict(a=a, k=k, n=n), (a, 1, k, n), kernel, (128, bn, 16), vec, ksplit, env)


TILED_CASES = _seeded([
    _t("G16c_t", 2048, 64, 40, C64, 16, T), _t("G16c_f", 1000, 40, 40, C64, 16, F),
    _t("G32c_t", 65536, 80, 32, C64, 32, T), _t("G32c_f", 65537, 81, 31, C64, 32, F),
    _t("G64c_t", 8192, 32, 500, C64, 64, T), _t("G64c_f", 8193, 33, 513, C64, 64, F),
    _t("G16f_t", 2048, 16, 16, FAST, 16, T), _t("G16f_f", 2048, 64, 64, FAST, 16, F, x=2),
    _t("G32f_t", 65536, 128, 32, FAST, 32, T), _t("G32f_f", 32768, 128, 32, FAST, 32, F, x=2),
    _t("G64f_t", 8192, 32, 512, FAST, 64, T), _t("G64f_f", 8192, 32, 256, FAST, 64, F, x=2),
    _t("G128f_f", 4096, 256, 1024, FAST, 128, F, x=2),
    # cut along k: the slabs of the k-splits and splitk_reduce_kernel
    _t("G128f_t_split", 1024, 2048, 512, FAST, 128, T, ksplit=True),
    _t("G16f_t_split", 128, 4096, 64, FAST, 16, T, ksplit=True),
    _t("G16c_f_split", 130, 4100, 70, C64, 16, F, ksplit=True),   # ragged in all three
    Row("G_split_batch", "xak,xkn->xan", dict(x=3, a=128, k=2048, n=64), (128, 3, 2048, 64), None, (), None, True),
    Row("G32f_t_batch", "xak,xkn->xan", dict(x=4, a=2048, k=64, n=256), (2048, 4, 64, 256), FAST, (128, 32, 16), T),
    # k_lo = 80 is not a power of two: neither the fast kernel nor the 16-bit pipe
    _t("G64c_t_k80", 8192, 80, 512, C64, 64, T),
], 500)

# 8192 x 64 x 512, the smallest step the 16-bit pipe takes (512 tiles of 128 x 64, K = 64), in its three arithmetics
_NO_ARITH = {"CTG_STEM_ARITH": None, "CTG_NO_PAIR_BF3": None}
PIPE16_CASES = _seeded([
    _t("P_h2", 8192, 64, 512, H2, 64, T, env=_NO_ARITH),
    _t("P_bf3", 8192, 64, 512, BF3, 64, T, env=dict(_NO_ARITH, CTG_STEM_ARITH="bf16x3")),
    _t("P_fast", 8192, 64, 512, FAST, 64, T, env=dict(_NO_ARITH, CTG_NO_PAIR_BF3="1")),
    # the pairs of A are not contiguous (s, sliced, is its fastest index): the element-wise gather of the 16-bit pipe
    Row("P_h2_f", "aks,kn->an", dict(a=8192, k=64, n=512, s=3), (8192, 1, 64, 512), H2, (128, 64, 16), F, False,
        _NO_ARITH, sliced=("s",)),
], 600)
for _r in PIPE16_CASES[:3]:
    _r.seed = 600   # (one set of operands and one reference for the three arithmetics)


# ---------------------------------------------------------------------------------------------------------------- #
# pair_skinny_kernel<K,N>: the nine instantiations (tests/test_gpu_pairwise.py: SKINNY runs five of them as well).
# ---------------------------------------------------------------------------------------------------------------- #
def _sk(k, n, eq="kab,kn->abn", sizes=None):
    sizes = dict(sizes or dict(a=256, b=256), k=k, n=n)
    if n == 1:
        eq, sizes = "kab,k->ab", {i: v for i, v in sizes.items() if i != "n"}
    return Row(f"N{k}_{n}", eq, sizes, (65536 if "c" not in sizes else 131072, 1, k, n), SKINNY_K, (k, n))


SKINNY_CASES = _seeded([
    _sk(2, 2), _sk(2, 4), _sk(4, 2), _sk(8, 2, eq="kabc,kn->abcn", sizes=dict(a=64, b=64, c=32)),
    _sk(2, 1), _sk(4, 1), _sk(8, 1), _sk(16, 1), _sk(4, 4),
], 700)


# ---------------------------------------------------------------------------------------------------------------- #
# pair_rowwise_kernel<NN,TS>: NN = N rounded up to 4, 8, 12, 16, 24, 32 accumulators; TS, the columns are the
# fastest index of the result and go through LDS.  27 x 32 x 12 rows, not 32-additive, K = 6.
# ---------------------------------------------------------------------------------------------------------------- #
def _r(nn, n, ts):
    eq = "abkc,kn->abcn" if ts else "abkc,kn->nabc"
    return Row(f"R{nn}{'t' if ts else 'f'}", eq, dict(a=27, b=32, c=12, k=6, n=n), (27 * 32 * 12, 1, 6, n), ROWWISE,
               (nn, ts))


ROWWISE_CASES = _seeded([_r(4, 3, T), _r(8, 7, T), _r(12, 9, T), _r(16, 16, T), _r(24, 18, T), _r(32, 30, T),
                         _r(4, 3, F), _r(8, 7, F), _r(12, 9, F), _r(16, 13, F), _r(24, 18, F), _r(32, 30, F)], 800)

ALL_CASES = (STREAM_CASES + DEEP_CASES + KSTREAM_CASES + [KSTREAM_REFUSED] + TILED_CASES + PIPE16_CASES + SKINNY_CASES
             + ROWWISE_CASES)
ORDINARY_CASES = STREAM_CASES + KSTREAM_CASES + TILED_CASES + SKINNY_CASES + ROWWISE_CASES


def by_id(ident):
    return next(c for c in ALL_CASES if c.id == ident)


def sliced_rows(case):
    """``case`` with an index s = 4 written in front of its first row index and sliced: four slices of the same step,
    in one launch or one by one; the operands are those of a case with four times the rows."""
    row = next(ix for ix in case.ta if ix in case.out and ix not in case.tb)
    eq = case.eq.replace(row, "s" + row)
    return case.like(case.id + "_z", eq, dict(case.sizes, s=4), case.step, sliced=("s",))


# One row per kernel family, where strip_exponent scales what the kernel stores (step_alpha) ...
STRIP_IDS = ["S1ttf8", "S1fff8", "K1t", "G32f_t", "G32c_f", "G16f_t_split", "R16t", "R16f"]
# ... and where several slices share a launch (gridDim.y, or the launcher's loop over the slices)
SLICE_BATCH_IDS = ["S1ttf8", "S1fff8", "K1t", "G16c_t", "G16f_t_split", "R16t", "N2_2"]
# ... and where half of the contraction is sliced, slow or as the fastest index of A
# (the batched row: at K = 64 and N = 32 an unbatched step of 65536 rows is the streaming kernel's)
SPLIT_K_IDS = ["S1ttf8_k32", "G32f_t_batch"]
