"""The single-term kernels (csrc/ctg_kernels_valu.hip: launch_single_t), one table of small one-input equations.
``single_route_wave`` sends a step with K >= 256 and R <= 2^14 to single_wave_kernel (a wave per output, lanes
along the summed group through split_k) and everything else to single_kernel (a thread per output, a serial
k_hi_len x k_lo loop).  tests/test_single_variant_plans.py checks on the host that the planner gives every row the
step this table records and that the table keeps every edge it is meant to hold; tests/test_gpu_single_variants.py
runs the rows in all four types, asserts the kernel the executor names and compares the numbers with numpy.

A row is ``ContractionTree.from_path([term], out, sizes, path=[])`` with the indices of ``sliced`` removed; its
step is ``(R, K, k_lo, k_hi_len)`` of ONE slice, and ``row`` -- where it matters -- ``(row_lo, row_hi_len)``."""
import numpy as np

import cotengra_amd as ca

ALL_DTYPES = ("float32", "float64", "complex64", "complex128")
WAVE, THREAD = "single_wave_kernel", "single_kernel"
WAVE_MIN_K, WAVE_MAX_R = 256, 1 << 14   # (the launcher's rule, quoted for the table's own checks)


class Case:
    def __init__(self, ident, eq, sizes, step, kernel, sliced=(), row=None, seed=0):
        self.id, self.eq, self.sizes, self.step, self.kernel = ident, eq, dict(sizes), tuple(step), kernel
        self.sliced, self.row, self.seed = tuple(sliced), row, seed
        self.terms, self.out = ca.eq_to_inputs_output(eq)

    def tree(self, sliced=None):
        path = [] if len(self.terms) == 1 else [(0, 1)]
        tree = ca.ContractionTree.from_path(list(self.terms), self.out, self.sizes, path=path)
        for ix in self.sliced if sliced is None else sliced:
            tree.remove_ind_(ix)
        return tree

    @property
    def nslices(self):
        n = 1
        for ix in self.sliced:
            n *= self.sizes[ix]
        return n

    @property
    def elems(self):
        return int(np.prod([self.sizes[i] for i in self.terms[0]], dtype=np.int64))

    def arrays(self, dtype):
        """Standard normal operands, seeded by the case."""
        rng = np.random.default_rng(self.seed)
        out = []
        for t in self.terms:
            shape = [self.sizes[i] for i in t]
            x = rng.standard_normal(shape)
            if "complex" in dtype:
                x = x + 1j * rng.standard_normal(shape)
            out.append(x.astype(dtype))
        return out

    def __repr__(self):
        return self.id


# id, equation, extents, (R, K, k_lo, k_hi_len), kernel.
WAVE_CASES = [
    # a full trace: one output, a diagonal stride of 301; K is no multiple of 64 and k_lo no power of two
    Case("W1", "aa->", dict(a=300), (1, 300, 300, 1), WAVE, seed=1),
    # the threshold itself and one above it: four full lane rounds, and a fifth with one lane
    Case("W2", "ak->a", dict(a=5, k=256), (5, 256, 256, 1), WAVE, seed=2),
    Case("W3", "ak->a", dict(a=5, k=257), (5, 257, 257, 1), WAVE, seed=3),
    # a two-level k table under the multiply-high split (k_lo = 100), K = 234 * 64 + 24
    Case("W4", "axyz->a", dict(a=3, x=3, y=50, z=100), (3, 15000, 100, 150), WAVE, seed=4),
    # ... and under the shift (k_lo = 4096)
    Case("W5", "axyz->a", dict(a=3, x=2, y=4, z=4096), (3, 32768, 4096, 8), WAVE, seed=5),
    # the last R on the wave form: 4096 workgroups of four waves
    Case("W6", "ak->a", dict(a=1 << 14, k=256), (1 << 14, 256, 256, 1), WAVE, seed=6),
    # a sum to a scalar: one wave, 2^14 rounds of its lane loop
    Case("W7", "abc->", dict(a=256, b=64, c=64), (1, 1 << 20, 4096, 256), WAVE, seed=7),
    # the summed index is the slowest in memory (stride 63), the rows are contiguous
    Case("W8", "kab->ab", dict(k=300, a=7, b=9), (63, 300, 300, 1), WAVE, seed=8),
]

THREAD_CASES = [
    # one below the threshold in K
    Case("T1", "ak->a", dict(a=5, k=255), (5, 255, 255, 1), THREAD, seed=11),
    # one row above the threshold in R: the serial loop runs K = 256
    Case("T2", "ak->a", dict(a=(1 << 14) + 1, k=256), ((1 << 14) + 1, 256, 256, 1), THREAD, seed=12),
    Case("T3", "axyz->a", dict(a=20000, x=3, y=5, z=17), (20000, 255, 255, 1), THREAD, row=(20000, 1), seed=13),
    # a diagonal, a double diagonal, a triple label
    Case("T4", "aab->b", dict(a=30, b=11), (11, 30, 30, 1), THREAD, seed=14),
    Case("T5", "aabb->ab", dict(a=6, b=7), (42, 1, 1, 1), THREAD, seed=15),
    Case("T6", "aaa->a", dict(a=9), (9, 1, 1, 1), THREAD, seed=16),
    # transposes, K = 1, the output scattered
    Case("T7", "ab->ba", dict(a=70, b=50), (3500, 1, 1, 1), THREAD, seed=17),
    # ... with a row table of two levels whose row_lo = 13 * 11 is no power of two
    Case("T8", "abc->cba", dict(a=13, b=11, c=37), (5291, 1, 1, 1), THREAD, row=(143, 37), seed=18),
    # K above the threshold under too many rows: a serial sum of 257 (tests/test_single_variant_plans.py checks that
    # a serial float32 fold of these rows stays inside the single-precision gate)
    Case("T9", "ak->a", dict(a=(1 << 14) + 16, k=257), ((1 << 14) + 16, 257, 257, 1), THREAD, seed=19),
    # (no row has k_hi_len > 1 on this kernel: a second level needs K > 4096, which under R > 2^14 is an operand of
    # 2^26 elements or more)
]

# Launches of several slices (gridDim.y = nz: the z offsets of A and C), each for one row of either kernel:
# a summed index sliced, an output index sliced, one of each, a sliced index under a diagonal, and the
# repeated label itself sliced (the tree accepts it: each slice is one element of the diagonal).
SLICED_CASES = [
    Case("S1w", "sab->b", dict(s=12, a=300, b=5), (5, 300, 300, 1), WAVE, sliced="s", seed=21),
    Case("S1t", "sab->b", dict(s=12, a=37, b=5), (5, 37, 37, 1), THREAD, sliced="s", seed=22),
    Case("S2w", "sab->sb", dict(s=12, a=300, b=5), (5, 300, 300, 1), WAVE, sliced="s", seed=23),
    Case("S2t", "sab->sb", dict(s=12, a=37, b=5), (5, 37, 37, 1), THREAD, sliced="s", seed=24),
    Case("S3w", "stab->tb", dict(s=5, t=3, a=300, b=5), (5, 300, 300, 1), WAVE, sliced="st", seed=25),
    Case("S3t", "stab->tb", dict(s=5, t=3, a=37, b=5), (5, 37, 37, 1), THREAD, sliced="st", seed=26),
    Case("S4w", "saab->sb", dict(s=6, a=300, b=5), (5, 300, 300, 1), WAVE, sliced="s", seed=27),
    Case("S4t", "saab->sb", dict(s=12, a=37, b=5), (5, 37, 37, 1), THREAD, sliced="s", seed=28),
    Case("S5t", "aab->b", dict(a=30, b=11), (11, 1, 1, 1), THREAD, sliced="a", seed=29),
]

UNSLICED_CASES = WAVE_CASES + THREAD_CASES
ALL_CASES = UNSLICED_CASES + SLICED_CASES

# The preprocessing of a leaf inside a two-input tree: the diagonal of the first leaf is taken, and summed over
# a = 300, by a single-term step of the wave form before the pair step runs.
LEAF_CASE = Case("L1", "aab,bc->c", dict(a=300, b=6, c=4), (6, 300, 300, 1), WAVE, seed=31)

# rows small enough for the gradient tests on the device (the issue's bound)
VJP_MAX_ELEMS = 1 << 16


def t_fast_ids(ns, nt):
    """The slice ids of a tree with a kept index t (extent ``nt``, the slow digit of the slice id) and a summed
    index s (``ns``, the fast digit) sliced, with t running fastest: consecutive slices never share a result
    element, and every result element still meets its slices in rising s (tests/test_gpu_slice_sum.py)."""
    return [t * ns + s for s in range(ns) for t in range(nt)]


def by_id(ident):
    return next(c for c in ALL_CASES + [LEAF_CASE] if c.id == ident)
