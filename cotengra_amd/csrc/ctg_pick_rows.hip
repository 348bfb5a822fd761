// ctg_pick_rows.hip -- the step of a row-sparse node below the root of a chained pick plan
// (cotengra_amd/plan.py: build_pick_rows_step).
//
//   C[rowC.hi[m] + rowC.lo[i] + nC[n]] = alpha * sum_k A[rowA.hi[m] + rowA.lo[i] + kA(k)]
//                                                      * B[rowB.hi[m] + rowB.lo[i] + kB(k) + nB[n]]
//   m < M (the rows of the node), i < row_lo, n < N;  R = M * row_lo
//
// Row m of the result is the product of one sub-tensor of each child: the `hi` level of the row tables holds the
// offsets of those sub-tensors (and of the result's row), the `lo` level and the n tables run over the dense legs.
// The rows are sorted by (rowA.hi, rowB.hi): consecutive rows share A.
//
//   pair_pick_rows_kernel<T, VEC>       vector form, all four dtypes: one output per lane.  A wave takes one row
//       and 64 of its row_lo * N outputs (i slow, n fast); a row of fewer outputs shares the wave with the rows
//       after it (64 / next power of two of them), so that a step of one output per row leaves no lane idle.  A
//       lane walks k in slots of VEC adjacent k (VEC = 2: one load of two elements where the host found both k
//       tables unit-stride and every other offset even), pick_rounds() slots in flight, and adds in slot order.
//       A lane that goes on to the next row of its run keeps its A values when that row has the same rowA.hi and
//       the contraction fits one round -- the same values, hence the same bits.
//   pair_pick_rows_mfma_kernel          matrix-core form, complex64: one wave per (row m, block of 32 i), n in
//       blocks of 32 (two tiles of 16 complex columns), v_mfma_f32_32x32x2_f32 with the complex product written as a
//       real one (one k per instruction); fragments are loaded straight through the tables, no LDS.
//
// No atomics, nothing shared between rows: the summation order of an output is a function of (K, VEC) in the
// vector form and of K in the matrix-core form -- not of the number of rows, of the row's place in the table, of
// the slice batch (gridDim.y) or of whether A was reused.
#include "ctg_common.h"

#include <cstdio>

namespace ctg {

namespace {

template <typename T>
struct alignas(2 * sizeof(T)) RowPair2 {
    T x, y;
};

// (as pair_pick_kernel: 64 bytes of each operand in flight per lane, no instantiation spills)
template <typename T, int VEC>
constexpr int pick_rows_rounds() { return sizeof(T) * VEC > 16 ? 2 : 4; }

typedef float pr_f32x16 __attribute__((ext_vector_type(16)));

}  // namespace

struct PickRowsShape {
    int ow_shift;     // log2 of the lanes a row has in a wave (64 >> ow_shift rows share it)
    int rps;          // rows a lane group takes one after the other (a performance parameter only)
    int64_t nblk;     // blocks of (1 << ow_shift) outputs per row
    int64_t M;        // rows
    int64_t P;        // outputs per row: row_lo * N
};

template <typename T, int VEC>
__global__ __launch_bounds__(256, 4) void pair_pick_rows_kernel(StepArgs p, PickRowsShape s) {
    constexpr int U = pick_rows_rounds<T, VEC>();
    const T* __restrict__ A = (const T*)p.A + zoffA(p);
    const T* __restrict__ B = (const T*)p.B + zoffB(p);
    T* __restrict__ C = (T*)p.C + zoffC(p);
    const double alpha = step_alpha(p);
    const int lane = threadIdx.x & 63;
    const int ow = 1 << s.ow_shift;
    const int G = 64 >> s.ow_shift;   // rows that share the wave
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t blk = w % s.nblk, rg = w / s.nblk;
    const int64_t o = blk * ow + (lane & (ow - 1));
    const bool in_row = o < s.P;
    const int64_t oc = in_row ? o : 0;
    const int64_t i = oc / p.N, n = oc - i * p.N;
    const int64_t la = p.rowA.lo[i], lb = p.rowB.lo[i] + p.nB[n], lc = p.rowC.lo[i] + p.nC[n];
    const int64_t slots = (p.K + VEC - 1) / VEC;
    const bool keep = slots <= U;

    T areg[U][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int v = 0; v < VEC; ++v) areg[u][v] = zero_of(T{});
    bool have = false;
    int64_t prev_a = 0;

    for (int t = 0; t < s.rps; ++t) {
        const int64_t m = (rg * G + (lane >> s.ow_shift)) * s.rps + t;
        const bool active = in_row && m < s.M;
        const int64_t mc = m < s.M ? m : s.M - 1;
        const int64_t ha = p.rowA.hi[mc];
        const bool same = keep && have && ha == prev_a;
        const T* __restrict__ a = A + ha + la;
        const T* __restrict__ b = B + p.rowB.hi[mc] + lb;
        T acc = zero_of(T{});
        for (int64_t r0 = 0; r0 < slots; r0 += U) {
            int64_t ia[U], ib[U];
            bool valid[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t j = r0 + u;
                valid[u] = active && j < slots;
                int64_t kh, kl;
                split_k(p, valid[u] ? j * VEC : 0, kh, kl);
                if constexpr (VEC == 2) {
                    // (the fast level of both k tables is unit-stride: kX.lo[kl] == kl, decided on the host)
                    ia[u] = p.kA.hi[kh] + kl;
                    ib[u] = p.kB.hi[kh] + kl;
                } else {
                    ia[u] = p.kA.hi[kh] + p.kA.lo[kl];
                    ib[u] = p.kB.hi[kh] + p.kB.lo[kl];
                }
            }
            T av[U][VEC], bv[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) av[u][v] = bv[u][v] = zero_of(T{});
                if (!valid[u]) continue;
                if constexpr (VEC == 2) {
                    const RowPair2<T> y = *(const RowPair2<T>*)(b + ib[u]);
                    bv[u][0] = y.x;
                    bv[u][VEC - 1] = y.y;
                    if (!same) {
                        const RowPair2<T> x = *(const RowPair2<T>*)(a + ia[u]);
                        av[u][0] = x.x;
                        av[u][VEC - 1] = x.y;
                    }
                } else {
                    bv[u][0] = b[ib[u]];
                    if (!same) av[u][0] = a[ia[u]];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    if (same) av[u][v] = areg[u][v];
                    else if (keep) areg[u][v] = av[u][v];
                    if (valid[u]) fma_acc(acc, av[u][v], bv[u][v]);
                }
            }
        }
        if (keep && active) {
            have = true;
            prev_a = ha;
        }
        if (active) C[p.rowC.hi[m] + lc] = scale_of(acc, alpha);
    }
}

// One wave per (row m, block of 32 positions i); blockIdx.x * 4 + wave = m * iblocks + iblock.
// The complex product as a real one on v_mfma_f32_32x32x2_f32 (D(32x32) += A'(32x2) B'(2x32)): row r of A' is
// (Re a, Im a) of position r at one k; column 2c of B' is (Re b, -Im b) and column 2c + 1 (Im b, Re b) of complex
// column c -- lane l supplies A'[l & 31][l >> 5] and B'[l >> 5][l & 31] -- so that D[r][2c] / D[r][2c + 1] are the
// real / imaginary part of C[r][c].  A tile is 32 positions by 16 complex columns; a wave carries two tiles.
__global__ __launch_bounds__(256, 2) void pair_pick_rows_mfma_kernel(StepArgs p, int64_t M, int64_t iblocks) {
    const float* __restrict__ A = (const float*)p.A + 2 * zoffA_s(p);
    const float* __restrict__ B = (const float*)p.B + 2 * zoffB_s(p);
    float2* __restrict__ C = (float2*)p.C + zoffC_s(p);
    const float alpha = (float)step_alpha(p);
    const int lane = threadIdx.x & 63;
    const int64_t w = uniform64((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= M * iblocks) return;
    const int64_t m = w / iblocks, i0 = (w - m * iblocks) * 32;
    const int half = lane >> 5, l32 = lane & 31;
    // A': position i0 + l32 (clamped: the rows past row_lo are computed and not stored), component `half`
    const int64_t ia = i0 + l32 < p.row_lo ? i0 + l32 : p.row_lo - 1;
    const float* __restrict__ a = A + 2 * (sload64(p.rowA.hi + m) + p.rowA.lo[ia]) + half;
    // B': complex column l32 >> 1 of a tile; (row 0: Re, Im), (row 1: -Im, Re)
    const int bcomp = (l32 & 1) ^ half;
    const float bsign = (half == 1 && (l32 & 1) == 0) ? -1.f : 1.f;
    const float* __restrict__ b = B + 2 * sload64(p.rowB.hi + m) + bcomp;
    const int64_t hc = sload64(p.rowC.hi + m);
    const bool odd = lane & 1;

    for (int64_t n0 = 0; n0 < p.N; n0 += 32) {
        const int64_t na = n0 + (l32 >> 1), nb = na + 16;
        const int64_t ob0 = 2 * p.nB[na < p.N ? na : p.N - 1], ob1 = 2 * p.nB[nb < p.N ? nb : p.N - 1];
        const bool two = n0 + 16 < p.N;   // (uniform: the second tile has columns)
        pr_f32x16 acc0, acc1;
#pragma unroll
        for (int t = 0; t < 16; ++t) acc0[t] = acc1[t] = 0.f;
        for (int64_t k0 = 0; k0 < p.K; k0 += 4) {
            float av[4], b0[4], b1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t k = k0 + u < p.K ? k0 + u : p.K - 1;
                int64_t kh, kl;
                split_k(p, k, kh, kl);
                const int64_t ka = 2 * (sload64(p.kA.hi + kh) + sload64(p.kA.lo + kl));
                const int64_t kb = 2 * (sload64(p.kB.hi + kh) + sload64(p.kB.lo + kl));
                av[u] = a[ka];
                b0[u] = b[kb + ob0];
                b1[u] = two ? b[kb + ob1] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (k0 + u < p.K) {   // (uniform)
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], b0[u] * bsign, acc0, 0, 0, 0);
                    if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], b1[u] * bsign, acc1, 0, 0, 0);
                }
            }
        }
        // D: register t of lane l is row 8 * (t >> 2) + 4 * (l >> 5) + (t & 3), column l & 31.  pair_rows gives the
        // even lane the complex number of the first row of a register pair, the odd lane that of the second.
#pragma unroll
        for (int t = 0; t < 16; t += 2) {
            const int64_t row = i0 + 8 * (t >> 2) + 4 * half + (t & 3) + (odd ? 1 : 0);
            const float2 v0 = pair_rows(acc0[t], acc0[t + 1], odd, alpha);
            const float2 v1 = pair_rows(acc1[t], acc1[t + 1], odd, alpha);
            if (row < p.row_lo) {
                const int64_t rc = hc + p.rowC.lo[row];
                if (na < p.N) C[rc + p.nC[na]] = v0;
                if (nb < p.N) C[rc + p.nC[nb]] = v1;
            }
        }
    }
}

namespace {

PickRowsShape pick_rows_shape(const StepArgs& p) {
    PickRowsShape s;
    s.M = p.R / p.row_lo;
    s.P = p.row_lo * p.N;
    s.ow_shift = 0;
    while (s.ow_shift < 6 && (1ll << s.ow_shift) < s.P) ++s.ow_shift;
    const int64_t ow = 1ll << s.ow_shift, G = 64 / ow;
    s.nblk = (s.P + ow - 1) / ow;
    const int64_t waves = (s.M + G - 1) / G * s.nblk;
    // (enough waves to fill the chip four times over, as pick_shape: a lane group walks four consecutive rows,
    // and those of one A sub-tensor share its registers)
    s.rps = waves >= 4 * 4096 ? 4 : 1;
    return s;
}

int64_t pick_rows_waves(const PickRowsShape& s) {
    const int64_t per_wave = (int64_t)(64 >> s.ow_shift) * s.rps;
    return (s.M + per_wave - 1) / per_wave * s.nblk;
}

template <typename T>
hipError_t launch_pick_rows_t(const StepArgs& p, int vec, hipStream_t stream) {
    const PickRowsShape s = pick_rows_shape(p);
    const int64_t blocks = (pick_rows_waves(s) + 3) / 4;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)(p.nz < 1 ? 1 : p.nz));
    if (vec)
        hipLaunchKernelGGL((pair_pick_rows_kernel<T, 2>), grid, dim3(256), 0, stream, p, s);
    else
        hipLaunchKernelGGL((pair_pick_rows_kernel<T, 1>), grid, dim3(256), 0, stream, p, s);
    return hipGetLastError();
}

bool pick_rows_mfma(int dtype, const StepArgs& p, int b_fixed) {
    return b_fixed && pick_rows_route_mfma(p.row_lo, p.K, p.N, dtype);
}

}  // namespace

hipError_t launch_pair_pick_rows(int dtype, const StepArgs& p, int vec, int b_fixed, hipStream_t stream) {
    if (p.Bt != 1 || p.row_lo < 1 || p.R % p.row_lo) return hipErrorInvalidValue;
    if (pick_rows_mfma(dtype, p, b_fixed)) {
        const int64_t M = p.R / p.row_lo, iblocks = (p.row_lo + 31) / 32;
        const int64_t blocks = (M * iblocks + 3) / 4;
        if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
        const dim3 grid((unsigned)blocks, (unsigned)(p.nz < 1 ? 1 : p.nz));
        hipLaunchKernelGGL(pair_pick_rows_mfma_kernel, grid, dim3(256), 0, stream, p, M, iblocks);
        return hipGetLastError();
    }
    switch (dtype) {
        case 0: return launch_pick_rows_t<float>(p, vec, stream);
        case 1: return launch_pick_rows_t<double>(p, vec, stream);
        case 2: return launch_pick_rows_t<c64>(p, vec, stream);
        case 3: return launch_pick_rows_t<c128>(p, vec, stream);
    }
    return hipErrorInvalidValue;
}

void pair_pick_rows_name(int dtype, const StepArgs& p, int vec, int b_fixed, char* buf, size_t n) {
    if (pick_rows_mfma(dtype, p, b_fixed)) {
        snprintf(buf, n, "pair_pick_rows_mfma_kernel<c64>");
        return;
    }
    static const char* const names[4] = {"float", "double", "c64", "c128"};
    snprintf(buf, n, "pair_pick_rows_kernel<%s,%d>", names[dtype & 3], vec ? 2 : 1);
}

}  // namespace ctg
