// ctg_rdm_wide.hip -- reduced density matrices of 65 .. CTG_RDM_WIDE_MAX_DIM rows of the executor's result tensor on
// the device (ctg_exec_result_rdm_wide and ctg_rdm_wide_plan of include/ctg_hip.h):
//
//   rho[a, b] = sum over r of x[a, r] * conj(x[b, r])
//
// as ctg_rdm.hip defines it for D <= CTG_RDM_MAX_DIM: a, b over the kept axes, r over all others (t = result_elems / D),
// every product and sum in fp64, every association a function of (dtype, extents, keep) alone, no atomics.  Here the
// matrix does not fit one workgroup's registers: a Hermitian rank-t update rho = X X^H tiled over the blocks of the
// lower triangle and split along r.  The axes are split as for a marginal (marginal_plan).  Two routes:
//
//   power of two (every extent a power of two, at least 4096 elements): a is the bit-extract of the flat index under
//   the keep mask K, r the one under its complement R.  The lowest 6 bits of a (Klo) are the row inside a panel of
//   EDGE = 64 rows, the others (Khi) number the panels; block (bi, bj <= bi) is panel bi times panel bj, numbered
//   bi (bi + 1) / 2 + bj.  A chunk is kWideCols = 32 consecutive values of r (the lowest 5 bits of R: Rlo; fewer when
//   t < 32) for the 64 rows of a panel: 2048 elements, which lie in runs of at least 32 consecutive ones (of the
//   lowest 5 bits of the flat index at most 5 are row bits and at most 5 column bits: all are chunk bits).
//
//     rdm_wide_kernel<T, 64>   workgroup (block, split) takes the chunks split * cps .. (split + 1) * cps - 1 in
//                              ascending order: 16-byte loads along the runs of its one (bi == bj) or two panels into
//                              registers (the next chunk's are in flight while this one is multiplied), widened to
//                              fp64 into LDS as X[plane][panel][row][col] (planes Re, Im; row stride 34 doubles, the
//                              bank-pair argument of ctg_rdm.hip), then v_mfma_f64_16x16x4_f64.  Wave w owns the
//                              tiles (w, 0 .. 3) of the block -- (w, 0 .. w) of a diagonal block -- over all columns:
//                              16 x 64 entries, 32 (real) or 64 (complex) accumulator registers kept across chunks,
//                              no sum across waves.  Columns past t (t < 32) are zeros written once.
//     rdm_wide_finish_kernel   adds the partials of a block split-ascending; writes b <= a, the conjugate half and
//                              the zero imaginary diagonal.
//
//   Why 64 x 64 and not 128 x 128: a 64-row block multiplies 64 flops per byte of complex64 it reads (32 for
//   complex128), above the machine's fp64-matrix-to-HBM ratio (78.6 TFLOP/s over 8 TB/s: 10), and needs 64 accumulator
//   registers per lane; 128 x 128 needs 256 (all AGPRs) and 136 KiB of LDS at 32 columns: one workgroup per CU and no
//   second one to hide the widen-and-store phase.  The panels a 64-row plan re-reads (D / 64 + 1 times the tensor)
//   come from L2 / MALL for all but the largest cases; DESIGN.md section 20 says which.
//
//   splits doubles while blocks * splits < 512 (two workgroups per CU) and every split keeps at least 32 chunks (a
//   workgroup's partial, 64 KiB complex, is at most a sixteenth of the complex64 it read); so with splits > 1 there are
//   fewer than 1024 partials: 64 MiB.
//
//   general (any other shape): rdm_wide_general_kernel<T>, one work item per (pair a >= b, chunk of complement
//   positions), pair = a (a + 1) / 2 + b, walks its chunk serially with the mixed-radix decode of marg_general_kernel;
//   rdm_wide_general_finish_kernel adds the chunks in ascending order.  chunk = max(1024, ceil(t / 1024)) positions,
//   grown until the per-chunk sums fit 64 MiB (one chunk from D = 2897 on for complex plans).  Not tuned.
//
//   purity = sum |rho[a, b]|^2 over the finished matrix: rdm_wide_purity_kernel sums pieces of 4096 entries (a lane
//   its 16 in ascending order, then a tree over the 256 lanes), rdm_wide_purity_sum_kernel the pieces likewise.
#include <algorithm>

#include "ctg_result_elem.h"
#include "ctg_result_host.h"

namespace ctg {

constexpr int kWideEdge = 64;                          // rows of a panel
constexpr int kWideColBits = 5;
constexpr int kWideCols = 1 << kWideColBits;           // columns of a chunk
constexpr int kWideChunkBits = 6 + kWideColBits;
constexpr int kWideChunk = 1 << kWideChunkBits;        // elements of a panel's chunk
constexpr int kWideGrid = 512;                         // workgroups the splits aim at: two per CU
constexpr int64_t kWideMinChunks = 32;                 // chunks of a split, at least
constexpr int64_t kWidePartBytes = 64ll << 20;         // bound of the partials (splits > 1) / per-chunk sums (general)
constexpr int kWidePiece = 4096;                       // entries of rho per workgroup of the purity sum
constexpr int64_t kWideGeneralChunk = 1024;            // complement positions per work item of the general route, at least
constexpr int64_t kWideGeneralMaxChunks = 1024;        // ... and at most this many chunks per pair

// planes (Re | Re, Im) of an element type and its components widened to fp64
template <typename T> struct WideElem;
template <> struct WideElem<float> {
    static constexpr int P = 1;
    static __device__ __forceinline__ double re(float v) { return (double)v; }
    static __device__ __forceinline__ double im(float) { return 0.0; }
};
template <> struct WideElem<double> {
    static constexpr int P = 1;
    static __device__ __forceinline__ double re(double v) { return v; }
    static __device__ __forceinline__ double im(double) { return 0.0; }
};
template <> struct WideElem<float2> {
    static constexpr int P = 2;
    static __device__ __forceinline__ double re(float2 v) { return (double)v.x; }
    static __device__ __forceinline__ double im(float2 v) { return (double)v.y; }
};
template <> struct WideElem<double2> {
    static constexpr int P = 2;
    static __device__ __forceinline__ double re(double2 v) { return v.x; }
    static __device__ __forceinline__ double im(double2 v) { return v.y; }
};

typedef double wide_f64x4 __attribute__((ext_vector_type(4)));

// Element e of a panel's chunk (bit i of e): gpos[i] is what the bit adds to the flat index, lw[i] what it adds to the
// element's place in the panel's LDS plane (row * LD or column).  The bits are those of the flat index under Klo | Rlo,
// lowest first: consecutive e are consecutive elements.  Bits at or above log2(nelem) are never set.
struct WideBits {
    int64_t gpos[kWideChunkBits];
    int32_t lw[kWideChunkBits];
};

__device__ __forceinline__ int64_t wide_goff(uint32_t e, const WideBits& b) {
    int64_t r = 0;
#pragma unroll
    for (int i = 0; i < kWideChunkBits; ++i) r += ((e >> i) & 1u) ? b.gpos[i] : 0;
    return r;
}
__device__ __forceinline__ int wide_loff(uint32_t e, const WideBits& b) {
    int r = 0;
#pragma unroll
    for (int i = 0; i < kWideChunkBits; ++i) r += ((e >> i) & 1u) ? b.lw[i] : 0;
    return r;
}

// (bi, bj <= bi) of block blk = bi (bi + 1) / 2 + bj; at most 64 panels
__device__ __forceinline__ void wide_block(int blk, int& bi, int& bj) {
    bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= blk) ++bi;
    bj = blk - bi * (bi + 1) / 2;
}

// part[((blk * splits + split) * P + p) * EDGE * EDGE + i * EDGE + j]: the split's share of rho[64 bi + i, 64 bj + j]
// (a diagonal block: the tiles with 16-row strip >= 16-column strip only; the others are not written)
template <typename T, int EDGE>
__global__ __launch_bounds__(kSampleThreads, 2) void rdm_wide_kernel(const T* __restrict__ x, int64_t n, int vec, WideBits bits,
                                                                     int nelem, int64_t khi, int64_t rhi, int splits,
                                                                     int64_t cps, double* __restrict__ part) {
    static_assert(EDGE == kWideEdge && kSampleThreads / 64 * 16 == EDGE, "a wave owns one 16-row strip of the block");
    constexpr int P = WideElem<T>::P;
    constexpr int V = 16 / sizeof(T);
    constexpr int G = kWideChunk / V / kSampleThreads;
    constexpr int TC = kWideCols, LD = TC + 2, PANEL = EDGE * LD, PLANE = 2 * PANEL;
    __shared__ __attribute__((aligned(16))) double xs[P * PLANE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x / splits, split = blockIdx.x % splits;
    int bi, bj;
    wide_block(blk, bi, bj);
    const bool diag = bi == bj;
    const int64_t pbase[2] = {deposit_bits(bi, khi), deposit_bits(bj, khi)};
    // element (g * kSampleThreads + tid) * V of a panel's chunk: this thread's share of its offsets
    const int64_t goff_t = wide_goff((uint32_t)tid * V, bits);
    const int loff_t = wide_loff((uint32_t)tid * V, bits);

    if (nelem < kWideChunk)   // (t < 32: the columns past t stay zero)
        for (int o = tid; o < P * PLANE; o += kSampleThreads) xs[o] = 0.0;

    wide_f64x4 acc[4][P];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int p = 0; p < P; ++p) acc[j][p] = wide_f64x4{0.0, 0.0, 0.0, 0.0};

    T st[2][G][V];
    auto fetch = [&](int64_t q) {
        const int64_t base = deposit_bits(q, rhi) + goff_t;
#pragma unroll
        for (int pn = 0; pn < 2; ++pn) {
            if (pn == 1 && diag) continue;
#pragma unroll
            for (int g = 0; g < G; ++g)
                if ((g * kSampleThreads + tid) * V < nelem)
                    load_group<T>(x, base + pbase[pn] + wide_goff((uint32_t)(g * kSampleThreads) * V, bits), n, vec != 0,
                                  st[pn][g]);
        }
    };

    // fragment coordinates of v_mfma_f64_16x16x4_f64: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15]
    const int r16 = lane & 15, k4 = lane >> 4;
    const int arow = (16 * wave + r16) * LD, bpan = diag ? 0 : PANEL;
    const int64_t q0 = (int64_t)split * cps, q1 = q0 + cps;
    fetch(q0);
    for (int64_t q = q0; q < q1; ++q) {
        __syncthreads();   // (the multiplications of the chunk before have read the planes; the zeros are written)
#pragma unroll
        for (int pn = 0; pn < 2; ++pn) {
            if (pn == 1 && diag) continue;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if ((g * kSampleThreads + tid) * V >= nelem) continue;
                const int o = pn * PANEL + loff_t + wide_loff((uint32_t)(g * kSampleThreads) * V, bits);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int ok = o + wide_loff((uint32_t)k, bits);
                    xs[ok] = WideElem<T>::re(st[pn][g][k]);
                    if (P == 2) xs[PLANE + ok] = WideElem<T>::im(st[pn][g][k]);
                }
            }
        }
        __syncthreads();
        if (q + 1 < q1) fetch(q + 1);
        // columns kb + 2 k4, kb + 2 k4 + 1: one 16-byte read feeds two MFMA steps (which four columns share a step is
        // free, as long as A and B agree)
#pragma unroll 2
        for (int kb = 0; kb < TC; kb += 8) {
            double2 fa[P], fb[4][P];
#pragma unroll
            for (int p = 0; p < P; ++p) fa[p] = *reinterpret_cast<const double2*>(&xs[p * PLANE + arow + kb + 2 * k4]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (diag && j > wave) continue;
#pragma unroll
                for (int p = 0; p < P; ++p)
                    fb[j][p] = *reinterpret_cast<const double2*>(&xs[p * PLANE + bpan + (16 * j + r16) * LD + kb + 2 * k4]);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (diag && j > wave) continue;
                    const double ar = h ? fa[0].y : fa[0].x, br = h ? fb[j][0].y : fb[j][0].x;
                    acc[j][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, acc[j][0], 0, 0, 0);
                    if (P == 2) {
                        const double ai = h ? fa[P - 1].y : fa[P - 1].x, bim = h ? fb[j][P - 1].y : fb[j][P - 1].x;
                        acc[j][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bim, acc[j][0], 0, 0, 0);
                        acc[j][P - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, acc[j][P - 1], 0, 0, 0);
                        acc[j][P - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, -bim, acc[j][P - 1], 0, 0, 0);
                    }
                }
            }
        }
    }
    // C/D: col = lane & 15, row = (lane >> 4) + 4 * reg
    double* mine = part + (int64_t)blockIdx.x * (P * EDGE * EDGE);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (diag && j > wave) continue;
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i) mine[p * EDGE * EDGE + (16 * wave + k4 + 4 * i) * EDGE + 16 * j + r16] = acc[j][p][i];
    }
}

// out[a][b], out[b][a] for b <= a: work item (blk, i, j) adds the splits' partials in ascending order
template <int P, int EDGE>
__global__ __launch_bounds__(kSampleThreads) void rdm_wide_finish_kernel(const double* __restrict__ part, int D, int splits,
                                                                         double* __restrict__ out) {
    const int blk = blockIdx.x / (EDGE * EDGE / kSampleThreads);
    const int ij = (blockIdx.x % (EDGE * EDGE / kSampleThreads)) * kSampleThreads + threadIdx.x;
    int bi, bj;
    wide_block(blk, bi, bj);
    const int64_t a = (int64_t)EDGE * bi + ij / EDGE, b = (int64_t)EDGE * bj + ij % EDGE;
    if (b > a) return;
    double v[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const double* src = part + ((int64_t)blk * splits * P + p) * (EDGE * EDGE) + ij;
        double w = src[0];
        for (int s = 1; s < splits; ++s) w += src[(int64_t)s * P * (EDGE * EDGE)];
        v[p] = w;
    }
    if (P == 1) {
        out[a * D + b] = v[0];
        out[b * D + a] = v[0];
    } else {
        double2* o2 = reinterpret_cast<double2*>(out);
        if (a == b) {
            o2[a * D + a] = double2{v[0], 0.0};
        } else {
            o2[a * D + b] = double2{v[0], v[P - 1]};
            o2[b * D + a] = double2{v[0], -v[P - 1]};
        }
    }
}

// (a, b <= a) of pair = a (a + 1) / 2 + b
__device__ __forceinline__ void wide_pair(int64_t pair, int64_t& a, int64_t& b) {
    a = (int64_t)((sqrt(8.0 * (double)pair + 1.0) - 1.0) * 0.5);
    while (a * (a + 1) / 2 > pair) --a;
    while ((a + 1) * (a + 2) / 2 <= pair) ++a;
    b = pair - a * (a + 1) / 2;
}

// Work item (pair, chunk ch): B[(ch npairs + pair) P + p] <- sum of x[a, c] conj(x[b, c]) over the complement
// positions c of the chunk, serially
template <typename T>
__global__ __launch_bounds__(kSampleThreads) void rdm_wide_general_kernel(const T* __restrict__ x, MargAxes ax, int64_t npairs,
                                                                          int64_t rc, int64_t chunk, int64_t total,
                                                                          double* __restrict__ B) {
#pragma clang fp contract(off)
    constexpr int P = WideElem<T>::P;
    const int64_t g = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
    if (g >= total) return;
    const int64_t pair = g % npairs, ch = g / npairs;
    int64_t a, b;
    wide_pair(pair, a, b);
    int64_t offa = 0, offb = 0, ta = a, tb = b;
    for (int k = ax.nk - 1; k >= 0; --k) {
        offa += (ta % ax.kext[k]) * ax.kstr[k];
        offb += (tb % ax.kext[k]) * ax.kstr[k];
        ta /= ax.kext[k];
        tb /= ax.kext[k];
    }
    const int64_t c0 = ch * chunk, c1 = c0 + chunk < rc ? c0 + chunk : rc;
    double sr = 0.0, si = 0.0;
    for (int64_t c = c0; c < c1; ++c) {
        int64_t o = 0, t = c;
        for (int k = ax.nd - 1; k >= 0; --k) {
            o += (t % ax.dext[k]) * ax.dstr[k];
            t /= ax.dext[k];
        }
        const T xa = x[offa + o], xb = x[offb + o];
        const double ar = WideElem<T>::re(xa), br = WideElem<T>::re(xb);
        double pr = ar * br, pi = 0.0;
        if (P == 2) {
            const double ai = WideElem<T>::im(xa), bim = WideElem<T>::im(xb);
            const double q = ai * bim, u = ai * br, w = ar * bim;
            pr = pr + q;
            pi = u - w;
        }
        sr = c == c0 ? pr : sr + pr;
        si = c == c0 ? pi : si + pi;
    }
    B[g * P] = sr;
    if (P == 2) B[g * P + P - 1] = si;
}

template <int P>
__global__ __launch_bounds__(kSampleThreads) void rdm_wide_general_finish_kernel(const double* __restrict__ B, int D,
                                                                                 int64_t npairs, int64_t nch,
                                                                                 double* __restrict__ out) {
    const int64_t pair = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
    if (pair >= npairs) return;
    int64_t a, b;
    wide_pair(pair, a, b);
    double v[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        double w = B[pair * P + p];
        for (int64_t ch = 1; ch < nch; ++ch) w += B[(ch * npairs + pair) * P + p];
        v[p] = w;
    }
    if (P == 1) {
        out[a * D + b] = v[0];
        out[b * D + a] = v[0];
    } else {
        double2* o2 = reinterpret_cast<double2*>(out);
        if (a == b) {
            o2[a * D + a] = double2{v[0], 0.0};
        } else {
            o2[a * D + b] = double2{v[0], v[P - 1]};
            o2[b * D + a] = double2{v[0], -v[P - 1]};
        }
    }
}

// the 256 lanes' values added as a tree: lane l += lane l + h for h = 128, 64, ..., 1; lane 0 returns the sum
__device__ __forceinline__ double wide_tree(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int h = kSampleThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + h];
        __syncthreads();
    }
    return sh[0];
}

// pp[wg] <- sum of |rho[e]|^2 over the entries e of piece wg: lane l takes e = 4096 wg + 256 k + l, k ascending
template <int P>
__global__ __launch_bounds__(kSampleThreads) void rdm_wide_purity_kernel(const double* __restrict__ rho, int64_t total,
                                                                         double* __restrict__ pp) {
#pragma clang fp contract(off)
    __shared__ double sh[kSampleThreads];
    double s = 0.0;
    for (int k = 0; k < kWidePiece / kSampleThreads; ++k) {
        const int64_t e = (int64_t)blockIdx.x * kWidePiece + k * kSampleThreads + threadIdx.x;
        if (e >= total) break;
        double m = rho[e * P] * rho[e * P];
        if (P == 2) {
            const double mi = rho[e * P + P - 1] * rho[e * P + P - 1];
            m = m + mi;
        }
        s = s + m;
    }
    const double r = wide_tree(s, sh);
    if (threadIdx.x == 0) pp[blockIdx.x] = r;
}

// *out <- the np pieces: lane l takes pp[l], pp[l + 256], ... in ascending order, then the tree
__global__ __launch_bounds__(kSampleThreads) void rdm_wide_purity_sum_kernel(const double* __restrict__ pp, int np,
                                                                             double* __restrict__ out) {
    __shared__ double sh[kSampleThreads];
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += kSampleThreads) s = s + pp[i];
    const double r = wide_tree(s, sh);
    if (threadIdx.x == 0) *out = r;
}

}  // namespace ctg

using namespace ctg;

namespace {

int wide_popcount(int64_t v) { return __builtin_popcountll((unsigned long long)v); }

// the lowest `k` set bits of mask
int64_t wide_lowest_bits(int64_t mask, int k) {
    int64_t r = 0;
    for (; k > 0 && mask; --k) {
        r |= mask & (0 - mask);
        mask &= mask - 1;
    }
    return r;
}

// What the host decides: everything a function of (dtype, extents, keep) alone.  The first CTG_RDM_WIDE_PLAN_WORDS
// members are the words of ctg_rdm_wide_plan, in its order.
struct WidePlan {
    int64_t route = 0;      // 0: power of two, 1: general
    int64_t D = 0;
    int64_t edge = 0;       // rows of a panel (general: 1, a block is one pair)
    int64_t panels = 0;
    int64_t blocks = 0;     // of the lower triangle
    int64_t splits = 1;     // along r (general: the chunks)
    int64_t cols = 0;       // values of r in a chunk
    int64_t chunks = 0;     // chunks along r; split s takes chunks s * chunks / splits .. (s + 1) * chunks / splits - 1
    int64_t grid = 0;       // workgroups of the tile kernel (general: work items, 256 to a workgroup)
    int64_t scratch = 0;    // bytes of the executor's scratch the call lays out
    int64_t code = 0;       // 4 * route + dtype: "rdm_wide_kernel<T,64>" | "rdm_wide_general_kernel<T>"
    // (not words)
    int P = 1;
    int64_t pieces = 0;     // of the purity sum
    WideBits bits{};
    int nelem = 0;
    int64_t khi = 0, rhi = 0;
};

int64_t wide_layout(const WidePlan& wp, void* base, double** d_out, double** part, double** pp, double** pur) {
    Carve c(base);
    *d_out = c.take<double>(wp.D * wp.D * wp.P * 8);
    *part = c.take<double>(wp.route == 0 ? wp.grid * kWideEdge * kWideEdge * wp.P * 8 : wp.blocks * wp.splits * wp.P * 8);
    *pp = c.take<double>(wp.pieces * 8);
    *pur = c.take<double>(8);
    return c.bytes();
}

void wide_plan(int dtype, const MarginalPlan& mp, WidePlan* out) {
    WidePlan wp;
    wp.P = (dtype == CTG_C64 || dtype == CTG_C128) ? 2 : 1;
    wp.D = mp.m;
    wp.route = mp.fast ? 0 : 1;
    wp.code = 4 * wp.route + dtype;
    wp.pieces = (wp.D * wp.D + kWidePiece - 1) / kWidePiece;
    if (mp.fast) {
        const int64_t K = mp.mask, R = (mp.n - 1) & ~K;
        const int64_t Klo = wide_lowest_bits(K, 6), Rlo = wide_lowest_bits(R, kWideColBits);
        const int c = wide_popcount(Rlo);
        wp.khi = K & ~Klo;
        wp.rhi = R & ~Rlo;
        wp.edge = kWideEdge;
        wp.cols = 1ll << c;
        wp.nelem = kWideEdge << c;
        wp.chunks = 1ll << wide_popcount(wp.rhi);
        wp.panels = wp.D / kWideEdge;
        wp.blocks = wp.panels * (wp.panels + 1) / 2;
        while (wp.blocks * wp.splits < kWideGrid && 2 * wp.splits * kWideMinChunks <= wp.chunks) wp.splits *= 2;
        wp.grid = wp.blocks * wp.splits;
        const int64_t M = Klo | Rlo;
        int i = 0;
        for (int b = 0; b < 63; ++b) {
            if (!((M >> b) & 1)) continue;
            const int64_t below = ((int64_t)1 << b) - 1;
            wp.bits.gpos[i] = (int64_t)1 << b;
            wp.bits.lw[i] = ((Klo >> b) & 1) ? (kWideCols + 2) << wide_popcount(Klo & below) : 1 << wide_popcount(Rlo & below);
            ++i;
        }
    } else {
        wp.edge = 1;
        wp.panels = wp.D;
        wp.blocks = wp.D * (wp.D + 1) / 2;
        int64_t chunk = std::max<int64_t>(kWideGeneralChunk, (mp.rc + kWideGeneralMaxChunks - 1) / kWideGeneralMaxChunks);
        const int64_t cap = std::max<int64_t>(1, kWidePartBytes / (wp.blocks * wp.P * 8));
        if ((mp.rc + chunk - 1) / chunk > cap) chunk = (mp.rc + cap - 1) / cap;
        wp.cols = chunk;
        wp.chunks = (mp.rc + chunk - 1) / chunk;
        wp.splits = wp.chunks;
        wp.grid = wp.blocks * wp.splits;
    }
    double *a, *b, *c, *d;
    wp.scratch = wide_layout(wp, nullptr, &a, &b, &c, &d);
    *out = wp;
}

// the refusals ctg_rdm_wide_plan and ctg_exec_result_rdm_wide share; nothing is allocated or launched before it
int wide_prologue(int dtype, int64_t rank, const int64_t* extents, const int32_t* keep, int64_t result_elems, MarginalPlan* mp,
                  WidePlan* wp) {
    const char* why = "";
    if (marginal_plan(rank, extents, keep, result_elems, mp, &why) != CTG_OK) return result_fail(CTG_E_INVALID, "rdm_wide: %s", why);
    if (mp->m <= CTG_RDM_MAX_DIM)
        return result_fail(CTG_E_INVALID,
                           "rdm_wide: the kept extents' product is %lld; up to CTG_RDM_MAX_DIM = %d it is ctg_exec_result_rdm that "
                           "computes the matrix",
                           (long long)mp->m, CTG_RDM_MAX_DIM);
    if (mp->m > CTG_RDM_WIDE_MAX_DIM)
        return result_fail(CTG_E_INVALID, "rdm_wide: the kept extents' product is %lld; at most CTG_RDM_WIDE_MAX_DIM = %d",
                           (long long)mp->m, CTG_RDM_WIDE_MAX_DIM);
    wide_plan(dtype, *mp, wp);
    return CTG_OK;
}

template <typename T>
int wide_run(ctg_exec* e, const MarginalPlan& mp, const WidePlan& wp, double* part, double* out) {
    constexpr int P = WideElem<T>::P;
    hipStream_t st = e->stream;
    const int D = (int)wp.D;
    if (wp.route == 0) {
        const int vec = ((uintptr_t)e->d_result & 15) == 0 ? 1 : 0;
        rdm_wide_kernel<T, kWideEdge><<<dim3((unsigned)wp.grid), dim3(kSampleThreads), 0, st>>>(
            (const T*)e->d_result, mp.n, vec, wp.bits, wp.nelem, wp.khi, wp.rhi, (int)wp.splits, wp.chunks / wp.splits, part);
        LAUNCH_CHECK("rdm_wide_kernel");
        rdm_wide_finish_kernel<P, kWideEdge>
            <<<dim3((unsigned)(wp.blocks * (kWideEdge * kWideEdge / kSampleThreads))), dim3(kSampleThreads), 0, st>>>(
                part, D, (int)wp.splits, out);
        LAUNCH_CHECK("rdm_wide_finish_kernel");
    } else {
        rdm_wide_general_kernel<T><<<dim3((unsigned)((wp.grid + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(
            (const T*)e->d_result, mp.ax, wp.blocks, mp.rc, wp.cols, wp.grid, part);
        LAUNCH_CHECK("rdm_wide_general_kernel");
        rdm_wide_general_finish_kernel<P>
            <<<dim3((unsigned)((wp.blocks + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(
                part, D, wp.blocks, wp.chunks, out);
        LAUNCH_CHECK("rdm_wide_general_finish_kernel");
    }
    return CTG_OK;
}

template <int P>
int wide_purity(ctg_exec* e, const WidePlan& wp, const double* rho, double* pp, double* pur) {
    rdm_wide_purity_kernel<P><<<dim3((unsigned)wp.pieces), dim3(kSampleThreads), 0, e->stream>>>(rho, wp.D * wp.D, pp);
    LAUNCH_CHECK("rdm_wide_purity_kernel");
    rdm_wide_purity_sum_kernel<<<dim3(1), dim3(kSampleThreads), 0, e->stream>>>(pp, (int)wp.pieces, pur);
    LAUNCH_CHECK("rdm_wide_purity_sum_kernel");
    return CTG_OK;
}

}  // namespace

extern "C" int ctg_rdm_wide_plan(int32_t dtype, int64_t rank, const int64_t* extents, const int32_t* keep, int64_t* words) {
    if (!words) return result_fail(CTG_E_INVALID, "null argument");
    if (dtype < CTG_F32 || dtype > CTG_C128) return result_fail(CTG_E_INVALID, "rdm_wide: dtype code %d", (int)dtype);
    // the product of the extents stands for result_elems (one that result_shape refuses is refused by it)
    int64_t n = 1;
    for (int64_t a = 0; a < rank && extents; ++a) {
        if (extents[a] < 1 || extents[a] > kReduceMaxElems / n) break;
        n *= extents[a];
    }
    MarginalPlan mp;
    WidePlan wp;
    const int rc = wide_prologue(dtype, rank, extents, keep, n, &mp, &wp);
    if (rc != CTG_OK) return rc;
    const int64_t w[CTG_RDM_WIDE_PLAN_WORDS] = {wp.route,  wp.D,      wp.edge, wp.panels,  wp.blocks, wp.splits,
                                                wp.cols,   wp.chunks, wp.grid, wp.scratch, wp.code};
    memcpy(words, w, sizeof(w));
    return CTG_OK;
}

extern "C" int ctg_exec_result_rdm_wide(ctg_exec* e, int64_t rank, const int64_t* extents, const int32_t* keep, void* out,
                                        double* purity) {
    if (!e) return result_fail(CTG_E_INVALID, "null argument");
    if (!out && !purity) return result_fail(CTG_E_INVALID, "rdm_wide: out and purity are both null");
    MarginalPlan mp;
    WidePlan wp;
    const int dtype = e->plan->dtype;
    int rc = wide_prologue(dtype, rank, extents, keep, e->plan->result_elems, &mp, &wp);
    if (rc != CTG_OK) return rc;
    rc = result_norm_finite(e, "no reduced density matrix of it");
    if (rc != CTG_OK) return rc;
    rc = reduce_reserve(e, wp.scratch);
    if (rc != CTG_OK) return rc;
    double *d_out = nullptr, *part = nullptr, *pp = nullptr, *pur = nullptr;
    wide_layout(wp, e->d_reduce, &d_out, &part, &pp, &pur);
    rc = dispatch_elem(dtype, [&](auto t) { return wide_run<decltype(t)>(e, mp, wp, part, d_out); });
    if (rc != CTG_OK) return rc;
    if (purity) {
        rc = wp.P == 2 ? wide_purity<2>(e, wp, d_out, pp, pur) : wide_purity<1>(e, wp, d_out, pp, pur);
        if (rc != CTG_OK) return rc;
        HIP_TRY(hipMemcpyAsync(purity, pur, 8, hipMemcpyDeviceToHost, e->stream));
    }
    if (out) HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)(wp.D * wp.D * wp.P * 8), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CTG_OK;
}
