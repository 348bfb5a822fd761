// ctg_rdm.hip -- the reduced density matrix of a few output indices of the executor's result tensor on the device
// (ctg_exec_result_rdm of include/ctg_hip.h):
//
//   rho[a, b] = sum over r of x[a, r] * conj(x[b, r])
//
// a, b over the kept axes (D = their product <= CTG_RDM_MAX_DIM), r over all others (t = result_elems / D).  Every
// product is formed in fp64 (exact for float / complex64 elements), every sum is in fp64 with an association that is a
// function of (extents, keep) alone; no atomics.  The axes are split as for a marginal (marginal_plan).  Two routes:
//
//   power of two (every extent a power of two, at least kResultChunk = 4096 elements): a is the bit-extract of the flat
//   index under the keep mask K, r the one under its complement.  For D < 16 the lowest 4 - log2(D) bits of r are
//   folded into the row: D' = 16 rows (a, s), and rho[a, b] is the sum over s of G'[(a, s), (b, s)].  A chunk is the
//   next 12 - log2(D') bits of r for all D' rows: kResultChunk elements that lie in runs of at least 64 consecutive ones
//   (every bit of the flat index below the chunk's highest complement bit is a row bit or a chunk bit).
//
//     rdm_chunk_kernel<T, NT>  NT = D' / 16 in {1, 2, 4}.  A workgroup takes the chunks wg, wg + grid, ... in
//                              ascending order: 16-byte loads along the runs into registers (the next chunk's are
//                              in flight while this one is multiplied; not for complex128 with NT = 4), widened
//                              to fp64 into LDS as X[plane][row][col] (planes Re, Im; row stride TC + 2 doubles: 16 rows x 2 doubles fall on 32 different
//                              bank pairs), then v_mfma_f64_16x16x4_f64 on the NT (NT + 1) / 2 tiles of the lower
//                              triangle: Re += Xr Xr^T + Xi Xi^T, Im += Xi Xr^T + Xr (-Xi)^T.  Each of the four waves
//                              multiplies a quarter of the chunk's columns for EVERY tile -- for D' = 16 there is one
//                              tile, so dealing tiles would idle three waves; a wave's fragment loads feed all
//                              tiles -- and keeps its accumulators in registers across chunks.  At the end the waves'
//                              accumulators are added in wave order through LDS and written as one partial.
//     rdm_gather_kernel        adds the partials of kRdmSumChunk consecutive workgroups in ascending order;
//     rdm_finish_kernel        adds those in ascending order, then the folded s ascending; writes b <= a, the
//                              conjugate half and the zero imaginary diagonal.
//
//   grid = result_chunk_grid(chunks) = min(512, ceil(chunks / 3)): two workgroups per CU at most (LDS: 66 KiB each for complex
//   elements), and at least three chunks per workgroup (all but the last ones), so that a workgroup's partial -- up
//   to 40 KiB -- is at most a third of what it read.
//
//   general (any other shape): rdm_general_kernel, one work item per (a, b <= a, chunk of complement positions),
//   walks its chunk serially with the mixed-radix decode of marg_general_kernel; rdm_general_finish_kernel adds the
//   chunks in ascending order.  Not tuned.
#include <algorithm>

#include "ctg_result_elem.h"
#include "ctg_result_host.h"

namespace ctg {

// (a chunk, kResultChunk elements of ctg_result_elem.h, is D' rows x TC columns here)
constexpr int kRdmSumChunk = 32;                 // partials per work item of rdm_gather_kernel
constexpr int64_t kRdmGeneralChunk = 1024;       // complement positions per work item of the general route, at least
constexpr int64_t kRdmGeneralMaxChunks = 1024;   // ... and at most this many chunks per pair

typedef double f64x4 __attribute__((ext_vector_type(4)));

// planes (Re | Re, Im) of an element type and its components widened to fp64
template <typename T> struct RdmElem;
template <> struct RdmElem<float> {
    static constexpr int P = 1;
    static __device__ __forceinline__ double re(float v) { return (double)v; }
    static __device__ __forceinline__ double im(float) { return 0.0; }
};
template <> struct RdmElem<double> {
    static constexpr int P = 1;
    static __device__ __forceinline__ double re(double v) { return v; }
    static __device__ __forceinline__ double im(double) { return 0.0; }
};
template <> struct RdmElem<float2> {
    static constexpr int P = 2;
    static __device__ __forceinline__ double re(float2 v) { return (double)v.x; }
    static __device__ __forceinline__ double im(float2 v) { return (double)v.y; }
};
template <> struct RdmElem<double2> {
    static constexpr int P = 2;
    static __device__ __forceinline__ double re(double2 v) { return v.x; }
    static __device__ __forceinline__ double im(double2 v) { return v.y; }
};

// Element e of a chunk (bit i of e): gpos[i] is what the bit adds to the flat index, lw[i] what it adds to the
// element's place in an LDS plane (row * LD or column).  The bits are those of the flat index under the chunk's mask,
// lowest first, so e and the flat index agree in their lowest bits: consecutive e are consecutive elements.
struct RdmChunkBits {
    int64_t gpos[kResultChunkBits];
    int32_t lw[kResultChunkBits];
};

__device__ __forceinline__ int64_t rdm_goff(uint32_t e, const RdmChunkBits& b) {
    int64_t r = 0;
#pragma unroll
    for (int i = 0; i < kResultChunkBits; ++i) r += ((e >> i) & 1u) ? b.gpos[i] : 0;
    return r;
}
__device__ __forceinline__ int rdm_loff(uint32_t e, const RdmChunkBits& b) {
    int r = 0;
#pragma unroll
    for (int i = 0; i < kResultChunkBits; ++i) r += ((e >> i) & 1u) ? b.lw[i] : 0;
    return r;
}

template <typename T, int NT>
__global__ __launch_bounds__(kSampleThreads, 2) void rdm_chunk_kernel(const T* __restrict__ x, int64_t n, int vec,
                                                                      RdmChunkBits bits, int64_t rhi, int64_t nchunks,
                                                                      double* __restrict__ part) {
    constexpr int P = RdmElem<T>::P;
    constexpr int V = 16 / sizeof(T);
    constexpr int G = kResultChunk / V / kSampleThreads;
    constexpr int DP = 16 * NT, TC = kResultChunk / DP, LD = TC + 2, PLANE = DP * LD;
    constexpr int NTL = NT * (NT + 1) / 2;
    constexpr int WC = TC / (kSampleThreads / 64);   // columns of a wave
    static_assert(WC % 8 == 0, "a wave multiplies eight columns per step");
    // (complex128 with 64 rows: 160 accumulator registers and 64 of loads in flight do not fit 256; that one loads,
    // then multiplies, and leaves the overlap to the second workgroup of the CU)
    constexpr bool PRE = !(sizeof(T) == 16 && NT == 4);
    static_assert(NTL * P * 256 <= P * PLANE, "the waves' accumulators are added in the planes' memory");
    __shared__ __attribute__((aligned(16))) double xs[P * PLANE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // element (g * kSampleThreads + tid) * V of a chunk: this thread's share of its offsets
    const int64_t goff_t = rdm_goff((uint32_t)tid * V, bits);
    const int loff_t = rdm_loff((uint32_t)tid * V, bits);

    f64x4 acc[NTL][P];
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
        for (int p = 0; p < P; ++p) acc[t][p] = f64x4{0.0, 0.0, 0.0, 0.0};

    T st[G][V];
    auto fetch = [&](int64_t q) {
        const int64_t base = deposit_bits(q, rhi);
#pragma unroll
        for (int g = 0; g < G; ++g)
            load_group<T>(x, base + goff_t + rdm_goff((uint32_t)(g * kSampleThreads) * V, bits), n, vec != 0, st[g]);
    };

    // fragment coordinates of v_mfma_f64_16x16x4_f64: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15]
    const int r16 = lane & 15, k4 = lane >> 4;
    int64_t q = blockIdx.x;
    if (PRE && q < nchunks) fetch(q);
    for (; q < nchunks; q += gridDim.x) {
        __syncthreads();   // (the multiplications of the chunk before have read the planes)
        if (!PRE) fetch(q);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int o = loff_t + rdm_loff((uint32_t)(g * kSampleThreads) * V, bits);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int ok = o + rdm_loff((uint32_t)k, bits);
                xs[ok] = RdmElem<T>::re(st[g][k]);
                if (P == 2) xs[PLANE + ok] = RdmElem<T>::im(st[g][k]);
            }
        }
        __syncthreads();
        if (PRE && q + gridDim.x < nchunks) fetch(q + gridDim.x);
        // columns kb + 2 k4, kb + 2 k4 + 1 of row 16 I + r16: one 16-byte read feeds two MFMA steps (which four
        // columns share a step is free, as long as A and B agree)
        for (int kb = wave * WC; kb < (wave + 1) * WC; kb += 8) {
            double2 fr[NT][P];
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int p = 0; p < P; ++p)
                    fr[i][p] = *reinterpret_cast<const double2*>(&xs[p * PLANE + (16 * i + r16) * LD + kb + 2 * k4]);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int t = 0;
#pragma unroll
                for (int i = 0; i < NT; ++i) {
#pragma unroll
                    for (int j = 0; j <= i; ++j, ++t) {
                        const double ar = h ? fr[i][0].y : fr[i][0].x, br = h ? fr[j][0].y : fr[j][0].x;
                        acc[t][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, acc[t][0], 0, 0, 0);
                        if (P == 2) {
                            const double ai = h ? fr[i][P - 1].y : fr[i][P - 1].x, bi = h ? fr[j][P - 1].y : fr[j][P - 1].x;
                            acc[t][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, acc[t][0], 0, 0, 0);
                            acc[t][P - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, acc[t][P - 1], 0, 0, 0);
                            acc[t][P - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, -bi, acc[t][P - 1], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    // the four waves' accumulators in wave order; C/D: col = lane & 15, row = (lane >> 4) + 4 * reg
    for (int w = 0; w < kSampleThreads / 64; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < NTL; ++t)
#pragma unroll
                for (int p = 0; p < P; ++p)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int o = ((t * P + p) * 4 + i) * 64 + lane;
                        xs[o] = w == 0 ? acc[t][p][i] : xs[o] + acc[t][p][i];
                    }
        }
    }
    __syncthreads();
    for (int o = tid; o < NTL * P * 256; o += kSampleThreads) part[(int64_t)blockIdx.x * (NTL * P * 256) + o] = xs[o];
}

// B[gr E + el] <- part[(gr kRdmSumChunk + i) E + el] for i = 0, 1, ... in that order (np partials of E doubles)
__global__ __launch_bounds__(kSampleThreads) void rdm_gather_kernel(const double* __restrict__ part, int64_t E, int np,
                                                                    int64_t total, double* __restrict__ B) {
    const int64_t g = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
    if (g >= total) return;
    const int64_t el = g % E, gr = g / E;
    const int p0 = (int)gr * kRdmSumChunk, p1 = p0 + kRdmSumChunk < np ? p0 + kRdmSumChunk : np;
    double s = part[(int64_t)p0 * E + el];
    for (int p = p0 + 1; p < p1; ++p) s += part[(int64_t)p * E + el];
    B[g] = s;
}

// row[a S + s]: the row of G' that holds (a, s) -- S = 1 and row[a] = a for D >= 16
struct RdmFold {
    int32_t D, S;
    uint8_t row[CTG_RDM_MAX_DIM];
};

// out[a][b], out[b][a] for b <= a from the ng group sums B[gr E + ...] of the lower tiles of G'
template <int P>
__global__ __launch_bounds__(kSampleThreads) void rdm_finish_kernel(const double* __restrict__ B, int64_t E, int ng,
                                                                    RdmFold f, double* __restrict__ out) {
    const int g = blockIdx.x * kSampleThreads + threadIdx.x;
    if (g >= f.D * f.D) return;
    const int a = g / f.D, b = g % f.D;
    if (b > a) return;
    double v[P];
    for (int s = 0; s < f.S; ++s) {
        const int ra = f.row[a * f.S + s], rb = f.row[b * f.S + s];   // (ra >= rb: the folded bits are equal)
        const int ti = ra >> 4, tj = rb >> 4, i = ra & 15, j = rb & 15;
        const int t = ti * (ti + 1) / 2 + tj;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int64_t o = ((int64_t)(t * P + p) * 4 + (i >> 2)) * 64 + (i & 3) * 16 + j;
            double w = B[o];
            for (int gr = 1; gr < ng; ++gr) w += B[(int64_t)gr * E + o];
            v[p] = s == 0 ? w : v[p] + w;
        }
    }
    if (P == 1) {
        out[a * f.D + b] = v[0];
        out[b * f.D + a] = v[0];
    } else {
        double2* o2 = reinterpret_cast<double2*>(out);
        if (a == b) {
            o2[a * f.D + a] = double2{v[0], 0.0};
        } else {
            o2[a * f.D + b] = double2{v[0], v[P - 1]};
            o2[b * f.D + a] = double2{v[0], -v[P - 1]};
        }
    }
}

// Work item (a, b <= a, chunk ch): B[(ch D D + a D + b) P + p] <- sum of x[a, c] conj(x[b, c]) over the complement
// positions c of the chunk, serially
template <typename T>
__global__ __launch_bounds__(kSampleThreads) void rdm_general_kernel(const T* __restrict__ x, MargAxes ax, int D, int64_t rc,
                                                                     int64_t chunk, int64_t total, double* __restrict__ B) {
#pragma clang fp contract(off)
    constexpr int P = RdmElem<T>::P;
    const int64_t g = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
    if (g >= total) return;
    const int ab = (int)(g % (D * D));
    const int64_t ch = g / (D * D);
    const int a = ab / D, b = ab % D;
    if (b > a) return;
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
        const double ar = RdmElem<T>::re(xa), br = RdmElem<T>::re(xb);
        double pr = ar * br, pi = 0.0;
        if (P == 2) {
            const double ai = RdmElem<T>::im(xa), bi = RdmElem<T>::im(xb);
            const double q = ai * bi, u = ai * br, w = ar * bi;
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
__global__ __launch_bounds__(kSampleThreads) void rdm_general_finish_kernel(const double* __restrict__ B, int D, int64_t nch,
                                                                            double* __restrict__ out) {
    const int g = blockIdx.x * kSampleThreads + threadIdx.x;
    if (g >= D * D) return;
    const int a = g / D, b = g % D;
    if (b > a) return;
    double v[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        double w = B[(int64_t)g * P + p];
        for (int64_t ch = 1; ch < nch; ++ch) w += B[(ch * D * D + g) * P + p];
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

}  // namespace ctg

using namespace ctg;

namespace {

int popcount64(int64_t v) { return __builtin_popcountll((unsigned long long)v); }

// the lowest `k` set bits of mask
int64_t lowest_bits(int64_t mask, int k) {
    int64_t r = 0;
    for (; k > 0 && mask; --k) {
        r |= mask & (0 - mask);
        mask &= mask - 1;
    }
    return r;
}

// What the host decides for the power-of-two route: everything a function of (n, keep mask) alone
struct RdmFastPlan {
    int nt = 1;             // D' / 16
    RdmChunkBits bits{};
    int64_t rhi = 0;        // the complement bits above a chunk: they count the chunks
    RdmFold fold{};
    int64_t nchunks = 1;
    int grid = 1, ngroups = 1;
    int64_t E = 0;          // doubles of one partial (per plane count P applied by the caller)
};

RdmFastPlan rdm_fast_plan(int64_t n, int64_t keepmask, int D, int P) {
    RdmFastPlan fp;
    const int d = popcount64(keepmask);
    const int64_t R = (n - 1) & ~keepmask;
    const int f = d < 4 ? 4 - d : 0;
    const int64_t F = lowest_bits(R, f), K2 = keepmask | F;
    const int d2 = d + f;
    fp.nt = 1 << (d2 - 4);
    const int64_t Rlo = lowest_bits(R & ~F, kResultChunkBits - d2);
    const int64_t M = K2 | Rlo;
    fp.rhi = R & ~F & ~Rlo;
    const int ld = kResultChunk / (16 * fp.nt) + 2;
    int i = 0;
    for (int b = 0; b < 63; ++b) {
        if (!((M >> b) & 1)) continue;
        const int64_t below = ((int64_t)1 << b) - 1;
        fp.bits.gpos[i] = (int64_t)1 << b;
        fp.bits.lw[i] = ((K2 >> b) & 1) ? ld << popcount64(K2 & below) : 1 << popcount64(Rlo & below);
        ++i;
    }
    fp.fold.D = D;
    fp.fold.S = 1 << f;
    for (int a = 0; a < D; ++a)
        for (int s = 0; s < fp.fold.S; ++s)
            fp.fold.row[a * fp.fold.S + s] = (uint8_t)extract_bits(deposit_bits(a, keepmask) | deposit_bits(s, F), K2);
    fp.nchunks = n / kResultChunk;
    fp.grid = result_chunk_grid(fp.nchunks);
    fp.ngroups = (fp.grid + kRdmSumChunk - 1) / kRdmSumChunk;
    fp.E = (int64_t)(fp.nt * (fp.nt + 1) / 2) * P * 256;
    return fp;
}

template <typename T, int NT>
int rdm_fast_launch(ctg_exec* e, const RdmFastPlan& fp, int64_t n, double* part, double* B, double* out) {
    constexpr int P = RdmElem<T>::P;
    hipStream_t st = e->stream;
    const int vec = ((uintptr_t)e->d_result & 15) == 0 ? 1 : 0;
    rdm_chunk_kernel<T, NT><<<dim3((unsigned)fp.grid), dim3(kSampleThreads), 0, st>>>((const T*)e->d_result, n, vec, fp.bits,
                                                                                     fp.rhi, fp.nchunks, part);
    LAUNCH_CHECK("rdm_chunk_kernel");
    const int64_t total = fp.E * fp.ngroups;
    rdm_gather_kernel<<<dim3((unsigned)((total + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(
        part, fp.E, fp.grid, total, B);
    LAUNCH_CHECK("rdm_gather_kernel");
    const int dd = fp.fold.D * fp.fold.D;
    rdm_finish_kernel<P><<<dim3((unsigned)((dd + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(
        B, fp.E, fp.ngroups, fp.fold, out);
    LAUNCH_CHECK("rdm_finish_kernel");
    return CTG_OK;
}

template <typename T>
int rdm_fast(ctg_exec* e, const RdmFastPlan& fp, int64_t n, double* part, double* B, double* out) {
    switch (fp.nt) {
        case 1: return rdm_fast_launch<T, 1>(e, fp, n, part, B, out);
        case 2: return rdm_fast_launch<T, 2>(e, fp, n, part, B, out);
        default: return rdm_fast_launch<T, 4>(e, fp, n, part, B, out);
    }
}

int64_t rdm_general_chunk(int64_t rc) {
    return std::max<int64_t>(kRdmGeneralChunk, (rc + kRdmGeneralMaxChunks - 1) / kRdmGeneralMaxChunks);
}

template <typename T>
int rdm_general(ctg_exec* e, const MargAxes& ax, int D, int64_t rc, double* B, double* out) {
    constexpr int P = RdmElem<T>::P;
    hipStream_t st = e->stream;
    const int64_t chunk = rdm_general_chunk(rc), nch = (rc + chunk - 1) / chunk, total = (int64_t)D * D * nch;
    rdm_general_kernel<T><<<dim3((unsigned)((total + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(
        (const T*)e->d_result, ax, D, rc, chunk, total, B);
    LAUNCH_CHECK("rdm_general_kernel");
    rdm_general_finish_kernel<P><<<dim3((unsigned)((D * D + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(
        B, D, nch, out);
    LAUNCH_CHECK("rdm_general_finish_kernel");
    return CTG_OK;
}

}  // namespace

extern "C" int ctg_exec_result_rdm(ctg_exec* e, int64_t rank, const int64_t* extents, const int32_t* keep, void* out) {
    if (!e || !out) return result_fail(CTG_E_INVALID, "null argument");
    MarginalPlan mp;
    const char* why = "";
    if (marginal_plan(rank, extents, keep, e->plan->result_elems, &mp, &why) != CTG_OK)
        return result_fail(CTG_E_INVALID, "rdm: %s", why);
    if (mp.m > CTG_RDM_MAX_DIM)
        return result_fail(CTG_E_INVALID, "rdm: the kept extents' product is %lld; at most CTG_RDM_MAX_DIM = %d", (long long)mp.m,
                     CTG_RDM_MAX_DIM);
    int rc = result_norm_finite(e, "no reduced density matrix of it");
    if (rc != CTG_OK) return rc;
    const int dtype = e->plan->dtype;
    const int P = (dtype == CTG_C64 || dtype == CTG_C128) ? 2 : 1;
    const int D = (int)mp.m;
    const int64_t out_bytes = (int64_t)D * D * P * 8;
    // [out: D D P | partials of the workgroups (general route: none) | sums of groups of partials / of chunks]
    RdmFastPlan fp;
    int64_t a_elems = 0, b_elems = 0;
    if (mp.fast) {
        fp = rdm_fast_plan(mp.n, mp.mask, D, P);
        a_elems = fp.E * fp.grid;
        b_elems = fp.E * fp.ngroups;
    } else {
        const int64_t chunk = rdm_general_chunk(mp.rc);
        b_elems = (int64_t)D * D * P * ((mp.rc + chunk - 1) / chunk);
    }
    double *d_out = nullptr, *A = nullptr, *B = nullptr;
    auto lay = [&](void* base) {
        Carve c(base);
        d_out = c.take<double>(out_bytes);
        A = c.take<double>(a_elems * 8);
        B = c.take<double>(b_elems * 8);
        return c.bytes();
    };
    rc = reduce_reserve(e, lay(nullptr));
    if (rc != CTG_OK) return rc;
    lay(e->d_reduce);
    if (mp.fast)
        rc = dispatch_elem(dtype, [&](auto t) { return rdm_fast<decltype(t)>(e, fp, mp.n, A, B, d_out); });
    else
        rc = dispatch_elem(dtype, [&](auto t) { return rdm_general<decltype(t)>(e, mp.ax, D, mp.rc, B, d_out); });
    if (rc != CTG_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)out_bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CTG_OK;
}
