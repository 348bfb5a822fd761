// ctg_cost.hip -- the distribution of a classical cost C(z) under p(z) = |x_z|^2 over the executor's result tensor on
// the device: conditional value at risk, quantiles, a histogram, moments, the optimum and its probability (DESIGN.md
// section 22; ctg_exec_result_cost and ctg_cost_plan of include/ctg_hip.h).
//
// The cost vector C[0 .. n) (fp64) is the caller's (dev_cost: any extents) or comes from m Z-type terms, C(z) = sum
// over s of c_s (-1)^popcount(z & m_s), n = 2^L: the host merges equal masks (ascending term order, fp64), the device
// zeroes the vector, scatters the unique (mask, coefficient) pairs -- one writer per entry -- and runs the butterflies
// of ctg_wht.h over the bits 0 .. L - 1 in ascending order, (a, c) -> (a + c, a - c), never contracted; the last pass
// adds +0.0, so no -0.0 survives.  A numpy model reproduces every bit.
//
// Every mass is a sum of INTEGER weights.  With S = sum p (ctg_exec_result_stats) = f 2^e, f in [1/2, 1), and s = 62 -
// e: w_i = (uint64) rint(p_i 2^s) -- the scaling exact, one rounding -- and W = sum w < 2^63.  Sums of w are 64-bit
// integer additions (LDS integer atomics, whose order cannot matter); there is no floating-point atomic anywhere.
//
//   cost_scatter_kernel     v[mask_i] = coeff_i over the zeroed vector
//   cost_tile_kernel        4096 consecutive doubles: the bits 0 .. min(L, 12) - 1, in place
//   cost_pass_kernel        a strided pass of up to 8 bits, in place, the tile geometry of spectrum_pass_kernel
//   cost_check_kernel       (dev_cost) a flag if an entry is not finite; nothing else is written
//   cost_digit_kernel<T>    a digit pass of the weighted radix select: keys are the order-preserving 64-bit image of
//                           C + 0.0 (negatives: all bits flipped; others: the sign bit), inverted for the upper tail;
//                           digits are 12 bits from the top, the last one 4.  The workgroups take the chunks b, b +
//                           gridDim.x, ... of 4096 elements; a thread reads 4 consecutive costs and elements with 16-byte
//                           loads, forms w and adds it, for the elements whose higher key bits equal the level's prefix,
//                           into a 4096-bin uint64 LDS histogram (32 KiB); a thread adds runs of equal digits in a
//                           register first.  One row per workgroup.
//   cost_rowsum_kernel      adds the rows (64-bit integers); the histogram's rows too
//   cost_select_kernel      one workgroup per level: the digit where the running mass, ascending, first reaches the
//                           target; {prefix, mass below, remaining target, mass at the digit} stay on the device
//   cost_final_kernel<T,H>  one pass over (C, x) for all levels at once: per level the fp64 sum of p C over the keys
//                           below the threshold, sum p C, sum (p C) C, min / max of C with their lowest indices, min /
//                           max over the support w > 0 with lowest index and mass, and (H) the histogram: edges in LDS,
//                           the bin by binary search, uint64 LDS bins.  A workgroup takes a contiguous span of chunks.
//   cost_finish_kernel      one workgroup: the workgroups' records in ascending order -> the output words
//
// The first digit pass is the same for all levels and runs once; its total is W, which the host reads to form A_l =
// ceil(alpha_l W) exactly (128-bit integers).  After that there is no host round trip: the levels run one after
// another, five digit passes each.  fp64 sums have a fixed association that depends on n alone: a thread adds its 16
// elements of a chunk in index order from +0.0, the wave by xor-butterflies 32 .. 1, the four waves in order, the chunks
// of a workgroup's span ascending, the spans ascending.
//
// Scratch (the executor's d_reduce, reduce_reserve): 8 n bytes for C unless dev_cost or dev_cost_out holds it, the
// rows, the records, the term table.
#include <algorithm>
#include <numeric>
#include <type_traits>

#include "ctg_result_host.h"
#include "ctg_wht.h"

namespace ctg {

constexpr int kCostDigitBits = 12;
constexpr int kCostBins = 1 << kCostDigitBits;
constexpr int kCostMaxGrid = 512;        // workgroups of a digit pass and of the final pass: two per CU
constexpr int kCostSelThreads = 1024;
constexpr int kCostHistBins = CTG_COST_MAX_EDGES + 1;

// {prefix chosen so far, mass below its class, target still to reach inside the class, mass at the last digit}
struct CostState {
    unsigned long long prefix, below, target, at;
};

// a minimum or maximum with its lowest index and the mass at the value (i < 0: none yet)
struct CostTrack {
    double v;
    long long i;
    unsigned long long m;
};

// what a workgroup of the final pass leaves
struct CostPartial {
    double sum[2 + CTG_COST_MAX_LEVELS];   // sum p C | sum (p C) C | the levels' tails
    CostTrack t[4];                        // min C | max C | min over the support | max over the support
};

// the order-preserving image of c + 0.0
__device__ __forceinline__ unsigned long long cost_key(double c) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(c + 0.0);
    return (b >> 63) ? ~b : b ^ 0x8000000000000000ull;
}

__device__ __forceinline__ unsigned long long cost_key_hi(unsigned long long key, int sh) { return sh >= 64 ? 0ull : key >> sh; }

// w = (uint64) rint(p 2^s): p 2^s < 2^63
__device__ __forceinline__ unsigned long long cost_weight(double p, int s) { return (unsigned long long)rint(ldexp(p, s)); }

// the 4 costs from e on (e a multiple of 4); entries at or past n are zero.  `vec`: C is 16-byte aligned
__device__ __forceinline__ void load_cost4(const double* __restrict__ C, int64_t e, int64_t n, bool vec, double (&c)[4]) {
    if (vec && e + 4 <= n) {
        const double2 a = *reinterpret_cast<const double2*>(C + e), b = *reinterpret_cast<const double2*>(C + e + 2);
        c[0] = a.x, c[1] = a.y, c[2] = b.x, c[3] = b.y;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = (e + k < n) ? C[e + k] : 0.0;
    }
}

// p of the 4 elements from e on: 16-byte loads where x is 16-byte aligned
template <typename T>
__device__ __forceinline__ void load_p4(const T* __restrict__ x, int64_t e, int64_t n, bool vec, double (&p)[4]) {
    constexpr int V = 16 / sizeof(T);
#pragma unroll
    for (int j = 0; j < 4 / V; ++j) {
        double q[V];
        load_group_p<T>(x, e + j * V, n, vec, q);
#pragma unroll
        for (int k = 0; k < V; ++k) p[j * V + k] = q[k];
    }
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double shfl_xor_f64(double v, int d) {
    return __longlong_as_double((long long)shfl_xor_u64((unsigned long long)__double_as_longlong(v), d));
}

// a <- the better of a and b (sign +1: the minimum, -1: the maximum); equal values add their masses, the lower index stays
__device__ __forceinline__ void track_merge(CostTrack& a, const CostTrack& b, int sign) {
    if (b.i < 0) return;
    const bool better = a.i < 0 || (sign > 0 ? b.v < a.v : b.v > a.v);
    if (better) {
        a = b;
    } else if (b.v == a.v) {
        a.m += b.m;
        a.i = b.i < a.i ? b.i : a.i;
    }
}

__global__ __launch_bounds__(kSampleThreads) void cost_scatter_kernel(const int64_t* __restrict__ masks, const double* __restrict__ coeffs,
                                                                      int64_t u, int64_t n, double* __restrict__ v) {
    const int64_t i = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
    if (i < u && masks[i] >= 0 && masks[i] < n) v[masks[i]] = coeffs[i];
}

// the local indices l, l + 1 of the tile in ds go to v[g], v[g + 1], g even
__device__ __forceinline__ void cost_store_pair(const double* ds, int l, double* __restrict__ v, int64_t g, int64_t n, int vec, int last) {
    double a = ds[spec_slot(l)], c = ds[spec_slot(l + 1)];
    if (last) {
        a = a + 0.0;
        c = c + 0.0;
    }
    if (vec && g + 1 < n) {
        *reinterpret_cast<double2*>(v + g) = make_double2(a, c);
    } else {
        if (g < n) v[g] = a;
        if (g + 1 < n) v[g + 1] = c;
    }
}

// bits 0 .. bits - 1 of chunk blockIdx.x, in place
__global__ __launch_bounds__(kSampleThreads, 2) void cost_tile_kernel(double* __restrict__ v, int64_t n, int bits, int last, int vvec) {
    __shared__ double ds[kResultChunk];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x << kResultChunkBits;
#pragma unroll
    for (int i = 0; i < kResultChunk / 2 / kSampleThreads; ++i) {
        const int l = (i * kSampleThreads + tid) * 2;
        const int64_t g = base + l;
        double a = 0.0, c = 0.0;
        if (vvec && g + 1 < n) {
            const double2 t = *reinterpret_cast<const double2*>(v + g);
            a = t.x, c = t.y;
        } else {
            if (g < n) a = v[g];
            if (g + 1 < n) c = v[g + 1];
        }
        ds[spec_slot(l)] = a;
        ds[spec_slot(l + 1)] = c;
    }
    wht_local(ds, tid, 0, bits);
#pragma unroll
    for (int i = 0; i < kResultChunk / 2 / kSampleThreads; ++i) {
        const int l = (i * kSampleThreads + tid) * 2;
        cost_store_pair(ds, l, v, base + l, n, vvec, last);
    }
}

// bits s .. s + nb - 1 of the vector (n = 2^L > 2^s: every tile lies inside it), in place
__global__ __launch_bounds__(kSampleThreads, 2) void cost_pass_kernel(double* __restrict__ v, int64_t n, int s, int nb, int vvec, int last) {
    __shared__ double ds[kResultChunk];
    const int tid = threadIdx.x;
    const int64_t base = wht_pass_base(blockIdx.x, s, nb);
#pragma unroll
    for (int i = 0; i < kResultChunk / 2 / kSampleThreads; ++i) {
        const int l = (i * kSampleThreads + tid) * 2;   // (l and l + 1 share a row: 4096 / 2^nb >= 16)
        const int64_t g = wht_pass_where(base, l, s, nb);
        double a, c;
        if (vvec) {
            const double2 t = *reinterpret_cast<const double2*>(v + g);
            a = t.x, c = t.y;
        } else {
            a = v[g], c = v[g + 1];
        }
        ds[spec_slot(l)] = a;
        ds[spec_slot(l + 1)] = c;
    }
    wht_local(ds, tid, kResultChunkBits - nb, kResultChunkBits);
#pragma unroll
    for (int i = 0; i < kResultChunk / 2 / kSampleThreads; ++i) {
        const int l = (i * kSampleThreads + tid) * 2;
        cost_store_pair(ds, l, v, wht_pass_where(base, l, s, nb), n, vvec, last);
    }
}

// *flag <- 1 if an entry of C is not finite (every writer stores the same word)
__global__ __launch_bounds__(kSampleThreads) void cost_check_kernel(const double* __restrict__ C, int64_t n, int cvec, int64_t nb,
                                                                    int32_t* __restrict__ flag) {
    const int tid = threadIdx.x;
    bool bad = false;
    for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
#pragma unroll
        for (int i = 0; i < kResultChunk / 4 / kSampleThreads; ++i) {
            const int64_t e = b * kResultChunk + ((int64_t)i * kSampleThreads + tid) * 4;
            double c[4];
            load_cost4(C, e, n, cvec != 0, c);
#pragma unroll
            for (int k = 0; k < 4; ++k) bad = bad || !isfinite(c[k]);
        }
    }
    if (bad) *flag = 1;
}

template <typename T>
__global__ __launch_bounds__(kSampleThreads) void cost_digit_kernel(const double* __restrict__ C, const T* __restrict__ x, int64_t n,
                                                                    int cvec, int xvec, int64_t nb, const CostState* __restrict__ st,
                                                                    int sh, int bits, int sexp, unsigned long long flip,
                                                                    unsigned long long* __restrict__ rows) {
    __shared__ unsigned long long hist[kCostBins];
    const int tid = threadIdx.x;
    for (int i = tid; i < kCostBins; i += kSampleThreads) hist[i] = 0ull;
    __syncthreads();
    const unsigned long long prefix = st->prefix;
    const int nsh = sh - bits;
    const uint32_t dmask = (1u << bits) - 1u;
    // a thread adds runs of equal digits in a register: integer-valued costs put most elements into a few bins
    uint32_t cur = 0;
    unsigned long long acc = 0ull;
    for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
#pragma unroll
        for (int i = 0; i < kResultChunk / 4 / kSampleThreads; ++i) {
            const int64_t e = b * kResultChunk + ((int64_t)i * kSampleThreads + tid) * 4;
            double c[4], p[4];
            load_cost4(C, e, n, cvec != 0, c);
            load_p4<T>(x, e, n, xvec != 0, p);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long key = cost_key(c[k]) ^ flip;
                if (e + k < n && cost_key_hi(key, sh) == prefix) {
                    const unsigned long long w = cost_weight(p[k], sexp);
                    const uint32_t d = (uint32_t)(key >> nsh) & dmask;
                    if (d == cur) {
                        acc += w;
                    } else {
                        if (acc) atomicAdd(&hist[cur], acc);
                        cur = d;
                        acc = w;
                    }
                }
            }
        }
    }
    if (acc) atomicAdd(&hist[cur], acc);
    __syncthreads();
    for (int i = tid; i < kCostBins; i += kSampleThreads) rows[(int64_t)blockIdx.x * kCostBins + i] = hist[i];
}

// tot[bin] <- sum over the rows, bin < nbins; workgroup w takes the bins 64 w ... 64 w + 63, its four waves every fourth row
__global__ __launch_bounds__(kSampleThreads) void cost_rowsum_kernel(const unsigned long long* __restrict__ rows, int nrows, int nbins,
                                                                     unsigned long long* __restrict__ tot) {
    __shared__ unsigned long long w[kSampleThreads / 64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bin = blockIdx.x * 64 + lane;
    unsigned long long s = 0;
    if (bin < nbins)
        for (int r = wave; r < nrows; r += kSampleThreads / 64) s += rows[(int64_t)r * nbins + bin];
    w[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && bin < nbins) tot[bin] = w[0][lane] + w[1][lane] + w[2][lane] + w[3][lane];
}

// Level level0 + blockIdx.x: the digit d with sum of tot[d' < d] < target <= that + tot[d] (1 <= target <= the class's
// mass); thread t owns the bins 4 t .. 4 t + 3.  A level whose target is 0 (W = 0) keeps its state.
__global__ __launch_bounds__(kCostSelThreads) void cost_select_kernel(const unsigned long long* __restrict__ tot, CostState* st, int level0,
                                                                      int bits) {
    __shared__ unsigned long long scan[kCostSelThreads];
    __shared__ unsigned long long res[3];
    CostState* my = st + level0 + blockIdx.x;
    const int t = threadIdx.x;
    const CostState cur = *my;
    unsigned long long c[4], s = 0;
    if (t == 0) res[0] = res[1] = res[2] = 0ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = tot[4 * t + j];
        s += c[j];
    }
    scan[t] = s;
    __syncthreads();
    for (int d = 1; d < kCostSelThreads; d <<= 1) {
        const unsigned long long v = t >= d ? scan[t - d] : 0ull;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    const unsigned long long incl = scan[t], excl = incl - s;
    if (excl < cur.target && cur.target <= incl) {
        unsigned long long run = excl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (cur.target <= run + c[j]) {
                res[0] = (unsigned long long)(4 * t + j);
                res[1] = run;
                res[2] = c[j];
                break;
            }
            run += c[j];
        }
    }
    __syncthreads();
    if (t == 0 && cur.target > 0) {
        my->prefix = (cur.prefix << bits) | res[0];
        my->below = cur.below + res[1];
        my->target = cur.target - res[1];
        my->at = res[2];
    }
}

template <typename T, bool H>
__global__ __launch_bounds__(kSampleThreads) void cost_final_kernel(const double* __restrict__ C, const T* __restrict__ x, int64_t n,
                                                                    int cvec, int xvec, int64_t nb, int64_t span,
                                                                    const CostState* __restrict__ st, int nl, int sexp,
                                                                    unsigned long long flip, const double* __restrict__ edges, int ne,
                                                                    CostPartial* __restrict__ part, unsigned long long* __restrict__ hrows) {
#pragma clang fp contract(off)
    constexpr int NS = 2 + CTG_COST_MAX_LEVELS;
    constexpr int W = kSampleThreads / 64;
    __shared__ double eds[H ? CTG_COST_MAX_EDGES : 1];
    __shared__ unsigned long long bins[H ? kCostHistBins : 1];
    __shared__ double ws[W][NS];
    __shared__ CostTrack wt[W][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (H) {
        for (int i = tid; i < ne; i += kSampleThreads) eds[i] = edges[i];
        for (int i = tid; i <= ne; i += kSampleThreads) bins[i] = 0ull;
        __syncthreads();
    }
    unsigned long long tkey[CTG_COST_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < CTG_COST_MAX_LEVELS; ++l) tkey[l] = l < nl ? st[l].prefix : 0ull;   // (key < 0 never holds)
    CostTrack tr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) tr[q] = CostTrack{0.0, -1ll, 0ull};
    double run = 0.0;   // thread j < NS: sum j over the chunks of the span so far
    const int64_t b0 = (int64_t)blockIdx.x * span, b1 = b0 + span < nb ? b0 + span : nb;
    for (int64_t b = b0; b < b1; ++b) {
        double s[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) s[j] = 0.0;
#pragma unroll
        for (int i = 0; i < kResultChunk / 4 / kSampleThreads; ++i) {
            const int64_t e = b * kResultChunk + ((int64_t)i * kSampleThreads + tid) * 4;
            double c[4], p[4];
            load_cost4(C, e, n, cvec != 0, c);
            load_p4<T>(x, e, n, xvec != 0, p);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e + k >= n) continue;
                const double cc = c[k] + 0.0;
                const unsigned long long key = cost_key(cc) ^ flip;
                const unsigned long long w = cost_weight(p[k], sexp);
                const double pc = p[k] * cc;
                const double pcc = pc * cc;
                s[0] = s[0] + pc;
                s[1] = s[1] + pcc;
#pragma unroll
                for (int l = 0; l < CTG_COST_MAX_LEVELS; ++l) s[2 + l] = s[2 + l] + (key < tkey[l] ? pc : 0.0);
                const CostTrack one{cc, (long long)(e + k), w};
                track_merge(tr[0], one, +1);
                track_merge(tr[1], one, -1);
                if (w) {
                    track_merge(tr[2], one, +1);
                    track_merge(tr[3], one, -1);
                }
                if (H && w) {
                    int lo = 0, hi = ne;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (eds[mid] <= cc)
                            lo = mid + 1;
                        else
                            hi = mid;
                    }
                    atomicAdd(&bins[lo], w);
                }
            }
        }
        // the chunk's sums: the wave by xor-butterflies, the four waves in order, then onto the span's
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            if (j >= 2 + nl) continue;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s[j] = s[j] + shfl_xor_f64(s[j], d);
            if (lane == 0) ws[wave][j] = s[j];
        }
        __syncthreads();
        if (tid < 2 + nl) {
            const double a = ws[0][tid] + ws[1][tid];
            const double c2 = a + ws[2][tid];
            const double c3 = c2 + ws[3][tid];
            run = run + c3;
        }
        __syncthreads();
    }
    // minima and maxima of the span: exact, any order
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int sign = (q & 1) ? -1 : +1;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            CostTrack o;
            o.v = shfl_xor_f64(tr[q].v, d);
            o.i = (long long)shfl_xor_u64((unsigned long long)tr[q].i, d);
            o.m = shfl_xor_u64(tr[q].m, d);
            // (both lanes of a pair must see the pair's merge: masses add once, a's and b's)
            track_merge(tr[q], o, sign);
        }
        if (lane == 0) wt[wave][q] = tr[q];
    }
    __syncthreads();
    CostPartial* out = part + blockIdx.x;
    if (tid < NS) out->sum[tid] = tid < 2 + nl ? run : 0.0;
    if (tid >= 64 && tid < 68) {
        const int q = tid - 64, sign = (q & 1) ? -1 : +1;
        CostTrack a = wt[0][q];
        for (int w2 = 1; w2 < W; ++w2) track_merge(a, wt[w2][q], sign);
        out->t[q] = a;
    }
    if (H)
        for (int i = tid; i <= ne; i += kSampleThreads) hrows[(int64_t)blockIdx.x * (ne + 1) + i] = bins[i];
}

// words <- the records of the `grid` workgroups in ascending order, and the levels' states (layout: include/ctg_hip.h)
__global__ __launch_bounds__(64) void cost_finish_kernel(const CostPartial* __restrict__ part, int grid, const CostState* __restrict__ st,
                                                         int nl, unsigned long long flip, int64_t* __restrict__ words) {
#pragma clang fp contract(off)
    constexpr int NS = 2 + CTG_COST_MAX_LEVELS;
    const int t = threadIdx.x;
    if (t < NS) {
        double s = 0.0;
        for (int g = 0; g < grid; ++g) s = s + part[g].sum[t];
        if (t < 2)
            words[2 + t] = __double_as_longlong(s);
        else if (t - 2 < nl)
            words[CTG_COST_LEVEL_WORD0 + CTG_COST_LEVEL_WORDS * (t - 2) + 4] = __double_as_longlong(s);
    } else if (t < NS + 4) {
        const int q = t - NS, sign = (q & 1) ? -1 : +1;
        CostTrack a = part[0].t[q];
        for (int g = 1; g < grid; ++g) track_merge(a, part[g].t[q], sign);
        const int w0 = q < 2 ? 4 + 2 * q : 8 + 3 * (q - 2);
        words[w0] = __double_as_longlong(a.i < 0 ? 0.0 : a.v);
        words[w0 + 1] = a.i;
        if (q >= 2) words[w0 + 2] = (int64_t)a.m;
    } else if (t - NS - 4 < nl) {
        const int l = t - NS - 4;
        int64_t* w = words + CTG_COST_LEVEL_WORD0 + CTG_COST_LEVEL_WORDS * l;
        // the threshold from its key: undo the inversion of the upper tail, then the order-preserving image
        const unsigned long long key = st[l].prefix ^ flip;
        const unsigned long long b = (key >> 63) ? key ^ 0x8000000000000000ull : ~key;
        w[1] = st[l].target || st[l].at ? (int64_t)b : 0ll;
        w[2] = (int64_t)st[l].below;
        w[3] = (int64_t)st[l].at;
    }
}

}  // namespace ctg

using namespace ctg;

namespace {

// what a call launches: a function of (dtype, extents, source, nl, ne) alone
struct CostPlan {
    int L = -1;          // terms: log2 n; values: -1
    int64_t n = 1;
    int tile_bits = 0, npass = 0, pass_bits[kSpecMaxPasses] = {0, 0, 0, 0};
    int64_t tiles = 0;   // workgroups of a transform launch
    int64_t chunks = 1, span = 1;
    int grid = 1;        // workgroups of a digit pass and of the final pass
    int64_t scratch = 0; // bytes without the term table; the vector counted
};

struct CostBufs {
    double* vec;
    CostState* st;
    unsigned long long *rows, *tot, *hrows, *htot;
    CostPartial* part;
    double* edges;
    int64_t* words;
    int32_t* flag;
    int64_t* masks;
    double* coeffs;
    int64_t bytes;
};

CostBufs cost_carve(void* base, const CostPlan& p, bool own_vec, int ne, int64_t u) {
    CostBufs b;
    Carve c(base);
    b.vec = c.take<double>(own_vec ? p.n * 8 : 0);
    b.st = c.take<CostState>(CTG_COST_MAX_LEVELS * sizeof(CostState));
    b.rows = c.take<unsigned long long>((int64_t)p.grid * kCostBins * 8);
    b.tot = c.take<unsigned long long>(kCostBins * 8);
    b.part = c.take<CostPartial>((int64_t)p.grid * sizeof(CostPartial));
    b.hrows = c.take<unsigned long long>(ne ? (int64_t)p.grid * (ne + 1) * 8 : 0);
    b.htot = c.take<unsigned long long>(ne ? (int64_t)(ne + 1) * 8 : 0);
    b.edges = c.take<double>(ne ? (int64_t)ne * 8 : 0);
    b.words = c.take<int64_t>(CTG_COST_WORDS * 8);
    b.flag = c.take<int32_t>(8);
    b.masks = c.take<int64_t>(u * 8);
    b.coeffs = c.take<double>(u * 8);
    b.bytes = c.bytes();
    return b;
}

// CTG_OK, or CTG_E_INVALID with the error set: everything about (rank, extents, source, nl, ne) that the call refuses
int cost_plan(const char* who, int64_t rank, const int64_t* extents, int terms, int64_t result_elems, bool have_elems, int64_t nl,
              int64_t ne, ResultShape* shape, CostPlan* out) {
    CostPlan& p = *out = CostPlan();
    if (rank < 0) return result_fail(CTG_E_INVALID, "%s: negative rank", who);
    if (terms)
        for (int64_t a = 0; a < rank; ++a)
            if (extents[a] > 2)
                return result_fail(CTG_E_INVALID, "%s: axis %lld has extent %lld; with terms every extent must be 1 or 2", who, (long long)a,
                                   (long long)extents[a]);
    if (!have_elems) {   // (the plan function: the extents' own product stands for result_elems)
        result_elems = 1;
        for (int64_t a = 0; a < rank && result_elems <= kReduceMaxElems; ++a)
            result_elems = extents[a] >= 1 && extents[a] <= kReduceMaxElems / result_elems ? result_elems * extents[a] : kReduceMaxElems + 1;
    }
    const char* why = "";
    if (result_shape(rank, extents, result_elems, shape, &why) != CTG_OK) return result_fail(CTG_E_INVALID, "%s: %s", who, why);
    if (nl < 0 || nl > CTG_COST_MAX_LEVELS)
        return result_fail(CTG_E_INVALID, "%s: %lld levels; between 0 and CTG_COST_MAX_LEVELS = %d", who, (long long)nl, CTG_COST_MAX_LEVELS);
    if (ne != 0 && (ne < 2 || ne > CTG_COST_MAX_EDGES))
        return result_fail(CTG_E_INVALID, "%s: %lld edges; none, or between 2 and CTG_COST_MAX_EDGES = %d", who, (long long)ne,
                           CTG_COST_MAX_EDGES);
    p.n = shape->n;
    if (terms) {
        p.L = 0;
        while (((int64_t)1 << p.L) < p.n) ++p.L;
        p.tile_bits = std::min(p.L, kResultChunkBits);
        for (int b = kResultChunkBits; b < p.L; b += kSpecPassBits) p.pass_bits[p.npass++] = std::min(kSpecPassBits, p.L - b);
        p.tiles = std::max<int64_t>(1, p.n >> kResultChunkBits);
    }
    p.chunks = (p.n + kResultChunk - 1) / kResultChunk;
    p.span = (p.chunks + kCostMaxGrid - 1) / kCostMaxGrid;
    p.grid = (int)((p.chunks + p.span - 1) / p.span);   // (at most kCostMaxGrid, and no workgroup without a chunk)
    p.scratch = cost_carve(nullptr, p, true, (int)ne, 0).bytes;
    return CTG_OK;
}

// ceil(alpha W) exactly: alpha = m 2^k, m a 53-bit integer
unsigned long long cost_target(double alpha, unsigned long long W) {
    int ex = 0;
    const double f = std::frexp(alpha, &ex);                         // alpha = f 2^ex, f in [1/2, 1)
    const unsigned long long m = (unsigned long long)std::ldexp(f, 53);   // an integer below 2^53
    const int k = ex - 53;                                           // alpha = m 2^k, k <= -52 (alpha <= 1)
    const unsigned __int128 prod = (unsigned __int128)m * W;
    const int r = -k;
    if (r >= 128) return prod ? 1ull : 0ull;
    const unsigned __int128 q = prod >> r, rem = prod - (q << r);
    return (unsigned long long)(q + (rem ? 1 : 0));
}

template <typename T>
int cost_select_and_finish(ctg_exec* e, const CostPlan& p, const CostBufs& b, const double* C, int tail, int64_t nl, const double* levels,
                           int ne, int sexp, int64_t* words) {
    hipStream_t st = e->stream;
    const T* x = (const T*)e->d_result;
    const int xvec = ((uintptr_t)x & 15) == 0 ? 1 : 0, cvec = ((uintptr_t)C & 15) == 0 ? 1 : 0;
    const unsigned long long flip = tail > 0 ? ~0ull : 0ull;
    CostState hs[CTG_COST_MAX_LEVELS];
    memset(hs, 0, sizeof(hs));
    HIP_TRY(upload(b.st, hs, sizeof(hs), st));
    unsigned long long W = 0;
    // the first digit pass is every level's, and its total is W (with no level it only gives W)
    cost_digit_kernel<T><<<dim3((unsigned)p.grid), dim3(kSampleThreads), 0, st>>>(C, x, p.n, cvec, xvec, p.chunks, b.st, 64, kCostDigitBits, sexp,
                                                                                 flip, b.rows);
    LAUNCH_CHECK("cost_digit_kernel");
    cost_rowsum_kernel<<<dim3(kCostBins / 64), dim3(kSampleThreads), 0, st>>>(b.rows, p.grid, kCostBins, b.tot);
    LAUNCH_CHECK("cost_rowsum_kernel");
    {
        std::vector<unsigned long long> tot(kCostBins);
        HIP_TRY(hipMemcpyAsync(tot.data(), b.tot, kCostBins * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (unsigned long long v : tot) W += v;
    }
    for (int64_t l = 0; l < nl; ++l) hs[l].target = cost_target(levels[l], W);
    if (nl && W) {
        HIP_TRY(upload(b.st, hs, sizeof(hs), st));
        cost_select_kernel<<<dim3((unsigned)nl), dim3(kCostSelThreads), 0, st>>>(b.tot, b.st, 0, kCostDigitBits);
        LAUNCH_CHECK("cost_select_kernel");
        for (int l = 0; l < (int)nl; ++l) {
            int sh = 64 - kCostDigitBits;
            while (sh > 0) {
                const int bits = sh < kCostDigitBits ? sh : kCostDigitBits;
                cost_digit_kernel<T><<<dim3((unsigned)p.grid), dim3(kSampleThreads), 0, st>>>(C, x, p.n, cvec, xvec, p.chunks, b.st + l, sh, bits,
                                                                                             sexp, flip, b.rows);
                LAUNCH_CHECK("cost_digit_kernel");
                cost_rowsum_kernel<<<dim3(kCostBins / 64), dim3(kSampleThreads), 0, st>>>(b.rows, p.grid, kCostBins, b.tot);
                LAUNCH_CHECK("cost_rowsum_kernel");
                cost_select_kernel<<<dim3(1), dim3(kCostSelThreads), 0, st>>>(b.tot, b.st, l, bits);
                LAUNCH_CHECK("cost_select_kernel");
                sh -= bits;
            }
        }
    }
    HIP_TRY(hipMemsetAsync(b.words, 0, CTG_COST_WORDS * 8, st));
    if (ne) {
        cost_final_kernel<T, true><<<dim3((unsigned)p.grid), dim3(kSampleThreads), 0, st>>>(C, x, p.n, cvec, xvec, p.chunks, p.span, b.st, (int)nl,
                                                                                           sexp, flip, b.edges, ne, b.part, b.hrows);
        LAUNCH_CHECK("cost_final_kernel");
        cost_rowsum_kernel<<<dim3((unsigned)((ne + 1 + 63) / 64)), dim3(kSampleThreads), 0, st>>>(b.hrows, p.grid, ne + 1, b.htot);
        LAUNCH_CHECK("cost_rowsum_kernel");
    } else {
        cost_final_kernel<T, false><<<dim3((unsigned)p.grid), dim3(kSampleThreads), 0, st>>>(C, x, p.n, cvec, xvec, p.chunks, p.span, b.st, (int)nl,
                                                                                            sexp, flip, nullptr, 0, b.part, nullptr);
        LAUNCH_CHECK("cost_final_kernel");
    }
    cost_finish_kernel<<<dim3(1), dim3(64), 0, st>>>(b.part, p.grid, b.st, (int)nl, flip, b.words);
    LAUNCH_CHECK("cost_finish_kernel");
    HIP_TRY(hipMemcpyAsync(words, b.words, CTG_COST_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    words[1] = (int64_t)W;
    for (int64_t l = 0; l < nl; ++l) words[CTG_COST_LEVEL_WORD0 + CTG_COST_LEVEL_WORDS * l] = (int64_t)hs[l].target;
    return CTG_OK;
}

// the arguments both entry points check, in the order the header lists them
int cost_args(const char* who, int64_t nl, const double* levels, int64_t ne, const double* edges, int tail) {
    if (tail != -1 && tail != 1) return result_fail(CTG_E_INVALID, "%s: tail = %d is neither -1 (lower) nor +1 (upper)", who, tail);
    if (nl > 0 && !levels) return result_fail(CTG_E_INVALID, "%s: levels is null", who);
    for (int64_t l = 0; l < nl; ++l)
        if (!(levels[l] > 0.0 && levels[l] <= 1.0))
            return result_fail(CTG_E_INVALID, "%s: level %lld = %g is outside (0, 1]", who, (long long)l, levels[l]);
    if (ne > 0 && !edges) return result_fail(CTG_E_INVALID, "%s: edges is null", who);
    for (int64_t i = 0; i < ne; ++i) {
        if (!std::isfinite(edges[i])) return result_fail(CTG_E_INVALID, "%s: edge %lld is not finite", who, (long long)i);
        if (i && !(edges[i - 1] < edges[i])) return result_fail(CTG_E_INVALID, "%s: the edges are not strictly ascending at %lld", who, (long long)i);
    }
    return CTG_OK;
}

}  // namespace

extern "C" int ctg_cost_plan(int32_t dtype, int64_t rank, const int64_t* extents, int32_t source, int64_t nl, int64_t ne, int64_t* words) {
    const char* who = "cost_plan";
    if (!extents || !words) return result_fail(CTG_E_INVALID, "%s: null argument", who);
    if (dtype < CTG_F32 || dtype > CTG_C128) return result_fail(CTG_E_INVALID, "%s: dtype %d is none of CTG_F32 .. CTG_C128", who, (int)dtype);
    if (source != CTG_COST_TERMS && source != CTG_COST_VALUES)
        return result_fail(CTG_E_INVALID, "%s: source %d is neither CTG_COST_TERMS nor CTG_COST_VALUES", who, (int)source);
    ResultShape shape;
    CostPlan p;
    const int rc = cost_plan(who, rank, extents, source == CTG_COST_TERMS, 0, false, nl, ne, &shape, &p);
    if (rc != CTG_OK) return rc;
    for (int i = 0; i < CTG_COST_PLAN_WORDS; ++i) words[i] = 0;
    words[0] = p.L;
    words[1] = p.n;
    words[2] = p.tile_bits;
    words[3] = p.npass;
    for (int i = 0; i < kSpecMaxPasses; ++i) words[4 + i] = p.pass_bits[i];
    words[8] = p.tiles;
    words[9] = nl ? 6 : 1;
    words[10] = 1 + 5 * nl;
    words[11] = p.grid;
    words[12] = p.scratch;
    words[13] = dtype;
    words[14] = p.chunks;
    words[15] = ne ? ne + 1 : 0;
    return CTG_OK;
}

extern "C" int ctg_exec_result_cost(ctg_exec* e, int64_t rank, const int64_t* extents, int64_t m, const uint8_t* ops, const double* coeffs,
                                    const void* dev_cost, int32_t tail, int64_t nl, const double* levels, int64_t ne, const double* edges,
                                    int64_t* out_words, int64_t* out_hist, void* dev_cost_out) {
    const char* who = "cost";
    if (!e || !extents || !out_words) return result_fail(CTG_E_INVALID, "%s: null argument", who);
    const bool terms = ops || coeffs;
    if (terms && dev_cost) return result_fail(CTG_E_INVALID, "%s: both terms and dev_cost are given", who);
    if (!terms && !dev_cost) return result_fail(CTG_E_INVALID, "%s: neither terms nor dev_cost is given", who);
    if (terms && (!ops || !coeffs)) return result_fail(CTG_E_INVALID, "%s: terms need both ops and coeffs", who);
    if (ne > 0 && !out_hist) return result_fail(CTG_E_INVALID, "%s: edges without out_hist", who);
    ResultShape shape;
    CostPlan p;
    int rc = cost_plan(who, rank, extents, terms, e->plan->result_elems, true, nl, ne, &shape, &p);
    if (rc != CTG_OK) return rc;
    rc = cost_args(who, nl, levels, ne, edges, tail);
    if (rc != CTG_OK) return rc;
    const int64_t n = p.n;
    const int dtype = e->plan->dtype;
    // the terms: a mask per row, equal masks added in ascending term order
    std::vector<int64_t> umask;
    std::vector<double> ucoef;
    if (terms) {
        if (m < 0 || m > CTG_COST_MAX_TERMS)
            return result_fail(CTG_E_INVALID, "%s: %lld terms; between 0 and CTG_COST_MAX_TERMS = %d", who, (long long)m, CTG_COST_MAX_TERMS);
        std::vector<int64_t> mask((size_t)m);
        double sum_abs = 0.0;
        for (int64_t s = 0; s < m; ++s) {
            int64_t mk = 0;
            for (int64_t a = 0; a < rank; ++a) {
                const int op = ops[s * rank + a];
                if (op != 0 && op != 3)
                    return result_fail(CTG_E_INVALID, "%s: term %lld, axis %lld: code %d is neither 0 (I) nor 3 (Z)", who, (long long)s,
                                       (long long)a, op);
                if (op && extents[a] != 2)
                    return result_fail(CTG_E_INVALID, "%s: term %lld has Z on axis %lld of extent %lld", who, (long long)s, (long long)a,
                                       (long long)extents[a]);
                if (op) mk |= shape.strides[a];
            }
            if (!std::isfinite(coeffs[s])) return result_fail(CTG_E_INVALID, "%s: coefficient %lld is not finite", who, (long long)s);
            sum_abs += std::fabs(coeffs[s]);
            mask[(size_t)s] = mk;
        }
        if (!std::isfinite(sum_abs)) return result_fail(CTG_E_INVALID, "%s: the coefficients' absolute sum is not finite", who);
        std::vector<int64_t> ord((size_t)m);
        std::iota(ord.begin(), ord.end(), (int64_t)0);
        std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t c) { return mask[(size_t)a] < mask[(size_t)c]; });
        for (int64_t i : ord) {
            if (!umask.empty() && umask.back() == mask[(size_t)i]) {
                ucoef.back() += coeffs[i];
            } else {
                umask.push_back(mask[(size_t)i]);
                ucoef.push_back(coeffs[i]);
            }
        }
    }
    const uintptr_t r0 = (uintptr_t)e->d_result, r1 = r0 + (uintptr_t)(n * ctg_item_size(dtype));
    if (dev_cost) {
        if ((uintptr_t)dev_cost & 7) return result_fail(CTG_E_INVALID, "%s: dev_cost is not 8-byte aligned", who);
    }
    if (dev_cost_out) {
        if ((uintptr_t)dev_cost_out & 7) return result_fail(CTG_E_INVALID, "%s: dev_cost_out is not 8-byte aligned", who);
        const uintptr_t d0 = (uintptr_t)dev_cost_out;
        if (d0 < r1 && r0 < d0 + (uintptr_t)(n * 8)) return result_fail(CTG_E_INVALID, "%s: dev_cost_out overlaps the result tensor", who);
        const uintptr_t c0 = (uintptr_t)dev_cost;
        if (dev_cost && d0 < c0 + (uintptr_t)(n * 8) && c0 < d0 + (uintptr_t)(n * 8))
            return result_fail(CTG_E_INVALID, "%s: dev_cost_out overlaps dev_cost", who);
    }
    // sum p and its exponent: s = 62 - e, 0 for an all-zero tensor (every weight is 0 then)
    double S = 0.0;
    rc = ctg_exec_result_stats(e, &S, nullptr, nullptr, nullptr);
    if (rc != CTG_OK) return rc;
    if (!std::isfinite(S)) return result_norm_fail(S, "no cost statistics of it");
    int ex = 0;
    if (S > 0.0) std::frexp(S, &ex);
    const int sexp = S > 0.0 ? 62 - ex : 0;
    const bool own_vec = terms && !dev_cost_out;
    const int64_t u = (int64_t)umask.size();
    rc = reduce_reserve(e, cost_carve(nullptr, p, own_vec, (int)ne, u).bytes);
    if (rc != CTG_OK) return rc;
    const CostBufs b = cost_carve(e->d_reduce, p, own_vec, (int)ne, u);
    hipStream_t st = e->stream;
    const double* C = nullptr;
    if (terms) {
        double* v = dev_cost_out ? (double*)dev_cost_out : b.vec;
        const int vvec = ((uintptr_t)v & 15) == 0 ? 1 : 0;
        HIP_TRY(hipMemsetAsync(v, 0, (size_t)(n * 8), st));
        if (u) {
            HIP_TRY(upload(b.masks, umask.data(), u * 8, st));
            HIP_TRY(upload(b.coeffs, ucoef.data(), u * 8, st));
            cost_scatter_kernel<<<dim3((unsigned)((u + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(b.masks, b.coeffs, u, n,
                                                                                                                          v);
            LAUNCH_CHECK("cost_scatter_kernel");
        }
        cost_tile_kernel<<<dim3((unsigned)p.tiles), dim3(kSampleThreads), 0, st>>>(v, n, p.tile_bits, p.npass == 0, vvec);
        LAUNCH_CHECK("cost_tile_kernel");
        int s = kResultChunkBits;
        for (int i = 0; i < p.npass; ++i) {
            cost_pass_kernel<<<dim3((unsigned)p.tiles), dim3(kSampleThreads), 0, st>>>(v, n, s, p.pass_bits[i], vvec, i == p.npass - 1);
            LAUNCH_CHECK("cost_pass_kernel");
            s += p.pass_bits[i];
        }
        C = v;
    } else {
        const int cvec = ((uintptr_t)dev_cost & 15) == 0 ? 1 : 0;
        int32_t flag = 0;
        HIP_TRY(hipMemsetAsync(b.flag, 0, 8, st));
        cost_check_kernel<<<dim3((unsigned)p.grid), dim3(kSampleThreads), 0, st>>>((const double*)dev_cost, n, cvec, p.chunks, b.flag);
        LAUNCH_CHECK("cost_check_kernel");
        HIP_TRY(hipMemcpyAsync(&flag, b.flag, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (flag) return result_fail(CTG_E_INVALID, "%s: dev_cost holds an entry that is not finite", who);
        if (dev_cost_out) HIP_TRY(hipMemcpyAsync(dev_cost_out, dev_cost, (size_t)(n * 8), hipMemcpyDeviceToDevice, st));
        C = (const double*)dev_cost;
    }
    if (ne) HIP_TRY(upload(b.edges, edges, ne * 8, st));
    int64_t words[CTG_COST_WORDS];
    rc = dispatch_elem(dtype, [&](auto t) {
        return cost_select_and_finish<decltype(t)>(e, p, b, C, tail, nl, levels, (int)ne, sexp, words);
    });
    if (rc != CTG_OK) return rc;
    std::vector<int64_t> hist((size_t)(ne ? ne + 1 : 0));
    if (ne) {
        HIP_TRY(hipMemcpyAsync(hist.data(), b.htot, (size_t)((ne + 1) * 8), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    words[0] = sexp;
    words[14] = nl;
    words[15] = tail;
    memcpy(&words[16], &S, 8);
    memcpy(out_words, words, sizeof(words));
    if (ne) memcpy(out_hist, hist.data(), hist.size() * 8);
    return CTG_OK;
}
