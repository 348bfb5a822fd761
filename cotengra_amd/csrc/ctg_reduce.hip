// ctg_reduce.hip -- the k most probable members, and marginals, of the executor's result tensor on the device
// (ctg_exec_result_topk / ctg_exec_result_marginal of include/ctg_hip.h).
//
// Both are reductions of p_i = |x_i|^2 (SampleElem of ctg_sample_elem.h: the double a host reference forms) over the
// tensor the executor holds; only the answer crosses the bus.
//
// Top-k is a radix select on the bit pattern of p (a non-negative double's pattern is monotone as a uint64; x * x is
// never -0; a NaN never gets here: sum p is checked first), then a collection in index order:
//
//   topk_hist_kernel     a digit pass over the tensor: the workgroups take the blocks b, b + gridDim.x, ... of
//                        kSampleBlock elements and count, in LDS, the digit of every element whose higher bits equal
//                        the prefix chosen so far; one row of counts per workgroup;
//   topk_rowsum_kernel   adds the rows (64-bit integers);
//   topk_select_kernel   one workgroup: the digit that holds the k-th largest key; prefix, remaining k, class size;
//   topk_count_kernel    per block: elements above the prefix, elements equal to it (under a shift);
//   topk_scan_kernel     one workgroup: exclusive integer scans of both over the blocks;
//   topk_write_kernel    per block: every element above, and the equal ones of global rank < take IN INDEX ORDER
//                        (wave ballots and popcount prefixes; the block's offsets from the scan) -> (index, element, p)
//                        records, or -- compacting -- the keys of the class;
//   topk_finish_kernel   one workgroup: the remaining digit passes on a compact list of keys.
//
// Digits are 12 bits from the top (sign and exponent first), the last one 4.  While the class of the prefix holds more
// than kTopkCompact keys the passes read the tensor; once it holds at most that many its keys are compacted and the
// select finishes on the list in one launch.  An all-equal tensor never shrinks: it takes all six passes over the
// tensor.  There is no floating-point sum anywhere in top-k; counts are integers (LDS atomics, whose order does not
// matter), every grid is a function of result_elems, and the k records are ordered (p descending, index ascending)
// on the host inside the call.
//
// Marginals: out[j] = sum of p over the elements whose kept coordinates are j.  Adjacent axes of equal keep status
// are merged and axes of extent 1 dropped on the host.  Two routes:
//
//   fast (every extent a power of two, at least kSampleBlock elements): j is a bit-extract of the flat index under
//   a keep bitmask.  marg_block_kernel reduces a block of kSampleBlock consecutive elements to 2^popcount(mask &
//   0xfff) partial sums by a tree over the dropped bits, highest first; marg_gather_kernel adds, per output and chunk
//   of kMargChunk of its blocks, the partials in ascending block order; marg_sum_kernel adds the chunks in ascending
//   order.  The tensor is walked in slabs (ascending) of at most CTG_MARGINAL_PARTIALS partial sums, a slab's result
//   added to the output serially.
//
//   general (any extents): marg_general_kernel, one work item per (output, chunk of kMargGeneralChunk complement
//   positions), walks its chunk serially with a mixed-radix decode; marg_sum_kernel adds the chunks.  Not tuned.
//
// Every sum has a fixed association that depends on (extents, keep) alone, and there are no atomics in either route.
#include <algorithm>
#include <numeric>

#include "ctg_result_host.h"
#include "ctg_sample_elem.h"

namespace ctg {

constexpr int kDigitBits = 12;
constexpr int kBins = 1 << kDigitBits;
constexpr int kHistMaxGrid = 1024;            // workgroups of a digit pass
constexpr int kSelThreads = 1024;
constexpr int64_t kTopkCompact = 1 << 16;     // finish on a compact list once the class holds at most this many keys
constexpr int kMargChunk = 64;                // blocks per (output, chunk) of the fast route
constexpr int64_t kMargGeneralChunk = 1024;   // complement positions per work item of the general route

// {prefix chosen so far, k still to find inside its class, size of the class, elements above the class}
struct TopkState {
    unsigned long long prefix;
    long long krem, cls, gt;
};

// the bits of `key` above the `sh` unresolved ones
__device__ __forceinline__ unsigned long long key_hi(unsigned long long key, int sh) { return sh >= 64 ? 0ull : key >> sh; }

template <typename T>
__global__ __launch_bounds__(kSampleThreads) void topk_hist_kernel(const T* __restrict__ x, int64_t n, int vec, int64_t nb,
                                                                   const TopkState* __restrict__ st, int sh, int bits,
                                                                   uint32_t* __restrict__ rows) {
    constexpr int V = 16 / sizeof(T);
    constexpr int G = kSampleBlock / V / kSampleThreads;
    __shared__ uint32_t hist[kBins];
    const int tid = threadIdx.x;
    for (int i = tid; i < kBins; i += kSampleThreads) hist[i] = 0;
    __syncthreads();
    const unsigned long long prefix = st->prefix;
    const int nsh = sh - bits;
    const uint32_t dmask = (1u << bits) - 1u;
    // a thread counts runs of equal digits in a register: real data puts most elements into a few bins
    uint32_t cur = 0, cnt = 0;
    for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const int64_t base = b * kSampleBlock;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int64_t e = base + ((int64_t)g * kSampleThreads + tid) * V;
            double p[V];
            load_group_p<T>(x, e, n, vec != 0, p);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const unsigned long long key = (unsigned long long)__double_as_longlong(p[k]);
                if (e + k < n && key_hi(key, sh) == prefix) {
                    const uint32_t d = (uint32_t)(key >> nsh) & dmask;
                    if (d == cur) {
                        ++cnt;
                    } else {
                        if (cnt) atomicAdd(&hist[cur], cnt);
                        cur = d;
                        cnt = 1;
                    }
                }
            }
        }
    }
    if (cnt) atomicAdd(&hist[cur], cnt);
    __syncthreads();
    for (int i = tid; i < kBins; i += kSampleThreads) rows[(int64_t)blockIdx.x * kBins + i] = hist[i];
}

// tot[bin] <- sum over the rows; workgroup w takes the bins 64 w ... 64 w + 63, its four waves every fourth row
__global__ __launch_bounds__(kSampleThreads) void topk_rowsum_kernel(const uint32_t* __restrict__ rows, int nrows,
                                                                     unsigned long long* __restrict__ tot) {
    __shared__ unsigned long long w[kSampleThreads / 64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bin = blockIdx.x * 64 + lane;
    unsigned long long s = 0;
    for (int r = wave; r < nrows; r += kSampleThreads / 64) s += rows[(int64_t)r * kBins + bin];
    w[wave][lane] = s;
    __syncthreads();
    if (wave == 0) tot[bin] = w[0][lane] + w[1][lane] + w[2][lane] + w[3][lane];
}

// The digit d that holds the krem-th largest key of a class: sum of tot[d' > d] < krem <= that + tot[d] (the class
// holds at least krem keys).  kSelThreads threads; thread t owns the bins kBins - 1 - 4 t downwards.
// res <- {d, keys of the class in higher digits, tot[d]}
template <typename C>
__device__ __forceinline__ void pick_digit(const C* __restrict__ tot, long long krem, unsigned long long* scan, long long* res) {
    const int t = threadIdx.x;
    unsigned long long c[4], s = 0;
    if (t == 0) res[0] = res[1] = res[2] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = (unsigned long long)tot[kBins - 1 - (4 * t + j)];
        s += c[j];
    }
    scan[t] = s;
    __syncthreads();
    for (int d = 1; d < kSelThreads; d <<= 1) {
        const unsigned long long v = t >= d ? scan[t - d] : 0ull;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    const unsigned long long incl = scan[t], excl = incl - s;
    if ((long long)excl < krem && krem <= (long long)incl) {
        unsigned long long run = excl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (krem <= (long long)(run + c[j])) {
                res[0] = kBins - 1 - (4 * t + j);
                res[1] = (long long)run;
                res[2] = (long long)c[j];
                break;
            }
            run += c[j];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kSelThreads) void topk_select_kernel(const unsigned long long* __restrict__ tot, TopkState* st,
                                                                  int bits) {
    __shared__ unsigned long long scan[kSelThreads];
    __shared__ long long res[3];
    const long long krem = st->krem;
    const unsigned long long prefix = st->prefix;
    const long long gt = st->gt;
    pick_digit(tot, krem, scan, res);
    if (threadIdx.x == 0) {
        st->prefix = (prefix << bits) | (unsigned long long)res[0];
        st->krem = krem - res[1];
        st->gt = gt + res[1];
        st->cls = res[2];
    }
}

// the remaining digit passes (sh unresolved bits) on the m keys of the class
__global__ __launch_bounds__(kSelThreads) void topk_finish_kernel(const unsigned long long* __restrict__ keys, int64_t m,
                                                                  TopkState* st, int sh) {
    __shared__ uint32_t hist[kBins];
    __shared__ unsigned long long scan[kSelThreads];
    __shared__ long long res[3];
    __shared__ TopkState s;
    const int t = threadIdx.x;
    if (t == 0) s = *st;
    __syncthreads();
    while (sh > 0) {
        const int bits = sh < kDigitBits ? sh : kDigitBits, nsh = sh - bits;
        const uint32_t dmask = (1u << bits) - 1u;
        for (int i = t; i < kBins; i += kSelThreads) hist[i] = 0;
        __syncthreads();
        const unsigned long long prefix = s.prefix;
        const long long krem = s.krem;
        for (int64_t i = t; i < m; i += kSelThreads) {
            const unsigned long long key = keys[i];
            if (key_hi(key, sh) == prefix) atomicAdd(&hist[(uint32_t)(key >> nsh) & dmask], 1u);
        }
        __syncthreads();
        pick_digit(hist, krem, scan, res);
        if (t == 0) {
            s.prefix = (prefix << bits) | (unsigned long long)res[0];
            s.krem = krem - res[1];
            s.gt += res[1];
            s.cls = res[2];
        }
        __syncthreads();
        sh = nsh;
    }
    if (t == 0) *st = s;
}

// cg[b], ce[b] <- elements of block b whose bits above `sh` are greater than / equal to the prefix
template <typename T>
__global__ __launch_bounds__(kSampleThreads) void topk_count_kernel(const T* __restrict__ x, int64_t n, int vec,
                                                                    const TopkState* __restrict__ st, int sh,
                                                                    uint32_t* __restrict__ cg, uint32_t* __restrict__ ce) {
    constexpr int V = 16 / sizeof(T);
    constexpr int G = kSampleBlock / V / kSampleThreads;
    __shared__ uint32_t wg[kSampleThreads / 64], we[kSampleThreads / 64];
    const int tid = threadIdx.x;
    const unsigned long long prefix = st->prefix;
    const int64_t base = (int64_t)blockIdx.x * kSampleBlock;
    uint32_t g_ = 0, e_ = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t e = base + ((int64_t)g * kSampleThreads + tid) * V;
        double p[V];
        load_group_p<T>(x, e, n, vec != 0, p);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const unsigned long long hi = key_hi((unsigned long long)__double_as_longlong(p[k]), sh);
            if (e + k < n) {
                g_ += hi > prefix ? 1u : 0u;
                e_ += hi == prefix ? 1u : 0u;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        g_ += (uint32_t)__shfl_xor((int)g_, d, 64);
        e_ += (uint32_t)__shfl_xor((int)e_, d, 64);
    }
    if ((tid & 63) == 0) {
        wg[tid >> 6] = g_;
        we[tid >> 6] = e_;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kSampleThreads / 64; ++w) {
            g_ += wg[w];
            e_ += we[w];
        }
        cg[blockIdx.x] = g_;
        ce[blockIdx.x] = e_;
    }
}

// og[b], oe[b] <- exclusive sums of cg, ce over the blocks; thread g owns the `gs` consecutive blocks from g gs on
__global__ __launch_bounds__(kSelThreads) void topk_scan_kernel(const uint32_t* __restrict__ cg, const uint32_t* __restrict__ ce,
                                                                int64_t nb, int64_t gs, int64_t* __restrict__ og,
                                                                int64_t* __restrict__ oe) {
    __shared__ int64_t tg[kSelThreads], te[kSelThreads];
    const int64_t b0 = (int64_t)threadIdx.x * gs;
    const int64_t b1 = b0 + gs < nb ? b0 + gs : nb;
    int64_t sg = 0, se = 0;
    for (int64_t b = b0; b < b1; ++b) {
        sg += cg[b];
        se += ce[b];
    }
    tg[threadIdx.x] = sg;
    te[threadIdx.x] = se;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t kg = 0, ke = 0;
        for (int g = 0; g < kSelThreads; ++g) {
            const int64_t a = tg[g], b = te[g];
            tg[g] = kg;
            te[g] = ke;
            kg += a;
            ke += b;
        }
    }
    __syncthreads();
    sg = tg[threadIdx.x];
    se = te[threadIdx.x];
    for (int64_t b = b0; b < b1; ++b) {
        og[b] = sg;
        oe[b] = se;
        sg += cg[b];
        se += ce[b];
    }
}

// Block b writes its elements above the prefix to the records og[b] ... and its elements equal to the prefix, in
// index order, to the records st->gt + oe[b] ... as long as that global rank among the equal ones is below st->krem.
// `compact`: only the equal ones, all of them, their keys to keys_out[oe[b] ...].  `cap`: records the outputs hold.
template <typename T>
__global__ __launch_bounds__(kSampleThreads) void topk_write_kernel(const T* __restrict__ x, int64_t n, int vec,
                                                                    const TopkState* __restrict__ st, int sh, int compact,
                                                                    const uint32_t* __restrict__ cg,
                                                                    const uint32_t* __restrict__ ce,
                                                                    const int64_t* __restrict__ og,
                                                                    const int64_t* __restrict__ oe, int64_t cap,
                                                                    unsigned long long* __restrict__ keys_out,
                                                                    int64_t* __restrict__ idx_out, T* __restrict__ el_out,
                                                                    double* __restrict__ p_out) {
    constexpr int V = 16 / sizeof(T);
    constexpr int G = kSampleBlock / V / kSampleThreads;
    constexpr int W = kSampleThreads / 64;
    __shared__ uint32_t wg[G][W], we[G][W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const unsigned long long prefix = st->prefix;
    const int64_t take = compact ? INT64_MAX : (int64_t)st->krem;
    const int64_t ebase = compact ? 0 : (int64_t)st->gt;
    const int64_t myg = og[b], mye = oe[b];
    const bool any_g = !compact && cg[b] > 0;
    const bool any_e = ce[b] > 0 && mye < take;
    if (!any_g && !any_e) return;   // (the whole workgroup: nothing of this block is wanted)
    const int64_t base = b * kSampleBlock;
    const unsigned long long below = (1ull << lane) - 1ull;
    double p[G][V];
#pragma unroll
    for (int g = 0; g < G; ++g) load_group_p<T>(x, base + ((int64_t)g * kSampleThreads + tid) * V, n, vec != 0, p[g]);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t e = base + ((int64_t)g * kSampleThreads + tid) * V;
        uint32_t ng = 0, ne = 0;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const unsigned long long hi = key_hi((unsigned long long)__double_as_longlong(p[g][k]), sh);
            const bool in = e + k < n;
            ng += (uint32_t)__popcll(__ballot(in && hi > prefix));
            ne += (uint32_t)__popcll(__ballot(in && hi == prefix));
        }
        if (lane == 0) {
            wg[g][wave] = ng;
            we[g][wave] = ne;
        }
    }
    __syncthreads();
    uint32_t rung = 0, rune = 0;   // elements of the block in front of this wave's share of group row g
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t e = base + ((int64_t)g * kSampleThreads + tid) * V;
        uint32_t offg = rung, offe = rune;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if (w < wave) {
                offg += wg[g][w];
                offe += we[g][w];
            }
            rung += wg[g][w];
            rune += we[g][w];
        }
        // in index order inside the wave's 64 V consecutive elements: lower lanes first, then this lane's lower k
        bool isg[V], ise[V];
        uint32_t lowg = 0, lowe = 0;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const unsigned long long hi = key_hi((unsigned long long)__double_as_longlong(p[g][k]), sh);
            const bool in = e + k < n;
            isg[k] = in && hi > prefix;
            ise[k] = in && hi == prefix;
            lowg += (uint32_t)__popcll(__ballot(isg[k]) & below);
            lowe += (uint32_t)__popcll(__ballot(ise[k]) & below);
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            int64_t pos = -1;
            if (isg[k] && !compact) {
                pos = myg + offg + lowg;
                ++lowg;
            } else if (ise[k]) {
                const int64_t r = mye + offe + lowe;
                ++lowe;
                if (r < take) pos = ebase + r;
            }
            if (pos >= 0 && pos < cap) {
                if (compact) {
                    keys_out[pos] = (unsigned long long)__double_as_longlong(p[g][k]);
                } else {
                    idx_out[pos] = e + k;
                    el_out[pos] = x[e + k];
                    p_out[pos] = p[g][k];
                }
            }
        }
    }
}

// ---- marginals ---------------------------------------------------------------------------------------------- //

// Block b0 + blockIdx.x (kSampleBlock consecutive elements) -> A[blockIdx.x][2^popcount(lomask)]: p into LDS at the
// element's offset, then for every dropped bit of the offset, highest first, v[i] <- v[i with 0 there] + v[i with 1
// there] on the array squeezed by that bit.  What is left is indexed by the kept bits of the offset, in their order.
template <typename T>
__global__ __launch_bounds__(kSampleThreads) void marg_block_kernel(const T* __restrict__ x, int64_t n, int vec, int64_t b0,
                                                                    uint32_t lomask, double* __restrict__ A) {
#pragma clang fp contract(off)
    constexpr int V = 16 / sizeof(T);
    constexpr int G = kSampleBlock / V / kSampleThreads;
    __shared__ double buf0[kSampleBlock], buf1[kSampleBlock / 2];
    const int tid = threadIdx.x;
    const int64_t base = (b0 + blockIdx.x) * kSampleBlock;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int o = (g * kSampleThreads + tid) * V;
        double p[V];
        load_group_p<T>(x, base + o, n, vec != 0, p);
#pragma unroll
        for (int k = 0; k < V; ++k) buf0[o + k] = p[k];
    }
    __syncthreads();
    double* src = buf0;
    double* dst = buf1;
    int size = kSampleBlock;
    for (int b = 11; b >= 0; --b) {
        if ((lomask >> b) & 1u) continue;
        const int half = size >> 1, low = (1 << b) - 1;
        for (int i = tid; i < half; i += kSampleThreads) {
            const int i0 = ((i >> b) << (b + 1)) | (i & low);
            dst[i] = src[i0] + src[i0 | (1 << b)];
        }
        __syncthreads();
        double* t = src;
        src = dst;
        dst = t;
        size = half;
    }
    for (int i = tid; i < size; i += kSampleThreads) A[(int64_t)blockIdx.x * size + i] = src[i];
}

// the bits of v dealt to the set bits of mask, lowest first
__device__ __forceinline__ uint32_t deposit_bits(uint32_t v, uint32_t mask) {
    uint32_t r = 0;
    for (uint32_t m = mask; m; m &= m - 1) {
        if (v & 1u) r |= m & (0u - m);
        v >>= 1;
    }
    return r;
}

// Work item (output jo of the slab, chunk ch): B[ch mo + jo] <- the partials A[block][q] of the blocks ch rc ... of
// that output, in ascending block order.  jo = (jl << clo) | q; the output's blocks are those whose bits under `keepm`
// spell jl, the others counting upwards.
__global__ __launch_bounds__(kSampleThreads) void marg_gather_kernel(const double* __restrict__ A, int clo, uint32_t keepm,
                                                                     uint32_t dropm, int64_t mo, int64_t rc, int64_t total,
                                                                     double* __restrict__ B) {
#pragma clang fp contract(off)
    const int64_t g = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
    if (g >= total) return;
    const int64_t jo = g % mo, ch = g / mo;
    const uint32_t q = (uint32_t)jo & ((1u << clo) - 1u);
    const uint32_t fixed = deposit_bits((uint32_t)(jo >> clo), keepm);
    uint32_t cur = deposit_bits((uint32_t)(ch * rc), dropm);
    double s = 0.0;
    for (int64_t i = 0; i < rc; ++i) {
        const double a = A[((int64_t)(fixed | cur) << clo) + q];
        s = i == 0 ? a : s + a;
        cur = ((cur | ~dropm) + 1u) & dropm;
    }
    B[g] = s;
}

// out[j] (+)= B[j] + B[mo + j] + ... in that order
__global__ __launch_bounds__(kSampleThreads) void marg_sum_kernel(const double* __restrict__ B, int64_t mo, int64_t nch,
                                                                  int accumulate, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
    if (j >= mo) return;
    double s = B[j];
    for (int64_t ch = 1; ch < nch; ++ch) s += B[ch * mo + j];
    out[j] = accumulate ? out[j] + s : s;
}

// Work item (output j, chunk ch): B[ch m + j] <- p at the complement positions ch chunk ... of output j, serially
template <typename T>
__global__ __launch_bounds__(kSampleThreads) void marg_general_kernel(const T* __restrict__ x, MargAxes ax, int64_t m,
                                                                      int64_t rc, int64_t chunk, int64_t total,
                                                                      double* __restrict__ B) {
#pragma clang fp contract(off)
    const int64_t g = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
    if (g >= total) return;
    const int64_t j = g % m, ch = g / m;
    int64_t off = 0, t = j;
    for (int a = ax.nk - 1; a >= 0; --a) {
        off += (t % ax.kext[a]) * ax.kstr[a];
        t /= ax.kext[a];
    }
    const int64_t c0 = ch * chunk, c1 = c0 + chunk < rc ? c0 + chunk : rc;
    double s = 0.0;
    for (int64_t c = c0; c < c1; ++c) {
        int64_t o = off;
        t = c;
        for (int a = ax.nd - 1; a >= 0; --a) {
            o += (t % ax.dext[a]) * ax.dstr[a];
            t /= ax.dext[a];
        }
        const double p = SampleElem<T>::p(x[o]);
        s = c == c0 ? p : s + p;
    }
    B[g] = s;
}

}  // namespace ctg

using namespace ctg;

namespace {

struct TopkBufs {
    TopkState* st;
    uint32_t* rows;
    unsigned long long* tot;
    uint32_t *cg, *ce;
    int64_t *og, *oe;
    unsigned long long* keys;
    char* el;
    int64_t* idx;
    double* p;
    int64_t bytes;
};

TopkBufs topk_carve(void* base, int64_t nb, int64_t grid, int64_t k) {
    TopkBufs b;
    Carve c(base);
    b.st = c.take<TopkState>(sizeof(TopkState));
    b.rows = c.take<uint32_t>(grid * kBins * 4);
    b.tot = c.take<unsigned long long>(kBins * 8);
    b.cg = c.take<uint32_t>(nb * 4);
    b.ce = c.take<uint32_t>(nb * 4);
    b.og = c.take<int64_t>(nb * 8);
    b.oe = c.take<int64_t>(nb * 8);
    b.keys = c.take<unsigned long long>(kTopkCompact * 8);
    b.el = c.take<char>(k * 16);
    b.idx = c.take<int64_t>(k * 8);
    b.p = c.take<double>(k * 8);
    b.bytes = c.bytes();
    return b;
}

template <typename T>
int topk_run(ctg_exec* e, const TopkBufs& b, int64_t n, int64_t nb, int grid, int64_t k) {
    const T* x = (const T*)e->d_result;
    const int vec = ((uintptr_t)e->d_result & 15) == 0 ? 1 : 0;
    hipStream_t s = e->stream;
    TopkState h{0ull, (long long)k, (long long)n, 0ll};
    HIP_TRY(hipMemcpyAsync(b.st, &h, sizeof(h), hipMemcpyHostToDevice, s));
    const int64_t gs = std::max<int64_t>((nb + kSelThreads - 1) / kSelThreads, 1);
    int sh = 64;
    while (sh > 0) {
        if (h.cls <= kTopkCompact) {
            // the class fits the list: its keys in index order, the rest of the select on them
            topk_count_kernel<T><<<dim3((unsigned)nb), dim3(kSampleThreads), 0, s>>>(x, n, vec, b.st, sh, b.cg, b.ce);
            LAUNCH_CHECK("topk_count_kernel");
            topk_scan_kernel<<<dim3(1), dim3(kSelThreads), 0, s>>>(b.cg, b.ce, nb, gs, b.og, b.oe);
            LAUNCH_CHECK("topk_scan_kernel");
            topk_write_kernel<T><<<dim3((unsigned)nb), dim3(kSampleThreads), 0, s>>>(
                x, n, vec, b.st, sh, 1, b.cg, b.ce, b.og, b.oe, kTopkCompact, b.keys, nullptr, nullptr, nullptr);
            LAUNCH_CHECK("topk_write_kernel");
            topk_finish_kernel<<<dim3(1), dim3(kSelThreads), 0, s>>>(b.keys, (int64_t)h.cls, b.st, sh);
            LAUNCH_CHECK("topk_finish_kernel");
            sh = 0;
            break;
        }
        const int bits = sh < kDigitBits ? sh : kDigitBits;
        topk_hist_kernel<T><<<dim3((unsigned)grid), dim3(kSampleThreads), 0, s>>>(x, n, vec, nb, b.st, sh, bits, b.rows);
        LAUNCH_CHECK("topk_hist_kernel");
        topk_rowsum_kernel<<<dim3(kBins / 64), dim3(kSampleThreads), 0, s>>>(b.rows, grid, b.tot);
        LAUNCH_CHECK("topk_rowsum_kernel");
        topk_select_kernel<<<dim3(1), dim3(kSelThreads), 0, s>>>(b.tot, b.st, bits);
        LAUNCH_CHECK("topk_select_kernel");
        sh -= bits;
        HIP_TRY(hipMemcpyAsync(&h, b.st, sizeof(h), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    // every key above the threshold, and the first krem equal to it by index
    topk_count_kernel<T><<<dim3((unsigned)nb), dim3(kSampleThreads), 0, s>>>(x, n, vec, b.st, 0, b.cg, b.ce);
    LAUNCH_CHECK("topk_count_kernel");
    topk_scan_kernel<<<dim3(1), dim3(kSelThreads), 0, s>>>(b.cg, b.ce, nb, gs, b.og, b.oe);
    LAUNCH_CHECK("topk_scan_kernel");
    topk_write_kernel<T><<<dim3((unsigned)nb), dim3(kSampleThreads), 0, s>>>(x, n, vec, b.st, 0, 0, b.cg, b.ce, b.og, b.oe, k,
                                                                             nullptr, b.idx, (T*)b.el, b.p);
    LAUNCH_CHECK("topk_write_kernel");
    return CTG_OK;
}

int floor_log2(int64_t v) {
    int l = 0;
    while ((v >> l) > 1) ++l;
    return l;
}

// fast route: out (device, m doubles) <- the marginal under the keep bitmask `mask` of the n = 2^L >= 4096 elements
template <typename T>
int marginal_fast(ctg_exec* e, int64_t n, int64_t mask, double* A, double* B, double* out) {
    const T* x = (const T*)e->d_result;
    const int vec = ((uintptr_t)e->d_result & 15) == 0 ? 1 : 0;
    hipStream_t st = e->stream;
    const uint32_t lomask = (uint32_t)(mask & (kSampleBlock - 1));
    const int clo = __builtin_popcount(lomask);
    const int64_t hm = mask >> 12, nb = n / kSampleBlock;
    const int s = std::min(floor_log2(nb), floor_log2(CTG_MARGINAL_PARTIALS) - clo);   // a slab: 2^s blocks
    const int64_t nbs = 1ll << s;
    const uint32_t keepm = (uint32_t)(hm & (nbs - 1)), dropm = (uint32_t)(~hm & (nbs - 1));
    const int chl = __builtin_popcount(keepm);
    const int64_t mo = 1ll << (chl + clo);   // outputs a slab adds to
    const int64_t r = 1ll << (s - chl);      // blocks per output inside a slab
    const int64_t rc = std::min<int64_t>(r, kMargChunk), nch = r / rc;
    const int64_t hs = hm >> s;              // the keep mask of the slab number
    for (int64_t sb = 0; sb < nb / nbs; ++sb) {
        marg_block_kernel<T><<<dim3((unsigned)nbs), dim3(kSampleThreads), 0, st>>>(x, n, vec, sb * nbs, lomask, A);
        LAUNCH_CHECK("marg_block_kernel");
        const int64_t total = mo * nch;
        marg_gather_kernel<<<dim3((unsigned)((total + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(
            A, clo, keepm, dropm, mo, rc, total, B);
        LAUNCH_CHECK("marg_gather_kernel");
        // the slab's outputs; the first slab that reaches them stores, the later ones add
        const int64_t jbase = extract_bits(sb, hs) << (chl + clo);
        const int accumulate = (sb & ~hs) != 0 ? 1 : 0;
        marg_sum_kernel<<<dim3((unsigned)((mo + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(
            B, mo, nch, accumulate, out + jbase);
        LAUNCH_CHECK("marg_sum_kernel");
    }
    return CTG_OK;
}

template <typename T>
int marginal_general(ctg_exec* e, const MargAxes& ax, int64_t m, int64_t rc, double* B, double* out) {
    hipStream_t st = e->stream;
    const int64_t nch = (rc + kMargGeneralChunk - 1) / kMargGeneralChunk, total = m * nch;
    marg_general_kernel<T><<<dim3((unsigned)((total + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(
        (const T*)e->d_result, ax, m, rc, kMargGeneralChunk, total, B);
    LAUNCH_CHECK("marg_general_kernel");
    marg_sum_kernel<<<dim3((unsigned)((m + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(B, m, nch, 0,
                                                                                                                 out);
    LAUNCH_CHECK("marg_sum_kernel");
    return CTG_OK;
}

}  // namespace

// marginal_plan (ctg_rdm.hip shares it) and reduce_reserve (every later result-tensor source does) of ctg_exec_state.h
namespace ctg {

// the executor's scratch of this file, at least `want` bytes (the stream is idle: the statistics call synchronised it)
int reduce_reserve(ctg_exec* e, int64_t want) {
    if (e->reduce_bytes >= want) return CTG_OK;
    if (e->d_reduce) {
        HIP_TRY(hipFree(e->d_reduce));
        e->d_reduce = nullptr;
        e->reduce_bytes = 0;
    }
    HIP_TRY(hipMalloc(&e->d_reduce, (size_t)want));
    e->reduce_bytes = want;
    return CTG_OK;
}

// CTG_OK, or CTG_E_INVALID with *why set
int marginal_plan(int64_t rank, const int64_t* extents, const int32_t* keep, int64_t result_elems, MarginalPlan* out,
                  const char** why) {
    MarginalPlan p;
    if (rank > 0 && (!extents || !keep)) return *why = "null argument", CTG_E_INVALID;
    // the shape; a keep entry in front of the place where the shape is refused is named first: the axes are checked
    // one by one, the extent, the keep entry and the running product of each
    ResultShape shape;
    const char* bad = nullptr;
    const bool whole = rank == 0 && result_elems > 1;
    if (!whole) result_shape(rank, extents, result_elems, &shape, &bad);
    for (int64_t a = 0; a < rank && (a < shape.stop || (a == shape.stop && extents[a] >= 1)); ++a)
        if (keep[a] != 0 && keep[a] != 1) return *why = "a keep entry is neither 0 nor 1", CTG_E_INVALID;
    if (bad) return *why = bad, CTG_E_INVALID;
    p.n = shape.n;
    std::vector<int64_t> ext;
    std::vector<int> kp;
    for (int64_t a = 0; a < rank; ++a) {
        if (keep[a]) p.m *= extents[a];
        if (extents[a] == 1) continue;
        if (!kp.empty() && kp.back() == keep[a]) {
            ext.back() *= extents[a];
        } else {
            ext.push_back(extents[a]);
            kp.push_back(keep[a]);
        }
    }
    if (whole) {
        // (no shape given: the whole tensor as one dropped axis)
        p.n = result_elems;
        ext.push_back(result_elems);
        kp.push_back(0);
    }
    p.rc = p.n / p.m;
    bool pow2 = true;
    for (int64_t v : ext) pow2 = pow2 && (v & (v - 1)) == 0;
    p.fast = pow2 && p.n >= kSampleBlock;
    int64_t stride = 1;
    for (int a = (int)ext.size() - 1; a >= 0; --a) {
        if (kp[a]) p.mask |= (ext[a] - 1) * stride;   // (for the fast route: the axis' bits of the flat index)
        stride *= ext[a];
    }
    stride = 1;
    std::vector<int64_t> str(ext.size());
    for (int a = (int)ext.size() - 1; a >= 0; --a) {
        str[a] = stride;
        stride *= ext[a];
    }
    for (size_t a = 0; a < ext.size(); ++a) {
        int& cnt = kp[a] ? p.ax.nk : p.ax.nd;
        if (cnt >= kMargMaxAxes) return *why = "too many axes", CTG_E_INVALID;   // (not reachable: extents >= 2 alternate)
        (kp[a] ? p.ax.kext : p.ax.dext)[cnt] = ext[a];
        (kp[a] ? p.ax.kstr : p.ax.dstr)[cnt] = str[a];
        ++cnt;
    }
    *out = p;
    return CTG_OK;
}

}  // namespace ctg

extern "C" {

int ctg_exec_result_topk(ctg_exec* e, int64_t k, int64_t* idx, void* elems, double* p) {
    if (!e || !idx) return result_fail(CTG_E_INVALID, "null argument");
    const int64_t n = e->plan->result_elems;
    if (k < 1 || k > n || k > CTG_TOPK_MAX)
        return result_fail(CTG_E_INVALID, "k = %lld: need 1 <= k <= min(result_elems = %lld, CTG_TOPK_MAX = %d)", (long long)k,
                     (long long)n, CTG_TOPK_MAX);
    if (n > kReduceMaxElems) return result_fail(CTG_E_INVALID, "result tensor too large (%lld elements)", (long long)n);
    int rc = result_norm_finite(e, "no top-k of it");
    if (rc != CTG_OK) return rc;
    const int64_t nb = (n + kSampleBlock - 1) / kSampleBlock;
    const int grid = (int)std::min<int64_t>(nb, kHistMaxGrid);
    rc = reduce_reserve(e, topk_carve(nullptr, nb, grid, k).bytes);
    if (rc != CTG_OK) return rc;
    const TopkBufs b = topk_carve(e->d_reduce, nb, grid, k);
    rc = dispatch_elem(e->plan->dtype, [&](auto t) { return topk_run<decltype(t)>(e, b, n, nb, grid, k); });
    if (rc != CTG_OK) return rc;
    const int64_t isz = ctg_item_size(e->plan->dtype);
    std::vector<int64_t> hi((size_t)k);
    std::vector<double> hp((size_t)k);
    std::vector<char> he((size_t)(k * isz));
    HIP_TRY(hipMemcpyAsync(hi.data(), b.idx, k * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(hp.data(), b.p, k * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(he.data(), b.el, k * isz, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    // the order of the k records: p descending, the lower index first among equals (host; only k records came over)
    std::vector<int64_t> ord((size_t)k);
    std::iota(ord.begin(), ord.end(), (int64_t)0);
    std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t c) { return hp[a] > hp[c] || (hp[a] == hp[c] && hi[a] < hi[c]); });
    for (int64_t r = 0; r < k; ++r) {
        const int64_t s = ord[r];
        idx[r] = hi[s];
        if (p) p[r] = hp[s];
        if (elems) memcpy((char*)elems + r * isz, he.data() + s * isz, (size_t)isz);
    }
    return CTG_OK;
}

int ctg_exec_result_marginal(ctg_exec* e, int64_t rank, const int64_t* extents, const int32_t* keep, double* out) {
    if (!e || !out) return result_fail(CTG_E_INVALID, "null argument");
    MarginalPlan mp;
    const char* why = "";
    if (marginal_plan(rank, extents, keep, e->plan->result_elems, &mp, &why) != CTG_OK)
        return result_fail(CTG_E_INVALID, "marginal: %s", why);
    int rc = result_norm_finite(e, "no marginal of it");
    if (rc != CTG_OK) return rc;
    // [out: m | A: partials of a slab | B: per-chunk sums]
    int64_t a_elems = 0, b_elems = 0;
    if (mp.fast) {
        a_elems = std::min<int64_t>(mp.n, CTG_MARGINAL_PARTIALS);
        b_elems = a_elems;
    } else {
        b_elems = mp.m * ((mp.rc + kMargGeneralChunk - 1) / kMargGeneralChunk);
    }
    double *d_out = nullptr, *A = nullptr, *B = nullptr;
    auto lay = [&](void* base) {
        Carve c(base);
        d_out = c.take<double>(mp.m * 8);
        A = c.take<double>(a_elems * 8);
        B = c.take<double>(b_elems * 8);
        return c.bytes();
    };
    rc = reduce_reserve(e, lay(nullptr));
    if (rc != CTG_OK) return rc;
    lay(e->d_reduce);
    if (mp.fast)
        rc = dispatch_elem(e->plan->dtype, [&](auto t) { return marginal_fast<decltype(t)>(e, mp.n, mp.mask, A, B, d_out); });
    else
        rc = dispatch_elem(e->plan->dtype, [&](auto t) { return marginal_general<decltype(t)>(e, mp.ax, mp.m, mp.rc, B, d_out); });
    if (rc != CTG_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, d_out, mp.m * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CTG_OK;
}

}  // extern "C"
