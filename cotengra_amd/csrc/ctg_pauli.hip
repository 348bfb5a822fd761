// ctg_pauli.hip -- expectation values <x| P |x> of Pauli strings P over the axes of the executor's result tensor on
// the device (ctg_exec_result_pauli of include/ctg_hip.h).
//
// A string gives every axis one of I, X, Y, Z (0 .. 3); an axis that is not I has extent 2.  On the flat index a string
// is xm (the bits of its X and Y axes), zm (the bits of its Z and Y axes) and ny (its number of Y):
//
//   S = sum over j of (-1)^popcount(j & zm) conj(x[j ^ xm]) x[j],     value = (-1)^ceil(ny / 2) (ny even ? Re S : Im S)
//
// The terms j and j ^ xm are conjugates of each other up to (-1)^ny, so for xm != 0 only one member of every unordered
// pair {j, j ^ xm} is summed -- the one whose lowest set bit of xm is clear -- and the sum is DOUBLED, exactly, at the
// end (pauli_finish_kernel); for xm = 0 the term is |x[j]|^2 and every j is summed.  Every product is formed in fp64
// (exact for float / complex64 elements) and never fused with a sum; every sum is in fp64; no atomics.  One
// accumulator per string: the bits of a value are a function of (dtype, extents, the string, the tensor's bytes) alone
// -- not of the other strings of the call, their order, earlier calls or the executor.
//
// The host groups the strings of a call by xm (groups in order of first appearance, the caller's order inside a group)
// and runs every group in passes of at most kPauliPass = 32 strings; a pass reads the tensor once.  Two routes:
//
//   power of two (every extent a power of two, at least kResultChunk = 4096 elements):
//
//     pauli_chunk_kernel<T>   256 threads, two workgroups per CU.  A chunk is 4096 consecutive elements, thread t holds
//                             the 16-byte groups g 256 + t (load_group).  xm = xm_hi 4096 + xm_lo:
//                               xm_hi = 0:  a workgroup takes the chunks wg, wg + grid, ...; the partner of element e is
//                                           element e ^ xm_lo of the same chunk;
//                               xm_hi != 0: a workgroup takes the chunk pairs (c, c ^ xm_hi), c the q-th chunk whose
//                                           lowest set bit of xm_hi is clear, q = wg, wg + grid, ...; it sums the
//                                           elements of c, the partner of e is element e ^ xm_lo of chunk c ^ xm_hi.
//                             The partner comes from an LDS copy of the (partner) chunk, read as the 16-byte group
//                             (g 256 + t) ^ (xm_lo / V) -- an xor permutes the groups inside aligned blocks, so the
//                             lanes of a wave stay on different banks -- and a partner inside the thread's own group
//                             (xm_lo < V = 16 / sizeof(T)) needs no LDS.  Signs: the word of sign bits of an element,
//                             one bit per string of the pass, is parity(e & zm) -- the same in every chunk, computed
//                             once per thread -- xor parity(chunk base & zm), one wave-uniform word per chunk.  Per
//                             element and string one component (Re or Im of conj(partner) x, by ny & 1), its sign bit
//                             flipped by the word's bit, is added to the string's accumulator: 32 fp64 accumulators
//                             per thread; a shift, a bit-field insert and the addition per (element, string).  At
//                             the end the waves are added in wave order and the lanes in lane order through LDS, and
//                             the workgroup writes one partial of 32 doubles.
//     pauli_gather_kernel     adds the partials of kPauliSumChunk = 32 consecutive workgroups in ascending order;
//     pauli_finish_kernel     adds those in ascending order, multiplies by (-1)^ceil(ny / 2) (x 2 for xm != 0) and
//                             writes the value to the string's place in the caller's order.
//
//     grid = result_chunk_grid(units) = min(512, ceil(units / 3)), units = chunks (xm_hi = 0) or chunk pairs: a function
//     of (n, xm_hi != 0) alone.
//
//   general (any other shape): pauli_general_kernel<T>, one work item per (string, chunk of max(1024, ceil(n / 1024))
//   flat indices), walks its chunk serially: the digit of a non-identity axis is (j / stride) & 1, the partner j +-
//   stride per X / Y axis, the sign the parity of the digits of the Z / Y axes; every j is summed (no halving).
//   pauli_general_finish_kernel adds the chunks in ascending order.  Not tuned.
//
// A string with odd ny of a real tensor is exactly 0.0 and is written on the host without a launch.
//
// Scratch (the executor's d_reduce, reduce_reserve): 8 m bytes of values; power-of-two route: 648
// bytes per pass (at most m passes), 128 KiB of partials, 4 KiB of group sums -- 2.8 MiB at most; general route: 32
// bytes per string, 12 bytes per non-identity letter and 8 bytes per (string, chunk of at most 1024): 35 MiB at most.
#include <algorithm>
#include <type_traits>
#include <unordered_map>

#include "ctg_result_elem.h"
#include "ctg_result_host.h"

namespace ctg {

constexpr int kPauliPass = 32;                   // strings of a pass: one bit each in a sign word
constexpr int kPauliSumChunk = 32;               // partials per work item of pauli_gather_kernel
constexpr int64_t kPauliGeneralChunk = 1024;     // flat indices per work item of the general route, at least
constexpr int64_t kPauliGeneralMaxChunks = 1024; // ... and at most this many chunks per string

// What a pass of the power-of-two route needs on the device
struct PauliPassMeta {
    int64_t zm[kPauliPass];    // the Z / Y bits of string s of the pass
    double fac[kPauliPass];    // (-1)^ceil(ny / 2), times 2 where pairs were halved
    int32_t pos[kPauliPass];   // its place in the caller's order
    uint32_t odd;              // bit s: ny of string s is odd (the imaginary component is summed)
    int32_t count;
};

// One string of the general route: its non-identity axes are ax0 .. ax0 + nax - 1 of the axis lists
struct PauliGenString {
    int64_t ax0;
    int32_t nax, odd;
    double fac;
    int32_t pos, pad;
};

// Re and Im of conj(p) x, each product rounded once (exact for float / complex64), never fused
template <typename T> struct PauliElem;
template <> struct PauliElem<float> {
    static constexpr int P = 1;
    static __device__ __forceinline__ void term(float p, float x, double& re, double& im) {
#pragma clang fp contract(off)
        re = (double)p * (double)x;
        im = 0.0;
    }
};
template <> struct PauliElem<double> {
    static constexpr int P = 1;
    static __device__ __forceinline__ void term(double p, double x, double& re, double& im) {
#pragma clang fp contract(off)
        re = p * x;
        im = 0.0;
    }
};
template <> struct PauliElem<float2> {
    static constexpr int P = 2;
    static __device__ __forceinline__ void term(float2 p, float2 x, double& re, double& im) {
#pragma clang fp contract(off)
        const double a = (double)p.x, b = (double)p.y, c = (double)x.x, d = (double)x.y;
        const double ac = a * c, bd = b * d, ad = a * d, bc = b * c;
        re = ac + bd;
        im = ad - bc;
    }
};
template <> struct PauliElem<double2> {
    static constexpr int P = 2;
    static __device__ __forceinline__ void term(double2 p, double2 x, double& re, double& im) {
#pragma clang fp contract(off)
        const double ac = p.x * x.x, bd = p.y * x.y, ad = p.x * x.y, bc = p.y * x.x;
        re = ac + bd;
        im = ad - bc;
    }
};

template <typename T>
__global__ __launch_bounds__(kSampleThreads, 2) void pauli_chunk_kernel(const T* __restrict__ x, int64_t n, int vec, int64_t xm,
                                                                        int64_t units, const PauliPassMeta* __restrict__ pass,
                                                                        double* __restrict__ part) {
#pragma clang fp contract(off)
    constexpr int P = PauliElem<T>::P;
    constexpr int V = 16 / sizeof(T);
    constexpr int LV = V == 4 ? 2 : V == 2 ? 1 : 0;
    constexpr int G = kResultChunk / V / kSampleThreads;
    constexpr int kChunkBytes = kResultChunk * (int)sizeof(T), kSumBytes = kPauliPass * 64 * 8;
    __shared__ __attribute__((aligned(16))) unsigned char raw[kChunkBytes > kSumBytes ? kChunkBytes : kSumBytes];
    __shared__ double r2[kPauliPass * 8];
    uint4* l4 = reinterpret_cast<uint4*>(raw);
    double* xs = reinterpret_cast<double*>(raw);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t xlo = (uint32_t)(xm & (kResultChunk - 1));
    const int64_t xhi = xm >> kResultChunkBits;
    const uint32_t xin = xlo & (V - 1), xg = xlo >> LV;
    const bool use_lds = xg != 0;
    // xm_hi = 0, xm != 0: of the pair {e, e ^ xm_lo} the member whose lowest set bit of xm_lo is clear is summed
    const uint32_t skip = (xhi == 0 && xlo != 0) ? (xlo & (0u - xlo)) : 0u;
    const int lb = xhi ? __builtin_ctzll((unsigned long long)xhi) : 0;
    const int count = pass->count;
    const uint32_t odd = pass->odd;
    const int64_t myzm = pass->zm[lane & (kPauliPass - 1)];

    // the sign words of this thread's elements: bit s = parity(e & zm_s), the same in every chunk
    uint32_t es[G * V];
#pragma unroll
    for (int i = 0; i < G * V; ++i) es[i] = 0;
    for (int s = 0; s < count; ++s) {
        const uint32_t z = (uint32_t)(pass->zm[s] & (kResultChunk - 1));
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const uint32_t e = (uint32_t)(g * kSampleThreads + tid) * V + k;
                es[g * V + k] |= (uint32_t)(__popc(e & z) & 1) << s;
            }
    }

    double acc[kPauliPass];
#pragma unroll
    for (int s = 0; s < kPauliPass; ++s) acc[s] = 0.0;

    // unit q's own chunk: c = q, or the q-th chunk whose lowest set bit of xm_hi is clear
    auto chunk_of = [&](int64_t q) { return xhi ? (((q >> lb) << (lb + 1)) | (q & (((int64_t)1 << lb) - 1))) : q; };
    // (loading the next unit's chunk while this one is summed was measured slower than leaving the overlap to the
    // second workgroup of the CU)
    Group<T> st[G];
    // ODD: some string of the pass has an odd number of Y and takes the imaginary component (never for xm = 0)
    auto sum_units = [&](auto odd_tag) {
        constexpr bool ODD = decltype(odd_tag)::value;
        for (int64_t q = blockIdx.x; q < units; q += gridDim.x) {
            const int64_t c = chunk_of(q);
            const int64_t base = c << kResultChunkBits, base2 = (c ^ xhi) << kResultChunkBits;
            // the chunk's sign word: lane s holds parity(base & zm_s); wave-uniform
            const uint32_t cw = (uint32_t)__ballot(__popcll((unsigned long long)(base & myzm)) & 1);
#pragma unroll
            for (int g = 0; g < G; ++g) load_group<T>(x, base + (int64_t)(g * kSampleThreads + tid) * V, n, vec != 0, st[g].v);
            if (use_lds) {
                __syncthreads();   // (the unit before has read the copy)
                if (xhi) {
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        Group<T> t;
                        load_group<T>(x, base2 + (int64_t)(g * kSampleThreads + tid) * V, n, vec != 0, t.v);
                        l4[g * kSampleThreads + tid] = t.raw;
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < G; ++g) l4[g * kSampleThreads + tid] = st[g].raw;
                }
                __syncthreads();
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                Group<T> pg;
                if (use_lds)
                    pg.raw = l4[(uint32_t)(g * kSampleThreads + tid) ^ xg];
                else if (xhi)
                    load_group<T>(x, base2 + (int64_t)(g * kSampleThreads + tid) * V, n, vec != 0, pg.v);
                else
                    pg = st[g];
                // the partner inside the group: element k ^ xin
                if (V >= 2 && (xin & 1u)) {
                    Group<T> t = pg;
#pragma unroll
                    for (int k = 0; k < V; ++k) pg.v[k] = t.v[k ^ (V >= 2 ? 1 : 0)];
                }
                if (V >= 4 && (xin & 2u)) {
                    Group<T> t = pg;
#pragma unroll
                    for (int k = 0; k < V; ++k) pg.v[k] = t.v[k ^ (V >= 4 ? 2 : 0)];
                }
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const uint32_t e = (uint32_t)(g * kSampleThreads + tid) * V + k;
                    if (e & skip) continue;
                    double re, im;
                    PauliElem<T>::term(pg.v[k], st[g].v[k], re, im);
                    const uint32_t w = es[g * V + k] ^ cw;
                    // the component's own sign goes into the word: bit s of wr is the sign of string s's term, which
                    // then replaces the sign bit -- a shift, a bit-field insert and the addition per string
                    // (the same bits as signed_by(re, w >> s), which the passes with a choice of component use)
                    const int rh = __double2hiint(re), rl = __double2loint(re);
                    const uint32_t wr = w ^ (uint32_t)(rh >> 31);
#pragma unroll
                    for (int s = 0; s < kPauliPass; ++s) {
                        // Wave-uniform exits after 1, 2, 4, 8 and 16 strings only: inside such a block the strings'
                        // additions are independent and interleave; a slot past the pass's last string sums a value
                        // nobody reads
                        if ((s & (s - 1)) == 0 && s >= count) break;
                        if (ODD) {
                            acc[s] = acc[s] + signed_by(((odd >> s) & 1u) ? im : re, w >> s);
                        } else {
                            const uint32_t t = wr << (31 - s);
                            acc[s] = acc[s] + __hiloint2double((int)((t & 0x80000000u) | ((uint32_t)rh & 0x7fffffffu)), rl);
                        }
                    }
                }
            }
        }
    };
    if (P == 2 && odd != 0)
        sum_units(std::true_type{});
    else
        sum_units(std::false_type{});

    // the waves in wave order, then the lanes in lane order (eight runs of eight), through LDS
    for (int w = 0; w < kSampleThreads / 64; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int s = 0; s < kPauliPass; ++s) xs[s * 64 + lane] = w == 0 ? acc[s] : xs[s * 64 + lane] + acc[s];
        }
    }
    __syncthreads();
    {
        double v = xs[tid * 8];
        for (int i = 1; i < 8; ++i) v = v + xs[tid * 8 + i];
        r2[tid] = v;
    }
    __syncthreads();
    if (tid < kPauliPass) {
        double v = r2[tid * 8];
        for (int i = 1; i < 8; ++i) v = v + r2[tid * 8 + i];
        part[(int64_t)blockIdx.x * kPauliPass + tid] = v;
    }
}

// B[gr 32 + s] <- part[(gr kPauliSumChunk + i) 32 + s] for i = 0, 1, ... in that order (np partials of 32 doubles)
__global__ __launch_bounds__(kSampleThreads) void pauli_gather_kernel(const double* __restrict__ part, int np, int total,
                                                                      double* __restrict__ B) {
    const int g = blockIdx.x * kSampleThreads + threadIdx.x;
    if (g >= total) return;
    const int s = g % kPauliPass, gr = g / kPauliPass;
    const int p0 = gr * kPauliSumChunk, p1 = p0 + kPauliSumChunk < np ? p0 + kPauliSumChunk : np;
    double v = part[(int64_t)p0 * kPauliPass + s];
    for (int p = p0 + 1; p < p1; ++p) v = v + part[(int64_t)p * kPauliPass + s];
    B[g] = v;
}

// out[pos[s]] <- fac[s] (B[s] + B[32 + s] + ...), the ng group sums in ascending order
__global__ __launch_bounds__(64) void pauli_finish_kernel(const double* __restrict__ B, int ng,
                                                          const PauliPassMeta* __restrict__ pass, double* __restrict__ out) {
    const int s = threadIdx.x;
    if (s >= pass->count) return;
    double v = B[s];
    for (int gr = 1; gr < ng; ++gr) v = v + B[gr * kPauliPass + s];
    out[pass->pos[s]] = pass->fac[s] * v;
}

// Work item (string i, chunk ch): B[ch ns + i] <- the sum of sign(j) comp(conj(x[partner(j)]) x[j]) over the flat
// indices j of the chunk, serially
template <typename T>
__global__ __launch_bounds__(kSampleThreads) void pauli_general_kernel(const T* __restrict__ x, int64_t n,
                                                                       const PauliGenString* __restrict__ strs,
                                                                       const int64_t* __restrict__ stride,
                                                                       const int32_t* __restrict__ kind, int ns, int64_t chunk,
                                                                       int64_t total, double* __restrict__ B) {
#pragma clang fp contract(off)
    const int64_t g = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
    if (g >= total) return;
    const int i = (int)(g % ns);
    const int64_t ch = g / ns;
    const PauliGenString st = strs[i];
    const int64_t j0 = ch * chunk, j1 = j0 + chunk < n ? j0 + chunk : n;
    double sum = 0.0;
    for (int64_t j = j0; j < j1; ++j) {
        int64_t p = j;
        uint32_t sign = 0;
        for (int a = 0; a < st.nax; ++a) {
            const int64_t sa = stride[st.ax0 + a];
            const int32_t ka = kind[st.ax0 + a];
            const uint32_t d = (uint32_t)((j / sa) & 1);
            if (ka != 3) p += d ? -sa : sa;   // X, Y: the other value of the axis
            if (ka != 1) sign ^= d;           // Z, Y: the digit's parity
        }
        double re, im;
        PauliElem<T>::term(x[p], x[j], re, im);
        const double v = signed_by(st.odd ? im : re, sign);
        sum = j == j0 ? v : sum + v;
    }
    B[g] = sum;
}

__global__ __launch_bounds__(kSampleThreads) void pauli_general_finish_kernel(const double* __restrict__ B, int ns, int64_t nch,
                                                                              const PauliGenString* __restrict__ strs,
                                                                              double* __restrict__ out) {
    const int i = blockIdx.x * kSampleThreads + threadIdx.x;
    if (i >= ns) return;
    double v = B[i];
    for (int64_t ch = 1; ch < nch; ++ch) v = v + B[ch * ns + i];
    out[strs[i].pos] = strs[i].fac * v;
}

}  // namespace ctg

using namespace ctg;

namespace {

double pauli_factor(int ny, bool halved) {
    const double f = (((ny + 1) / 2) & 1) ? -1.0 : 1.0;   // (-1)^ceil(ny / 2)
    return halved ? 2.0 * f : f;
}

// one pass of the power-of-two route: the grid is a function of (n, xm_hi != 0) alone
template <typename T>
int pauli_pass_launch(ctg_exec* e, int64_t n, int64_t xm, const PauliPassMeta* d_pass, double* part, double* B, double* d_out) {
    hipStream_t st = e->stream;
    const int vec = ((uintptr_t)e->d_result & 15) == 0 ? 1 : 0;
    const int64_t nchunks = n / kResultChunk;
    const int64_t units = (xm >> kResultChunkBits) ? nchunks / 2 : nchunks;
    const int grid = result_chunk_grid(units);
    const int ngroups = (grid + kPauliSumChunk - 1) / kPauliSumChunk;
    pauli_chunk_kernel<T><<<dim3((unsigned)grid), dim3(kSampleThreads), 0, st>>>((const T*)e->d_result, n, vec, xm, units, d_pass, part);
    LAUNCH_CHECK("pauli_chunk_kernel");
    const int total = ngroups * kPauliPass;
    pauli_gather_kernel<<<dim3((unsigned)((total + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(part, grid,
                                                                                                                        total, B);
    LAUNCH_CHECK("pauli_gather_kernel");
    pauli_finish_kernel<<<dim3(1), dim3(64), 0, st>>>(B, ngroups, d_pass, d_out);
    LAUNCH_CHECK("pauli_finish_kernel");
    return CTG_OK;
}

template <typename T>
int pauli_general_launch(ctg_exec* e, int64_t n, const PauliGenString* d_strs, const int64_t* d_stride, const int32_t* d_kind,
                         int ns, int64_t chunk, int64_t nch, double* B, double* d_out) {
    hipStream_t st = e->stream;
    const int64_t total = (int64_t)ns * nch;
    pauli_general_kernel<T><<<dim3((unsigned)((total + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(
        (const T*)e->d_result, n, d_strs, d_stride, d_kind, ns, chunk, total, B);
    LAUNCH_CHECK("pauli_general_kernel");
    pauli_general_finish_kernel<<<dim3((unsigned)((ns + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, st>>>(
        B, ns, nch, d_strs, d_out);
    LAUNCH_CHECK("pauli_general_finish_kernel");
    return CTG_OK;
}

}  // namespace

extern "C" int ctg_exec_result_pauli(ctg_exec* e, int64_t rank, const int64_t* extents, int64_t m, const uint8_t* ops,
                                     double* out) {
    if (!e || !extents || !ops || !out) return result_fail(CTG_E_INVALID, "pauli: null argument");
    ResultShape shape;
    const char* why = "";
    if (result_shape(rank, extents, e->plan->result_elems, &shape, &why) != CTG_OK) return result_fail(CTG_E_INVALID, "pauli: %s", why);
    const int64_t n = shape.n;
    const std::vector<int64_t>& stride = shape.strides;
    if (m < 0 || m > CTG_PAULI_MAX_STRINGS)
        return result_fail(CTG_E_INVALID, "pauli: %lld strings; between 0 and CTG_PAULI_MAX_STRINGS = %d", (long long)m,
                     CTG_PAULI_MAX_STRINGS);
    for (int64_t s = 0; s < m; ++s)
        for (int64_t a = 0; a < rank; ++a) {
            const uint8_t op = ops[s * rank + a];
            if (op > 3) return result_fail(CTG_E_INVALID, "pauli: string %lld, axis %lld: code %d is none of 0 .. 3", (long long)s, (long long)a, (int)op);
            if (op != 0 && extents[a] != 2)
                return result_fail(CTG_E_INVALID, "pauli: string %lld puts a letter other than I on axis %lld of extent %lld", (long long)s,
                             (long long)a, (long long)extents[a]);
        }
    if (m == 0) return CTG_OK;
    int rc = result_norm_finite(e, "no expectation values of it");
    if (rc != CTG_OK) return rc;
    const int dtype = e->plan->dtype;
    const bool real = dtype == CTG_F32 || dtype == CTG_F64;
    // a string of a real tensor with an odd number of Y is exactly zero: no launch
    std::vector<int> ny((size_t)m, 0);
    std::vector<char> launched((size_t)m, 1);
    int64_t nlaunched = 0;
    for (int64_t s = 0; s < m; ++s) {
        for (int64_t a = 0; a < rank; ++a) ny[s] += ops[s * rank + a] == 2;
        if (real && (ny[s] & 1)) launched[s] = 0;
        nlaunched += launched[s];
    }
    std::vector<double> values((size_t)m, 0.0);
    const int64_t out_bytes = m * 8;
    if (nlaunched == 0) {
        for (int64_t s = 0; s < m; ++s) out[s] = 0.0;
        return CTG_OK;
    }
    if (shape.pow2 && n >= kResultChunk) {
        // groups by xm in order of first appearance, the caller's order inside; passes of at most kPauliPass
        std::vector<int64_t> gx;
        std::vector<std::vector<int64_t>> members;
        std::unordered_map<int64_t, size_t> where;
        std::vector<int64_t> zm((size_t)m, 0);
        for (int64_t s = 0; s < m; ++s) {
            if (!launched[s]) continue;
            int64_t xm = 0;
            for (int64_t a = 0; a < rank; ++a) {
                const uint8_t op = ops[s * rank + a];
                if (op == 1 || op == 2) xm |= stride[a];
                if (op == 3 || op == 2) zm[s] |= stride[a];
            }
            auto it = where.find(xm);
            if (it == where.end()) {
                it = where.emplace(xm, gx.size()).first;
                gx.push_back(xm);
                members.emplace_back();
            }
            members[it->second].push_back(s);
        }
        std::vector<PauliPassMeta> passes;
        std::vector<int64_t> pass_xm;
        for (size_t g = 0; g < gx.size(); ++g)
            for (size_t i0 = 0; i0 < members[g].size(); i0 += kPauliPass) {
                PauliPassMeta pm{};
                pm.count = (int32_t)std::min<size_t>(kPauliPass, members[g].size() - i0);
                for (int i = 0; i < pm.count; ++i) {
                    const int64_t s = members[g][i0 + i];
                    pm.zm[i] = zm[s];
                    pm.fac[i] = pauli_factor(ny[s], gx[g] != 0);
                    pm.pos[i] = (int32_t)s;
                    if (ny[s] & 1) pm.odd |= 1u << i;
                }
                passes.push_back(pm);
                pass_xm.push_back(gx[g]);
            }
        // [values: m | the passes | partials of the workgroups | sums of groups of partials]
        const int64_t pass_bytes = (int64_t)passes.size() * (int64_t)sizeof(PauliPassMeta);
        const int64_t part_bytes = (int64_t)kResultMaxGrid * kPauliPass * 8;
        const int64_t b_bytes = (int64_t)((kResultMaxGrid + kPauliSumChunk - 1) / kPauliSumChunk) * kPauliPass * 8;
        double *d_out = nullptr, *part = nullptr, *B = nullptr;
        PauliPassMeta* d_pass = nullptr;
        auto lay = [&](void* base) {
            Carve c(base);
            d_out = c.take<double>(out_bytes);
            d_pass = c.take<PauliPassMeta>(pass_bytes);
            part = c.take<double>(part_bytes);
            B = c.take<double>(b_bytes);
            return c.bytes();
        };
        rc = reduce_reserve(e, lay(nullptr));
        if (rc != CTG_OK) return rc;
        lay(e->d_reduce);
        HIP_TRY(hipMemcpyAsync(d_pass, passes.data(), (size_t)pass_bytes, hipMemcpyHostToDevice, e->stream));
        for (size_t p = 0; p < passes.size(); ++p) {
            rc = dispatch_elem(dtype, [&](auto t) { return pauli_pass_launch<decltype(t)>(e, n, pass_xm[p], d_pass + p, part, B, d_out); });
            if (rc != CTG_OK) return rc;
        }
        HIP_TRY(hipMemcpyAsync(values.data(), d_out, (size_t)out_bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    } else {
        std::vector<PauliGenString> strs;
        std::vector<int64_t> ax_stride;
        std::vector<int32_t> ax_kind;
        for (int64_t s = 0; s < m; ++s) {
            if (!launched[s]) continue;
            PauliGenString gs{};
            gs.ax0 = (int64_t)ax_stride.size();
            for (int64_t a = 0; a < rank; ++a) {
                const uint8_t op = ops[s * rank + a];
                if (op == 0) continue;
                ax_stride.push_back(stride[a]);
                ax_kind.push_back((int32_t)op);
                ++gs.nax;
            }
            gs.odd = ny[s] & 1;
            gs.fac = pauli_factor(ny[s], false);
            gs.pos = (int32_t)s;
            strs.push_back(gs);
        }
        const int ns = (int)strs.size();
        const int64_t chunk = std::max<int64_t>(kPauliGeneralChunk, (n + kPauliGeneralMaxChunks - 1) / kPauliGeneralMaxChunks);
        const int64_t nch = (n + chunk - 1) / chunk;
        // [values: m | the strings | strides of their axes | kinds of their axes | one sum per (chunk, string)]
        const int64_t str_bytes = (int64_t)ns * (int64_t)sizeof(PauliGenString);
        const int64_t sa_bytes = (int64_t)ax_stride.size() * 8, ka_bytes = (int64_t)ax_kind.size() * 4;
        const int64_t b_bytes = (int64_t)ns * nch * 8;
        double *d_out = nullptr, *B = nullptr;
        PauliGenString* d_strs = nullptr;
        int64_t* d_stride = nullptr;
        int32_t* d_kind = nullptr;
        auto lay = [&](void* base) {
            Carve c(base);
            d_out = c.take<double>(out_bytes);
            d_strs = c.take<PauliGenString>(str_bytes);
            d_stride = c.take<int64_t>(sa_bytes);
            d_kind = c.take<int32_t>(ka_bytes);
            B = c.take<double>(b_bytes);
            return c.bytes();
        };
        rc = reduce_reserve(e, lay(nullptr));
        if (rc != CTG_OK) return rc;
        lay(e->d_reduce);
        HIP_TRY(hipMemcpyAsync(d_strs, strs.data(), (size_t)str_bytes, hipMemcpyHostToDevice, e->stream));
        if (sa_bytes) {
            HIP_TRY(hipMemcpyAsync(d_stride, ax_stride.data(), (size_t)sa_bytes, hipMemcpyHostToDevice, e->stream));
            HIP_TRY(hipMemcpyAsync(d_kind, ax_kind.data(), (size_t)ka_bytes, hipMemcpyHostToDevice, e->stream));
        }
        rc = dispatch_elem(dtype, [&](auto t) { return pauli_general_launch<decltype(t)>(e, n, d_strs, d_stride, d_kind, ns, chunk, nch, B, d_out); });
        if (rc != CTG_OK) return rc;
        HIP_TRY(hipMemcpyAsync(values.data(), d_out, (size_t)out_bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    for (int64_t s = 0; s < m; ++s) out[s] = launched[s] ? values[s] : 0.0;
    return CTG_OK;
}
