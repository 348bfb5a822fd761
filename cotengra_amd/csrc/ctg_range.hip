// ctg_range.hip -- where a tensor's components lie below its largest one: the device pass of the range audit
// (ctg_exec_range_audit in ctg_runtime.hip drives it).
//
// The fp16 x 2 arithmetic keeps ONE power of two per operand tensor, so its absolute error is a fraction of the
// tensor's largest element and a component far below that loses its low bits.  Whether a tensor has such components
// is a question about its exponents.  For a contiguous run of n fp32 components (a float32 tensor as it is, a
// complex64 tensor as 2 elems floats) two kernels produce
//
//   hist[256]   component counts by biased exponent field (bits >> 23) & 0xff: bin 0 zeros and subnormals, bin 255
//               inf and NaN;
//   zeros       components equal to +-0;
//   sumsq       sum of x^2 in double over the finite components.
//
//   range_hist_kernel     workgroup b takes the chunks b, b + gridDim.x, ... of kRangeChunk components and leaves
//                         ONE row of per-workgroup counts and one partial sum;
//   range_reduce_kernel   one workgroup adds the rows and the partial sums.
//
// Counts are integers (LDS integer atomics; their order does not matter).  sumsq has a fixed association -- per
// thread in load order, then lanes (butterfly), then waves, then workgroups -- and the grid is a function of n
// alone, so the same bytes give the same 258 numbers on every run and on every executor.  No float atomics.
//
// A real tensor puts almost every component into a handful of neighbouring bins, and one LDS atomic per component
// would serialise on them.  Per chunk a wave therefore picks a WINDOW of kRangeWindow bins below the largest
// exponent its lanes see first; a lane counts the components inside the window in eight 8-bit fields of one 64-bit
// register (a shift and an add per component, equal bins of a lane combined for free), the wave adds the registers
// of its lanes by a butterfly on 16-bit fields and eight lanes make one LDS add each.  A component outside the
// window -- every zero, subnormal, inf and NaN among them: the window never holds bin 0 or 255 -- takes the slow
// path: the lanes that hold such a component agree on the first one's bin, a ballot counts its holders and one
// lane adds the count (up to kRangeFewLanes such lanes make one LDS add each instead: Gaussian-like data leaves a
// few per cent of its components below the window, a lane or two of most groups, each in a bin of its own).
#include <cstdint>

#include "ctg_exec_state.h"

namespace ctg {

constexpr int kRangeThreads = 256;
constexpr int kRangeGroups = 16;                                   // 16-byte groups per thread and chunk
constexpr int kRangeChunk = kRangeThreads * kRangeGroups * 4;      // components per chunk (64 KiB)
constexpr int kRangeWindow = 8;                                    // bins counted in registers
constexpr int kRangeFewLanes = 8;                                  // up to this many lanes on the slow path add one by one
static_assert(kRangeGroups * 4 < 256, "a lane's 8-bit fields hold the components of one chunk");
static_assert(kRangeGroups * 4 * 64 < 65536, "a wave's 16-bit fields hold the components of one chunk");

// x^2 in double: the product rounded once, never fused with the sum it goes into (SampleElem of ctg_sample.hip)
__device__ __forceinline__ double range_sq(uint32_t bits) {
#pragma clang fp contract(off)
    const double d = (double)__uint_as_float(bits);
    const double a = d * d;
    return a;
}

// The slow path, entered by any subset of a wave's lanes: hist[ex] += 1 for every lane in it, as one LDS add per
// distinct bin (the lanes agree on the first one's bin, a ballot counts the lanes that hold it).
__device__ __forceinline__ void range_count_slow(uint32_t ex, uint32_t* __restrict__ hist) {
    // (a few stragglers below the window, the usual case in the register path: they seldom share a bin and one add
    // each is cheaper than agreeing on bins)
    if (__popcll(__ballot(true)) <= kRangeFewLanes) {
        atomicAdd(&hist[ex], 1u);
        return;
    }
    bool todo = true;
    while (todo) {
        const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)ex);
        const bool mine = ex == b;
        const unsigned long long m = __ballot(mine);
        if (mine) {
            if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&hist[b], (uint32_t)__popcll(m));
            todo = false;
        }
    }
}

// The four components of the group at x + e (e a multiple of 4).  `vec`: x is 16-byte aligned (one 16-byte load);
// a group past the end, or any group of a misaligned tensor, is read component by component (0 past n: the caller
// does not count those).
__device__ __forceinline__ uint4 range_load(const uint32_t* __restrict__ x, int64_t e, int64_t n, bool vec) {
    if (vec && e + 4 <= n) return *reinterpret_cast<const uint4*>(x + e);
    uint4 r;
    r.x = e + 0 < n ? x[e + 0] : 0u;
    r.y = e + 1 < n ? x[e + 1] : 0u;
    r.z = e + 2 < n ? x[e + 2] : 0u;
    r.w = e + 3 < n ? x[e + 3] : 0u;
    return r;
}

// bh [gridDim.x][256] counts, bz [gridDim.x] zeros, bs [gridDim.x] partial sums of squares
__global__ __launch_bounds__(kRangeThreads) void range_hist_kernel(const uint32_t* __restrict__ x, int64_t n, int vec,
                                                                   int64_t nchunks, uint32_t* __restrict__ bh,
                                                                   uint32_t* __restrict__ bz, double* __restrict__ bs) {
#pragma clang fp contract(off)
    __shared__ uint32_t hist[256];
    __shared__ double ws[kRangeThreads / 64];
    __shared__ uint32_t wz[kRangeThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    hist[tid] = 0;
    __syncthreads();
    double s = 0.0;
    uint32_t zeros = 0;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t base = c * kRangeChunk;
        if (base + kRangeChunk <= n) {
            uint4 raw[kRangeGroups];
#pragma unroll
            for (int g = 0; g < kRangeGroups; ++g)
                raw[g] = range_load(x, base + ((int64_t)g * kRangeThreads + tid) * 4, n, vec != 0);
            // the window: kRangeWindow bins, the wave's largest finite exponent of its first groups second from the
            // top, never bin 0 or 255
            uint32_t top = 0;
            {
                const uint32_t u[4] = {raw[0].x, raw[0].y, raw[0].z, raw[0].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t ex = (u[k] >> 23) & 0xffu;
                    top = max(top, ex == 255u ? 0u : ex);
                }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, d, 64));
            top = (uint32_t)__builtin_amdgcn_readfirstlane((int)top);
            const uint32_t lo = min(max((int)top - (kRangeWindow - 2), 1), 255 - kRangeWindow);
            const uint32_t lo8 = lo * 8;
            unsigned long long pk = 0;   // eight 8-bit counts: bins lo ... lo + 7
#pragma unroll
            for (int g = 0; g < kRangeGroups; ++g) {
                const uint32_t u[4] = {raw[g].x, raw[g].y, raw[g].z, raw[g].w};
                uint32_t sh[4];
                double sq[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    sh[k] = ((u[k] >> 20) & 0x7f8u) - lo8;   // 8 (bin - lo): below 64 inside the window
                    pk += 1ull << (sh[k] & 63u);
                    sq[k] = range_sq(u[k]);
                }
                if ((sh[0] | sh[1] | sh[2] | sh[3]) >= 64u) {
                    // some component outside the window: take its count back out of the register
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (sh[k] >= 64u) {
                            const uint32_t ex = (u[k] >> 23) & 0xffu;
                            pk -= 1ull << (sh[k] & 63u);
                            range_count_slow(ex, hist);
                            zeros += (u[k] << 1) == 0u ? 1u : 0u;
                            if (ex == 255u) sq[k] = 0.0;
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) s += sq[k];
            }
            // the lanes' counts: even and odd fields apart (four 16-bit sums each), a butterfly, one LDS add per bin
            unsigned long long ev = pk & 0x00ff00ff00ff00ffull, od = (pk >> 8) & 0x00ff00ff00ff00ffull;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                ev += (unsigned long long)__shfl_xor((long long)ev, d, 64);
                od += (unsigned long long)__shfl_xor((long long)od, d, 64);
            }
            if (lane < kRangeWindow) {
                const uint32_t cnt = (uint32_t)(((lane & 1) ? od : ev) >> (16 * (lane >> 1))) & 0xffffu;
                if (cnt) atomicAdd(&hist[lo + lane], cnt);
            }
        } else {
            // the last chunk of a tensor whose size is no multiple of the chunk: every component by the slow path,
            // in the same order
#pragma unroll 1
            for (int g = 0; g < kRangeGroups; ++g) {
                const int64_t e = base + ((int64_t)g * kRangeThreads + tid) * 4;
                const uint4 raw = range_load(x, e, n, vec != 0);
                const uint32_t u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (e + k < n) {
                        const uint32_t ex = (u[k] >> 23) & 0xffu;
                        range_count_slow(ex, hist);
                        zeros += (u[k] << 1) == 0u ? 1u : 0u;
                        s += ex == 255u ? 0.0 : range_sq(u[k]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s += __shfl_xor(s, d, 64);
        zeros += (uint32_t)__shfl_xor((int)zeros, d, 64);
    }
    if (lane == 0) {
        ws[tid >> 6] = s;
        wz[tid >> 6] = zeros;
    }
    __syncthreads();
    bh[(int64_t)blockIdx.x * 256 + tid] = hist[tid];
    if (tid == 0) {
        for (int w = 1; w < kRangeThreads / 64; ++w) {
            s += ws[w];
            zeros += wz[w];
        }
        bs[blockIdx.x] = s;
        bz[blockIdx.x] = zeros;
    }
}

// row <- {1, n, zeros, 0, hist[256]} (CTG_RANGE_WORDS words), *sumsq <- the sum: thread t adds bin t of every
// workgroup's row and the partial sums t, t + 256, ... in that order; lanes, then waves, as above.
__global__ __launch_bounds__(kRangeThreads) void range_reduce_kernel(const uint32_t* __restrict__ bh,
                                                                     const uint32_t* __restrict__ bz,
                                                                     const double* __restrict__ bs, int nb, int64_t n,
                                                                     int64_t* __restrict__ row, double* __restrict__ sumsq) {
#pragma clang fp contract(off)
    __shared__ double ws[kRangeThreads / 64];
    __shared__ unsigned long long wz[kRangeThreads / 64];
    const int tid = threadIdx.x;
    unsigned long long cnt = 0, z = 0;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) cnt += bh[(int64_t)b * 256 + tid];
    for (int b = tid; b < nb; b += kRangeThreads) {
        z += bz[b];
        s += bs[b];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s += __shfl_xor(s, d, 64);
        z += (unsigned long long)__shfl_xor((long long)z, d, 64);
    }
    if ((tid & 63) == 0) {
        ws[tid >> 6] = s;
        wz[tid >> 6] = z;
    }
    __syncthreads();
    row[4 + tid] = (int64_t)cnt;
    if (tid == 0) {
        for (int w = 1; w < kRangeThreads / 64; ++w) {
            s += ws[w];
            z += wz[w];
        }
        row[0] = 1;
        row[1] = n;
        row[2] = (int64_t)z;
        row[3] = 0;
        *sumsq = s;
    }
}

int64_t range_blocks(int64_t n) {
    const int64_t nchunks = (n + kRangeChunk - 1) / kRangeChunk;
    return nchunks < 1 ? 1 : (nchunks < kRangeMaxBlocks ? nchunks : kRangeMaxBlocks);
}

int64_t range_partial_bytes(int64_t blocks) { return blocks * (256 * 4 + 4 + 8); }

hipError_t launch_range_hist(const void* x, int64_t n, void* partials, int64_t blocks, int64_t* row, double* sumsq,
                             hipStream_t stream) {
    const int64_t nb = range_blocks(n);
    if (n < 0 || n > kRangeMaxComponents || nb > blocks) return hipErrorInvalidValue;
    // [bs: blocks doubles | bh: blocks x 256 counts | bz: blocks counts]
    double* bs = (double*)partials;
    uint32_t* bh = (uint32_t*)(bs + blocks);
    uint32_t* bz = bh + blocks * 256;
    const int64_t nchunks = (n + kRangeChunk - 1) / kRangeChunk;
    const int vec = ((uintptr_t)x & 15) == 0 ? 1 : 0;
    range_hist_kernel<<<dim3((unsigned)nb), dim3(kRangeThreads), 0, stream>>>((const uint32_t*)x, n, vec, nchunks, bh, bz, bs);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    range_reduce_kernel<<<dim3(1), dim3(kRangeThreads), 0, stream>>>(bh, bz, bs, (int)nb, n, row, sumsq);
    return hipGetLastError();
}

}  // namespace ctg
