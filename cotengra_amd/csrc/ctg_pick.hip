// ctg_pick.hip -- the sparse root step of a pick plan (cotengra_amd/plan.py: build_pick_step).
//
//   C[rowC(m)] = alpha * sum_k A[rowA(m) + kA(k)] * B[rowB(m) + kB(k)]        m = 0 .. M - 1
//
// One row per requested member of the tree's output: rowA / rowB are per-request offsets (the `hi` level of
// the row tables, row_lo = 1), rowC the request's position in the caller's table.  Every request reads one
// row of K elements of each operand and writes one element: the step is a gather of whole rows, bound by memory.
//
//   pair_pick_kernel<T, VEC, SEG>: SEG lanes (1, 2, 4 .. 64) share a request, a wave carries 64 / SEG
//   consecutive requests of the sorted list.  A lane takes the slots sl, sl + SEG, ... of its request's row
//   (a slot = VEC adjacent k; VEC = 2: one load of two elements, 16 bytes in complex64), four slots in
//   flight (two of the 32-byte slots of complex128): the table lookups of a round first, then its loads, then the multiply-adds in slot order.  The
//   SEG partial sums are added in a fixed butterfly.  Nothing is shared between requests and nothing is
//   atomic: the bits of a request are a function of its two rows and of (K, VEC, SEG) alone.
//
// All loads go through the offset tables (ctg_common.h); wave = 64 lanes.
#include "ctg_common.h"

#include <cstdio>

namespace ctg {

namespace {

template <typename T>
struct alignas(2 * sizeof(T)) Pair2 {
    T x, y;
};

__device__ __forceinline__ float xor_of(float v, int o) { return __shfl_xor(v, o, 64); }
__device__ __forceinline__ double xor_of(double v, int o) { return __shfl_xor(v, o, 64); }
template <typename F>
__device__ __forceinline__ cplx<F> xor_of(cplx<F> v, int o) {
    return cplx<F>{xor_of(v.re, o), xor_of(v.im, o)};
}

// Slots a lane has in flight; a row of at most this many rounds stays in registers.  Four, 64 bytes of each
// operand at the widest 16-byte slot; a 32-byte slot (complex128, VEC = 2) takes two -- the same 64 bytes --
// so that the two operands, the kept A row and the offsets fit the 128 registers of four waves per SIMD
// without scratch.  A lane adds its slots in slot order whatever the number in flight: no bit depends on it.
template <typename T, int VEC>
constexpr int pick_rounds() { return sizeof(T) * VEC > 16 ? 2 : 4; }

}  // namespace

// `rps`: consecutive requests a segment takes one after the other (a performance parameter: a request's
// lanes, slots and order of operations do not depend on it).  Consecutive requests of the sorted list that
// address the same A row reuse it from registers when the row is at most pick_rounds() rounds long -- the same
// values, hence the same bits; longer rows are read again and hit the L2.
template <typename T, int VEC, int SEG>
__global__ __launch_bounds__(256, 4) void pair_pick_kernel(StepArgs p, int rps) {
    constexpr int U = pick_rounds<T, VEC>();
    const T* __restrict__ A = (const T*)p.A + zoffA(p);
    const T* __restrict__ B = (const T*)p.B + zoffB(p) + p.nB[0];
    T* __restrict__ C = (T*)p.C + zoffC(p) + p.nC[0];
    const double alpha = step_alpha(p);
    const int lane = threadIdx.x & 63;
    const int sl = lane & (SEG - 1);
    const int64_t seg = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / SEG) + lane / SEG;
    const int64_t slots = (p.K + VEC - 1) / VEC;
    const int64_t rounds = (slots + SEG - 1) / SEG;
    const bool keep = rounds <= U;
    const int64_t loA = p.rowA.lo[0], loB = p.rowB.lo[0], loC = p.rowC.lo[0];

    T areg[U][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int v = 0; v < VEC; ++v) areg[u][v] = zero_of(T{});
    bool have = false;
    int64_t prev_a = 0;

    // (the same trip count for every segment of the wave: the butterfly below takes all 64 lanes)
    for (int i = 0; i < rps; ++i) {
        const int64_t m = seg * rps + i;
        const bool active = m < p.R;
        const int64_t mc = active ? m : p.R - 1;
        const int64_t ra = p.rowA.hi[mc] + loA, rb = p.rowB.hi[mc] + loB;
        const bool same = keep && have && ra == prev_a;
        const T* __restrict__ a = A + ra;
        const T* __restrict__ b = B + rb;
        T acc = zero_of(T{});
        for (int64_t r0 = 0; r0 < rounds; r0 += U) {
            int64_t ia[U], ib[U];
            bool valid[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t j = sl + (int64_t)SEG * (r0 + u);
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
                    const Pair2<T> y = *(const Pair2<T>*)(b + ib[u]);
                    bv[u][0] = y.x;
                    bv[u][VEC - 1] = y.y;
                    if (!same) {
                        const Pair2<T> x = *(const Pair2<T>*)(a + ia[u]);
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
            prev_a = ra;
        }
#pragma unroll
        for (int o = SEG / 2; o > 0; o >>= 1) acc = add_of(acc, xor_of(acc, o));
        if (active && sl == 0) C[p.rowC.hi[m] + loC] = scale_of(acc, alpha);
    }
}

namespace {

struct PickShape {
    int seg;        // lanes per request
    int rps;        // requests a segment takes one after the other
    int64_t blocks;
};

// SEG: the smallest power of two that covers the slots of a row, at most a wave.
PickShape pick_shape(const StepArgs& p, int vec) {
    const int64_t slots = (p.K + vec - 1) / vec;
    int seg = 1;
    while (seg < 64 && seg < slots) seg <<= 1;
    const int64_t per_wave = 64 / seg;
    const int64_t waves = (p.R + per_wave - 1) / per_wave;
    // (enough waves to fill the chip four times over -- 256 CUs x 16 waves -- : a segment walks four
    // consecutive requests, and those of one A row share its registers)
    const int rps = waves >= 4 * 4096 ? 4 : 1;
    const int64_t segs = (p.R + rps - 1) / rps;
    const int64_t w = (segs + per_wave - 1) / per_wave;
    return PickShape{seg, rps, (w + 3) / 4};
}

template <typename T, int VEC>
hipError_t launch_pick_seg(const StepArgs& p, const PickShape& s, hipStream_t stream) {
    const dim3 grid((unsigned)s.blocks, (unsigned)(p.nz < 1 ? 1 : p.nz));
    switch (s.seg) {
        case 1: hipLaunchKernelGGL((pair_pick_kernel<T, VEC, 1>), grid, dim3(256), 0, stream, p, s.rps); break;
        case 2: hipLaunchKernelGGL((pair_pick_kernel<T, VEC, 2>), grid, dim3(256), 0, stream, p, s.rps); break;
        case 4: hipLaunchKernelGGL((pair_pick_kernel<T, VEC, 4>), grid, dim3(256), 0, stream, p, s.rps); break;
        case 8: hipLaunchKernelGGL((pair_pick_kernel<T, VEC, 8>), grid, dim3(256), 0, stream, p, s.rps); break;
        case 16: hipLaunchKernelGGL((pair_pick_kernel<T, VEC, 16>), grid, dim3(256), 0, stream, p, s.rps); break;
        case 32: hipLaunchKernelGGL((pair_pick_kernel<T, VEC, 32>), grid, dim3(256), 0, stream, p, s.rps); break;
        case 64: hipLaunchKernelGGL((pair_pick_kernel<T, VEC, 64>), grid, dim3(256), 0, stream, p, s.rps); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <typename T>
hipError_t launch_pick_t(const StepArgs& p, int vec, hipStream_t stream) {
    const PickShape s = pick_shape(p, vec ? 2 : 1);
    return vec ? launch_pick_seg<T, 2>(p, s, stream) : launch_pick_seg<T, 1>(p, s, stream);
}

}  // namespace

hipError_t launch_pair_pick(int dtype, const StepArgs& p, int vec, void* scratch, int64_t scratch_bytes,
                            hipStream_t stream) {
    if (p.N != 1 || p.Bt != 1 || p.row_lo != 1) return hipErrorInvalidValue;
    // few requests under a very long contraction: the k-reduction kernels spread K over the chip
    if (pick_route_kred(p.R, p.K)) return launch_pair_valu(dtype, p, scratch, scratch_bytes, stream);
    switch (dtype) {
        case 0: return launch_pick_t<float>(p, vec, stream);
        case 1: return launch_pick_t<double>(p, vec, stream);
        case 2: return launch_pick_t<c64>(p, vec, stream);
        case 3: return launch_pick_t<c128>(p, vec, stream);
    }
    return hipErrorInvalidValue;
}

void pair_pick_name(int dtype, const StepArgs& p, int vec, int64_t scratch_bytes, char* buf, size_t n) {
    if (pick_route_kred(p.R, p.K)) {
        pair_valu_name(dtype, p, scratch_bytes, buf, n);
        return;
    }
    static const char* const names[4] = {"float", "double", "c64", "c128"};
    const PickShape s = pick_shape(p, vec ? 2 : 1);
    snprintf(buf, n, "pair_pick_kernel<%s,%d,%d>", names[dtype & 3], vec ? 2 : 1, s.seg);
}

}  // namespace ctg
