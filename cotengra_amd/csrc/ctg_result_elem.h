// ctg_result_elem.h -- what the chunk kernels over the executor's result tensor share on the device: the chunk
// geometry (ctg_rdm.hip, ctg_pauli.hip, ctg_pauli_apply.hip, ctg_op_apply.hip), and for the two apply sources the
// arithmetic of acc += W p and the 16-byte groups y is stored in.  The loads and p = |x|^2: ctg_sample_elem.h.
#pragma once

#include "ctg_sample_elem.h"

namespace ctg {

constexpr int kResultChunk = kSampleBlock;   // elements of a chunk
constexpr int kResultChunkBits = 12;         // log2(kResultChunk)
constexpr int kResultMaxGrid = 512;          // workgroups of a chunk kernel: two per CU
constexpr int kResultMinChunks = 3;          // chunks per workgroup before the grid grows
static_assert(kResultChunk == 1 << kResultChunkBits, "a chunk is addressed by kResultChunkBits bits");

// the workgroups that share nchunks chunks (chunk pairs): a function of the count alone
inline int result_chunk_grid(int64_t nchunks) {
    const int64_t g = (nchunks + kResultMinChunks - 1) / kResultMinChunks;
    return (int)(g < kResultMaxGrid ? g : kResultMaxGrid);
}

// the bits of v dealt to the set bits of mask, lowest first (its inverse: extract_bits of ctg_result_host.h)
__host__ __device__ __forceinline__ int64_t deposit_bits(int64_t v, int64_t mask) {
    int64_t r = 0;
    for (int64_t m = mask; m && v; m &= m - 1) {
        if (v & 1) r |= m & (0 - m);
        v >>= 1;
    }
    return r;
}

// v with its sign flipped where bit 0 of `bit` is set
__device__ __forceinline__ double signed_by(double v, uint32_t bit) {
    return __hiloint2double(__double2hiint(v) ^ (int)(bit << 31), __double2loint(v));
}

// The V = 16 / sizeof(T) elements of a 16-byte group.  (The store of a group of y -- one 16-byte store when y is
// 16-byte aligned, else element by element -- stays written out in the two apply kernels: as a function it lets the
// compiler merge the two stores of the complex128 instantiations, a different kernel.)
template <typename T>
union Group {
    uint4 raw;
    T v[16 / sizeof(T)];
};

// acc += W p in fp64 for a weight W = (wre, wim) -- W: the type it is stored as, a double on real plans -- and the
// rounding of acc to T.  The four products, the difference, the sum and the addition to acc are each rounded once,
// nothing is fused: the bits of y that the headers of the apply sources define.
template <typename T> struct ApplyElem;
template <> struct ApplyElem<float> {
    static constexpr int P = 1;
    typedef double W;
    static __device__ __forceinline__ void mac(float p, double wre, double, double& are, double&) {
#pragma clang fp contract(off)
        const double a = wre * (double)p;
        are = are + a;
    }
    static __device__ __forceinline__ void mac(float p, W w, double& are, double& aim) { mac(p, w, 0.0, are, aim); }
    static __device__ __forceinline__ float round(double are, double) { return (float)are; }
};
template <> struct ApplyElem<double> {
    static constexpr int P = 1;
    typedef double W;
    static __device__ __forceinline__ void mac(double p, double wre, double, double& are, double&) {
#pragma clang fp contract(off)
        const double a = wre * p;
        are = are + a;
    }
    static __device__ __forceinline__ void mac(double p, W w, double& are, double& aim) { mac(p, w, 0.0, are, aim); }
    static __device__ __forceinline__ double round(double are, double) { return are; }
};
template <> struct ApplyElem<float2> {
    static constexpr int P = 2;
    typedef double2 W;
    static __device__ __forceinline__ void mac(float2 p, double wre, double wim, double& are, double& aim) {
#pragma clang fp contract(off)
        const double pr = (double)p.x, pi = (double)p.y;
        const double a = wre * pr, b = wim * pi, c = wre * pi, d = wim * pr;
        const double tr = a - b, ti = c + d;
        are = are + tr;
        aim = aim + ti;
    }
    static __device__ __forceinline__ void mac(float2 p, W w, double& are, double& aim) { mac(p, w.x, w.y, are, aim); }
    static __device__ __forceinline__ float2 round(double are, double aim) { return make_float2((float)are, (float)aim); }
};
template <> struct ApplyElem<double2> {
    static constexpr int P = 2;
    typedef double2 W;
    static __device__ __forceinline__ void mac(double2 p, double wre, double wim, double& are, double& aim) {
#pragma clang fp contract(off)
        const double a = wre * p.x, b = wim * p.y, c = wre * p.y, d = wim * p.x;
        const double tr = a - b, ti = c + d;
        are = are + tr;
        aim = aim + ti;
    }
    static __device__ __forceinline__ void mac(double2 p, W w, double& are, double& aim) { mac(p, w.x, w.y, are, aim); }
    static __device__ __forceinline__ double2 round(double are, double aim) { return make_double2(are, aim); }
};

}  // namespace ctg
