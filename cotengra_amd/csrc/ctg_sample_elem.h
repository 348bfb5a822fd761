// ctg_sample_elem.h -- p = |x|^2 of one element of the result tensor and the 16-byte loads that feed it: shared by
// the kernels that reduce p over the result (ctg_sample.hip: statistics and draws; ctg_reduce.hip: top-k and
// marginals), so that every one of them forms the same double for the same element.  ctg_rdm.hip (reduced density
// matrices), ctg_pauli.hip, ctg_pauli_apply.hip and ctg_op_apply.hip take the same loads without the square (load_group);
// what those chunk kernels share beyond the loads is in ctg_result_elem.h.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace ctg {

constexpr int kSampleBlock = 4096;        // elements per block of pass 1 (B)
constexpr int kSampleThreads = 256;

// p of one element: products and sum each rounded once, never fused with each other or with the sum p goes into
// (what a host reference computes, and the same value wherever a kernel forms it)
template <typename T> struct SampleElem;
template <> struct SampleElem<float> {
    static __device__ __forceinline__ double p(float x) {
#pragma clang fp contract(off)
        const double a = (double)x * (double)x;
        return a;
    }
};
template <> struct SampleElem<double> {
    static __device__ __forceinline__ double p(double x) {
#pragma clang fp contract(off)
        const double a = x * x;
        return a;
    }
};
template <> struct SampleElem<float2> {
    static __device__ __forceinline__ double p(float2 x) {
#pragma clang fp contract(off)
        const double a = (double)x.x * (double)x.x, b = (double)x.y * (double)x.y;
        return a + b;
    }
};
template <> struct SampleElem<double2> {
    static __device__ __forceinline__ double p(double2 x) {
#pragma clang fp contract(off)
        const double a = x.x * x.x, b = x.y * x.y;
        return a + b;
    }
};

// p of the V = 16 / sizeof(T) elements from e on (e a multiple of V); elements at or past n count as 0.
// `vec`: x is 16-byte aligned (one 16-byte load where the group lies inside the tensor).
template <typename T>
__device__ __forceinline__ void load_group_p(const T* __restrict__ x, int64_t e, int64_t n, bool vec,
                                             double (&p)[16 / sizeof(T)]) {
    constexpr int V = 16 / sizeof(T);
    if (vec && e + V <= n) {
        union {
            uint4 raw;
            T v[V];
        } g;
        g.raw = *reinterpret_cast<const uint4*>(x + e);
#pragma unroll
        for (int k = 0; k < V; ++k) p[k] = SampleElem<T>::p(g.v[k]);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) p[k] = (e + k < n) ? SampleElem<T>::p(x[e + k]) : 0.0;
    }
}

// The V elements themselves, for the kernels that need more than p (ctg_rdm.hip); elements at or past n are zero.
template <typename T>
__device__ __forceinline__ void load_group(const T* __restrict__ x, int64_t e, int64_t n, bool vec, T (&v)[16 / sizeof(T)]) {
    constexpr int V = 16 / sizeof(T);
    if (vec && e + V <= n) {
        union {
            uint4 raw;
            T v[V];
        } g;
        g.raw = *reinterpret_cast<const uint4*>(x + e);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = g.v[k];
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (e + k < n) ? x[e + k] : T{};
    }
}

}  // namespace ctg
