// ctg_pauli_spectrum.hip -- the expectation values of ALL 2^L Pauli strings that share one X / Y pattern, over the axes
// of the executor's result tensor, by one Walsh-Hadamard transform on the device (DESIGN.md section 21;
// ctg_exec_result_pauli_spectrum and ctg_pauli_spectrum_plan of include/ctg_hip.h).
//
// The result x has n = 2^L elements (every extent 1 or 2); xm is the mask of the flat-index bits of the flipped axes.
// The string P(xm, z), z in [0, n), has Y on the bits of xm & z, X on xm & ~z, Z on z & ~xm, I elsewhere, and
// ny(z) = popcount(xm & z) letters Y.  With p = x[j ^ xm], w = x[j]:
//
//   u[j] = (p.re w.re + p.im w.im) + (p.re w.im - p.im w.re)   (complex plans)       u[j] = p w   (real plans)
//   W[z] = sum over j of (-1)^popcount(j & z) u[j]                                    out[z] = (-1)^ceil(ny(z) / 2) W[z]
//
// and for real plans out[z] = +0.0 where ny(z) is odd.  Re conj(p) w is symmetric under j <-> j ^ xm and Im conj(p) w
// antisymmetric, so in W[z] the part that does not belong to the parity of ny(z) cancels to rounding noise: one real
// transform serves both parities.  Every product and sum is fp64, never contracted, associated as written.
//
// THE ORDER IS THE CONTRACT: the butterflies run over the bits in ascending order, bit 0 first; at bit b the pair
// (a, c) = (v[j], v[j | 2^b]) becomes (a + c, a - c).  Tiles and pass boundaries do not change that, so every bit of out
// is a function of (dtype, extents, flips, the tensor's bytes) alone and a numpy model reproduces it bit for bit.
//
//   spectrum_tile_kernel<T>   256 threads, two workgroups per CU, one workgroup per chunk of 4096 consecutive elements
//                             (one workgroup in all below 4096).  A thread loads the 16-byte groups g 256 + t of the
//                             chunk (load_group) and their partners -- its own group (xm = 0, or xm inside a group),
//                             the group (g 256 + t) ^ (xm / V) of the same chunk (a cache hit), or that group of the
//                             chunk c ^ (xm >> 12) -- with a second 16-byte load: forming u is fused into this pass for
//                             every xm and no form kernel runs.  u goes to LDS (4096 doubles), the butterflies of bits
//                             0 .. min(L, 12) - 1 run there, the chunk is written to the vector.
//   spectrum_pass_kernel      a strided pass over the bits s .. s + nb - 1 of the vector, s >= 12, nb <= 8, in place: a
//                             workgroup holds 2^nb rows (stride 2^s) of 4096 / 2^nb >= 16 consecutive doubles -- runs
//                             of 128 bytes at least.  L <= 12: no such pass; 13 .. 20: one; 21 .. 28: two; ...
//   wht_local (ctg_wht.h)     what both share, and the kernels of ctg_cost.hip with them: the butterflies of the local bits b0 .. b1 - 1 of 4096 doubles in LDS in
//                             rounds of four bits; in a round a thread holds the 16 values that differ in those four
//                             bits.  Slot i of the LDS image is i ^ ((i >> 5) & 31): the three rounds' 8-byte reads are
//                             then conflict-free or 2-way (linear: 16-way in the first round).
//   the last pass             flips the sign bit where ceil(ny / 2) is odd -- no multiplication -- and writes +0.0 to
//                             the odd-ny entries of real plans.
//   spectrum_gather_kernel    vals[s] = vector[select[s]].
//
// Scratch (the executor's d_reduce, reduce_reserve): 8 n bytes for the vector unless dev_out is given, 16 m bytes for
// the select table and its values.
#include <algorithm>
#include <type_traits>

#include "ctg_result_elem.h"
#include "ctg_result_host.h"
#include "ctg_wht.h"

namespace ctg {

// u of one element: every product and sum rounded once, never fused
template <typename T> struct SpecElem;
template <> struct SpecElem<float> {
    static __device__ __forceinline__ double u(float p, float w) {
#pragma clang fp contract(off)
        const double a = (double)p * (double)w;
        return a;
    }
};
template <> struct SpecElem<double> {
    static __device__ __forceinline__ double u(double p, double w) {
#pragma clang fp contract(off)
        const double a = p * w;
        return a;
    }
};
template <> struct SpecElem<float2> {
    static __device__ __forceinline__ double u(float2 p, float2 w) {
#pragma clang fp contract(off)
        const double a = (double)p.x, b = (double)p.y, c = (double)w.x, d = (double)w.y;
        const double ac = a * c, bd = b * d, ad = a * d, bc = b * c;
        const double re = ac + bd, im = ad - bc;
        return re + im;
    }
};
template <> struct SpecElem<double2> {
    static __device__ __forceinline__ double u(double2 p, double2 w) {
#pragma clang fp contract(off)
        const double ac = p.x * w.x, bd = p.y * w.y, ad = p.x * w.y, bc = p.y * w.x;
        const double re = ac + bd, im = ad - bc;
        return re + im;
    }
};

// entry z of the spectrum from W[z]: the sign (-1)^ceil(ny / 2) as a flip of the sign bit; +0.0 for odd ny of a real plan
__device__ __forceinline__ double spec_finish(double w, int64_t z, int64_t xm, int real) {
    const int ny = __popcll((unsigned long long)(z & xm));
    if (real && (ny & 1)) return 0.0;
    return signed_by(w, (uint32_t)((ny + 1) >> 1) & 1u);
}

// The local indices 2 q, 2 q + 1 (q = i 256 + tid) of the tile in ds go to v[g], v[g + 1], g even: one 16-byte store
// where v is 16-byte aligned (vec) and both lie below n
__device__ __forceinline__ void spec_store_pair(const double* ds, int l, double* __restrict__ v, int64_t g, int64_t n, int vec,
                                                int last, int64_t xm, int real) {
    double a = ds[spec_slot(l)], c = ds[spec_slot(l + 1)];
    if (last) {
        a = spec_finish(a, g, xm, real);
        c = spec_finish(c, g + 1, xm, real);
    }
    if (vec && g + 1 < n) {
        *reinterpret_cast<double2*>(v + g) = make_double2(a, c);
    } else {
        if (g < n) v[g] = a;
        if (g + 1 < n) v[g + 1] = c;
    }
}

// bits 0 .. bits - 1 of chunk blockIdx.x: v[chunk] <- the butterflies of u[chunk]
template <typename T>
__global__ __launch_bounds__(kSampleThreads, 2) void spectrum_tile_kernel(const T* __restrict__ x, int64_t n, int xvec, int64_t xm,
                                                                          int bits, int last, double* __restrict__ v, int vvec) {
    constexpr int V = 16 / sizeof(T);
    constexpr int G = kResultChunk / V / kSampleThreads;
    constexpr int real = std::is_same<T, float>::value || std::is_same<T, double>::value;
    __shared__ double ds[kResultChunk];

    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x << kResultChunkBits;
    const int64_t xgrp = xm & ~(int64_t)(V - 1);   // the partner's group: e ^ xgrp
    const uint32_t xin = (uint32_t)xm & (V - 1);   // ... and its place there: k ^ xin
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int l = (g * kSampleThreads + tid) * V;
        const int64_t e = base + l;
        Group<T> w, p;
        load_group<T>(x, e, n, xvec != 0, w.v);
        if (xgrp)
            load_group<T>(x, e ^ xgrp, n, xvec != 0, p.v);   // (e >= n only when n < 4096: then e ^ xgrp >= n too)
        else
            p = w;
        if (V >= 2 && (xin & 1u)) {
            Group<T> t = p;
#pragma unroll
            for (int k = 0; k < V; ++k) p.v[k] = t.v[k ^ (V >= 2 ? 1 : 0)];
        }
        if (V >= 4 && (xin & 2u)) {
            Group<T> t = p;
#pragma unroll
            for (int k = 0; k < V; ++k) p.v[k] = t.v[k ^ (V >= 4 ? 2 : 0)];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) ds[spec_slot(l + k)] = SpecElem<T>::u(p.v[k], w.v[k]);
    }
    wht_local(ds, tid, 0, bits);
#pragma unroll
    for (int i = 0; i < kResultChunk / 2 / kSampleThreads; ++i) {
        const int l = (i * kSampleThreads + tid) * 2;
        spec_store_pair(ds, l, v, base + l, n, vvec, last, xm, real);
    }
}

// bits s .. s + nb - 1 of the vector, in place: tile blockIdx.x is 2^nb rows of 2^cb = 4096 / 2^nb consecutive doubles;
// the bits cb .. s - 1 and s + nb .. of its base come from the tile's number
__global__ __launch_bounds__(kSampleThreads, 2) void spectrum_pass_kernel(double* __restrict__ v, int64_t n, int s, int nb, int vvec,
                                                                          int last, int64_t xm, int real) {
    __shared__ double ds[kResultChunk];
    const int tid = threadIdx.x;
    const int cb = kResultChunkBits - nb;
    const int64_t q = blockIdx.x;
    const int64_t base = wht_pass_base(q, s, nb);
    auto where = [&](int l) { return wht_pass_where(base, l, s, nb); };
#pragma unroll
    for (int i = 0; i < kResultChunk / 2 / kSampleThreads; ++i) {
        const int l = (i * kSampleThreads + tid) * 2;   // (l and l + 1 share a row: cb >= 4)
        const int64_t g = where(l);
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
    wht_local(ds, tid, cb, kResultChunkBits);
#pragma unroll
    for (int i = 0; i < kResultChunk / 2 / kSampleThreads; ++i) {
        const int l = (i * kSampleThreads + tid) * 2;
        spec_store_pair(ds, l, v, where(l), n, vvec, last, xm, real);
    }
}

__global__ __launch_bounds__(kSampleThreads) void spectrum_gather_kernel(const double* __restrict__ v, const int64_t* __restrict__ select,
                                                                         int64_t m, double* __restrict__ vals) {
    const int64_t s = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
    if (s < m) vals[s] = v[select[s]];
}

}  // namespace ctg

using namespace ctg;

namespace {

// what a call launches: a function of (dtype, extents, flips) alone
struct SpecPlan {
    int L = 0;
    int64_t n = 1, xm = 0;
    int partner = 0;     // 0: xm = 0; 1: inside the 16-byte group; 2: another group of the chunk; 3: another chunk
    int tile_bits = 0;   // min(L, 12)
    int npass = 0, pass_bits[kSpecMaxPasses] = {0, 0, 0, 0};
    int64_t tiles = 1;   // workgroups of every launch
};

// CTG_E_INVALID for an extent other than 1 and 2 (before result_shape multiplies them)
int spec_extents(const char* who, int64_t rank, const int64_t* extents) {
    for (int64_t a = 0; a < rank; ++a)
        if (extents[a] > 2)
            return result_fail(CTG_E_INVALID, "%s: axis %lld has extent %lld; every extent must be 1 or 2", who, (long long)a,
                               (long long)extents[a]);
    return CTG_OK;
}

// CTG_OK, or CTG_E_INVALID with the error set; the extents have passed spec_extents and result_shape (`shape`)
int spec_plan(const char* who, int dtype, int64_t rank, const int64_t* extents, const uint8_t* flips, const ResultShape& shape,
              SpecPlan* out) {
    SpecPlan& p = *out = SpecPlan();
    for (int64_t a = 0; a < rank; ++a) {
        if (flips[a] > 1) return result_fail(CTG_E_INVALID, "%s: axis %lld: flip code %d is neither 0 nor 1", who, (long long)a, (int)flips[a]);
        if (flips[a] && extents[a] != 2)
            return result_fail(CTG_E_INVALID, "%s: a flip on axis %lld of extent %lld; only an axis of extent 2 carries X or Y", who,
                               (long long)a, (long long)extents[a]);
        if (flips[a]) p.xm |= shape.strides[a];
    }
    p.n = shape.n;
    while (((int64_t)1 << p.L) < p.n) ++p.L;
    const int64_t V = 16 / ctg_item_size(dtype);
    p.partner = p.xm == 0 ? 0 : p.xm < V ? 1 : p.xm < kResultChunk ? 2 : 3;
    p.tile_bits = std::min(p.L, kResultChunkBits);
    for (int b = kResultChunkBits; b < p.L; b += kSpecPassBits) p.pass_bits[p.npass++] = std::min(kSpecPassBits, p.L - b);
    p.tiles = std::max<int64_t>(1, p.n >> kResultChunkBits);
    return CTG_OK;
}

template <typename T>
int spec_launch(ctg_exec* e, const SpecPlan& p, double* v) {
    hipStream_t st = e->stream;
    const int xvec = ((uintptr_t)e->d_result & 15) == 0 ? 1 : 0, vvec = ((uintptr_t)v & 15) == 0 ? 1 : 0;
    const int real = std::is_same<T, float>::value || std::is_same<T, double>::value;
    spectrum_tile_kernel<T><<<dim3((unsigned)p.tiles), dim3(kSampleThreads), 0, st>>>((const T*)e->d_result, p.n, xvec, p.xm, p.tile_bits,
                                                                                    p.npass == 0, v, vvec);
    LAUNCH_CHECK("spectrum_tile_kernel");
    int s = kResultChunkBits;
    for (int i = 0; i < p.npass; ++i) {
        spectrum_pass_kernel<<<dim3((unsigned)p.tiles), dim3(kSampleThreads), 0, st>>>(v, p.n, s, p.pass_bits[i], vvec, i == p.npass - 1,
                                                                                     p.xm, real);
        LAUNCH_CHECK("spectrum_pass_kernel");
        s += p.pass_bits[i];
    }
    return CTG_OK;
}

}  // namespace

extern "C" int ctg_pauli_spectrum_plan(int32_t dtype, int64_t rank, const int64_t* extents, const uint8_t* flips, int64_t* words) {
    const char* who = "pauli_spectrum_plan";
    if (!extents || !flips || !words) return result_fail(CTG_E_INVALID, "%s: null argument", who);
    if (dtype < CTG_F32 || dtype > CTG_C128) return result_fail(CTG_E_INVALID, "%s: dtype %d is none of CTG_F32 .. CTG_C128", who, (int)dtype);
    ResultShape shape;
    const char* why = "";
    if (spec_extents(who, rank, extents) != CTG_OK) return CTG_E_INVALID;
    int64_t n = 1;   // (the extents' own product stands for result_elems)
    for (int64_t a = 0; a < rank && n <= kReduceMaxElems; ++a) n *= extents[a] == 2 ? 2 : 1;
    if (result_shape(rank, extents, n, &shape, &why) != CTG_OK) return result_fail(CTG_E_INVALID, "%s: %s", who, why);
    SpecPlan p;
    const int rc = spec_plan(who, dtype, rank, extents, flips, shape, &p);
    if (rc != CTG_OK) return rc;
    for (int i = 0; i < CTG_PAULI_SPECTRUM_PLAN_WORDS; ++i) words[i] = 0;
    words[0] = p.L;
    words[1] = p.xm;
    words[2] = p.partner;
    words[3] = p.tile_bits;
    words[4] = p.npass;
    for (int i = 0; i < kSpecMaxPasses; ++i) words[5 + i] = p.pass_bits[i];
    words[9] = p.tiles;
    words[10] = up256(p.n * 8);
    words[11] = dtype;
    return CTG_OK;
}

extern "C" int ctg_exec_result_pauli_spectrum(ctg_exec* e, int64_t rank, const int64_t* extents, const uint8_t* flips, int64_t m,
                                              const int64_t* select, double* out, void* dev_out) {
    const char* who = "pauli_spectrum";
    if (!e || !extents || !flips) return result_fail(CTG_E_INVALID, "%s: null argument", who);
    if (spec_extents(who, rank, extents) != CTG_OK) return CTG_E_INVALID;
    ResultShape shape;
    const char* why = "";
    if (result_shape(rank, extents, e->plan->result_elems, &shape, &why) != CTG_OK) return result_fail(CTG_E_INVALID, "%s: %s", who, why);
    const int dtype = e->plan->dtype;
    SpecPlan p;
    int rc = spec_plan(who, dtype, rank, extents, flips, shape, &p);
    if (rc != CTG_OK) return rc;
    const int64_t n = p.n;
    if (!out && !dev_out) return result_fail(CTG_E_INVALID, "%s: neither out nor dev_out is given", who);
    if (select) {
        if (!out) return result_fail(CTG_E_INVALID, "%s: a select table without out", who);
        if (m < 0 || m > CTG_PAULI_SPECTRUM_MAX_SELECT)
            return result_fail(CTG_E_INVALID, "%s: %lld selected entries; between 0 and CTG_PAULI_SPECTRUM_MAX_SELECT = %d", who, (long long)m,
                               CTG_PAULI_SPECTRUM_MAX_SELECT);
        for (int64_t s = 0; s < m; ++s)
            if (select[s] < 0 || select[s] >= n)
                return result_fail(CTG_E_INVALID, "%s: select[%lld] = %lld is outside [0, %lld)", who, (long long)s, (long long)select[s],
                                   (long long)n);
    }
    if (dev_out) {
        if ((uintptr_t)dev_out & 7) return result_fail(CTG_E_INVALID, "%s: dev_out is not 8-byte aligned", who);
        const uintptr_t d0 = (uintptr_t)dev_out, r0 = (uintptr_t)e->d_result;
        if (d0 < r0 + (uintptr_t)(n * ctg_item_size(dtype)) && r0 < d0 + (uintptr_t)(n * 8))
            return result_fail(CTG_E_INVALID, "%s: dev_out overlaps the result tensor", who);
    }
    rc = result_norm_finite(e, "no spectrum of it");
    if (rc != CTG_OK) return rc;
    const int64_t nsel = select ? m : 0;
    // [the vector: n, unless dev_out holds it | the select table | its values]
    double *vec = nullptr, *d_vals = nullptr;
    int64_t* d_select = nullptr;
    auto lay = [&](void* base) {
        Carve c(base);
        vec = c.take<double>(dev_out ? 0 : n * 8);
        d_select = c.take<int64_t>(nsel * 8);
        d_vals = c.take<double>(nsel * 8);
        return c.bytes();
    };
    rc = reduce_reserve(e, lay(nullptr));
    if (rc != CTG_OK) return rc;
    lay(e->d_reduce);
    double* v = dev_out ? (double*)dev_out : vec;
    if (nsel) HIP_TRY(upload(d_select, select, nsel * 8, e->stream));
    rc = dispatch_elem(dtype, [&](auto t) { return spec_launch<decltype(t)>(e, p, v); });
    if (rc != CTG_OK) return rc;
    if (select) {
        if (nsel) {
            spectrum_gather_kernel<<<dim3((unsigned)((nsel + kSampleThreads - 1) / kSampleThreads)), dim3(kSampleThreads), 0, e->stream>>>(
                v, d_select, nsel, d_vals);
            LAUNCH_CHECK("spectrum_gather_kernel");
            HIP_TRY(hipMemcpyAsync(out, d_vals, (size_t)(nsel * 8), hipMemcpyDeviceToHost, e->stream));
        }
    } else if (out) {
        HIP_TRY(hipMemcpyAsync(out, v, (size_t)(n * 8), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CTG_OK;
}
