// ctg_wht.h -- the Walsh-Hadamard butterflies of a tile of 4096 doubles in LDS and the geometry of a strided pass:
// what the kernels of ctg_pauli_spectrum.hip and ctg_cost.hip (section 22) share.  The library
// is built one object per source without relocatable device code, so each source has its own kernels over these
// device functions.
//
// THE ORDER IS THE CONTRACT: the butterflies run over the bits in ascending order; at bit b the pair (a, c) =
// (v[j], v[j | 2^b]) becomes (a + c, a - c).  Tiles and pass boundaries do not change that.
#pragma once

#include "ctg_result_elem.h"

namespace ctg {

constexpr int kSpecPassBits = 8;     // bits of a strided pass, at most
constexpr int kSpecMaxPasses = 4;    // 12 + 4 * 8 >= 40 = log2(kReduceMaxElems)

// where local index i of a tile lives in its LDS image
__device__ __forceinline__ int spec_slot(int i) { return i ^ ((i >> 5) & 31); }

// The butterflies of the local bits b0 .. b1 - 1 (wave-uniform, within 0 .. 12) of the tile in ds, ascending.  Begins
// and ends with a barrier: the caller's writes are seen, and so is the result.
__device__ __forceinline__ void wht_local(double* ds, int tid, int b0, int b1) {
    __syncthreads();
#pragma unroll
    for (int lo = 0; lo < kResultChunkBits; lo += 4) {
        if (b1 <= lo || b0 >= lo + 4) continue;
        // the 16 local indices that differ in the bits lo .. lo + 3: those bits are k, the others tid's
        const int rest = ((tid >> lo) << (lo + 4)) | (tid & ((1 << lo) - 1));
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = ds[spec_slot(rest | (k << lo))];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (lo + j < b0 || lo + j >= b1) continue;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k & (1 << j)) continue;
                const double a = v[k], c = v[k | (1 << j)];
                v[k] = a + c;
                v[k | (1 << j)] = a - c;
            }
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) ds[spec_slot(rest | (k << lo))] = v[k];
        __syncthreads();
    }
}

// A strided pass over the bits s .. s + nb - 1 (s >= 12, nb <= 8): tile q is 2^nb rows (stride 2^s) of 2^cb = 4096 /
// 2^nb consecutive doubles; the bits cb .. s - 1 and s + nb .. of its base come from the tile's number.
__device__ __forceinline__ int64_t wht_pass_base(int64_t q, int s, int nb) {
    const int cb = kResultChunkBits - nb, lowbits = s - cb;
    return ((q & (((int64_t)1 << lowbits) - 1)) << cb) | ((q >> lowbits) << (s + nb));
}

// the element of the vector that local index l of such a tile holds
__device__ __forceinline__ int64_t wht_pass_where(int64_t base, int l, int s, int nb) {
    const int cb = kResultChunkBits - nb;
    return base | ((int64_t)(l >> cb) << s) | (int64_t)(l & ((1 << cb) - 1));
}

}  // namespace ctg
