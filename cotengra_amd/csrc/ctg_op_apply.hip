// ctg_op_apply.hip -- y = (sum over t of O_t (x) 1) x for small dense matrices O_t on named axes of the executor's
// result tensor x, of any extent, written on the device next to x (ctg_exec_result_op_apply of
// include/ctg_hip.h).  Term t acts on naxes[t] distinct axes given in ascending position; D_t is the product of their
// extents; O_t is D_t x D_t, rows and columns row-major over those axes:
//
//   y[a, r] = sum over t, b of O_t[a, b] x[b, r]      a, b over the term's axes, r over all others.
//
// conj(2 y) is the cotangent of <x| H |x> for a VJP plan when H = sum O_t is Hermitian.
//
// The definition of the bits of y (a host reference can mirror it, tests/test_op_apply_host.py):
//   - per element j a complex fp64 accumulator acc starts at +0; terms in the caller's order; inside a term b = 0 ..
//     D_t - 1 ascending (ascending partner flat index, because the axes ascend);
//   - with p = x[partner(j, b)] widened to fp64 and W = O_t[a(j), b]:  acc_re <- acc_re + (W_re p_re - W_im p_im),
//     acc_im <- acc_im + (W_re p_im + W_im p_re); the four products, the difference / sum and the addition to acc each
//     rounded once, nothing fused (fp contract(off)) -- ApplyElem<T>::mac of ctg_result_elem.h;  real plans: acc <- acc
//     + W_re p;
//   - after the last term acc is rounded once to the plan's dtype.
// No atomics; no sum crosses a thread: the bits of y are a function of (dtype, extents, terms in order, the tensor's
// bytes) alone.  An entry of O_t that is zero in both parts may be skipped: its update adds +-0 to an accumulator that
// is never -0 (it starts at +0, and x + (-x) rounds to +0), so for a finite tensor -- the call refuses any other --
// no bit changes.  Both kernels skip; where, is said at the place.
//
//   power of two (every extent a power of two, at least kResultChunk = 4096 elements):
//
//     op_apply_kernel<T>   the geometry of pauli_apply_kernel: 256 threads, two workgroups per CU, one launch; a
//                          workgroup owns the output chunks wg, wg + grid, ... of 4096 elements, grid = min(512,
//                          ceil(chunks / 3)); thread t holds the 16-byte groups g 256 + t of a chunk (16 elements) as
//                          fp64 accumulators.  A term's flat-index bits split into lo (below 12: inside a chunk, nlo
//                          of them) and hi (chunk-uniform, nhi): a = (a_hi, a_lo), b = (b_hi, b_lo).  The host lays
//                          O_t out as 2^nhi x 2^nhi blocks [a_hi][b_hi] of 2^nlo x 2^nlo entries, a block column by
//                          column ([b_lo][a_lo]: lanes with consecutive a_lo read consecutive entries), and gives every
//                          block a 64-bit column mask: bit b_lo set when column b_lo of the block holds a non-zero.
//                          Per (chunk, term) the workgroup walks b_hi ascending; a block whose mask is 0 is not
//                          visited -- a workgroup-uniform branch, the partner chunk is never read (a diagonal term
//                          reads the tensor once; XX + YY + ZZ on two high bits two partner chunks, not four); else the
//                          partner chunk (c & ~hi) | deposit(b_hi) is staged in LDS (one 16-byte load and store per
//                          lane and group) and the block in LDS when it is at most 8 KiB (else it is read from the
//                          scratch: a c128 chunk is 64 KiB, 72 KiB with the block keeps two workgroups per CU); then
//                          b_lo ascending, columns with a clear mask bit skipped (uniform), the thread reads x at
//                          (l & ~lo) | deposit(b_lo) and W at [b_lo][a_lo(l)] for each of its 16 elements l.  A term
//                          with lo = 0 has its partner at the thread's own position: it is loaded straight from
//                          memory, no LDS, no barrier.  y: one 16-byte store per lane and group (element stores for a
//                          dev_out that is not 16-byte aligned).
//
//   general (any other shape): op_apply_general_kernel<T>, a thread per output element (grid-stride); a(j) and the
//   partners from the digits (j / stride) % extent; same order; an entry that is zero is skipped; not tuned.
//
// Scratch (the executor's d_reduce, reduce_reserve): 456 bytes per term (general
// route: 88), the matrices (16 bytes per entry, 8 on real plans of the power-of-two route: at most 16 MiB), 8 bytes per
// block and, when only host_out is given, result_elems elements of y.
#include <algorithm>

#include "ctg_result_elem.h"
#include "ctg_result_host.h"

namespace ctg {

constexpr int kOpMatLds = 1024;          // doubles of a block kept in LDS (8 KiB)
constexpr int kOpMaxAxes = 6;            // axes of extent >= 2 of a term (D <= 64)
constexpr int64_t kOpGeneralMaxBlocks = 1 << 20;
static_assert(CTG_OP_MAX_DIM == 1 << kOpMaxAxes, "a column mask has one bit per b_lo");

// What a term of the power-of-two route needs on the device
struct OpTermMeta {
    int64_t hi;              // its flat-index bits at and above kResultChunkBits, shifted down: bits of the chunk index
    int64_t blocks;          // where its blocks start in the matrices (in doubles)
    int64_t cmask;           // where its 2^nhi x 2^nhi column masks start
    int32_t lo;              // its flat-index bits below kResultChunkBits
    int32_t nlo, nhi;
    int32_t in_lds;          // 1: a block is at most kOpMatLds doubles
    uint8_t hipos[8];        // the positions of the bits of hi, ascending
    uint16_t dep[64];        // b_lo deposited into lo
    uint8_t at[kSampleThreads];   // the bits of a_lo that thread t's position gives
    uint8_t ag[16];          // ... group row g's
    uint8_t ak[4];           // ... element k's of a 16-byte group
};

// A term of the general route: its axes of extent >= 2, ascending
struct OpGenTerm {
    int64_t mat;             // where its matrix starts (in doubles; D x D (re, im) pairs, the caller's layout)
    int64_t stride[kOpMaxAxes];
    int32_t ext[kOpMaxAxes];
    int32_t nax, dim;
};

// (acc += W p, the type W of a stored weight and the rounding of acc to T: ApplyElem<T> of ctg_result_elem.h)
template <typename T>
__global__ __launch_bounds__(kSampleThreads, 2) void op_apply_kernel(const T* __restrict__ x, int64_t n, int vec, int vec_out,
                                                                     int64_t nchunks, const OpTermMeta* __restrict__ terms, int nterms,
                                                                     const double* __restrict__ mats,
                                                                     const unsigned long long* __restrict__ cmasks, T* __restrict__ y) {
#pragma clang fp contract(off)
    typedef typename ApplyElem<T>::W W;
    constexpr int P = ApplyElem<T>::P;
    constexpr int V = 16 / sizeof(T);
    constexpr int LV = V == 4 ? 2 : V == 2 ? 1 : 0;
    constexpr int G = kResultChunk / V / kSampleThreads;
    constexpr int E = G * V;   // elements of a thread: 16
    static_assert(G <= 16 && V <= 4, "ag and ak of OpTermMeta");
    __shared__ __attribute__((aligned(16))) unsigned char raw[kResultChunk * (int)sizeof(T)];
    __shared__ __attribute__((aligned(16))) double lmat[kOpMatLds];
    uint4* l4 = reinterpret_cast<uint4*>(raw);
    const T* lx = reinterpret_cast<const T*>(raw);
    const int tid = threadIdx.x;

    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        double acc_re[E], acc_im[P == 2 ? E : 1];
#pragma unroll
        for (int i = 0; i < E; ++i) {
            acc_re[i] = 0.0;
            if (P == 2) acc_im[i] = 0.0;
        }
        for (int t = 0; t < nterms; ++t) {
            const OpTermMeta* tm = terms + t;
            const int64_t hi = tm->hi;
            const uint32_t lo = (uint32_t)tm->lo;
            const int nlo = tm->nlo, nhi = tm->nhi, NL = 1 << nlo, NH = 1 << nhi;
            int a_hi = 0;
            for (int q = 0; q < nhi; ++q) a_hi |= (int)((c >> tm->hipos[q]) & 1) << q;
            const int64_t c0 = c & ~hi;
            // per element: its row inside a block and its position with the term's low bits cleared
            uint32_t alo[E], pos0[E];
            {
                const uint32_t at = lo ? tm->at[tid] : 0u;
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        const uint32_t l = ((uint32_t)(g * kSampleThreads + tid) << LV) + (uint32_t)k;
                        alo[g * V + k] = lo ? (at | tm->ag[g] | tm->ak[k]) : 0u;
                        pos0[g * V + k] = l & ~lo;
                    }
            }
            for (int b_hi = 0; b_hi < NH; ++b_hi) {
                // the block [a_hi][b_hi] is all zero: the partner chunk is not read (uniform over the workgroup)
                const unsigned long long cm = cmasks[tm->cmask + (int64_t)a_hi * NH + b_hi];
                if (!cm) continue;
                int64_t c2 = c0;
                for (int q = 0; q < nhi; ++q) c2 |= (int64_t)((b_hi >> q) & 1) << tm->hipos[q];
                const int64_t base2 = c2 << kResultChunkBits;
                const W* blk = reinterpret_cast<const W*>(mats + tm->blocks + ((int64_t)a_hi * NH + b_hi) * NL * NL * P);
                if (!lo) {
                    // the partner is the thread's own position in chunk c2: no LDS, no barrier; one entry
                    const W w = blk[0];
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        Group<T> pg;
                        load_group<T>(x, base2 + (int64_t)(g * kSampleThreads + tid) * V, n, vec != 0, pg.v);
#pragma unroll
                        for (int k = 0; k < V; ++k) ApplyElem<T>::mac(pg.v[k], w, acc_re[g * V + k], acc_im[P == 2 ? g * V + k : 0]);
                    }
                    continue;
                }
                __syncthreads();   // (the block before has read the copies)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    Group<T> s;
                    load_group<T>(x, base2 + (int64_t)(g * kSampleThreads + tid) * V, n, vec != 0, s.v);
                    l4[g * kSampleThreads + tid] = s.raw;
                }
                const int in_lds = tm->in_lds;
                if (in_lds) {
                    const double* src = reinterpret_cast<const double*>(blk);
                    for (int i = tid; i < NL * NL * P; i += kSampleThreads) lmat[i] = src[i];
                }
                __syncthreads();
                if (in_lds) {
                    const W* lw = reinterpret_cast<const W*>(lmat);
                    for (int b_lo = 0; b_lo < NL; ++b_lo) {
                        if (!((cm >> b_lo) & 1ull)) continue;   // a zero column of the block (uniform)
                        const uint32_t d = tm->dep[b_lo];
                        const W* col = lw + b_lo * NL;
#pragma unroll
                        for (int i = 0; i < E; ++i) ApplyElem<T>::mac(lx[pos0[i] | d], col[alo[i]], acc_re[i], acc_im[P == 2 ? i : 0]);
                    }
                } else {
                    for (int b_lo = 0; b_lo < NL; ++b_lo) {
                        if (!((cm >> b_lo) & 1ull)) continue;   // a zero column of the block (uniform)
                        const uint32_t d = tm->dep[b_lo];
                        const W* col = blk + b_lo * NL;
#pragma unroll
                        for (int i = 0; i < E; ++i) ApplyElem<T>::mac(lx[pos0[i] | d], col[alo[i]], acc_re[i], acc_im[P == 2 ? i : 0]);
                    }
                }
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            Group<T> o;
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = ApplyElem<T>::round(acc_re[g * V + k], acc_im[P == 2 ? g * V + k : 0]);
            const int64_t e = (c << kResultChunkBits) + (int64_t)(g * kSampleThreads + tid) * V;   // (e + V <= n: n is a multiple of 4096)
            if (vec_out) {
                *reinterpret_cast<uint4*>(y + e) = o.raw;
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) y[e + k] = o.v[k];
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kSampleThreads) void op_apply_general_kernel(const T* __restrict__ x, int64_t n,
                                                                          const OpGenTerm* __restrict__ terms, int nterms,
                                                                          const double* __restrict__ mats, T* __restrict__ y) {
#pragma clang fp contract(off)
    for (int64_t j = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kSampleThreads) {
        double are = 0.0, aim = 0.0;
        for (int t = 0; t < nterms; ++t) {
            const OpGenTerm* tm = terms + t;
            const int nax = tm->nax, D = tm->dim;
            int64_t j0 = j;
            int a = 0;
            for (int q = 0; q < nax; ++q) {
                const int dg = (int)((j / tm->stride[q]) % tm->ext[q]);
                a = a * tm->ext[q] + dg;
                j0 -= dg * tm->stride[q];
            }
            const double* row = mats + tm->mat + (int64_t)a * D * 2;
            for (int b = 0; b < D; ++b) {
                const double wre = row[2 * b], wim = row[2 * b + 1];
                if (wre == 0.0 && wim == 0.0) continue;   // a zero entry: skipped (the header says why no bit changes)
                int rem = b;
                int64_t off = 0;
                for (int q = nax - 1; q >= 0; --q) {
                    off += (rem % tm->ext[q]) * tm->stride[q];
                    rem /= tm->ext[q];
                }
                ApplyElem<T>::mac(x[j0 + off], wre, wim, are, aim);
            }
        }
        y[j] = ApplyElem<T>::round(are, aim);
    }
}

}  // namespace ctg

using namespace ctg;

namespace {

template <typename T>
int op_fast_launch(ctg_exec* e, int64_t n, const OpTermMeta* d_terms, int nterms, const double* d_mats,
                   const unsigned long long* d_cmasks, void* y) {
    const int vec = ((uintptr_t)e->d_result & 15) == 0 ? 1 : 0;
    const int vec_out = ((uintptr_t)y & 15) == 0 ? 1 : 0;
    const int64_t nchunks = n / kResultChunk;
    op_apply_kernel<T><<<dim3((unsigned)result_chunk_grid(nchunks)), dim3(kSampleThreads), 0, e->stream>>>((const T*)e->d_result, n, vec, vec_out, nchunks,
                                                                                      d_terms, nterms, d_mats, d_cmasks, (T*)y);
    LAUNCH_CHECK("op_apply_kernel");
    return CTG_OK;
}

template <typename T>
int op_general_launch(ctg_exec* e, int64_t n, const OpGenTerm* d_terms, int nterms, const double* d_mats, void* y) {
    const int64_t blocks = std::min<int64_t>(kOpGeneralMaxBlocks, (n + kSampleThreads - 1) / kSampleThreads);
    op_apply_general_kernel<T><<<dim3((unsigned)blocks), dim3(kSampleThreads), 0, e->stream>>>((const T*)e->d_result, n, d_terms, nterms,
                                                                                                d_mats, (T*)y);
    LAUNCH_CHECK("op_apply_general_kernel");
    return CTG_OK;
}

}  // namespace

extern "C" int ctg_exec_result_op_apply(ctg_exec* e, int64_t rank, const int64_t* extents, int64_t m, const int32_t* naxes,
                                        const int32_t* axes, const double* mats, void* dev_out, void* host_out) {
    if (!e || !extents) return result_fail(CTG_E_INVALID, "op_apply: null argument");
    ApplyOut out{"op_apply", dev_out, host_out};
    if (out.given() != CTG_OK) return CTG_E_INVALID;
    ResultShape shape;
    const char* why = "";
    if (result_shape(rank, extents, e->plan->result_elems, &shape, &why) != CTG_OK)
        return result_fail(CTG_E_INVALID, "op_apply: %s", why);
    const int64_t n = shape.n;
    const std::vector<int64_t>& stride = shape.strides;
    if (m < 0 || m > CTG_OP_MAX_TERMS)
        return result_fail(CTG_E_INVALID, "op_apply: %lld terms; between 0 and CTG_OP_MAX_TERMS = %d", (long long)m, CTG_OP_MAX_TERMS);
    if (m > 0 && (!naxes || !axes || !mats)) return result_fail(CTG_E_INVALID, "op_apply: null naxes, axes or mats");
    const int dtype = e->plan->dtype;
    const bool real = dtype == CTG_F32 || dtype == CTG_F64;
    const int64_t item = ctg_item_size(dtype);
    if (out.overlap(e, n * item) != CTG_OK) return CTG_E_INVALID;
    // per term: where its axes and its matrix start, and D
    std::vector<int64_t> ax0((size_t)m), mat0((size_t)m);
    std::vector<int> dim((size_t)m);
    int64_t nax_total = 0, entries = 0;
    for (int64_t t = 0; t < m; ++t) {
        if (naxes[t] < 1) return result_fail(CTG_E_INVALID, "op_apply: term %lld names %d axes; at least one is expected", (long long)t, (int)naxes[t]);
        if (naxes[t] > rank) return result_fail(CTG_E_INVALID, "op_apply: term %lld names %d axes of a tensor of rank %lld", (long long)t, (int)naxes[t], (long long)rank);
        ax0[t] = nax_total;
        int64_t d = 1;
        for (int32_t q = 0; q < naxes[t]; ++q) {
            const int32_t a = axes[nax_total + q];
            if (a < 0 || a >= rank) return result_fail(CTG_E_INVALID, "op_apply: term %lld: axis %d is outside the rank %lld", (long long)t, (int)a, (long long)rank);
            if (q > 0 && a <= axes[nax_total + q - 1])
                return result_fail(CTG_E_INVALID, "op_apply: term %lld: its axes are not ascending and distinct", (long long)t);
            d *= extents[a];
            if (d > CTG_OP_MAX_DIM)
                return result_fail(CTG_E_INVALID, "op_apply: term %lld: the product of its extents exceeds CTG_OP_MAX_DIM = %d", (long long)t, CTG_OP_MAX_DIM);
        }
        nax_total += naxes[t];
        dim[t] = (int)d;
        mat0[t] = 2 * entries;
        entries += d * d;
        if (entries > CTG_OP_MAX_ENTRIES)
            return result_fail(CTG_E_INVALID, "op_apply: more than CTG_OP_MAX_ENTRIES = %d matrix entries", CTG_OP_MAX_ENTRIES);
    }
    for (int64_t i = 0; i < entries; ++i) {
        if (!std::isfinite(mats[2 * i]) || !std::isfinite(mats[2 * i + 1])) return result_fail(CTG_E_INVALID, "op_apply: matrix entry %lld is not finite", (long long)i);
        if (real && mats[2 * i + 1] != 0.0)
            return result_fail(CTG_E_INVALID, "op_apply: matrix entry %lld has an imaginary part: O x of a real tensor is not real", (long long)i);
    }
    hipStream_t st = e->stream;
    if (m == 0) return out.zero(st);
    int rc = result_norm_finite(e, "no operator is applied to it");
    if (rc != CTG_OK) return rc;
    void* y = nullptr;
    if (shape.pow2 && n >= kResultChunk) {
        const int LV = item == 4 ? 2 : item == 8 ? 1 : 0, V = 1 << LV, G = kResultChunk / V / kSampleThreads, P = real ? 1 : 2;
        std::vector<OpTermMeta> metas((size_t)m);
        std::vector<double> blocks;
        std::vector<unsigned long long> cmasks;
        blocks.reserve((size_t)entries * P);
        for (int64_t t = 0; t < m; ++t) {
            int64_t mask = 0;   // the term's flat-index bits (an axis of extent 2^k and stride s: s (2^k - 1))
            for (int32_t q = 0; q < naxes[t]; ++q) {
                const int32_t a = axes[ax0[t] + q];
                mask |= stride[a] * (extents[a] - 1);
            }
            OpTermMeta& tm = metas[t];
            memset(&tm, 0, sizeof(tm));
            tm.lo = (int32_t)(mask & (kResultChunk - 1));
            tm.hi = mask >> kResultChunkBits;
            tm.nlo = __builtin_popcount((unsigned)tm.lo);
            tm.nhi = __builtin_popcountll((unsigned long long)tm.hi);
            const int NL = 1 << tm.nlo, NH = 1 << tm.nhi, D = dim[t];   // (NL NH = D: the axes ascend, so a = (a_hi, a_lo))
            tm.in_lds = NL * NL * P <= kOpMatLds ? 1 : 0;
            tm.blocks = (int64_t)blocks.size();
            tm.cmask = (int64_t)cmasks.size();
            {
                int q = 0;
                for (int bit = 0; bit < 63; ++bit)
                    if ((tm.hi >> bit) & 1) tm.hipos[q++] = (uint8_t)bit;
            }
            const uint32_t lo = (uint32_t)tm.lo;
            for (int b = 0; b < NL; ++b) tm.dep[b] = (uint16_t)deposit_bits((uint32_t)b, lo);
            for (int th = 0; th < kSampleThreads; ++th) tm.at[th] = (uint8_t)extract_bits(((uint32_t)th << LV) & lo, lo);
            for (int g = 0; g < G; ++g) tm.ag[g] = (uint8_t)extract_bits(((uint32_t)(g * kSampleThreads) << LV) & lo, lo);
            for (int k = 0; k < V; ++k) tm.ak[k] = (uint8_t)extract_bits((uint32_t)k & lo, lo);
            const double* O = mats + mat0[t];
            for (int a_hi = 0; a_hi < NH; ++a_hi)
                for (int b_hi = 0; b_hi < NH; ++b_hi) {
                    unsigned long long cm = 0;
                    for (int b_lo = 0; b_lo < NL; ++b_lo)
                        for (int a_lo = 0; a_lo < NL; ++a_lo) {
                            const int64_t at = ((int64_t)(a_hi * NL + a_lo) * D + (b_hi * NL + b_lo)) * 2;
                            blocks.push_back(O[at]);
                            if (P == 2) blocks.push_back(O[at + 1]);
                            if (O[at] != 0.0 || O[at + 1] != 0.0) cm |= 1ull << b_lo;
                        }
                    cmasks.push_back(cm);
                }
        }
        // [the terms | their blocks | the column masks | y, when it is staged for host_out]
        const int64_t t_bytes = m * (int64_t)sizeof(OpTermMeta), b_bytes = (int64_t)blocks.size() * 8, c_bytes = (int64_t)cmasks.size() * 8;
        OpTermMeta* d_terms = nullptr;
        double* d_blocks = nullptr;
        unsigned long long* d_cmasks = nullptr;
        auto lay = [&](void* base) {
            Carve c(base);
            d_terms = c.take<OpTermMeta>(t_bytes);
            d_blocks = c.take<double>(b_bytes);
            d_cmasks = c.take<unsigned long long>(c_bytes);
            y = out.y(c.take<char>(out.stage_bytes()));
            return c.bytes();
        };
        rc = reduce_reserve(e, lay(nullptr));
        if (rc != CTG_OK) return rc;
        lay(e->d_reduce);
        HIP_TRY(upload(d_terms, metas.data(), t_bytes, st));
        HIP_TRY(upload(d_blocks, blocks.data(), b_bytes, st));
        HIP_TRY(upload(d_cmasks, cmasks.data(), c_bytes, st));
        rc = dispatch_elem(dtype, [&](auto t) { return op_fast_launch<decltype(t)>(e, n, d_terms, (int)m, d_blocks, d_cmasks, y); });
    } else {
        std::vector<OpGenTerm> terms((size_t)m);
        for (int64_t t = 0; t < m; ++t) {
            OpGenTerm& tm = terms[t];
            memset(&tm, 0, sizeof(tm));
            tm.mat = mat0[t];
            tm.dim = dim[t];
            for (int32_t q = 0; q < naxes[t]; ++q) {
                const int32_t a = axes[ax0[t] + q];
                if (extents[a] == 1) continue;   // (its digit is 0 in a and in b; at most kOpMaxAxes are left: D <= 64)
                tm.stride[tm.nax] = stride[a];
                tm.ext[tm.nax] = (int32_t)extents[a];
                ++tm.nax;
            }
        }
        // [the terms | the matrices as given | y, when it is staged for host_out]
        const int64_t t_bytes = m * (int64_t)sizeof(OpGenTerm), b_bytes = entries * 16;
        OpGenTerm* d_terms = nullptr;
        double* d_mats = nullptr;
        auto lay = [&](void* base) {
            Carve c(base);
            d_terms = c.take<OpGenTerm>(t_bytes);
            d_mats = c.take<double>(b_bytes);
            y = out.y(c.take<char>(out.stage_bytes()));
            return c.bytes();
        };
        rc = reduce_reserve(e, lay(nullptr));
        if (rc != CTG_OK) return rc;
        lay(e->d_reduce);
        HIP_TRY(upload(d_terms, terms.data(), t_bytes, st));
        HIP_TRY(upload(d_mats, mats, b_bytes, st));
        rc = dispatch_elem(dtype, [&](auto t) { return op_general_launch<decltype(t)>(e, n, d_terms, (int)m, d_mats, y); });
    }
    return out.finish(rc, y, st);
}
