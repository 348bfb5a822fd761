// ctg_pauli_apply.hip -- y = (sum over s of c_s P_s) x for Pauli strings P_s over the axes of the executor's result
// tensor x and real coefficients c_s, written on the device next to x (DESIGN.md section 17;
// ctg_exec_result_pauli_apply of include/ctg_hip.h).  conj(2 y) is the cotangent of <x| H |x> for a VJP plan.
//
// Strings, codes and masks are those of ctg_pauli.hip: xm the flat-index bits of the X and Y axes, zm those of the Z
// and Y axes, ny the number of Y, and
//
//   (P x)[j] = i^ny (-1)^popcount((j ^ xm) & zm) x[j ^ xm] = (-i)^ny (-1)^popcount(j & zm) x[j ^ xm]
//
// (popcount(xm & zm) = ny).  So string s adds +-c_s to ONE component of a complex weight: the real one for even ny, the
// imaginary one for odd ny, with the sign (-1)^popcount(j & zm) flipped for ny mod 4 in {1, 2}.
//
// The definition of the bits of y (a host reference can mirror it, tests/pauli_apply_util.py):
//   - the strings are grouped by their X / Y axis set (xm), groups in order of first appearance, the caller's order
//     inside a group;
//   - per element j and group g:  W_re = 0.0, W_im = 0.0, then string after string W_re (even ny) or W_im (odd ny)
//     <- W + (+-c_s) in fp64;
//   - with p = x[j ^ xm_g] widened to fp64:  acc_re <- acc_re + (W_re p_re - W_im p_im),
//     acc_im <- acc_im + (W_re p_im + W_im p_re); the four products, the difference / sum and the addition to acc each
//     rounded once, nothing fused (fp contract(off)); acc starts at 0.0;  real plans: acc <- acc + W_re p;
//   - after the last group acc is rounded once to the plan's dtype.
// No atomics; no sum crosses a thread: the bits of y are a function of (dtype, extents, ops in order, coeffs, the
// tensor's bytes) alone.
//
//   power of two (every extent a power of two, at least kResultChunk = 4096 elements):
//
//     pauli_apply_kernel<T>   256 threads, two workgroups per CU; one launch.  A workgroup owns the output chunks wg,
//                             wg + grid, ... of 4096 elements; thread t holds the 16-byte groups g 256 + t of a chunk
//                             (16 / V groups of V = 16 / sizeof(T) elements: 16 elements) as fp64 accumulators acc
//                             and W.  The strings of a group run in passes of at most 32; a pass gives every element a
//                             32-bit sign word, bit s for string s:
//                                tw[t] ^ gw[g] ^ kw[k] ^ cw
//                             -- the parities of zm_s with the thread's, the group's and the in-group bits of the
//                             element's position, all three from the host in the pass metadata (kw also carries the
//                             sign of the folded coefficient, so the coefficient itself is |c_s|), and with the chunk
//                             base: one ballot per (chunk, pass).  Per (element, string): a shift, an and-or and the
//                             fp64 addition.  After the last pass of a group the partner chunk c ^ (xm >> 12) is read
//                             once: straight from memory as the thread's own groups when xm_lo < V (partner inside
//                             the 16-byte group: a swap in registers), else through an LDS copy of the chunk read at
//                             group (g 256 + t) ^ (xm_lo / V) -- the xor permutes groups inside aligned blocks, so a
//                             wave's lanes stay on distinct banks (section 16).  The tensor is read once per group
//                             and y written once: one coalesced 16-byte store per lane and group.
//                             grid = min(512, ceil(chunks / 3)): a function of n alone.
//
//   general (any other shape): pauli_apply_general_kernel<T>, a thread per output element (grid-stride), the same
//   groups and order; partner and signs from the digits (j / stride) & 1 as in pauli_general_kernel.  Not tuned.
//
// Scratch (the executor's d_reduce, reduce_reserve): the pass metadata (1640 bytes
// per pass, at most m passes; general route: 24 bytes per group, 24 per string, 8 per non-identity letter) and, when
// only host_out is given, result_elems elements of y.
#include <algorithm>
#include <string>
#include <unordered_map>

#include "ctg_result_elem.h"
#include "ctg_result_host.h"

namespace ctg {

constexpr int kApplyPass = 32;              // strings of a pass: one bit each in a sign word
constexpr int64_t kApplyGeneralMaxBlocks = 1 << 20;

// What a pass of the power-of-two route needs on the device
struct ApplyPassMeta {
    int64_t zm[kApplyPass];          // the Z / Y bits of string s of the pass
    double coef[kApplyPass];         // |c_s|
    uint32_t tw[kSampleThreads];     // bit s: parity(zm_s & the bits of thread t in an element's position)
    uint32_t gw[16];                 // ... & the bits of group row g
    uint32_t kw[4];                  // ... & the bits of element k of a 16-byte group, xor the sign of (-i)^ny c_s
    int64_t xm;                      // the X / Y bits of the pass's group
    uint32_t odd;                    // bit s: ny of string s is odd (it adds to W_im)
    int32_t count;
    int32_t last;                    // 1: the last pass of its group (the partner is multiplied in)
    int32_t pad;
};

// A group and a string of the general route: axes are entries of the stride lists
struct ApplyGenGroup {
    int64_t xax0;       // its X / Y axes: xstride[xax0 .. xax0 + nx)
    int32_t nx, s0, s1, pad;   // its strings: strs[s0 .. s1)
};
struct ApplyGenString {
    int64_t zax0;       // its Z / Y axes: zstride[zax0 .. zax0 + nz)
    int32_t nz, odd;
    double coef;        // (-i)^ny c_s without the i: the signed real factor
};

// (acc += W p and the rounding of acc to T: ApplyElem<T> of ctg_result_elem.h)
template <typename T>
__global__ __launch_bounds__(kSampleThreads, 2) void pauli_apply_kernel(const T* __restrict__ x, int64_t n, int vec, int vec_out,
                                                                        int64_t nchunks, const ApplyPassMeta* __restrict__ pass,
                                                                        int npass, T* __restrict__ y) {
#pragma clang fp contract(off)
    constexpr int P = ApplyElem<T>::P;
    constexpr int V = 16 / sizeof(T);
    constexpr int LV = V == 4 ? 2 : V == 2 ? 1 : 0;
    constexpr int G = kResultChunk / V / kSampleThreads;
    constexpr int E = G * V;   // elements of a thread: 16
    static_assert(G <= 16 && V <= 4, "gw and kw of ApplyPassMeta");
    __shared__ __attribute__((aligned(16))) unsigned char raw[kResultChunk * (int)sizeof(T)];
    uint4* l4 = reinterpret_cast<uint4*>(raw);
    const int tid = threadIdx.x, lane = tid & 63;

    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t base = c << kResultChunkBits;
        double acc_re[E], acc_im[P == 2 ? E : 1], w_re[E], w_im[P == 2 ? E : 1];
#pragma unroll
        for (int i = 0; i < E; ++i) {
            acc_re[i] = 0.0;
            w_re[i] = 0.0;
            if (P == 2) {
                acc_im[i] = 0.0;
                w_im[i] = 0.0;
            }
        }
        for (int p = 0; p < npass; ++p) {
            const ApplyPassMeta* pm = pass + p;
            const int count = pm->count;
            const uint32_t odd = pm->odd;
            // the chunk's sign word: lane s holds parity(base & zm_s); wave-uniform
            const int64_t myzm = pm->zm[lane & (kApplyPass - 1)];
            const uint32_t cw = (uint32_t)__ballot(__popcll((unsigned long long)(base & myzm)) & 1);
            const uint32_t tw = pm->tw[tid] ^ cw;
            uint32_t sw[E];
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int k = 0; k < V; ++k) sw[g * V + k] = tw ^ pm->gw[g] ^ pm->kw[k];
            for (int s = 0; s < count; ++s) {
                const double cs = pm->coef[s];   // (not negative: its sign is in kw)
                const uint32_t hi = (uint32_t)__double2hiint(cs);
                const int lo = __double2loint(cs);
                const int sh = 31 - s;
                if (P == 2 && ((odd >> s) & 1u)) {
#pragma unroll
                    for (int i = 0; i < E; ++i)
                        w_im[P == 2 ? i : 0] = w_im[P == 2 ? i : 0] + __hiloint2double((int)(((sw[i] << sh) & 0x80000000u) | hi), lo);
                } else {
#pragma unroll
                    for (int i = 0; i < E; ++i) w_re[i] = w_re[i] + __hiloint2double((int)(((sw[i] << sh) & 0x80000000u) | hi), lo);
                }
            }
            if (!pm->last) continue;
            // the group's weights are complete: multiply the partner in
            const int64_t xm = pm->xm;
            const uint32_t xlo = (uint32_t)(xm & (kResultChunk - 1));
            const int64_t base2 = (c ^ (xm >> kResultChunkBits)) << kResultChunkBits;
            const uint32_t xin = xlo & (V - 1), xg = xlo >> LV;
            if (xg) {
                __syncthreads();   // (the group before has read the copy)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    Group<T> t;
                    load_group<T>(x, base2 + (int64_t)(g * kSampleThreads + tid) * V, n, vec != 0, t.v);
                    l4[g * kSampleThreads + tid] = t.raw;
                }
                __syncthreads();
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                Group<T> pg;
                if (xg)
                    pg.raw = l4[(uint32_t)(g * kSampleThreads + tid) ^ xg];
                else
                    load_group<T>(x, base2 + (int64_t)(g * kSampleThreads + tid) * V, n, vec != 0, pg.v);
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
                    const int i = g * V + k;
                    ApplyElem<T>::mac(pg.v[k], w_re[i], w_im[P == 2 ? i : 0], acc_re[i], acc_im[P == 2 ? i : 0]);
                    w_re[i] = 0.0;
                    if (P == 2) w_im[i] = 0.0;
                }
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            Group<T> o;
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = ApplyElem<T>::round(acc_re[g * V + k], acc_im[P == 2 ? g * V + k : 0]);
            const int64_t e = base + (int64_t)(g * kSampleThreads + tid) * V;   // (e + V <= n: n is a multiple of 4096)
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
__global__ __launch_bounds__(kSampleThreads) void pauli_apply_general_kernel(const T* __restrict__ x, int64_t n,
                                                                             const ApplyGenGroup* __restrict__ groups, int ngroups,
                                                                             const ApplyGenString* __restrict__ strs,
                                                                             const int64_t* __restrict__ xstride,
                                                                             const int64_t* __restrict__ zstride, T* __restrict__ y) {
#pragma clang fp contract(off)
    for (int64_t j = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kSampleThreads) {
        double are = 0.0, aim = 0.0;
        for (int gi = 0; gi < ngroups; ++gi) {
            const ApplyGenGroup gr = groups[gi];
            int64_t p = j;
            for (int a = 0; a < gr.nx; ++a) {
                const int64_t sa = xstride[gr.xax0 + a];
                p += ((j / sa) & 1) ? -sa : sa;   // X, Y: the other value of the axis
            }
            double wre = 0.0, wim = 0.0;
            for (int s = gr.s0; s < gr.s1; ++s) {
                const ApplyGenString st = strs[s];
                uint32_t sign = 0;
                for (int a = 0; a < st.nz; ++a) sign ^= (uint32_t)((j / zstride[st.zax0 + a]) & 1);   // Z, Y: the digit's parity
                const double v = signed_by(st.coef, sign);
                if (st.odd)
                    wim = wim + v;
                else
                    wre = wre + v;
            }
            ApplyElem<T>::mac(x[p], wre, wim, are, aim);
        }
        y[j] = ApplyElem<T>::round(are, aim);
    }
}

}  // namespace ctg

using namespace ctg;

namespace {

uint32_t parity64(int64_t v) { return (uint32_t)(__builtin_popcountll((unsigned long long)v) & 1); }

// (-i)^ny c: the signed real factor (the component is chosen by ny & 1)
double folded(double c, int ny) { return ((ny & 3) == 1 || (ny & 3) == 2) ? -c : c; }

template <typename T>
int apply_fast_launch(ctg_exec* e, int64_t n, const ApplyPassMeta* d_pass, int npass, void* y) {
    const int vec = ((uintptr_t)e->d_result & 15) == 0 ? 1 : 0;
    const int vec_out = ((uintptr_t)y & 15) == 0 ? 1 : 0;
    const int64_t nchunks = n / kResultChunk;
    pauli_apply_kernel<T><<<dim3((unsigned)result_chunk_grid(nchunks)), dim3(kSampleThreads), 0, e->stream>>>((const T*)e->d_result, n, vec, vec_out, nchunks,
                                                                                         d_pass, npass, (T*)y);
    LAUNCH_CHECK("pauli_apply_kernel");
    return CTG_OK;
}

template <typename T>
int apply_general_launch(ctg_exec* e, int64_t n, const ApplyGenGroup* d_groups, int ngroups, const ApplyGenString* d_strs,
                         const int64_t* d_xs, const int64_t* d_zs, void* y) {
    const int64_t blocks = std::min<int64_t>(kApplyGeneralMaxBlocks, (n + kSampleThreads - 1) / kSampleThreads);
    pauli_apply_general_kernel<T><<<dim3((unsigned)blocks), dim3(kSampleThreads), 0, e->stream>>>((const T*)e->d_result, n, d_groups,
                                                                                                   ngroups, d_strs, d_xs, d_zs, (T*)y);
    LAUNCH_CHECK("pauli_apply_general_kernel");
    return CTG_OK;
}

}  // namespace

extern "C" int ctg_exec_result_pauli_apply(ctg_exec* e, int64_t rank, const int64_t* extents, int64_t m, const uint8_t* ops,
                                           const double* coeffs, void* dev_out, void* host_out) {
    if (!e || !extents || !ops) return result_fail(CTG_E_INVALID, "pauli_apply: null argument");
    ApplyOut out{"pauli_apply", dev_out, host_out};
    if (out.given() != CTG_OK) return CTG_E_INVALID;
    ResultShape shape;
    const char* why = "";
    if (result_shape(rank, extents, e->plan->result_elems, &shape, &why) != CTG_OK)
        return result_fail(CTG_E_INVALID, "pauli_apply: %s", why);
    const int64_t n = shape.n;
    const std::vector<int64_t>& stride = shape.strides;
    if (m < 0 || m > CTG_PAULI_MAX_STRINGS)
        return result_fail(CTG_E_INVALID, "pauli_apply: %lld strings; between 0 and CTG_PAULI_MAX_STRINGS = %d", (long long)m,
                     CTG_PAULI_MAX_STRINGS);
    if (m > 0 && !coeffs) return result_fail(CTG_E_INVALID, "pauli_apply: null coeffs");
    const int dtype = e->plan->dtype;
    const bool real = dtype == CTG_F32 || dtype == CTG_F64;
    const int64_t item = ctg_item_size(dtype);
    if (out.overlap(e, n * item) != CTG_OK) return CTG_E_INVALID;
    std::vector<int> ny((size_t)m, 0);
    for (int64_t s = 0; s < m; ++s) {
        for (int64_t a = 0; a < rank; ++a) {
            const uint8_t op = ops[s * rank + a];
            if (op > 3)
                return result_fail(CTG_E_INVALID, "pauli_apply: string %lld, axis %lld: code %d is none of 0 .. 3", (long long)s, (long long)a,
                             (int)op);
            if (op != 0 && extents[a] != 2)
                return result_fail(CTG_E_INVALID, "pauli_apply: string %lld puts a letter other than I on axis %lld of extent %lld",
                             (long long)s, (long long)a, (long long)extents[a]);
            ny[s] += op == 2;
        }
        if (!std::isfinite(coeffs[s])) return result_fail(CTG_E_INVALID, "pauli_apply: coefficient %lld is not finite", (long long)s);
        if (real && (ny[s] & 1))
            return result_fail(CTG_E_INVALID, "pauli_apply: string %lld has an odd number of Y: P x of a real tensor is not real", (long long)s);
    }
    hipStream_t st = e->stream;
    if (m == 0) return out.zero(st);
    {
        const int rc = result_norm_finite(e, "no Pauli sum is applied to it");
        if (rc != CTG_OK) return rc;
    }
    // groups by the X / Y axis set in order of first appearance, the caller's order inside
    std::vector<std::vector<int64_t>> members;
    {
        std::unordered_map<std::string, size_t> where;
        std::string key((size_t)rank, '0');
        for (int64_t s = 0; s < m; ++s) {
            for (int64_t a = 0; a < rank; ++a) key[(size_t)a] = (ops[s * rank + a] == 1 || ops[s * rank + a] == 2) ? '1' : '0';
            auto it = where.find(key);
            if (it == where.end()) {
                it = where.emplace(key, members.size()).first;
                members.emplace_back();
            }
            members[it->second].push_back(s);
        }
    }
    void* y = nullptr;
    int rc;
    if (shape.pow2 && n >= kResultChunk) {
        const int LV = item == 4 ? 2 : item == 8 ? 1 : 0, V = 1 << LV, G = kResultChunk / V / kSampleThreads;
        std::vector<ApplyPassMeta> passes;
        for (const auto& mem : members) {
            int64_t xm = 0;
            for (int64_t a = 0; a < rank; ++a) {
                const uint8_t op = ops[mem[0] * rank + a];
                if (op == 1 || op == 2) xm |= stride[a];
            }
            for (size_t i0 = 0; i0 < mem.size(); i0 += kApplyPass) {
                ApplyPassMeta pm{};
                pm.xm = xm;
                pm.count = (int32_t)std::min<size_t>(kApplyPass, mem.size() - i0);
                pm.last = i0 + kApplyPass >= mem.size() ? 1 : 0;
                for (int i = 0; i < pm.count; ++i) {
                    const int64_t s = mem[i0 + i];
                    int64_t zm = 0;
                    for (int64_t a = 0; a < rank; ++a) {
                        const uint8_t op = ops[s * rank + a];
                        if (op == 3 || op == 2) zm |= stride[a];
                    }
                    const double c = folded(coeffs[s], ny[s]);
                    pm.zm[i] = zm;
                    pm.coef[i] = std::fabs(c);
                    if (ny[s] & 1) pm.odd |= 1u << i;
                    const int64_t zlo = zm & (kResultChunk - 1);
                    for (int t = 0; t < kSampleThreads; ++t) pm.tw[t] |= parity64(((int64_t)t << LV) & zlo) << i;
                    for (int g = 0; g < G; ++g) pm.gw[g] |= parity64(((int64_t)g * kSampleThreads << LV) & zlo) << i;
                    for (int k = 0; k < V; ++k) pm.kw[k] |= (parity64((int64_t)k & zlo) ^ (std::signbit(c) ? 1u : 0u)) << i;
                }
                passes.push_back(pm);
            }
        }
        // [the passes | y, when it is staged for host_out]
        const int64_t pass_bytes = (int64_t)passes.size() * (int64_t)sizeof(ApplyPassMeta);
        ApplyPassMeta* d_pass = nullptr;
        auto lay = [&](void* base) {
            Carve c(base);
            d_pass = c.take<ApplyPassMeta>(pass_bytes);
            y = out.y(c.take<char>(out.stage_bytes()));
            return c.bytes();
        };
        rc = reduce_reserve(e, lay(nullptr));
        if (rc != CTG_OK) return rc;
        lay(e->d_reduce);
        HIP_TRY(upload(d_pass, passes.data(), pass_bytes, st));
        const int np = (int)passes.size();
        rc = dispatch_elem(dtype, [&](auto t) { return apply_fast_launch<decltype(t)>(e, n, d_pass, np, y); });
    } else {
        std::vector<ApplyGenGroup> groups;
        std::vector<ApplyGenString> strs;
        std::vector<int64_t> xs, zs;
        for (const auto& mem : members) {
            ApplyGenGroup gr{};
            gr.xax0 = (int64_t)xs.size();
            for (int64_t a = 0; a < rank; ++a) {
                const uint8_t op = ops[mem[0] * rank + a];
                if (op == 1 || op == 2) {
                    xs.push_back(stride[a]);
                    ++gr.nx;
                }
            }
            gr.s0 = (int32_t)strs.size();
            for (int64_t s : mem) {
                ApplyGenString gs{};
                gs.zax0 = (int64_t)zs.size();
                for (int64_t a = 0; a < rank; ++a) {
                    const uint8_t op = ops[s * rank + a];
                    if (op == 3 || op == 2) {
                        zs.push_back(stride[a]);
                        ++gs.nz;
                    }
                }
                gs.odd = ny[s] & 1;
                gs.coef = folded(coeffs[s], ny[s]);
                strs.push_back(gs);
            }
            gr.s1 = (int32_t)strs.size();
            groups.push_back(gr);
        }
        // [the groups | the strings | strides of the X / Y axes | strides of the Z / Y axes | y, when it is staged]
        const int64_t g_bytes = (int64_t)groups.size() * (int64_t)sizeof(ApplyGenGroup);
        const int64_t s_bytes = (int64_t)strs.size() * (int64_t)sizeof(ApplyGenString);
        const int64_t x_bytes = (int64_t)xs.size() * 8, z_bytes = (int64_t)zs.size() * 8;
        ApplyGenGroup* d_groups = nullptr;
        ApplyGenString* d_strs = nullptr;
        int64_t *d_xs = nullptr, *d_zs = nullptr;
        auto lay = [&](void* base) {
            Carve c(base);
            d_groups = c.take<ApplyGenGroup>(g_bytes);
            d_strs = c.take<ApplyGenString>(s_bytes);
            d_xs = c.take<int64_t>(x_bytes);
            d_zs = c.take<int64_t>(z_bytes);
            y = out.y(c.take<char>(out.stage_bytes()));
            return c.bytes();
        };
        rc = reduce_reserve(e, lay(nullptr));
        if (rc != CTG_OK) return rc;
        lay(e->d_reduce);
        HIP_TRY(upload(d_groups, groups.data(), g_bytes, st));
        HIP_TRY(upload(d_strs, strs.data(), s_bytes, st));
        if (x_bytes) HIP_TRY(upload(d_xs, xs.data(), x_bytes, st));
        if (z_bytes) HIP_TRY(upload(d_zs, zs.data(), z_bytes, st));
        const int ng = (int)groups.size();
        rc = dispatch_elem(dtype, [&](auto t) { return apply_general_launch<decltype(t)>(e, n, d_groups, ng, d_strs, d_xs, d_zs, y); });
    }
    return out.finish(rc, y, st);
}
