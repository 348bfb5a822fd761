// ctg_sample.hip -- statistics of, and draws from, the executor's result tensor on the device.
//
// An amplitude batch (a tree with open output qubits) is rarely wanted as a tensor: its users draw bitstrings
// from p_i = |x_i|^2, ask for its norm, its largest member, the sums a cross-entropy estimate needs.  The result
// tensor stays where the executor left it; three kernels read it:
//
//   prob_block_kernel   one workgroup per block of kSampleBlock consecutive elements: S_b = sum p, Q_b = sum p^2,
//                       the block's largest p and the lowest index attaining it;
//   prob_scan_kernel    one workgroup: the inclusive prefix sums C_b of S_b, sum Q_b, the global maximum;
//   sample_kernel       one wavefront per draw: t = u C_last, the first block with C_b > t, then the first element
//                       of that block whose running sum exceeds t - C_{b-1}.
//
// p is formed and summed in double for every dtype (an fp32 square of a Sycamore-depth amplitude is zero).  Every
// sum has a fixed association -- no atomics -- so the same tensor gives the same bits on every run.
//
// C is built so that a binary search on it is safe: C_b = K_g + s_k, with s_k the SERIAL sum of S inside the
// group g of consecutive blocks that holds b and K_{g+1} = K_g + s_last the serial chain over groups.  Hence C
// never decreases, C_b == C_{b-1} when S_b == 0 and S_b > 0 when C_b > C_{b-1}: the search skips empty blocks and
// never lands in one.  The sum that sample_kernel forms again inside the chosen block (64 lanes x serial runs, a
// wave scan) does NOT have the association of S_b, and t - C_{b-1} carries the rounding of C: a target just below
// C_b may exceed every running sum of the block.  The draw is then the block's last element with p > 0; and both
// predicates ask for p > 0 (L > 0 of a lane), so that no rounding of the scan can return an element of
// probability zero.
#include "ctg_result_host.h"
#include "ctg_sample_elem.h"

namespace ctg {

constexpr int kSampleRun = kSampleBlock / 64;   // contiguous elements per lane in sample_kernel
constexpr int kScanThreads = 1024;
constexpr int64_t kSampleChunk = 1 << 18; // draws per launch of sample_kernel

// (kSampleBlock, kSampleThreads, SampleElem<T>::p and load_group_p: ctg_sample_elem.h, shared with ctg_reduce.hip)

// (m, i) <- the larger p, the lower index among equals
__device__ __forceinline__ void max_merge(double& m, int64_t& i, double mo, int64_t io) {
    if (mo > m || (mo == m && io < i)) {
        m = mo;
        i = io;
    }
}

// Pass 1.  Thread t of block b takes the 16-byte groups t, t + 256, ... of the block (a wave instruction reads
// 1 KiB), adds them in that order; lanes are combined by a butterfly (lane l with l ^ 32, ^ 16, ... ^ 1), waves by
// thread 0 in wave order.
template <typename T>
__global__ __launch_bounds__(kSampleThreads) void prob_block_kernel(const T* __restrict__ x, int64_t n, int vec,
                                                                    double* __restrict__ S, double* __restrict__ Q,
                                                                    double* __restrict__ M, int64_t* __restrict__ I) {
    constexpr int V = 16 / sizeof(T);
    constexpr int G = kSampleBlock / V / kSampleThreads;   // groups per thread
    const int64_t base = (int64_t)blockIdx.x * kSampleBlock;
    double s = 0.0, q = 0.0, m = -1.0;
    int64_t mi = INT64_MAX;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t e = base + ((int64_t)g * kSampleThreads + threadIdx.x) * V;
        double p[V];
        load_group_p<T>(x, e, n, vec != 0, p);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            s += p[k];
            q += p[k] * p[k];
            if (e + k < n) max_merge(m, mi, p[k], e + k);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s += __shfl_xor(s, d, 64);
        q += __shfl_xor(q, d, 64);
        const double mo = __shfl_xor(m, d, 64);
        const int64_t io = (int64_t)__shfl_xor((long long)mi, d, 64);
        max_merge(m, mi, mo, io);
    }
    __shared__ double ws[kSampleThreads / 64], wq[kSampleThreads / 64], wm[kSampleThreads / 64];
    __shared__ int64_t wi[kSampleThreads / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        ws[wave] = s;
        wq[wave] = q;
        wm[wave] = m;
        wi[wave] = mi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kSampleThreads / 64; ++w) {
            s += ws[w];
            q += wq[w];
            max_merge(m, mi, wm[w], wi[w]);
        }
        S[blockIdx.x] = s;
        Q[blockIdx.x] = q;
        M[blockIdx.x] = m;
        I[blockIdx.x] = mi;
    }
}

// Pass 2, one workgroup.  Thread g owns the group of `gs` consecutive blocks [g gs, (g + 1) gs): it adds their S
// serially (s_k), thread 0 chains the group totals (K_g), every thread walks its group again and stores
// C_b = K_g + s_k.  stats <- {C_last, sum Q, max p, (bits of) its lowest index}.
__global__ __launch_bounds__(kScanThreads) void prob_scan_kernel(const double* __restrict__ S, const double* __restrict__ Q,
                                                                 const double* __restrict__ M, const int64_t* __restrict__ I,
                                                                 int64_t nb, int64_t gs, double* __restrict__ C,
                                                                 double* __restrict__ stats) {
    __shared__ double tot[kScanThreads];
    __shared__ double wq[kScanThreads / 64], wm[kScanThreads / 64];
    __shared__ int64_t wi[kScanThreads / 64];
    const int64_t b0 = (int64_t)threadIdx.x * gs;
    const int64_t b1 = b0 + gs < nb ? b0 + gs : nb;
    double s = 0.0, q = 0.0, m = -1.0;
    int64_t mi = INT64_MAX;
    for (int64_t b = b0; b < b1; ++b) {
        s += S[b];
        q += Q[b];
        max_merge(m, mi, M[b], I[b]);
    }
    tot[threadIdx.x] = s;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        q += __shfl_xor(q, d, 64);
        const double mo = __shfl_xor(m, d, 64);
        const int64_t io = (int64_t)__shfl_xor((long long)mi, d, 64);
        max_merge(m, mi, mo, io);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        wq[wave] = q;
        wm[wave] = m;
        wi[wave] = mi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // tot[g] <- K_g, the serial chain of the group totals
        double k = 0.0;
        for (int g = 0; g < kScanThreads; ++g) {
            const double t = tot[g];
            tot[g] = k;
            k += t;
        }
        for (int w = 1; w < kScanThreads / 64; ++w) {
            q += wq[w];
            max_merge(m, mi, wm[w], wi[w]);
        }
        stats[1] = q;
        stats[2] = m;
        reinterpret_cast<int64_t*>(stats)[3] = mi;
    }
    __syncthreads();
    const double k = tot[threadIdx.x];
    s = 0.0;
    for (int64_t b = b0; b < b1; ++b) {
        s += S[b];
        C[b] = k + s;
    }
    if (b0 < nb && b1 == nb) stats[0] = k + s;
}

// Pass 3, one wavefront per draw (kSampleThreads / 64 draws per workgroup).
template <typename T>
__global__ __launch_bounds__(kSampleThreads) void sample_kernel(const T* __restrict__ x, int64_t n, int vec,
                                                                const double* __restrict__ C, int64_t nb,
                                                                const double* __restrict__ u, int64_t ns,
                                                                int64_t* __restrict__ idx, T* __restrict__ elems,
                                                                double* __restrict__ pout) {
    constexpr int V = 16 / sizeof(T);
    const int lane = threadIdx.x & 63;
    const int64_t sid = (int64_t)blockIdx.x * (kSampleThreads / 64) + (threadIdx.x >> 6);
    if (sid >= ns) return;   // (the whole wave)
    const double clast = C[nb - 1];
    const double t = u[sid] * clast;
    // the first block with C_b > t; when the product rounded up to C_last, the last block that is not empty
    // (the first with C_b >= C_last)
    int64_t lo = 0, hi = nb;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (C[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    if (lo == nb) {
        lo = 0;
        hi = nb - 1;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (C[mid] >= clast) hi = mid;
            else lo = mid + 1;
        }
    }
    const int64_t blk = lo;
    const double r = t - (blk > 0 ? C[blk - 1] : 0.0);   // (>= 0: C_{b-1} <= t)
    // lane l: the serial sum L of elements [l R, (l + 1) R) of the block, R = kSampleRun
    const int64_t base = blk * kSampleBlock;
    const int64_t run0 = base + (int64_t)lane * kSampleRun;
    double L = 0.0;
#pragma unroll 4
    for (int g = 0; g < kSampleRun / V; ++g) {
        double p[V];
        load_group_p<T>(x, run0 + (int64_t)g * V, n, vec != 0, p);
#pragma unroll
        for (int k = 0; k < V; ++k) L += p[k];
    }
    // exclusive scan over the lanes
    double inc = L;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    double E = __shfl_up(inc, 1, 64);
    if (lane == 0) E = 0.0;
    // the first lane whose run reaches past r (and holds an element with p > 0); else the last that holds one
    const unsigned long long hit = __ballot(L > 0.0 && E + L > r);
    const unsigned long long any = __ballot(L > 0.0);
    const bool clamp = hit == 0;
    int j;
    if (!clamp) j = __ffsll((long long)hit) - 1;
    else if (any != 0) j = 63 - __clzll((long long)any);
    else j = 0;   // (an empty block: not reachable through C, see the head of the file)
    const double Ej = __shfl(E, j, 64);
    // lane k reads element k of lane j's run; s_k in lane j's own order
    const int64_t ek = base + (int64_t)j * kSampleRun + lane;
    T xe{};
    double pk = 0.0;
    if (ek < n) {
        xe = x[ek];
        pk = SampleElem<T>::p(xe);
    }
    double sk = 0.0, run = 0.0;
#pragma unroll
    for (int k = 0; k < kSampleRun; ++k) {
        run += __shfl(pk, k, 64);
        if (lane == k) sk = run;
    }
    const unsigned long long pos = __ballot(pk > 0.0);
    const unsigned long long hit2 = clamp ? 0ull : __ballot(pk > 0.0 && Ej + sk > r);
    int ksel;
    if (hit2 != 0) ksel = __ffsll((long long)hit2) - 1;
    else if (pos != 0) ksel = 63 - __clzll((long long)pos);
    else ksel = 0;
    if (lane == ksel) {
        idx[sid] = ek < n ? ek : n - 1;
        if (elems) elems[sid] = xe;
        if (pout) pout[sid] = pk;
    }
}

}  // namespace ctg

using namespace ctg;

namespace {

// per-block arrays [S | Q | M | I | C] of nb words each, then 4 words of statistics
int64_t blocks_bytes(int64_t nb) { return (5 * nb + 4) * 8; }
// per draw: the element (16 bytes reserved, first: aligned for every dtype), u, idx, p (8 bytes each)
int64_t io_bytes(int64_t ns) { return ns * 40; }

int grow(void** buf, int64_t* have, int64_t want) {
    if (*have >= want) return CTG_OK;
    if (*buf) {
        HIP_TRY(hipFree(*buf));
        *buf = nullptr;
        *have = 0;
    }
    HIP_TRY(hipMalloc(buf, (size_t)want));
    *have = want;
    return CTG_OK;
}

struct Blocks {
    int64_t nb;
    double *S, *Q, *M, *C, *stats;
    int64_t* I;
};

Blocks carve(const ctg_exec* e) {
    Blocks b;
    b.nb = (e->plan->result_elems + kSampleBlock - 1) / kSampleBlock;
    b.S = (double*)e->d_sample_blocks;
    b.Q = b.S + b.nb;
    b.M = b.Q + b.nb;
    b.I = (int64_t*)(b.M + b.nb);
    b.C = (double*)(b.I + b.nb);
    b.stats = b.C + b.nb;
    return b;
}

template <typename T>
void launch_block_pass(const ctg_exec* e, const Blocks& b, int vec) {
    prob_block_kernel<T><<<dim3((unsigned)b.nb), dim3(kSampleThreads), 0, e->stream>>>(
        (const T*)e->d_result, e->plan->result_elems, vec, b.S, b.Q, b.M, b.I);
}

template <typename T>
void launch_sample(const ctg_exec* e, const Blocks& b, int vec, const double* d_u, int64_t ns, int64_t* d_idx,
                         void* d_el, double* d_p) {
    const int per = kSampleThreads / 64;
    sample_kernel<T><<<dim3((unsigned)((ns + per - 1) / per)), dim3(kSampleThreads), 0, e->stream>>>(
        (const T*)e->d_result, e->plan->result_elems, vec, b.C, b.nb, d_u, ns, d_idx, (T*)d_el, d_p);
}

// passes 1 and 2 on the executor's stream, the four statistics on the host (synchronises)
int run_stats(ctg_exec* e, Blocks* out, int* vec_out, double host[4]) {
    const ctg_plan* p = e->plan;
    const int64_t n = p->result_elems;
    const int64_t nb = (n + kSampleBlock - 1) / kSampleBlock;
    if (nb > 0x7fffffffll) return result_fail(CTG_E_INVALID, "result tensor too large to sample (%lld elements)", (long long)n);
    HIP_TRY(hipSetDevice(e->device));
    if (e->sample_blocks_bytes < blocks_bytes(nb)) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        const int rc = grow(&e->d_sample_blocks, &e->sample_blocks_bytes, blocks_bytes(nb));
        if (rc != CTG_OK) return rc;
    }
    const Blocks b = carve(e);
    const int vec = ((uintptr_t)e->d_result & 15) == 0 ? 1 : 0;
    for (hipEvent_t& ev : e->sample_ev)
        if (!ev) HIP_TRY(hipEventCreate(&ev));
    e->sample_last_valid = false;
    HIP_TRY(hipEventRecord(e->sample_ev[0], e->stream));
    dispatch_elem(p->dtype, [&](auto t) { launch_block_pass<decltype(t)>(e, b, vec); });
    LAUNCH_CHECK("prob_block_kernel");
    HIP_TRY(hipEventRecord(e->sample_ev[1], e->stream));
    const int64_t gs = (nb + kScanThreads - 1) / kScanThreads;
    prob_scan_kernel<<<dim3(1), dim3(kScanThreads), 0, e->stream>>>(b.S, b.Q, b.M, b.I, nb, gs < 1 ? 1 : gs, b.C, b.stats);
    LAUNCH_CHECK("prob_scan_kernel");
    HIP_TRY(hipEventRecord(e->sample_ev[2], e->stream));
    HIP_TRY(hipMemcpyAsync(host, b.stats, 32, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipEventElapsedTime(&e->sample_pass_ms[0], e->sample_ev[0], e->sample_ev[1]));
    HIP_TRY(hipEventElapsedTime(&e->sample_pass_ms[1], e->sample_ev[1], e->sample_ev[2]));
    memcpy(e->sample_last, host, 32);
    e->sample_last_valid = true;
    if (out) *out = b;
    if (vec_out) *vec_out = vec;
    return CTG_OK;
}

}  // namespace

extern "C" {

int ctg_exec_result_stats(ctg_exec* e, double* sum_p, double* sum_p2, double* max_p, int64_t* argmax) {
    if (!e) return result_fail(CTG_E_INVALID, "null argument");
    double host[4];
    const int rc = run_stats(e, nullptr, nullptr, host);
    if (rc != CTG_OK) return rc;
    if (sum_p) *sum_p = host[0];
    if (sum_p2) *sum_p2 = host[1];
    if (max_p) *max_p = host[2];
    if (argmax) memcpy(argmax, &host[3], 8);
    return CTG_OK;
}

int ctg_exec_sample_info(ctg_exec* e, double* sum_p, double* sum_p2, double* max_p, int64_t* argmax, float* pass_ms) {
    if (!e) return result_fail(CTG_E_INVALID, "null argument");
    if (!e->sample_last_valid) return result_fail(CTG_E_INVALID, "no statistics or sample call has completed on this executor");
    if (sum_p) *sum_p = e->sample_last[0];
    if (sum_p2) *sum_p2 = e->sample_last[1];
    if (max_p) *max_p = e->sample_last[2];
    if (argmax) memcpy(argmax, &e->sample_last[3], 8);
    if (pass_ms) {
        pass_ms[0] = e->sample_pass_ms[0];
        pass_ms[1] = e->sample_pass_ms[1];
    }
    return CTG_OK;
}

int ctg_exec_sample_result(ctg_exec* e, const double* u, int64_t n, int64_t* idx, void* elems, double* p) {
    if (!e) return result_fail(CTG_E_INVALID, "null argument");
    if (n < 0) return result_fail(CTG_E_INVALID, "negative number of draws");
    if (n == 0) return CTG_OK;
    if (!u || !idx) return result_fail(CTG_E_INVALID, "null argument");
    for (int64_t s = 0; s < n; ++s)
        if (!(u[s] >= 0.0 && u[s] < 1.0))
            return result_fail(CTG_E_INVALID, "uniform %lld is %g: not in [0, 1)", (long long)s, u[s]);
    Blocks b;
    int vec = 0;
    double host[4];
    {
        const int rc = run_stats(e, &b, &vec, host);
        if (rc != CTG_OK) return rc;
    }
    if (!(host[0] > 0.0) || !std::isfinite(host[0])) return result_norm_fail(host[0], "nothing to draw from");
    const int64_t isz = ctg_item_size(e->plan->dtype);
    const int64_t chunk = n < kSampleChunk ? n : kSampleChunk;
    {
        // (the stream is idle: run_stats synchronised it)
        const int rc = grow(&e->d_sample_io, &e->sample_io_bytes, io_bytes(chunk));
        if (rc != CTG_OK) return rc;
    }
    char* d_el = (char*)e->d_sample_io;
    double* d_u = (double*)(d_el + chunk * 16);
    int64_t* d_idx = (int64_t*)(d_u + chunk);
    double* d_p = (double*)(d_idx + chunk);
    for (int64_t s0 = 0; s0 < n; s0 += chunk) {
        const int64_t ns = n - s0 < chunk ? n - s0 : chunk;
        HIP_TRY(hipMemcpyAsync(d_u, u + s0, ns * 8, hipMemcpyHostToDevice, e->stream));
        dispatch_elem(e->plan->dtype, [&](auto t) { launch_sample<decltype(t)>(e, b, vec, d_u, ns, d_idx, d_el, d_p); });
        LAUNCH_CHECK("sample_kernel");
        HIP_TRY(hipMemcpyAsync(idx + s0, d_idx, ns * 8, hipMemcpyDeviceToHost, e->stream));
        if (elems)
            HIP_TRY(hipMemcpyAsync((char*)elems + s0 * isz, d_el, ns * isz, hipMemcpyDeviceToHost, e->stream));
        if (p) HIP_TRY(hipMemcpyAsync(p + s0, d_p, ns * 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    return CTG_OK;
}

}  // extern "C"
