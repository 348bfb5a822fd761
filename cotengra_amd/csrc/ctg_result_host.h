// ctg_result_host.h -- the host prologue of the entry points that read the executor's result tensor in place
// (ctg_sample.hip, ctg_reduce.hip, ctg_rdm.hip, ctg_pauli.hip, ctg_pauli_apply.hip, ctg_op_apply.hip): the error
// return, the shape check, the norm gate, the dispatch on the plan's dtype, the layout of the scratch and the outputs
// of the two apply entry points.  Every refusal here comes before anything is allocated or launched.
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ctg_exec_state.h"

#pragma GCC visibility push(hidden)
namespace ctg {

// records the message as ctg_last_error() and returns `code`
inline int result_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    ctg_set_error_(buf);
    return code;
}

#define HIP_TRY(expr)                                                                                             \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess)                                                                                     \
            return ctg::result_fail(_e == hipErrorOutOfMemory ? CTG_E_NOMEM : CTG_E_HIP, "%s failed: %s", #expr,  \
                                    hipGetErrorString(_e));                                                       \
    } while (0)

#define LAUNCH_CHECK(name)                                                                                              \
    do {                                                                                                                \
        hipError_t _e = hipGetLastError();                                                                              \
        if (_e != hipSuccess) return ctg::result_fail(CTG_E_HIP, name " launch failed: %s", hipGetErrorString(_e));     \
    } while (0)

inline int64_t up256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// host -> device from a vector of the caller's frame, complete on return: no copy outlives the frame, on any path
inline hipError_t upload(void* dst, const void* src, int64_t bytes, hipStream_t st) {
    const hipError_t e = hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// the bits of v under the set bits of mask, squeezed together (its inverse: deposit_bits of ctg_result_elem.h)
inline int64_t extract_bits(int64_t v, int64_t mask) {
    int64_t r = 0;
    int o = 0;
    for (int b = 0; b < 63; ++b)
        if ((mask >> b) & 1) r |= ((v >> b) & 1) << o++;
    return r;
}

// The caller's view of the result tensor: n elements, row-major strides; pow2: every extent is a power of two.
// stop: the axis a refusal names (rank: the product as a whole).
struct ResultShape {
    int64_t n = 1, stop = 0;
    bool pow2 = true;
    std::vector<int64_t> strides;
};

// CTG_OK, or CTG_E_INVALID with *why set (the caller prefixes its name)
inline int result_shape(int64_t rank, const int64_t* extents, int64_t result_elems, ResultShape* out, const char** why) {
    ResultShape& s = *out = ResultShape();
    if (rank < 0) return *why = "negative rank", CTG_E_INVALID;
    for (; s.stop < rank; ++s.stop) {
        const int64_t ext = extents[s.stop];
        if (ext < 1) return *why = "an extent is not positive", CTG_E_INVALID;
        if (ext > kReduceMaxElems / s.n) return *why = "the extents' product does not equal result_elems", CTG_E_INVALID;
        s.n *= ext;
        s.pow2 = s.pow2 && (ext & (ext - 1)) == 0;
    }
    if (s.n != result_elems) return *why = "the extents' product does not equal result_elems", CTG_E_INVALID;
    s.strides = std::vector<int64_t>((size_t)rank);
    int64_t st = 1;
    for (int64_t a = rank - 1; a >= 0; --a) {
        s.strides[a] = st;
        st *= extents[a];
    }
    return CTG_OK;
}

// CTG_E_NORM: a result tensor whose sum p is `sum_p` answers no question; `what` ends the sentence
inline int result_norm_fail(double sum_p, const char* what) {
    return result_fail(CTG_E_NORM, "the result tensor's sum of |x|^2 is %g: %s", sum_p, what);
}

// sum p of the result by the statistics passes of ctg_sample.hip (synchronises): CTG_E_NORM unless finite
inline int result_norm_finite(ctg_exec* e, const char* what) {
    double sum_p = 0.0;
    const int rc = ctg_exec_result_stats(e, &sum_p, nullptr, nullptr, nullptr);
    if (rc != CTG_OK) return rc;
    return std::isfinite(sum_p) ? CTG_OK : result_norm_fail(sum_p, what);
}

// f(T{}) for the element type T of a CTG_* dtype code
template <typename F>
auto dispatch_elem(int dtype, F&& f) {
    switch (dtype) {
        case CTG_F32: return f(float{});
        case CTG_F64: return f(double{});
        case CTG_C64: return f(float2{});
        default: return f(double2{});
    }
}

// Consecutive 256-byte-aligned pieces of one buffer.  Over a null base it only measures: an entry point lays its
// scratch out in one function, once for bytes() to reserve and once over the reserved buffer.
struct Carve {
    char* base;
    int64_t off = 0;
    explicit Carve(void* b) : base((char*)b) {}
    template <typename T>
    T* take(int64_t bytes) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += up256(bytes);
        return p;
    }
    int64_t bytes() const { return off; }
};

// The outputs of an apply entry point (`who`): y goes to dev_out, to host_out, or to both; it is staged at the end
// of the scratch when only host_out is given.
struct ApplyOut {
    const char* who;
    void *dev_out, *host_out;
    int64_t bytes = 0;   // of y: set by overlap()

    int given() const {
        return dev_out || host_out ? CTG_OK : result_fail(CTG_E_INVALID, "%s: neither dev_out nor host_out is given", who);
    }
    int overlap(const ctg_exec* e, int64_t y_bytes) {
        bytes = y_bytes;
        const uintptr_t d0 = (uintptr_t)dev_out, r0 = (uintptr_t)e->d_result;
        if (dev_out && d0 < r0 + (uintptr_t)bytes && r0 < d0 + (uintptr_t)bytes)
            return result_fail(CTG_E_INVALID, "%s: dev_out overlaps the result tensor", who);
        return CTG_OK;
    }
    // y of an empty sum
    int zero(hipStream_t st) const {
        if (dev_out) {
            HIP_TRY(hipMemsetAsync(dev_out, 0, (size_t)bytes, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        if (host_out) memset(host_out, 0, (size_t)bytes);
        return CTG_OK;
    }
    int64_t stage_bytes() const { return dev_out ? 0 : bytes; }
    // where the kernel writes: `staged` is the scratch's piece of stage_bytes()
    void* y(void* staged) const { return dev_out ? dev_out : staged; }
    // after the launch (`rc`: what it returned): the copy to host_out, and the call is synchronous
    int finish(int rc, void* y, hipStream_t st) const {
        if (rc != CTG_OK) return rc;
        if (host_out) HIP_TRY(hipMemcpyAsync(host_out, y, (size_t)bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return CTG_OK;
    }
};

}  // namespace ctg
#pragma GCC visibility pop
