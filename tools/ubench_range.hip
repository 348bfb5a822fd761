// ubench_range.hip -- the range pass (csrc/ctg_range.hip: range_hist_kernel + range_reduce_kernel) next to the
// max-abs pass the fp16 x 2 arithmetic already runs over operands without a recorded maximum (launch_maxabs_f32,
// csrc/ctg_kernels_valu.hip), over the SAME bytes: n complex64 elements of unit Gaussian-like data, both passes
// alternating in one process after a warm-up of each, device events around each launch; one JSON line per size.
// Both only read.  (tools/range_audit.py runs this and keeps the lines.)
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/ubench_range tools/ubench_range.hip \
//            -Lcotengra_amd/lib -lctg_hip -Wl,-rpath,'$ORIGIN/../cotengra_amd/lib'
// Run:   tools/ubench_range [log2 of the element count ...]      (default 20 24 28)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cotengra_amd/csrc/ctg_exec_state.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

// sums of four uniforms: a bell shape over about six binades, as a contraction's intermediates have
__global__ void fill_kernel(float* x, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t s = (uint64_t)i * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
        float v = 0.f;
        for (int k = 0; k < 4; ++k) {
            s ^= s >> 29; s *= 0xBF58476D1CE4E5B9ull; s ^= s >> 32;
            v += (float)(s >> 40) * (1.0f / 16777216.0f) - 0.5f;
        }
        x[i] = v;
    }
}

static float median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv) {
    std::vector<int> sizes;
    for (int i = 1; i < argc; ++i) sizes.push_back(atoi(argv[i]));
    if (sizes.empty()) sizes = {20, 24, 28};
    hipStream_t stream;
    CK(hipStreamCreate(&stream));
    hipEvent_t ev[3];
    for (auto& e : ev) CK(hipEventCreate(&e));
    const int reps = 11;
    for (int lg : sizes) {
        if (lg < 4 || lg > 32) continue;
        const int64_t elems = 1ll << lg, n = 2 * elems;   // complex64 elements, fp32 components
        float* x;
        CK(hipMalloc(&x, (size_t)n * 4));
        fill_kernel<<<4096, 256, 0, stream>>>(x, n);
        const int64_t blocks = ctg::range_blocks(n);
        void* part;
        CK(hipMalloc(&part, (size_t)ctg::range_partial_bytes(blocks)));
        int64_t* row;
        double* sumsq;
        float* mx;
        CK(hipMalloc(&row, CTG_RANGE_WORDS * 8));
        CK(hipMalloc(&sumsq, 8));
        CK(hipMalloc(&mx, sizeof(float) * ctg::kMaxSub));
        std::vector<float> tr, tm;
        for (int r = 0; r < reps + 2; ++r) {
            CK(hipMemsetAsync(mx, 0, sizeof(float) * ctg::kMaxSub, stream));
            CK(hipEventRecord(ev[0], stream));
            CK(ctg::launch_range_hist(x, n, part, blocks, row, sumsq, stream));
            CK(hipEventRecord(ev[1], stream));
            CK(ctg::launch_maxabs_f32(x, nullptr, 0, 0, 0, elems, mx, stream));
            CK(hipEventRecord(ev[2], stream));
            CK(hipStreamSynchronize(stream));
            float a, b;
            CK(hipEventElapsedTime(&a, ev[0], ev[1]));
            CK(hipEventElapsedTime(&b, ev[1], ev[2]));
            if (r >= 2) {   // (the first two: warm-up)
                tr.push_back(a);
                tm.push_back(b);
            }
        }
        int64_t hrow[CTG_RANGE_WORDS];
        double hs;
        float hm;
        CK(hipMemcpy(hrow, row, sizeof(hrow), hipMemcpyDeviceToHost));
        CK(hipMemcpy(&hs, sumsq, 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(&hm, mx, 4, hipMemcpyDeviceToHost));
        int bins = 0;
        for (int b = 0; b < 256; ++b) bins += hrow[4 + b] != 0;
        const double bytes = (double)n * 4;
        const float mr = median(tr), mm = median(tm);
        printf("{\"what\": \"pass_timing\", \"log2_elems\": %d, \"bytes\": %.0f, \"range_pass_ms\": %.4f, \"range_pass_min_ms\": %.4f, "
               "\"maxabs_pass_ms\": %.4f, \"maxabs_pass_min_ms\": %.4f, \"range_over_maxabs\": %.3f, \"range_bytes_per_s\": %.4g, "
               "\"maxabs_bytes_per_s\": %.4g, \"reps\": %d, \"bins_filled\": %d, \"components\": %lld, \"sumsq\": %.6g, \"maxabs\": %.6g}\n",
               lg, bytes, mr, *std::min_element(tr.begin(), tr.end()), mm, *std::min_element(tm.begin(), tm.end()), mr / mm,
               bytes / (mr * 1e-3), bytes / (mm * 1e-3), reps, bins, (long long)hrow[1], hs, hm);
        fflush(stdout);
        CK(hipFree(x)); CK(hipFree(part)); CK(hipFree(row)); CK(hipFree(sumsq)); CK(hipFree(mx));
    }
    return 0;
}
