// ctg_stem_h2.hip -- the fused stem kernels in the fp16 x 2 arithmetic (stem2h_kernel, round 6): this object's entry
// points.  It holds the 16-bit instantiations only -- the pairs of CTG_STEM_GEO in the forms stem2_bf3_form<Fp16x2> can
// answer and the static single steps of CTG_STEM_ONE; a step they do not cover is ctg_stem.hip's (launch_stem2).
#include "ctg_stem_impl.h"

namespace ctg {
#ifdef CTG_STEM_DEV_ONE
#ifdef CTG_STEM_DEV_P16   // (... its form with paired stores)
template __global__ void stem2h_kernel_p16<CTG_STEM_DEV_ONE>(StemArgs);
#else
template __global__ void stem2h_kernel<CTG_STEM_DEV_ONE>(StemArgs);
#endif
#else
int stem2h_last_paired() { return stem_last_paired; }
bool stem2h_supported(const StemArgs& p) { return stem2_supported_shape(p); }
bool stem2h_uses_h2(const StemArgs& p) { return stem_uses_16bit(p); }
void stem2h_kernel_name(const StemArgs& p, char* buf, size_t n) { stem_kernel_name<Fp16x2>(p, buf, n); }
hipError_t launch_stem2h(const StemArgs& p, hipStream_t stream) { return launch_stem<Fp16x2>(p, stream); }
#endif
}  // namespace ctg

// (experiment builds only; not in include/ctg_hip.h)
#ifdef CTG_STEM_TIMELINE
extern "C" int ctg_debug_stem_timeline_h2(unsigned long long* out, int reset) { return ctg::stem_debug_timeline<ctg::Fp16x2>(out, reset); }
#endif
#ifdef CTG_STEM_BOUNDS
extern "C" int ctg_debug_stem_oob_h2(unsigned long long out[2], int reset) { return ctg::stem_debug_oob<ctg::Fp16x2>(out, reset); }
#endif
