// ctg_stem.hip -- the fused stem kernels with fp32 products and in the bf16 x 3 arithmetic (stem2_kernel): this
// object's entry points.  The kernels, the shape rules and the launch logic are ctg_stem_impl.h; the fp16 x 2
// arithmetic of the same kernels (stem2h_kernel) is the object of ctg_stem_h2.hip.
#include "ctg_stem_impl.h"

namespace ctg {
#ifdef CTG_STEM_DEV_ONE
#ifdef CTG_STEM_DEV_P16   // (... its form with paired stores)
template __global__ void stem2_kernel_p16<CTG_STEM_DEV_ONE>(StemArgs);
#else
template __global__ void stem2_kernel<CTG_STEM_DEV_ONE>(StemArgs);
#endif
#else
int stem2_last_paired() { return stem_last_paired; }
bool stem2_supported(const StemArgs& p) { return stem2_supported_shape(p); }
bool stem3_supported(const StemArgs& p) { return stem3_supported_shape(p); }
bool stem2_uses_bf3(const StemArgs& p) { return stem_uses_16bit(p); }
void stem2_kernel_name(const StemArgs& p, char* buf, size_t n) { stem_kernel_name<Bf16x3>(p, buf, n); }
hipError_t launch_stem2(const StemArgs& p, hipStream_t stream) { return launch_stem<Bf16x3>(p, stream); }
#endif
}  // namespace ctg

#ifndef CTG_STEM_DEV_ONE
// (include/ctg_hip.h) is there a three-step tile kernel for this shape?  A pure function of the shape.
extern "C" int ctg_stem_triple_instantiated(int p1, int pm, int p2, int rt1, int cs1, int nch, int itm, int it2, int vec) {
    return ctg::stem3_instantiated(p1 != 0, pm != 0, p2 != 0, rt1, cs1, nch, itm, it2, vec != 0) ? 1 : 0;
}
#endif
// (experiment builds only; not in include/ctg_hip.h)
#ifdef CTG_STEM_TIMELINE
extern "C" int ctg_debug_stem_timeline(unsigned long long* out, int reset) { return ctg::stem_debug_timeline<ctg::Bf16x3>(out, reset); }
#endif
#ifdef CTG_STEM_BOUNDS
extern "C" int ctg_debug_stem_oob(unsigned long long out[2], int reset) { return ctg::stem_debug_oob<ctg::Bf16x3>(out, reset); }
#endif
