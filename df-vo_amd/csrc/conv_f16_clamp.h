// The device side of the saturation report of the f16 hi / lo split: the counter of activations beyond f16's range.
// Only conv_f16.hip includes this header.  It defines a device variable, the build has no relocatable device code and a
// device symbol does not cross translation units: every kernel that names g_f16s_clamped sits in the unit that defines it,
// and a second includer would count into a copy of its own that nobody reads.  (conv_taps_f16s.hip, a unit of its own, gets
// the counter's address through ConvParams::f16s_clamp_ctr.)  The weights' share of the report is counted on the host, in
// conv_pack.hip; conv_f16s_overflow_count (conv_f16.hip) adds the two.
#pragma once
#include "conv_f16_split.h"

namespace dfvo {

// |x| > 65504 does not fit the hi plane.  It is neither clamped (a silently wrong product) nor ignored: the conversion
// yields +-inf, which propagates as inf / NaN into the layer's output, and every kernel that splits activations keeps the
// running max |x| of what it split (one v_max3_f32 per two elements -- cheaper than the clamp it replaces) and bumps
// g_f16s_clamped once per thread that saw such a value; dfvo_f16s_overflow_count() reads it (the -m gpu tests assert
// zero after every f16x3 test).
__device__ unsigned int g_f16s_clamped = 0;
__device__ __forceinline__ void f16s_report_clamp(float amax) {
    if (amax > F16S_MAX) atomicAdd(&g_f16s_clamped, 1u);
}
// the counter's device address, for the f16x3 kernels that live in other translation units
static unsigned* f16s_clamp_counter() {
    static unsigned* ptr = nullptr;
    if (!ptr && hipGetSymbolAddress((void**)&ptr, HIP_SYMBOL(g_f16s_clamped)) != hipSuccess) ptr = nullptr;
    return ptr;
}

}  // namespace dfvo
