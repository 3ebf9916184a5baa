// The saturation report of the f16 hi / lo split: a device counter for the activations, a host counter for the weights, and
// the library's entry points that read them.  Included by conv_igemm_f32.hip ONLY: the device symbol does not cross
// translation units (conv_taps_f16s.hip gets the counter's address through ConvParams::f16s_clamp_ctr).
#pragma once
// (included inside namespace dfvo)

#include "conv_f16_split.h"

// |x| > 65504 does not fit the hi plane.  It is neither clamped (a silently wrong product) nor ignored: the conversion
// yields +-inf, which propagates as inf / NaN into the layer's output, and every kernel that splits activations keeps the
// running max |x| of what it split (one v_max3_f32 per two elements -- cheaper than the clamp it replaces) and bumps
// g_f16s_clamped once per thread that saw such a value; dfvo_f16s_overflow_count() reads it (the -m gpu tests assert
// zero after every f16x3 test).
__device__ unsigned int g_f16s_clamped = 0;
__device__ __forceinline__ void f16s_report_clamp(float amax) {
    if (amax > F16S_MAX) atomicAdd(&g_f16s_clamped, 1u);
}
// the counter's device address, for the f16x3 kernels that live in other translation units (device symbols do not cross TUs)
static unsigned* f16s_clamp_counter() {
    static unsigned* ptr = nullptr;
    if (!ptr && hipGetSymbolAddress((void**)&ptr, HIP_SYMBOL(g_f16s_clamped)) != hipSuccess) ptr = nullptr;
    return ptr;
}

static unsigned long long g_f16s_clamped_host = 0;  // weights beyond f16's range at pack time (same report as the device counter)

unsigned* conv_f16s_overflow_counter() { return f16s_clamp_counter(); }

// number of threads (activations) + weights (pack time) that hit the +-65504 saturation of the hi plane since the last reset
int conv_f16s_overflow_count(unsigned long long* n, int reset) {
    unsigned int dev = 0;
    DFVO_HIP_CHECK(hipMemcpyFromSymbol(&dev, HIP_SYMBOL(g_f16s_clamped), sizeof(dev)));
    if (n) *n = (unsigned long long)dev + g_f16s_clamped_host;
    if (reset) {
        const unsigned int zero = 0;
        DFVO_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_f16s_clamped), &zero, sizeof(zero)));
        g_f16s_clamped_host = 0;
    }
    return DFVO_OK;
}
