// The f16 kernel families (DFVO_CONV_PRECISION=f16x3 / f16) as one translation unit: the two LDS-window skeletons
// (conv_win_f16s.h, conv_win_f16s2.h) and the register-ring kernel (conv_gemm_f16s.h), kernels and launchers each in their
// header, with the device counter of their saturation report (conv_f16_clamp.h: why they share a unit).  Here: what the
// dispatcher calls -- which layers the families take, the ring kernel's shape choice -- and the report's entry points.
#include "conv.h"

#include <cstdlib>
#include <vector>

#include "conv_win_f16s.h"
#include "conv_gemm_f16s.h"
#include "conv_win_f16s2.h"
#include "conv_f16_clamp.h"

namespace dfvo {

unsigned* conv_f16s_overflow_counter() { return f16s_clamp_counter(); }

// number of threads (activations) + weights (pack time) that hit the +-65504 saturation of the hi plane since the last reset
int conv_f16s_overflow_count(unsigned long long* n, int reset) {
    unsigned int dev = 0;
    DFVO_HIP_CHECK(hipMemcpyFromSymbol(&dev, HIP_SYMBOL(g_f16s_clamped), sizeof(dev)));
    if (n) *n = (unsigned long long)dev + conv_f16s_weights_clamped(false);
    if (reset) {
        const unsigned int zero = 0;
        DFVO_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_f16s_clamped), &zero, sizeof(zero)));
        conv_f16s_weights_clamped(true);
    }
    return DFVO_OK;
}

bool conv_f16s_ok(const ConvParams& p) {
    if (p.kh != 3 || p.kw != 3 || p.stride != 1 || p.pad_h != 1 || p.pad_w != 1) return false;
    if (p.wf16_cout_pad % 32 != 0 || p.Wo < 24 || p.Ho < 4) return false;
    // small maps stay on the fp32 split-K kernels: with fewer than ~200 of the smallest (32 couts x 4 x 32 px) tiles the
    // grid cannot fill the chip and the un-split K loop makes the launch longer than the fp32 one (measured: pyramid
    // levels 5 / 6 and the depth net's inner layers 2-4x slower, level 4 1.5-2x faster)
    const long long e = (long long)p.N * ((p.Ho + 3) / 4) * ((p.Wo + 31) / 32) * (p.wf16_cout_pad / 32);
    // (round 4: raising the bound to 450 / 900 tiles sends pyramid level 4 / 3 to the generic kernel instead -- the window
    // family's average TFLOP/s rises, 0.265 -> 0.30 / 0.31 of its roofline, and the pair rate FALLS, 287 -> 280 / 272: kept at 200)
    return e >= 200;
}

// the one-wave-per-SIMD skeleton where the grid is large enough, else the first skeleton; both file under profile row 19
int launch_f16_window(const ConvParams& p, hipStream_t stream) {
    const int rc2 = launch_f16s2(p, stream, 19);
    return rc2 != F16S2_NOT_APPLICABLE ? rc2 : launch_f16s(p, stream, 19);  // errors (negative) propagate
}

bool conv_f16g_ok(const ConvParams& p) { return p.wf16g && p.f16g_tab && p.kh <= 31 && p.kw <= 31; }

// Shape choice: ring_shape (conv_dispatch.hip), shared with the fp32 twin.  Large maps (thousands of pixel blocks) run
// KSP = 1 with four pixel blocks per workgroup.
int launch_f16g(const ConvParams& p, hipStream_t stream) {
    const auto [tc2, ksp] = ring_shape((long long)p.N * p.Ho * p.Wo, p.wf16g_cout_pad / 32, p.f16g_steps);
    // Measured and dropped (records under profiles/): an eight-stage ring with twice the waves (r3: K-sliced layers 1.24 vs
    // 1.10 ms per pair), K divided over workgroups as well (r3af_nz_ab.txt: launches 7 % shorter one at a time, pair rate
    // -1.3 %), one cout block per wave on the streaming shapes (r3j_stream_tc1_ab.txt: no gain).
    const int cfg = ksp == 1 ? 20 : 21;  // profile rows: 20 streaming (KSP = 1), 21 K-sliced small maps
    // multi-tap layers among the streaming shapes: the tap-window kernel of conv_taps_f16s.hip (only where this kernel would
    // not slice K: the two then sum in the same order).  DFVO_TAPS=0 (test hook, tests/test_nets_gpu.py): the <4, 1, TC>
    // shape of the ring kernel instead -- the form the tap-window kernel is compared with bit for bit
    static const bool taps_on = env_flag("DFVO_TAPS", true);
    if (taps_on && ksp == 1 && conv_taps_f16s_ok(p)) {
        ConvParams pt = p;
        pt.f16s_clamp_ctr = f16s_clamp_counter();
        return launch_taps_f16s(pt, stream);
    }
    // ragged cout on a streaming shape: the store-only epilogue (profiles/r4j_rag_ab.txt: the 7 x 1 / 1 x 7 distance layers
    // 80 -> 68 / 104 -> 98 us, +0.8 % pairs/s, bit-identical)
    const bool rag = ksp == 1 && (p.cout % (tc2 ? 64 : 32)) != 0 && !p.res && ((p.dst_cs | p.dst_co) & 3) == 0 &&
                     p.cout_pad >= 4 && (p.act == ACT_NONE || p.act == ACT_LEAKY || p.act == ACT_RELU);
    if (rag) return tc2 ? launch_f16g_cfg<4, 1, 2, 3, true>(p, stream, cfg) : launch_f16g_cfg<4, 1, 1, 3, true>(p, stream, cfg);
    if (tc2) {
        switch (ksp) {
            case 1: return launch_f16g_cfg<4, 1, 2>(p, stream, cfg);
            case 2: return launch_f16g_cfg<2, 2, 2>(p, stream, cfg);
            case 4: return launch_f16g_cfg<1, 4, 2>(p, stream, cfg);
            default: return launch_f16g_cfg<1, 8, 2>(p, stream, cfg);
        }
    }
    switch (ksp) {
        case 1: return launch_f16g_cfg<4, 1, 1>(p, stream, cfg);
        case 2: return launch_f16g_cfg<2, 2, 1>(p, stream, cfg);
        case 4: return launch_f16g_cfg<1, 4, 1>(p, stream, cfg);
        case 8: return launch_f16g_cfg<1, 8, 1>(p, stream, cfg);
        default: return launch_f16g_cfg<1, 16, 1>(p, stream, cfg);
    }
}

}  // namespace dfvo
