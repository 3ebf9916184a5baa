// The convolution dispatcher: the tile rules and launch_conv().  Host only -- it holds no kernel and reaches the kernel
// families through the entry points they export (conv.h).
#include "conv.h"

namespace dfvo {

int conv_pick_bn(int cout, long long) {
    if (cout <= 16) return 16;
    if (cout <= 32) return 32;
    if (cout % 128 == 0) return 128;
    if (cout % 64 == 0) return 64;
    if (cout % 32 == 0) return 32;  // 96 -> 3 x 32
    return 64;                      // 49 -> 64
}

// the direct kernel serves the square, stride-1, "same"-padded heads with one or two output channels
static bool conv_use_head(const ConvParams& p) {
    if (p.cout > 2 || !p.wh) return false;
    if (p.kh != p.kw || p.stride != 1 || p.pad_h != p.kh / 2 || p.pad_w != p.kw / 2) return false;
    if (p.kh != 3 && p.kh != 5 && p.kh != 7) return false;
    return (long long)p.N * p.Ho * p.Wo >= 1024;
}

// the LDS-window kernel serves 3x3 / stride-1 layers on maps large enough to fill the chip with TH x 16 tiles
static bool conv_use_window(const ConvParams& p, int bn) {
    if (p.kh != p.kw || p.stride != 1 || p.pad_h != p.kh / 2 || p.pad_w != p.kw / 2) return false;
    const long long M = (long long)p.N * p.Ho * p.Wo;
    if (p.kh == 3) return bn >= 32 && M >= 30000;
    // 5x5 / 7x7 flow heads (32 -> 2 channels): the whole tap loop runs out of one window
    return (p.kh == 5 || p.kh == 7) && bn == 16 && (p.G0 + p.G1) >= 4 && M >= 8000;
}

// the profile row (12-15) of the window kernel's tile class for a 3x3 layer: launch_conv's window branch and the Winograd
// launcher (which files its launches under the row of the class they replace) both go by it.  Under
// dfvo_set_fp32_winograd(2), the unit-test mode, layers that never were window layers (bn 16, small maps) land on a row too.
static int conv_window_cfg(const ConvParams& p, int bn) {
    const long long tiles8 = (long long)p.N * ((p.Ho + 7) / 8) * ((p.Wo + 15) / 16) * (p.cout_pad / bn);
    // 128-wide layers on the largest maps run as two 64-wide column blocks: 2x the workgroups at 4 (instead of 3) per CU
    // shortens the under-filled last round of the grid (+5 % measured at 2 x 192 x 624)
    if (bn == 128) return tiles8 >= 1200 ? 13 : (tiles8 >= 400 ? 12 : 15);
    return bn == 64 ? 13 : 14;
}
// fp32 Winograd under dfvo_set_fp32_winograd(1), EXPERIMENTAL: the window kernel's own size rule without the 32-wide class,
// whose Winograd workgroup is two waves (half of a CU's SIMDs).  A class stays here only where tools/wino_bench.py shows
// Winograd at <= 0.90 x the direct kernel's time (DESIGN.md section 5d holds the table this rule goes by)
constexpr long long WINO_MIN_PIXELS = 30000;  // conv_use_window's
bool conv_wino_rule_may_accept(int cout, long long max_pixels) {
    return conv_pick_bn(cout, max_pixels) >= 64 && (max_pixels <= 0 || max_pixels >= WINO_MIN_PIXELS);
}
static bool conv_wino_size_rule(const ConvParams& p, int bn) {
    return conv_use_window(p, bn) && conv_wino_rule_may_accept(p.cout, (long long)p.N * p.Ho * p.Wo);
}

// Tile choice: the widest N tile the layer's cout allows (conv_pick_bn); the M tile from a sweep on MI355X
// (tools/sweep_conv.sh): 64-row tiles win or tie on every layer with BN <= 64 and on BN = 128 below ~1200
// workgroups (more resident workgroups hide the global -> LDS staging latency; the per-tap gather is served by
// L2 either way); 128 x 128 keeps the largest maps.  Small grids additionally split K (conv_splitk_slices).
static int conv_pick_bm(const ConvParams& p, int bn) {
    const long long M = (long long)p.N * p.Ho * p.Wo;
    const long long ntiles_n = p.cout_pad / bn;
    auto blocks = [&](int bm) { return ((M + bm - 1) / bm) * ntiles_n; };
    if (bn == 128) {
        int bm = blocks(128) >= 1200 ? 128 : 64;
        if (M <= 4096) bm = 32;
        return bm;
    }
    return M >= 400000 ? 128 : 64;
}

// exact-fp32 mode: which layers leave conv_igemm_f32_kernel for the register-ring kernel (conv_gemm_f32g.hip).  Not the
// 3x3 / stride-1 layers the LDS-window kernel takes, not the one- / two-channel heads.
// Measured (profiles/r4e_fp32_f32g_ab.txt): the small maps only 156.5 -> 160 pairs/s; every non-window layer 158 (the
// streaming layers are no faster than on conv_igemm_f32_kernel).
static bool conv_f32g_takes(const ConvParams& p, int bn) {
    if (conv_use_head(p) || conv_use_window(p, bn)) return false;
    // pyramid levels 5 / 6 (2 x 11 x 38 .. 2 x 44 x 152) and the depth net's 6 x 20 .. 48 x 160 maps
    return (long long)p.N * p.Ho * p.Wo <= 8192;
}

// Shape of the ring kernels, f16 and fp32 alike.  TC = 2 (a pixel fragment, whose split costs the VALU work, feeds two cout
// blocks) whenever the layer has an even number of 32-cout blocks.  The K split fills the chip: ~2 waves per SIMD in total,
// at least 4 steps per wave.
RingShape ring_shape(long long M, int nblk, int steps) {
    const long long mblocks = (M + 31) / 32;
    const long long target = 2048;  // waves on the chip: ~2 per SIMD
    // two cout blocks per wave only while that still leaves enough (pixel block, cout pair) tiles to fill the chip with at
    // most eight K slices; tiny maps with many couts (the depth net's 6 x 20 / 12 x 40 layers: the launch is one pass over
    // megabytes of weights) take one block per wave and up to 16 slices -- more waves, more loads in flight
    bool tc2 = (nblk % 2) == 0;
    if (tc2 && mblocks * (nblk / 2) * 8 * 2 < target && steps >= 64) tc2 = false;
    const long long tiles = mblocks * (tc2 ? nblk / 2 : nblk);
    int ksp = 1;
    // (16 slices only with one cout block per wave: a 1024-thread workgroup leaves 128 registers per lane)
    while (ksp < (tc2 ? 8 : 16) && tiles * ksp * 2 <= target && steps >= 4 * ksp * 2) ksp *= 2;
    return {tc2, ksp};
}

int launch_conv(const ConvParams& p, hipStream_t stream, bool wino_all) {
    const long long M = (long long)p.N * p.Ho * p.Wo;
    const int bn = conv_pick_bn(p.cout, M);
    DFVO_ARG_CHECK(p.cout_pad % bn == 0, "launch_conv: cout_pad not a multiple of the N tile");
    DFVO_ARG_CHECK((p.cs0 % 4) == 0 && (p.co0 % 4) == 0, "launch_conv: src0 stride/offset must be multiples of 4");
    DFVO_ARG_CHECK(p.G1 == 0 || ((p.cs1 % 4) == 0 && (p.co1 % 4) == 0), "launch_conv: src1 stride/offset");
    if (conv_use_head(p)) return launch_head_f32(p, stream);
    if (p.wf16 && conv_f16s_ok(p)) return launch_f16_window(p, stream);  // f16x3: the 3x3 / stride-1 layers whose map fills the chip
    if (conv_f16g_ok(p)) return launch_f16g(p, stream);  // f16x3: everything else (small maps, 1x1, k x 1, stride 2, 7x7)
    // fp32 Winograd (opt-in, decided when the layer was packed): ahead of every direct fp32 kernel.  Its launches are filed
    // under the window row of the tile class they replace, with the direct convolution's FLOP count
    if (conv_wino_applicable(p) && (wino_all || conv_wino_size_rule(p, bn))) return launch_wino(p, stream, conv_window_cfg(p, bn));
    if (conv_f32g_ok(p) && conv_f32g_takes(p, bn)) return launch_f32g(p, stream);  // exact fp32: the same skeleton on fp32 MFMAs
    if (conv_use_window(p, bn)) return launch_win_f32(p, stream, p.kh == 7 ? 16 : (p.kh == 5 ? 17 : conv_window_cfg(p, bn)));
    return launch_igemm_f32(p, stream, conv_pick_bm(p, bn), bn);
}

}  // namespace dfvo
