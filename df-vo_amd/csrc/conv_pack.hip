// The host packers of the convolution kernels: OIHW weights (cin = c0 + c1 channels of up to two sources) into each
// family's layout, the BatchNorm scale folded in.  Host only and free of device code: a plain C++ compiler builds this file
// (tests/host_harness/conv_pack_check.cpp compares its output with the loops it replaced, byte for byte).
#include "conv.h"

#include <algorithm>
#include <cstring>

#include "conv_pack_wino_f32.h"

namespace dfvo {

// The walk in k-group order that the fp32 implicit GEMM and both ring kernels share: a k-group g = tap (G0 + G1) + channel
// group is 4 consecutive channels (q) of one tap of one source, each source rounded up to whole groups on its own.
// store(g, q, cout index, folded weight) for every weight that exists; the padding is the caller's zero fill.
template <class Store>
static void walk_kgroups(const float* w, int cout, int c0, int c1, int taps, const float* fold_scale, Store store) {
    const int G0 = cdiv(c0, 4), G = G0 + cdiv(c1, 4), cin = c0 + c1;
    for (int tap = 0; tap < taps; ++tap)
        for (int cg = 0; cg < G; ++cg)
            for (int q = 0; q < 4; ++q) {
                int ci;
                if (cg < G0) {
                    ci = cg * 4 + q;
                    if (ci >= c0) continue;
                } else {
                    ci = (cg - G0) * 4 + q;
                    if (ci >= c1) continue;
                    ci += c0;
                }
                for (int co = 0; co < cout; ++co) {
                    float v = w[((size_t)co * cin + ci) * taps + tap];
                    if (fold_scale) v *= fold_scale[co];
                    store(tap * G + cg, q, co, v);
                }
            }
}

// ---- fp32: conv_igemm_f32_kernel / conv_win_f32_kernel, [k-group][cout_pad][4] ------------------------------------------
void conv_pack_weights(const float* w, const float* bias, int cout, int c0, int c1, int kh, int kw, int cout_pad,
                       const float* fold_scale, const float* fold_shift, float* out_w, float* out_b) {
    std::fill(out_w, out_w + (size_t)conv_ksteps(kh, kw, c0, c1) * 4 * cout_pad * 4, 0.f);
    walk_kgroups(w, cout, c0, c1, kh * kw, fold_scale,
                 [&](int g, int q, int co, float v) { out_w[((size_t)g * cout_pad + co) * 4 + q] = v; });
    for (int o = 0; o < cout_pad; ++o) {
        float b = 0.f;
        if (o < cout) {
            b = bias ? bias[o] : 0.f;
            if (fold_scale) b *= fold_scale[o];
            if (fold_shift) b += fold_shift[o];
        }
        out_b[o] = b;
    }
}

// ---- fp32: conv_head_f32_kernel ------------------------------------------------------------------------------------------
size_t conv_head_weight_floats(int cout, int c0, int c1, int k) {
    return (size_t)(cdiv(c0, 8) + cdiv(c1, 8)) * k * 2 * k * cout * 4;
}
void conv_pack_head_weights(const float* w, int cout, int c0, int c1, int k, const float* fold_scale, float* out) {
    const int nchunk0 = cdiv(c0, 8), nchunks = nchunk0 + cdiv(c1, 8), cin = c0 + c1;
    std::fill(out, out + conv_head_weight_floats(cout, c0, c1, k), 0.f);
    for (int c = 0; c < nchunks; ++c)
        for (int kx = 0; kx < k; ++kx)
            for (int cg = 0; cg < 2; ++cg)
                for (int ky = 0; ky < k; ++ky)
                    for (int o = 0; o < cout; ++o)
                        for (int q = 0; q < 4; ++q) {
                            const int cl = (c < nchunk0 ? c : c - nchunk0) * 8 + cg * 4 + q;  // channel inside its source
                            if (cl >= (c < nchunk0 ? c0 : c1)) continue;
                            const int ci = c < nchunk0 ? cl : c0 + cl;
                            float v = w[(((size_t)o * cin + ci) * k + ky) * k + kx];
                            if (fold_scale) v *= fold_scale[o];
                            out[(((((size_t)c * k + kx) * 2 + cg) * k + ky) * cout + o) * 4 + q] = v;
                        }
}

// ---- f16 hi / lo planes --------------------------------------------------------------------------------------------------
static unsigned long long g_f16s_clamped_host = 0;  // weights beyond f16's range at pack time (same report as the device counter)
unsigned long long conv_f16s_weights_clamped(bool reset) {
    const unsigned long long n = g_f16s_clamped_host;
    if (reset) g_f16s_clamped_host = 0;
    return n;
}

// f32 -> (hi, lo) exactly as split_f16_planes does on the device
static inline void f16s_split_host(float x, unsigned short* hi, unsigned short* lo) {
    float v = x < -F16S_MAX ? -F16S_MAX : (x > F16S_MAX ? F16S_MAX : x);
    if (v != x && x == x) ++g_f16s_clamped_host;
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)((v - (float)h) * F16S_LO_SCALE);
    memcpy(hi, &h, 2);
    memcpy(lo, &l, 2);
}

// the 3x3 window kernels (conv_win_f16s.h, conv_win_f16s2.h)
size_t conv_pack_weights_f16s(const float* w, int cout, int c0, int c1, const float* fold_scale, unsigned short* out) {
    const int nch0 = (c0 + 15) / 16, nch1 = (c1 + 15) / 16, nch = nch0 + nch1;
    const int cp = round_up(cout, 32);
    const size_t total = (size_t)9 * nch * cp * 32;
    if (!out) return total;
    memset(out, 0, total * sizeof(unsigned short));
    const int cin = c0 + c1;
    for (int tap = 0; tap < 9; ++tap)
        for (int c = 0; c < nch; ++c)
            for (int co = 0; co < cout; ++co)
                for (int k = 0; k < 16; ++k) {
                    const bool s1 = c >= nch0;
                    const int ch = s1 ? (c - nch0) * 16 + k : c * 16 + k;
                    if (ch >= (s1 ? c1 : c0)) continue;
                    const int ci = s1 ? c0 + ch : ch;
                    float v = w[((size_t)co * cin + ci) * 9 + tap];
                    if (fold_scale) v *= fold_scale[co];
                    // [tap][chunk][cout / 32][plane][k / 8][cout % 32][k % 8]
                    unsigned short* o = out + (((size_t)tap * nch + c) * cp + (co & ~31)) * 32 + ((k >> 3) * 32 + (co & 31)) * 8 + (k & 7);
                    f16s_split_host(v, o, o + 512);
                }
    return total;
}

// ---- the ring kernels (conv_gemm_f16s.h, conv_gemm_f32g.hip, conv_taps_f16s.hip) ----------------------------------------
// Weights in k-group order: [step][cout_pad / 32][plane hi, lo -- f16 only][k-block (2)][32 couts][8 k], where the 16 k of a
// step are k-groups 4 step .. 4 step + 3, 4 channels each.  `unit` = elements per cout of a step: 32 with the two planes, 16
// without.  put(address of the element -- of its hi half --, folded weight).  Returns the number of elements (out may be null)
template <class T, class Put>
static size_t pack_ring(const float* w, int cout, int c0, int c1, int kh, int kw, const float* fold_scale, int unit, T* out, Put put) {
    const int cp = round_up(cout, 32);
    const size_t total = (size_t)conv_ksteps(kh, kw, c0, c1) * cp * unit;
    if (!out) return total;
    memset(out, 0, total * sizeof(T));
    walk_kgroups(w, cout, c0, c1, kh * kw, fold_scale, [&](int g, int q, int co, float v) {
        const int step = g >> 2, k = (g & 3) * 4 + q;
        put(out + ((size_t)step * cp + (co & ~31)) * unit + ((k >> 3) * 32 + (co & 31)) * 8 + (k & 7), v);
    });
    return total;
}
size_t conv_pack_weights_f16g(const float* w, int cout, int c0, int c1, int kh, int kw, const float* fold_scale,
                              unsigned short* out) {
    return pack_ring(w, cout, c0, c1, kh, kw, fold_scale, 32, out, [](unsigned short* o, float v) { f16s_split_host(v, o, o + 512); });
}
size_t conv_pack_weights_f32g(const float* w, int cout, int c0, int c1, int kh, int kw, const float* fold_scale, float* out) {
    return pack_ring(w, cout, c0, c1, kh, kw, fold_scale, 16, out, [](float* o, float v) { *o = v; });
}

// the k-group table of a layer: 4 entries per step, the padding of the last step invalid
void conv_build_f16g_table(int c0, int c1, int kh, int kw, std::vector<uint32_t>* tab) {
    const int G0 = cdiv(c0, 4), G1 = cdiv(c1, 4), G = G0 + G1, taps = kh * kw;
    const int steps = cdiv(taps * G, 4);
    tab->assign((size_t)steps * 4, f16g_entry(0, 0, 0, 0, 0));
    for (int tap = 0; tap < taps; ++tap)
        for (int cg = 0; cg < G; ++cg)
            (*tab)[(size_t)tap * G + cg] = f16g_entry(tap / kw, tap % kw, 1, cg < G0 ? 0 : 1, cg < G0 ? cg * 4 : (cg - G0) * 4);
}

// ---- fp32 Winograd (conv_pack_wino_f32.h) --------------------------------------------------------------------------------
size_t conv_wino_f32_weight_floats(int cout, int c0, int c1) { return conv_wino_f32_floats(cout, c0, c1); }
void conv_pack_weights_wino_f32(const float* w_oihw, int cout, int c0, int c1, const float* fold_scale, float* out) {
    conv_pack_wino_f32(w_oihw, cout, c0, c1, fold_scale, out);
}

}  // namespace dfvo
