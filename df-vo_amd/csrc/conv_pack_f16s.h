// Weights as f16 hi / lo planes, packed on the host for the f16 kernel families (included by conv_igemm_f32.hip).
#pragma once
// (included inside namespace dfvo)

#include "conv_f16_clamp.h"

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
