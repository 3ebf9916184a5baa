// Winograd F(2x2,3x3) weights for conv_wino_f32_kernel (conv_wino_f32.hip), packed on the host.  Host-only and free of HIP:
// a plain C++ compiler builds it (tests/test_wino_cpu.py does, under the address and undefined-behaviour sanitizers).
// conv_pack.hip wraps the packer for the library; conv_wino_f32.hip takes the layout's sizes from here.
#pragma once
#include <cstddef>
#include <cstring>

// U = G g G^T of one 3x3 filter, G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], in float64
static inline void wino_f32_filter_transform(const double g[9], double U[16]) {
    double t[4][3];  // G g
    for (int j = 0; j < 3; ++j) {
        t[0][j] = g[j];
        t[1][j] = 0.5 * ((g[j] + g[3 + j]) + g[6 + j]);
        t[2][j] = 0.5 * ((g[j] - g[3 + j]) + g[6 + j]);
        t[3][j] = g[6 + j];
    }
    for (int i = 0; i < 4; ++i) {  // (G g) G^T
        U[i * 4 + 0] = t[i][0];
        U[i * 4 + 1] = 0.5 * ((t[i][0] + t[i][1]) + t[i][2]);
        U[i * 4 + 2] = 0.5 * ((t[i][0] - t[i][1]) + t[i][2]);
        U[i * 4 + 3] = t[i][2];
    }
}

constexpr int WINO_F32_KC = 8;  // channels per K chunk of the kernel: each source is padded to a multiple of it
static inline int wino_f32_cout_pad(int cout) { return (cout + 31) / 32 * 32; }
static inline int wino_f32_chunks(int c) { return (c + WINO_F32_KC - 1) / WINO_F32_KC; }
static inline size_t conv_wino_f32_floats(int cout, int c0, int c1) {
    return (size_t)(wino_f32_chunks(c0) + wino_f32_chunks(c1)) * 16 * WINO_F32_KC * wino_f32_cout_pad(cout);
}

// OIHW 3x3 weights (cin = c0 + c1) -> [chunk][pos 16][h 2][cout_pad][4]: channel h * 4 + q of the chunk, the chunks of source 0
// first.  The BatchNorm scale is folded in fp32 first (as conv_pack_weights folds it), U is formed in float64 from that
// value and rounded to fp32 once.  Rows of the cout padding and of the channel padding of either source are zero.
static inline void conv_pack_wino_f32(const float* w, int cout, int c0, int c1, const float* fold_scale, float* out) {
    const int nch0 = wino_f32_chunks(c0), nch = nch0 + wino_f32_chunks(c1), cp = wino_f32_cout_pad(cout), cin = c0 + c1;
    memset(out, 0, conv_wino_f32_floats(cout, c0, c1) * sizeof(float));
    for (int c = 0; c < nch; ++c)
        for (int k = 0; k < WINO_F32_KC; ++k) {
            const bool s1 = c >= nch0;
            const int ch = (s1 ? c - nch0 : c) * WINO_F32_KC + k;
            if (ch >= (s1 ? c1 : c0)) continue;
            const int ci = s1 ? c0 + ch : ch;
            for (int co = 0; co < cout; ++co) {
                double g[9], U[16];
                for (int tap = 0; tap < 9; ++tap) {
                    float v = w[((size_t)co * cin + ci) * 9 + tap];
                    if (fold_scale) v *= fold_scale[co];
                    g[tap] = (double)v;
                }
                wino_f32_filter_transform(g, U);
                for (int pos = 0; pos < 16; ++pos)
                    out[((((size_t)c * 16 + pos) * 2 + (k >> 2)) * cp + co) * 4 + (k & 3)] = (float)U[pos];
            }
        }
}
