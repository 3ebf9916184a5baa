// Stand-alone check of the ring kernels' host packers (df-vo_amd/csrc/conv_pack.hip): conv_pack_weights_f16g,
// conv_pack_weights_f32g and conv_build_f16g_table -- and conv_pack_weights, which shares their walk -- against the loops
// they had before the k-group walk became one function, kept here word for word (namespace before).  Every output is compared
// with memcmp over its whole length, the padding included, from buffers that start out as garbage; the count of weights
// beyond f16's range must agree too.  Linked with conv_pack.hip compiled as plain C++; no HIP library, no GPU.
// Built and run by tests/test_conv_pack_cpu.py: conv_pack_check ; exit status 0 = every shape holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../df-vo_amd/csrc/conv.h"

namespace before {
using dfvo::cdiv;
using dfvo::round_up;
constexpr float F16S_LO_SCALE = 2048.0f;
constexpr float F16S_MAX = 65504.0f;
static unsigned long long g_f16s_clamped_host = 0;

static inline void f16s_split_host(float x, unsigned short* hi, unsigned short* lo) {
    float v = x < -F16S_MAX ? -F16S_MAX : (x > F16S_MAX ? F16S_MAX : x);
    if (v != x && x == x) ++g_f16s_clamped_host;
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)((v - (float)h) * F16S_LO_SCALE);
    memcpy(hi, &h, 2);
    memcpy(lo, &l, 2);
}

static inline uint32_t f16g_entry(int ky, int kx, int valid, int src, int choff) {
    return (uint32_t)ky | ((uint32_t)kx << 5) | ((uint32_t)valid << 10) | ((uint32_t)src << 11) | ((uint32_t)choff << 16);
}

size_t conv_pack_weights_f16g(const float* w, int cout, int c0, int c1, int kh, int kw, const float* fold_scale,
                              unsigned short* out) {
    const int G0 = cdiv(c0, 4), G1 = cdiv(c1, 4), G = G0 + G1, taps = kh * kw;
    const int steps = cdiv(taps * G, 4);
    const int cp = round_up(cout, 32);
    const size_t total = (size_t)steps * cp * 32;
    if (!out) return total;
    memset(out, 0, total * sizeof(unsigned short));
    const int cin = c0 + c1;
    for (int tap = 0; tap < taps; ++tap)
        for (int cg = 0; cg < G; ++cg) {
            const int g = tap * G + cg, step = g >> 2, gl = g & 3;
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
                const int k = gl * 4 + q;
                for (int co = 0; co < cout; ++co) {
                    float v = w[((size_t)co * cin + ci) * taps + tap];
                    if (fold_scale) v *= fold_scale[co];
                    unsigned short* o = out + ((size_t)step * cp + (co & ~31)) * 32 + ((k >> 3) * 32 + (co & 31)) * 8 + (k & 7);
                    f16s_split_host(v, o, o + 512);
                }
            }
        }
    return total;
}

void conv_build_f16g_table(int c0, int c1, int kh, int kw, std::vector<uint32_t>* tab) {
    const int G0 = cdiv(c0, 4), G1 = cdiv(c1, 4), G = G0 + G1, taps = kh * kw;
    const int steps = cdiv(taps * G, 4);
    tab->assign((size_t)steps * 4, f16g_entry(0, 0, 0, 0, 0));
    for (int tap = 0; tap < taps; ++tap)
        for (int cg = 0; cg < G; ++cg)
            (*tab)[(size_t)tap * G + cg] = f16g_entry(tap / kw, tap % kw, 1, cg < G0 ? 0 : 1, cg < G0 ? cg * 4 : (cg - G0) * 4);
}

size_t conv_pack_weights_f32g(const float* w, int cout, int c0, int c1, int kh, int kw, const float* fold_scale, float* out) {
    const int G0 = cdiv(c0, 4), G1 = cdiv(c1, 4), G = G0 + G1, taps = kh * kw;
    const int steps = cdiv(taps * G, 4);
    const int cp = round_up(cout, 32);
    const size_t total = (size_t)steps * cp * 16;
    if (!out) return total;
    memset(out, 0, total * sizeof(float));
    const int cin = c0 + c1;
    for (int tap = 0; tap < taps; ++tap)
        for (int cg = 0; cg < G; ++cg) {
            const int g = tap * G + cg, step = g >> 2, gl = g & 3;
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
                const int k = gl * 4 + q;
                for (int co = 0; co < cout; ++co) {
                    float v = w[((size_t)co * cin + ci) * taps + tap];
                    if (fold_scale) v *= fold_scale[co];
                    out[((size_t)step * cp + (co & ~31)) * 16 + ((k >> 3) * 32 + (co & 31)) * 8 + (k & 7)] = v;
                }
            }
        }
    return total;
}

void conv_pack_weights(const float* w, const float* bias, int cout, int c0, int c1, int kh, int kw, int cout_pad,
                       const float* fold_scale, const float* fold_shift, float* out_w, float* out_b) {
    const int G0 = cdiv(c0, 4), G1 = cdiv(c1, 4), G = G0 + G1;
    const int taps = kh * kw;
    const int ksteps = cdiv(taps * G, 4);
    const int cin = c0 + c1;
    std::fill(out_w, out_w + (size_t)ksteps * 4 * cout_pad * 4, 0.f);
    for (int tap = 0; tap < taps; ++tap) {
        const int ky = tap / kw, kx = tap % kw;
        for (int cg = 0; cg < G; ++cg) {
            const int g = tap * G + cg;
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
                for (int o = 0; o < cout; ++o) {
                    float v = w[(((size_t)o * cin + ci) * kh + ky) * kw + kx];
                    if (fold_scale) v *= fold_scale[o];
                    out_w[((size_t)g * cout_pad + o) * 4 + q] = v;
                }
            }
        }
    }
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
}  // namespace before

static int g_failed = 0;
#define CHECK(cond)                                                                                           \
    do {                                                                                                      \
        if (!(cond)) {                                                                                        \
            fprintf(stderr, "line %d, shape %s: CHECK(%s) failed\n", __LINE__, g_shape, #cond);                \
            ++g_failed;                                                                                       \
        }                                                                                                     \
    } while (0)
static char g_shape[96];

static uint32_t g_rng = 12345u;
static float rnd() {  // [-2, 2)
    g_rng = g_rng * 1664525u + 1013904223u;
    return (float)(g_rng >> 8) / 4194304.0f - 2.0f;
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static void check_shape(int cout, int c0, int c1, int kh, int kw, bool fold) {
    snprintf(g_shape, sizeof(g_shape), "(%d, %d, %d, %d, %d)%s", cout, c0, c1, kh, kw, fold ? " fold_scale" : "");
    const size_t nw = (size_t)cout * (c0 + c1) * kh * kw;
    std::vector<float> w(nw), scale(cout), shift(cout), bias(cout);
    for (float& v : w) v = rnd();
    for (int o = 0; o < cout; ++o) scale[o] = 0.5f + 0.25f * rnd(), shift[o] = rnd(), bias[o] = rnd();
    // values beyond f16's range, a subnormal low plane, a NaN and an infinity: the split's clamp and its count
    const float odd[] = {1.0e6f, -7.0e4f, 65504.0f, 3.0e-8f, __builtin_nanf(""), -__builtin_inff()};
    for (size_t i = 0; i < sizeof(odd) / sizeof(odd[0]) && i * 7 + 3 < nw; ++i) w[i * 7 + 3] = odd[i];
    const float* fs = fold ? scale.data() : nullptr;

    // f16 hi / lo planes
    const size_t n16 = dfvo::conv_pack_weights_f16g(w.data(), cout, c0, c1, kh, kw, fs, nullptr);
    CHECK(n16 == before::conv_pack_weights_f16g(w.data(), cout, c0, c1, kh, kw, fs, nullptr));
    std::vector<unsigned short> h_new(n16, 0xCDCD), h_old(n16, 0xABAB);
    dfvo::conv_f16s_weights_clamped(true);
    before::g_f16s_clamped_host = 0;
    CHECK(dfvo::conv_pack_weights_f16g(w.data(), cout, c0, c1, kh, kw, fs, h_new.data()) == n16);
    CHECK(before::conv_pack_weights_f16g(w.data(), cout, c0, c1, kh, kw, fs, h_old.data()) == n16);
    CHECK(same(h_new, h_old));
    CHECK(dfvo::conv_f16s_weights_clamped(false) == before::g_f16s_clamped_host);
    CHECK(dfvo::conv_f16s_weights_clamped(true) == before::g_f16s_clamped_host && dfvo::conv_f16s_weights_clamped(false) == 0);

    // plain fp32
    const size_t n32 = dfvo::conv_pack_weights_f32g(w.data(), cout, c0, c1, kh, kw, fs, nullptr);
    CHECK(n32 == before::conv_pack_weights_f32g(w.data(), cout, c0, c1, kh, kw, fs, nullptr));
    std::vector<float> f_new(n32, -123.f), f_old(n32, 456.f);
    CHECK(dfvo::conv_pack_weights_f32g(w.data(), cout, c0, c1, kh, kw, fs, f_new.data()) == n32);
    CHECK(before::conv_pack_weights_f32g(w.data(), cout, c0, c1, kh, kw, fs, f_old.data()) == n32);
    CHECK(same(f_new, f_old));

    // the k-group table
    std::vector<uint32_t> t_new(3, 0xdeadbeefu), t_old;
    dfvo::conv_build_f16g_table(c0, c1, kh, kw, &t_new);
    before::conv_build_f16g_table(c0, c1, kh, kw, &t_old);
    CHECK(same(t_new, t_old) && t_new.size() == (size_t)dfvo::conv_ksteps(kh, kw, c0, c1) * 4);

    // the implicit-GEMM layout, which goes through the same walk (cout_pad a multiple of 16, wider than cout)
    const int cout_pad = dfvo::round_up(cout, 16) + 16;
    const size_t ng = (size_t)dfvo::conv_ksteps(kh, kw, c0, c1) * 4 * cout_pad * 4;
    std::vector<float> g_new(ng, -123.f), g_old(ng, 456.f), b_new(cout_pad, -1.f), b_old(cout_pad, -2.f);
    dfvo::conv_pack_weights(w.data(), bias.data(), cout, c0, c1, kh, kw, cout_pad, fs, fold ? shift.data() : nullptr, g_new.data(), b_new.data());
    before::conv_pack_weights(w.data(), bias.data(), cout, c0, c1, kh, kw, cout_pad, fs, fold ? shift.data() : nullptr, g_old.data(), b_old.data());
    CHECK(same(g_new, g_old) && same(b_new, b_old));
}

int main() {
    const int shapes[][5] = {{5, 3, 0, 1, 1}, {17, 4, 0, 3, 3}, {49, 20, 20, 3, 3}, {33, 6, 3, 7, 1}, {128, 36, 0, 1, 7}, {2, 32, 0, 5, 5}};
    for (const auto& s : shapes)
        for (int fold = 0; fold < 2; ++fold) check_shape(s[0], s[1], s[2], s[3], s[4], fold != 0);
    if (g_failed) return 1;
    printf("conv_pack_check: ok (%zu shapes x 2)\n", sizeof(shapes) / sizeof(shapes[0]));
    return 0;
}
