// The library's internal convolution interface: the kernel argument ConvParams, the host packers (conv_pack.hip), the
// per-launch profile (conv_profile.hip), the dispatcher (conv_dispatch.hip) and the entry points the kernel families export
// to it -- conv_igemm_f32.hip (exact fp32), conv_f16.hip (the families of conv_win_f16s.h, conv_win_f16s2.h,
// conv_gemm_f16s.h), conv_taps_f16s.hip, conv_gemm_f32g.hip, conv_wino_f32.hip: one translation unit each.
// Activations are NHWC float32; "cs" = floats per pixel of the underlying buffer, "co" = channel offset of the view inside
// the pixel.
#pragma once
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

#include "dfvo_common.h"

namespace dfvo {

enum Act { ACT_NONE = 0, ACT_LEAKY = 1, ACT_RELU = 2, ACT_ELU = 3, ACT_SIGMOID = 4 };
enum PadMode { PAD_ZERO = 0, PAD_REFLECT = 1 };

// Implicit-GEMM convolution parameters (device-visible, passed by value).
struct ConvParams {
    // logical input spatial dims the taps index into (after optional x2 nearest upsample of src0)
    int N, H, W;
    int Ho, Wo;
    int kh, kw, stride, pad_h, pad_w;
    int pad_mode;
    // source 0: c0 logical channels, G0 = ceil(c0/4) k-groups per tap
    const float* src0;
    int G0, cs0, co0, up0;
    // source 1 (optional; G1 == 0 when absent)
    const float* src1;
    int G1, cs1, co1;
    // packed weights [ksteps*4][cout_pad][4], bias[cout_pad]
    const float* wp;
    const float* bias;
    // head layout of the same weights (one- / two-channel square layers only, else null): see conv_pack_head_weights
    const float* wh;
    // f16 hi/lo planes of the weights in the split window kernel's layout (DFVO_CONV_PRECISION=f16x3, 3x3 layers only):
    // [tap][16-channel chunk][wf16_cout_pad / 32][plane hi, lo][k / 8][32 couts][8] halves, see conv_pack_weights_f16s
    const unsigned short* wf16;
    int wf16_cout_pad;
    // f16 hi/lo planes in k-group order for the generic split kernel (conv_gemm_f16s.h; every layer in f16x3 mode):
    // [16-k step][wf16g_cout_pad / 32][plane][k / 8][32 couts][8] halves + the layer's k-group table (4 words per step)
    const unsigned short* wf16g;
    int wf16g_cout_pad;
    const uint32_t* f16g_tab;
    int f16g_steps;
    // products per term of the f16 kernels: 3 (or 0) = f16x3 (hi x hi + the two cross products, fp32-class), 1 = "f16" mode
    // (hi x hi only: plain f16 operands, fp32 accumulate -- BASELINE config 5's "fp16 flow"; the lo planes are never read)
    int f16_terms;
    // exact-fp32 twin of the above for conv_gemm_f32g_kernel (fp32 mode): [16-k step][cout_pad / 32][k / 8][32 couts][8]
    // floats, same k-group table and cout padding (wf16g_cout_pad, f16g_tab, f16g_steps are set in both modes)
    const float* wf32g;
    int cout, cout_pad, ksteps;
    // optional residual (added before activation)
    const float* res;
    int res_cs, res_co;
    int act;
    float act_param;
    float* dst;
    int dst_cs, dst_co;
    // when != 0 the epilogue also zero-fills channels [cout, dst_zero_to) of dst
    int dst_zero_to;
    // split-K workspace (optional): partial accumulators [splits][M][cout_pad]
    float* ws;
    size_t ws_floats;
    // split-K tickets (optional, zero between launches): one counter per output tile.  With them the workgroup that writes
    // a tile's last partial also reduces and finishes the tile -- no second launch (see splitk_last_arriver)
    unsigned* tile_flags;
    int tile_flags_n;
    // 2 * MACs of the unpadded convolution (bookkeeping for the bench's roofline leg; not read on device)
    double useful_flops;
    // Winograd F(2x2,3x3) weights U = G g G^T of a layer packed in "fp32" with dfvo_set_fp32_winograd on (else null):
    // [8-channel chunk][pos 16][h 2][round_up(cout, 32)][4], see conv_pack_wino_f32.h.  (These eight bytes were padding of the
    // kernel ABI: ConvParams is a kernel argument, the layout of every other field is what it was.)
    const float* wu32;
    // the device counter of activations beyond f16's range (g_f16s_clamped of conv_f16_clamp.h) for the f16 kernels that
    // live in their own translation units (conv_taps_f16s.hip: device symbols do not cross TUs)
    unsigned* f16s_clamp_ctr;
};

// the f16 hi / lo split, x = hi + 2^-11 lo (conv_f16_split.h on the device, conv_pack.hip for the weights)
constexpr float F16S_LO_SCALE = 2048.0f;  // 2^11
constexpr float F16S_LO_UNSCALE = 1.0f / 2048.0f;
constexpr float F16S_MAX = 65504.0f;

// ---- host packers (conv_pack.hip) ---------------------------------------------------------------------------------------
// number of K-steps (16 k-values = 4 groups of 4 channels) for a conv
static inline int conv_ksteps(int kh, int kw, int c0, int c1) {
    int G = cdiv(c0, 4) + cdiv(c1, 4);
    return cdiv(kh * kw * G, 4);
}
// N-tile (BN) the launcher will use for a given cout; cout_pad is a multiple of it
int conv_pick_bn(int cout, long long M);
static inline int conv_cout_pad(int cout, long long M) {
    int bn = conv_pick_bn(cout, M);
    return round_up(cout, bn);
}
// Pack OIHW weights (cin = c0 + c1) into the kernel layout. `out` must hold
// conv_ksteps*4*cout_pad*4 floats. fold_scale/fold_shift (per-cout, may be null)
// implement eval-mode BatchNorm folding: w' = w*scale, b' = b*scale + shift.
void conv_pack_weights(const float* w_oihw, const float* bias, int cout, int c0, int c1, int kh, int kw,
                       int cout_pad, const float* fold_scale, const float* fold_shift, float* out_w,
                       float* out_b);
// weights of a one- / two-channel k x k layer in the order the direct head kernel consumes them:
// [8-channel chunk (source 0 first, each source rounded up)][kx][4-channel group of the chunk (2)][ky][cout][4]
size_t conv_head_weight_floats(int cout, int c0, int c1, int k);
void conv_pack_head_weights(const float* w_oihw, int cout, int c0, int c1, int k, const float* fold_scale, float* out);
// the precision the nets are packed in (DFVO_CONV_PRECISION, nets.hip)
int conv_split_mode();  // 0 exact fp32 (default), 4 = f16x3 (f16 hi/lo planes, fp32-class), 5 = f16 (hi plane only: one product per term)
// weights of a 3x3 layer as f16 hi / lo planes (ConvParams::wf16); returns the number of halves (out may be null: the size)
size_t conv_pack_weights_f16s(const float* w_oihw, int cout, int c0, int c1, const float* fold_scale, unsigned short* out);
// the ring kernels' weights in k-group order (f16 hi / lo planes, plain fp32) and their k-group table, 4 entries per step:
// ky [0,5) | kx [5,10) | valid 10 | source 11 | channel offset inside the source << 16
static inline uint32_t f16g_entry(int ky, int kx, int valid, int src, int choff) {
    return (uint32_t)ky | ((uint32_t)kx << 5) | ((uint32_t)valid << 10) | ((uint32_t)src << 11) | ((uint32_t)choff << 16);
}
void conv_build_f16g_table(int c0, int c1, int kh, int kw, std::vector<uint32_t>* tab);
size_t conv_pack_weights_f16g(const float* w_oihw, int cout, int c0, int c1, int kh, int kw, const float* fold_scale,
                              unsigned short* out);
size_t conv_pack_weights_f32g(const float* w_oihw, int cout, int c0, int c1, int kh, int kw, const float* fold_scale, float* out);
// the packer of a 3x3 layer's Winograd U (conv_pack_wino_f32.h)
size_t conv_wino_f32_weight_floats(int cout, int c0, int c1);
void conv_pack_weights_wino_f32(const float* w_oihw, int cout, int c0, int c1, const float* fold_scale, float* out);
// weights beyond f16's range met by the f16 packers since the last reset (conv_f16s_overflow_count adds it to its report)
unsigned long long conv_f16s_weights_clamped(bool reset);

// ---- the dispatcher (conv_dispatch.hip) ---------------------------------------------------------------------------------
constexpr int CONV_NUM_CFGS = 24;  // tile configurations of the implicit-GEMM kernel (profile arrays have this size)
// wino_all: a layer with Winograd weights (p.wu32) takes that kernel whatever its size (dfvo_set_fp32_winograd(2))
int launch_conv(const ConvParams& p, hipStream_t stream, bool wino_all = false);
// mode 1: can launch_conv's size rule accept a launch of this layer, of at most max_pixels output pixels (0: unknown)?
bool conv_wino_rule_may_accept(int cout, long long max_pixels);
// the shape of a ring kernel (conv_gemm_f16s.h, conv_gemm_f32g.hip) for M pixels, nblk 32-cout blocks and `steps` K steps:
// two cout blocks per wave or one, K slices per workgroup (1 2 4 8, 16 only without tc2)
struct RingShape { bool tc2; int ksp; };
RingShape ring_shape(long long M, int nblk, int steps);

// ---- the families' entry points -----------------------------------------------------------------------------------------
// conv_igemm_f32.hip: the tile of bm x bn, the window kernel of a profile row (12-17), the head kernel of the layer's k, cout
int launch_igemm_f32(const ConvParams& p, hipStream_t stream, int bm, int bn);
int launch_win_f32(const ConvParams& p, hipStream_t stream, int cfg_id);
int launch_head_f32(const ConvParams& p, hipStream_t stream);
// conv_f16.hip: the window skeletons (3x3 / stride 1, profile row 19), the ring kernel (rows 20 / 21), the saturation report
bool conv_f16s_ok(const ConvParams& p);
int launch_f16_window(const ConvParams& p, hipStream_t stream);
bool conv_f16g_ok(const ConvParams& p);
int launch_f16g(const ConvParams& p, hipStream_t stream);
unsigned* conv_f16s_overflow_counter();  // device address of the counter behind it (session.hip reads it behind each net)
int conv_f16s_overflow_count(unsigned long long* n, int reset);
// conv_taps_f16s.hip (bit-identical to the ring kernel's <4, 1, TC> shape; p.f16s_clamp_ctr set; row 20), conv_gemm_f32g.hip
bool conv_taps_f16s_ok(const ConvParams& p);
int launch_taps_f16s(const ConvParams& p, hipStream_t stream);
bool conv_f32g_ok(const ConvParams& p);
int launch_f32g(const ConvParams& p, hipStream_t stream);
// conv_wino_f32.hip: the process-wide switch (0 off, 1 by the size rule, 2 every applicable layer; read once from
// DFVO_FP32_WINOGRAD), the count of launches of its kernel, what the kernel computes, its launcher (cfg_id: a window row)
int conv_fp32_winograd_mode();
int conv_set_fp32_winograd(int mode);
int conv_fp32_winograd_launches(unsigned long long* n, int reset);
bool conv_wino_applicable(const ConvParams& p);
int launch_wino(const ConvParams& p, hipStream_t stream, int cfg_id);

// ---- the per-launch profile (conv_profile.hip) --------------------------------------------------------------------------
void conv_profile_begin();
int conv_profile_end(double* ms, double* flops, int* launches, double* bytes = nullptr);

// "family<a,b,c>" from a launcher's own template arguments, `last` (a word such as "rag" or "py2") appended when given: the
// variant column of the per-launch profile.  A launcher builds it once per instantiation, into a function-local static.
static inline std::string conv_variant_name(const char* family, std::initializer_list<int> args, const char* last = nullptr) {
    std::string s(family);
    s += '<';
    bool first = true;
    for (int a : args) {
        if (!first) s += ',';
        s += std::to_string(a);
        first = false;
    }
    if (last) {
        if (!first) s += ',';
        s += last;
    }
    s += '>';
    return s;
}
enum { CONV_SPLITK_NONE = 0, CONV_SPLITK_TICKETS = 1, CONV_SPLITK_EPILOGUE = 2 };

// One profiled launch.  Between conv_profile_begin() and conv_profile_end() the constructor creates two events and records
// the first on the stream, done() records the second and files the entry; a scope that is left without done() -- an error
// return of the launcher -- destroys its events.  Outside a profile both do nothing.
class ConvProfScope {
  public:
    ConvProfScope(const ConvParams& p, hipStream_t stream, int cfg_id);
    ~ConvProfScope();
    ConvProfScope(const ConvProfScope&) = delete;
    ConvProfScope& operator=(const ConvProfScope&) = delete;
    // after the launch(es): DFVO_OK, or DFVO_ERR_HIP if an event call failed.  gx gy gz: see ConvProfEntry.  variant: the
    // instantiation that ran, as conv_variant_name() spells the launcher's template arguments (read only while a profile
    // runs); f16_terms: 3 / 1 for the kernels that come in f16x3 and f16 form, else 0; splitk: how a launch with K slices
    // over grid.z was finished (CONV_SPLITK_*)
    int done(int gx, int gy, int gz, const char* variant, int f16_terms = 0, int splitk = 0);

  private:
    const ConvParams& p_;
    hipStream_t stream_;
    int cfg_;
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
    hipError_t err_ = hipSuccess;
};

// f(std::integral_constant<int, NP>) for the NP (products per term) of p.f16_terms: 1 = "f16" mode, 3 = f16x3.  An f16
// launcher names its kernel once, as kernel<..., decltype(np)::value>, and both instantiations exist.
template <class F>
static inline auto with_f16_terms(const ConvParams& p, F&& f) {
    return p.f16_terms == 1 ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 3>{});
}

}  // namespace dfvo
