// Winograd F(2x2,3x3) on the fp32 MFMA: the opt-in path of the 3x3 / stride-1 / zero-pad layers packed in "fp32"
// (dfvo_set_fp32_winograd): the kernel, its switch, launch counter and launcher.  All-fp32 arithmetic, 16 instead of 36
// multiplications per 2x2 output tile, not bit-identical to the direct kernels.
//
// One launch per layer; neither the transformed input V nor the product M leaves the chip.  A workgroup of WN * 2 waves owns
// a 16 x 16 output block (8 x 8 tiles of 2 x 2) and BN = 32 * WN couts.  Per chunk of 8 input channels (each source padded
// to a multiple of 8, as the weights are: conv_pack_wino_f32.h):
//   - the raw 18 x 18 window of the chunk goes global -> registers -> LDS (zero outside the map, the two sources and their
//     cs / co views resolved here),
//   - V = B^T d B is formed with adds only, one thread per (tile, channel quad, upper / lower half of the 4 x 4), and written
//     to LDS as the MFMA B operand [pos 16][h 2][tile][4],
//   - U of the chunk, [pos 16][h 2][cout][4] in global memory already, is copied to LDS as the A operand,
//   - wave (cb, tb) runs the 16 independent [32 couts] x [32 tiles] GEMMs on v_mfma_f32_32x32x2_f32: MFMA kk of a position
//     contracts channel kk of the chunk (lanes 0-31) and channel 4 + kk (lanes 32-63), one ds_read_b128 per operand per
//     position.  Sixteen 32 x 32 accumulators = 256 registers per lane: one wave per SIMD on the unified 512-entry file.
// The next chunk's window and U travel under the current chunk's MFMAs (V and U are double-buffered in LDS).
// Epilogue: a lane holds, for its tile, 4 quads of consecutive couts in every accumulator, so Y = A^T M A is formed in
// registers and goes through the library's epilogue (bias, residual, activation, dst view, dst_zero_to).
// Resources on gfx950 (both instantiations): 512 VGPRs (256 of them accumulators), no VGPR spill, no scratch; 26 SGPRs are
// spilled to VGPR lanes (the window masks and offsets), outside the MFMA sequence.
// The grid is exactly N * tiles_y * tiles_x workgroups in x (the XCD-aware remap of blockIdx.x is a permutation of that
// range only) and round_up(cout, 32) / BN in y; the launcher below is the only caller.
#include "conv.h"

#include <cstdlib>
#include <mutex>

#include "conv_epi.h"
#include "conv_pack_wino_f32.h"

namespace dfvo {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WINO_VT = 72;               // tile stride of V in LDS (64 tiles + 8: the two h planes land on different slots)
constexpr int WINO_WW = 18;               // window rows / columns
constexpr int WINO_PS = 12;               // floats per window pixel in LDS (8 channels + 4: conflict-free b128 reads)
constexpr int WINO_VBUF = 32 * WINO_VT * 4;
constexpr int WINO_RAW = WINO_WW * WINO_WW * WINO_PS;
template <int WN>
constexpr int wino_lds_floats() { return 2 * WINO_VBUF + 2 * (32 * 32 * WN * 4) + WINO_RAW; }

template <int WN>
__global__ __launch_bounds__(128 * WN) void conv_wino_f32_kernel(const ConvParams p, const float* __restrict__ wu, int wcp) {
    constexpr int NT = 128 * WN, BN = 32 * WN;
    constexpr int UBUF = 32 * BN * 4;
    constexpr int W_ITEMS = WINO_WW * WINO_WW * 2;  // (pixel, channel quad of the chunk)
    constexpr int W_CNT = (W_ITEMS + NT - 1) / NT;
    constexpr int U_CNT = 32 * BN / NT;             // float4 per thread and chunk
    constexpr int T_CNT = 256 / NT;                 // transform items per thread
    extern __shared__ __attribute__((aligned(16))) float wino_lds[];
    float* const vbuf = wino_lds;
    float* const ubuf = wino_lds + 2 * WINO_VBUF;
    float* const raw = ubuf + 2 * UBUF;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int cb = wave % WN, tb = wave / WN;  // cout block, tile block (4 tile rows) of the wave
    const int l31 = lane & 31, hi = lane >> 5;
    const int tiles_x = (p.Wo + 15) / 16, tiles_y = (p.Ho + 15) / 16;
    const int nb = gridDim.x;
    int bid = blockIdx.x;
    {  // XCD-aware order, as in the window kernel
        const int q = nb >> 3, r = nb & 7, xcd = bid & 7, k = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
    }
    const int n = bid / (tiles_y * tiles_x);
    const int trem = bid - n * (tiles_y * tiles_x);
    const int ty0 = (trem / tiles_x) * 16, tx0 = (trem % tiles_x) * 16;
    const int n0 = blockIdx.y * BN;
    const int nchunk0 = (p.G0 + 1) >> 1, nchunks = nchunk0 + ((p.G1 + 1) >> 1);

    // window items of this thread
    unsigned w_off0[W_CNT], w_off1[W_CNT];
    int w_lds[W_CNT];
    bool w_ok[W_CNT];
#pragma unroll
    for (int r = 0; r < W_CNT; ++r) {
        const int id = t + NT * r;
        const int px = id >> 1, q = id & 1;
        const int wy = px / WINO_WW, wx = px - wy * WINO_WW;
        int iy = ty0 - 1 + wy, ix = tx0 - 1 + wx;
        const bool v = id < W_ITEMS && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        iy = iy < 0 ? 0 : (iy >= p.H ? p.H - 1 : iy);
        ix = ix < 0 ? 0 : (ix >= p.W ? p.W - 1 : ix);
        const unsigned pix = ((unsigned)n * p.H + iy) * p.W + ix;
        w_off0[r] = pix * (unsigned)p.cs0 + p.co0 + q * 4;
        w_off1[r] = pix * (unsigned)p.cs1 + p.co1 + q * 4;
        w_ok[r] = v;
        w_lds[r] = (id < W_ITEMS ? px : 0) * WINO_PS + q * 4;
    }
    f32x4 rw[W_CNT], ru[U_CNT];
    bool rwv[W_CNT];
    auto load_window = [&](int c) {
        const bool s1 = c >= nchunk0;
        const int cg0 = s1 ? (c - nchunk0) * 2 : c * 2;
        const int Gs = s1 ? p.G1 : p.G0;
        const float* base = s1 ? p.src1 : p.src0;
#pragma unroll
        for (int r = 0; r < W_CNT; ++r) {
            const int q = (t + NT * r) & 1;
            const bool v = w_ok[r] && (cg0 + q) < Gs;
            const unsigned off = (s1 ? w_off1[r] : w_off0[r]) + (v ? cg0 * 4 : -(q * 4));  // masked lanes re-read channel 0
            rw[r] = *reinterpret_cast<const f32x4*>(base + off);
            rwv[r] = v;  // (zeroed when the window is written to LDS: nothing waits for the load here)
        }
    };
    auto store_window = [&]() {
#pragma unroll
        for (int r = 0; r < W_CNT; ++r)
            if (t + NT * r < W_ITEMS) *reinterpret_cast<f32x4*>(raw + w_lds[r]) = rwv[r] ? rw[r] : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto load_u = [&](int c) {
#pragma unroll
        for (int r = 0; r < U_CNT; ++r) {
            const int f = t + NT * r, ph = f / BN, j = f - ph * BN;
            ru[r] = *reinterpret_cast<const f32x4*>(wu + (((size_t)c * 32 + ph) * wcp + n0 + j) * 4);
        }
    };
    // V = B^T d B, B^T = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]].  An item is (tile, channel quad, half):
    // rows 2 half and 2 half + 1 of V from window rows half .. half + 2.  The work of a thread is cut into eight pieces that
    // the second half of a chunk's MFMAs carries one by one: pieces 0-3 read window column j and form rows ra / rb of B^T d,
    // pieces 4-7 form and write two positions each; every piece also writes one quad of the next chunk's U.
    f32x4 ra[T_CNT][4], rb[T_CNT][4];
    auto tpiece = [&](int i, float* V, float* U) {
#pragma unroll
        for (int it = 0; it < T_CNT; ++it) {
            const int id = t + NT * it;
            const int h = id & 1, tx = (id >> 1) & 7, ty = (id >> 4) & 7, half = id >> 7;  // half is wave-uniform
            if (i < 4) {
                const float* d0 = raw + ((2 * ty + half) * WINO_WW + 2 * tx + i) * WINO_PS + h * 4;
                const f32x4 a = *reinterpret_cast<const f32x4*>(d0);
                const f32x4 b = *reinterpret_cast<const f32x4*>(d0 + WINO_WW * WINO_PS);
                const f32x4 c = *reinterpret_cast<const f32x4*>(d0 + 2 * WINO_WW * WINO_PS);
                ra[it][i] = half == 0 ? a - c : b - a;  // rows 0 / 2 of B^T d:  d0 - d2  /  d2 - d1
                rb[it][i] = half == 0 ? b + c : a - c;  // rows 1 / 3:           d1 + d2  /  d1 - d3
            } else {
                constexpr int PSTR = 2 * WINO_VT * 4;  // floats between two positions
                float* o = V + (size_t)(((half * 8) * 2 + h) * WINO_VT + ty * 8 + tx) * 4;
                const f32x4* r = i < 6 ? ra[it] : rb[it];
                o += (i < 6 ? 0 : 4) * PSTR;
                if ((i & 1) == 0) {
                    *reinterpret_cast<f32x4*>(o + 0 * PSTR) = r[0] - r[2];
                    *reinterpret_cast<f32x4*>(o + 1 * PSTR) = r[1] + r[2];
                } else {
                    *reinterpret_cast<f32x4*>(o + 2 * PSTR) = r[2] - r[1];
                    *reinterpret_cast<f32x4*>(o + 3 * PSTR) = r[1] - r[3];
                }
            }
        }
#pragma unroll
        for (int r = i * U_CNT / 8; r < (i + 1) * U_CNT / 8; ++r) *reinterpret_cast<f32x4*>(U + (t + NT * r) * 4) = ru[r];
    };

    f32x16 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    const int a_off = (hi * BN + cb * 32 + l31) * 4;        // + pos * 2 * BN * 4
    const int b_off = (hi * WINO_VT + tb * 32 + l31) * 4;   // + pos * 2 * WINO_VT * 4
    // eight positions of the chunk; the operands of position i + 1 are requested before the MFMAs of position i issue, and
    // piece(i) -- a slice of the next chunk's transform, or nothing -- rides behind them
    auto contract = [&](const float* U, const float* V, int pos0, auto piece) {
        f32x4 a = *reinterpret_cast<const f32x4*>(U + pos0 * (2 * BN * 4) + a_off);
        f32x4 b = *reinterpret_cast<const f32x4*>(V + pos0 * (2 * WINO_VT * 4) + b_off);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int pos = pos0 + i;
            f32x4 an = a, bn = b;
            if (i < 7) {
                an = *reinterpret_cast<const f32x4*>(U + (pos + 1) * (2 * BN * 4) + a_off);
                bn = *reinterpret_cast<const f32x4*>(V + (pos + 1) * (2 * WINO_VT * 4) + b_off);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc[pos] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b[kk], acc[pos], 0, 0, 0);
            piece(i);
            __builtin_amdgcn_sched_barrier(0);
            a = an;
            b = bn;
        }
    };
    auto nothing = [](int) {};

    // The loop body has no branch: behind the last chunk the "next" chunk is the last one again -- its window and U are
    // loaded, transformed and written to the idle buffers a second time, under MFMAs that have to run anyway -- so the
    // sixteen accumulators see one straight-line sequence of MFMAs per chunk.
    const int last = nchunks - 1;
    load_window(0);
    load_u(0);
    store_window();
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) tpiece(i, vbuf, ubuf);
    load_window(last < 1 ? last : 1);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int cur = c & 1;
        const float* Uc = ubuf + cur * UBUF;
        const float* Vc = vbuf + cur * WINO_VBUF;
        float* Vn = vbuf + (cur ^ 1) * WINO_VBUF;
        float* Un = ubuf + (cur ^ 1) * UBUF;
        store_window();  // chunk c + 1 (the window of chunk c was consumed before the last barrier)
        load_u(c + 1 < last ? c + 1 : last);
        contract(Uc, Vc, 0, nothing);
        __syncthreads();
        load_window(c + 2 < last ? c + 2 : last);
        contract(Uc, Vc, 8, [&](int i) { tpiece(i, Vn, Un); });
        __syncthreads();
    }

    // Y = A^T M A, A^T = [[1, 1, 1, 0], [0, 1, -1, -1]]; accumulator register 4 q + e of a lane is cout 8 q + 4 hi + e of its
    // wave's block, for the tile (l31 >> 3, l31 & 7) of the wave's four tile rows
    ConvEpi<4> epi;
    conv_epi_init(p, epi, [&](int q) { return n0 + cb * 32 + q * 8 + hi * 4; });
    const int oy0 = ty0 + (tb * 4 + (l31 >> 3)) * 2, ox0 = tx0 + (l31 & 7) * 2;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int oy = oy0 + dy, ox = ox0 + dx;
            const bool valid = oy < p.Ho && ox < p.Wo;
            conv_epi_row(p, epi, valid ? ((size_t)n * p.Ho + oy) * p.Wo + ox : 0, valid, [&](int q) {
                f32x4 y = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = dy; i < dy + 3; ++i)
#pragma unroll
                    for (int j = dx; j < dx + 3; ++j) {
                        const bool neg = (dy == 1 && i > 1) != (dx == 1 && j > 1);
                        const f32x16& m = acc[i * 4 + j];
                        const f32x4 v = {m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]};
                        y = neg ? y - v : y + v;
                    }
                return y;
            });
        }
}

// ---- the switch, the launch counter and the launcher ---------------------------------------------------------------------
static int g_fp32_winograd = -1;  // -1: not yet read from DFVO_FP32_WINOGRAD
int conv_fp32_winograd_mode() {
    if (g_fp32_winograd < 0) {
        const char* e = getenv("DFVO_FP32_WINOGRAD");
        const int m = e ? atoi(e) : 0;
        g_fp32_winograd = m >= 0 && m <= 2 ? m : 0;
    }
    return g_fp32_winograd;
}
int conv_set_fp32_winograd(int mode) {
    DFVO_ARG_CHECK(mode >= 0 && mode <= 2, "dfvo_set_fp32_winograd: expected 0, 1 or 2");
    g_fp32_winograd = mode;
    return DFVO_OK;
}
static std::mutex g_wino_mu;
static unsigned long long g_wino_launches = 0;
int conv_fp32_winograd_launches(unsigned long long* n, int reset) {
    DFVO_ARG_CHECK(n, "dfvo_fp32_winograd_launches: null argument");
    std::lock_guard<std::mutex> lock(g_wino_mu);
    *n = g_wino_launches;
    if (reset) g_wino_launches = 0;
    return DFVO_OK;
}

// what the kernel computes: 3x3, stride 1, zero padding of 1, no upsampled source, not the one- / two-channel heads
bool conv_wino_applicable(const ConvParams& p) {
    return p.wu32 && p.kh == 3 && p.kw == 3 && p.stride == 1 && p.pad_h == 1 && p.pad_w == 1 && p.pad_mode == PAD_ZERO &&
           p.up0 == 0 && p.cout > 2;
}

template <int WN>
static int launch_wino_cfg(const ConvParams& p, hipStream_t stream, int cfg_id) {
    const int wcp = wino_f32_cout_pad(p.cout);
    const size_t lds = (size_t)wino_lds_floats<WN>() * sizeof(float);
    if (int rc_lds = ensure_dyn_lds((const void*)conv_wino_f32_kernel<WN>, lds)) return rc_lds;
    dim3 grid((unsigned)(p.N * ((p.Ho + 15) / 16) * ((p.Wo + 15) / 16)), (unsigned)(wcp / (32 * WN)), 1);
    ConvProfScope prof(p, stream, cfg_id);
    hipLaunchKernelGGL(conv_wino_f32_kernel<WN>, grid, dim3(128 * WN), lds, stream, p, p.wu32, wcp);
    DFVO_HIP_CHECK(hipGetLastError());
    {
        std::lock_guard<std::mutex> lock(g_wino_mu);
        ++g_wino_launches;
    }
    static const std::string variant = conv_variant_name("wino", {WN});
    return prof.done((int)grid.x, (int)grid.y, 1, variant.c_str());
}
// cfg_id: the window row of the class the launch replaces (12-15), with the direct convolution's FLOP count
int launch_wino(const ConvParams& p, hipStream_t stream, int cfg_id) {
    return wino_f32_cout_pad(p.cout) % 64 == 0 ? launch_wino_cfg<2>(p, stream, cfg_id) : launch_wino_cfg<1>(p, stream, cfg_id);
}

}  // namespace dfvo
