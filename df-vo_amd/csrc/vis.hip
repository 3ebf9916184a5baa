// Dense panels of the frame drawer (/root/reference/libs/general/frame_drawer.py:410-512) on the device: the Middlebury wheel
// of the two flows (flowlib.py:186-219, 298-339), the magma map of the depth / disparity and the jet maps of the consistency
// maps, each resized into its cell of the window canvas in HBM with cv2.resize's 8-bit INTER_LINEAR arithmetic.
//
// A cell pixel reads at most four source pixels, so nothing is coloured at full resolution: one fused kernel evaluates the
// colour of the <= 4 pixels an output pixel samples and blends them with the fixed-point coefficients of k_resize_linear_u8
// (resize_lanczos.hip; the exact-half 2 x 2 area path is folded in).  In front of it run the two things that need the whole
// map: the maximum flow radius (one reduction per flow) and the exact 90th percentile of the disparity (a radix select on
// order-preserving keys, 11 bits per pass, histograms in LDS -- no sort).  All of it is stream ordered; the host reads
// nothing between the stages.
//
// Arithmetic contract = what the reference's numpy / matplotlib code computes under numpy 2 (NEP 50):
//   wheel     rad = sqrt(u*u + v*v) in float32 for the maximum; u / (maxrad + eps) and everything behind it in float64,
//             products and sums rounded one by one (no contraction: this file is built with -ffp-contract=off and says so
//             below); arctan2's signed zeros select the wheel entry; NaN pixels -> 0, unknown pixels (|u|, |v| > 1e7) -> 0;
//   maps      Normalize(0, vmax) then Colormap.__call__ in the map's dtype: x / vmax computed in float64 and rounded to the
//             dtype, * 256, == 256 -> 255, < 0 -> first entry, >= 256 -> last entry, NaN -> black; vmax == 0 -> first entry;
//   disparity 1 / (d + 1e-3) in the map's dtype, d == 0 -> 0; vmax = np.percentile(.., 90): virtual index (n - 1) * 0.9 and
//             gamma in the map's dtype, _lerp with its t >= 0.5 branch, NaN anywhere -> NaN.
#include <cmath>
#include <cstring>
#include <mutex>
#include <set>

#include "capi_types.h"
#include "vis.h"
#include "vis_tables.h"

#pragma clang fp contract(off)

using namespace dfvo;

namespace {

__constant__ unsigned char c_magma[256][3];
__constant__ unsigned char c_jet[256][3];
__constant__ unsigned char c_wheel[55][3];

constexpr int SEL_BINS = 2048;   // 11-bit digits
constexpr int SEL_MAX_PASSES = 6;
constexpr unsigned NAN_BITS = 0x7fc00000u;

struct Rgb {
    int c[3];
};

// ---- Middlebury wheel of one pixel (compute_color, flowlib.py:298-339, on u / den, v / den) -------------------------
__device__ __forceinline__ double atan2_signed(double y, double x) {
    // the zero cases spelled out (C99 F.9.1.4): they decide between the first and the last wheel entry
    if (y == 0.0) return signbit(x) ? copysign(3.14159265358979323846, y) : copysign(0.0, y);
    return atan2(y, x);
}

__device__ __forceinline__ bool flow_unknown(float u, float v) { return fabsf(u) > 1e7f || fabsf(v) > 1e7f; }

__device__ Rgb wheel_px(float u, float v, double den) {
    Rgb o = {{0, 0, 0}};
    if (flow_unknown(u, v)) return o;
    double ud = (double)u / den, vd = (double)v / den;
    const bool bad = isnan(ud) || isnan(vd);
    if (bad) return o;  // 255 * col * (1 - nanIdx)
    const double rad = sqrt(__dadd_rn(__dmul_rn(ud, ud), __dmul_rn(vd, vd)));
    const double a = atan2_signed(-vd, -ud) / 3.14159265358979323846;
    const double fk = __dadd_rn(__dmul_rn(__dadd_rn(a, 1.0) / 2.0, 54.0), 1.0);
    int k0 = (int)floor(fk);
    k0 = k0 < 1 ? 1 : (k0 > 55 ? 55 : k0);
    const int k1 = k0 + 1 == 56 ? 1 : k0 + 1;
    const double f = __dsub_rn(fk, (double)k0);
    for (int i = 0; i < 3; ++i) {
        const double col0 = (double)c_wheel[k0 - 1][i] / 255.0, col1 = (double)c_wheel[k1 - 1][i] / 255.0;
        double col = __dadd_rn(__dmul_rn(__dsub_rn(1.0, f), col0), __dmul_rn(f, col1));
        if (rad <= 1.0)
            col = __dsub_rn(1.0, __dmul_rn(rad, __dsub_rn(1.0, col)));
        else
            col = __dmul_rn(col, 0.75);
        const double x = floor(__dmul_rn(255.0, col));
        o.c[i] = x < 0.0 ? 0 : (x > 255.0 ? 255 : (int)x);
    }
    return o;
}

__device__ __forceinline__ double wheel_den(unsigned maxrad_bits) {
    // maxrad = max(-1, np.max(rad)): a NaN maximum compares false and leaves -1
    const double maxrad = maxrad_bits > 0x7f800000u ? -1.0 : (double)__uint_as_float(maxrad_bits);
    return __dadd_rn(maxrad, 2.220446049250313e-16);
}

// ---- matplotlib: Normalize(0, vmax) + Colormap.__call__ on one value, in its dtype ---------------------------------
template <class T>
__device__ __forceinline__ T disparity(T d);
template <>
__device__ __forceinline__ float disparity<float>(float d) {
    return d == 0.f ? 0.f : __fdiv_rn(1.f, __fadd_rn(d, 1e-3f));
}
template <>
__device__ __forceinline__ double disparity<double>(double d) {
    return d == 0.0 ? 0.0 : __ddiv_rn(1.0, __dadd_rn(d, 1e-3));
}

template <class T>
__device__ Rgb cmap_px(T x, double vmax, int cmap) {
    T xn = (T)0;
    if (vmax != 0.0) xn = (T)((double)x / vmax);  // (NaN vmax: every value NaN)
    T xa = xn * (T)256;
    if (xa == (T)256) xa = (T)255;
    Rgb o = {{0, 0, 0}};
    if (isnan(xa)) return o;
    const int idx = xa < (T)0 ? 0 : (xa >= (T)256 ? 255 : (int)xa);
    const unsigned char* e = cmap == VIS_CMAP_JET ? c_jet[idx] : c_magma[idx];
    o.c[0] = e[0], o.c[1] = e[1], o.c[2] = e[2];
    return o;
}

__device__ Rgb panel_px(const VisPanel& p, int y, int x, double den, double vmax) {
    const size_t i = (size_t)y * p.W + x;
    if (p.kind == VIS_WHEEL) {
        const float* f = (const float*)p.src;
        return wheel_px(f[i], f[(size_t)p.H * p.W + i], den);
    }
    if (p.f64) {
        const double d = ((const double*)p.src)[i];
        return cmap_px<double>(p.kind == VIS_DISP ? disparity<double>(d) : d, vmax, p.cmap);
    }
    const float d = ((const float*)p.src)[i];
    return cmap_px<float>(p.kind == VIS_DISP ? disparity<float>(d) : d, vmax, p.cmap);
}

// the coefficient of k_resize_linear_u8 (resize_lanczos.hip)
__device__ __forceinline__ void lin_coef(int d, double scale, int* s_out, int* c0, int* c1) {
    float f = (float)__dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5);
    const int s = (int)floorf(f);
    f = __fsub_rn(f, (float)s);
    *s_out = s;
    *c0 = (int)rintf(__fmul_rn(__fsub_rn(1.f, f), 2048.f));
    *c1 = (int)rintf(__fmul_rn(f, 2048.f));
}

// One thread per cell pixel, blockIdx.z = panel.  Writes BGR (update_data: cvtColor(RGB2BGR) before the resize).
__global__ __launch_bounds__(256) void k_vis_panels(VisPanels ps, uint8_t* __restrict__ canvas, int win_h, int win_w) {
    const VisPanel& p = ps.p[blockIdx.z];
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y * blockDim.y + threadIdx.y;
    if (dx >= p.cw || dy >= p.ch) return;
    const int oy = p.y0 + dy, ox = p.x0 + dx;
    if (oy < 0 || oy >= win_h || ox < 0 || ox >= win_w) return;
    double den = 1.0, vmax = p.vmax;
    if (p.kind == VIS_WHEEL) den = wheel_den(*p.maxrad_bits);
    else if (p.vmax_dev) vmax = *p.vmax_dev;
    if (p.kind != VIS_WHEEL && vmax < 0.0) return;  // Normalize raises (vmin > vmax): the cell keeps what it held
    uint8_t* o = canvas + ((size_t)oy * win_w + ox) * 3;
    if (p.area2) {
        const Rgb a = panel_px(p, 2 * dy, 2 * dx, den, vmax), b = panel_px(p, 2 * dy, 2 * dx + 1, den, vmax);
        const Rgb c = panel_px(p, 2 * dy + 1, 2 * dx, den, vmax), d = panel_px(p, 2 * dy + 1, 2 * dx + 1, den, vmax);
        for (int k = 0; k < 3; ++k) o[2 - k] = (uint8_t)((a.c[k] + b.c[k] + c.c[k] + d.c[k] + 2) >> 2);
        return;
    }
    int sx, a0, a1, sy, b0, b1;
    lin_coef(dx, p.scale_x, &sx, &a0, &a1);
    if (sx < 0) sx = 0, a0 = 2048, a1 = 0;
    if (sx >= p.W - 1) sx = p.W - 1, a0 = 2048, a1 = 0;
    lin_coef(dy, p.scale_y, &sy, &b0, &b1);
    const int y0 = sy < 0 ? 0 : (sy < p.H ? sy : p.H - 1), y1 = sy + 1 < 0 ? 0 : (sy + 1 < p.H ? sy + 1 : p.H - 1);
    const int sx1 = sx + 1 < p.W ? sx + 1 : sx;
    // (a source pixel whose weight is zero is not coloured: the identity cell evaluates one pixel, not four)
    const Rgb zero = {{0, 0, 0}};
    const Rgb p00 = panel_px(p, y0, sx, den, vmax);
    const Rgb p01 = a1 ? panel_px(p, y0, sx1, den, vmax) : zero;
    const Rgb p10 = b1 ? (y1 == y0 ? p00 : panel_px(p, y1, sx, den, vmax)) : zero;
    const Rgb p11 = (a1 && b1) ? (y1 == y0 ? p01 : panel_px(p, y1, sx1, den, vmax)) : zero;
    for (int k = 0; k < 3; ++k) {
        const int h0 = p00.c[k] * a0 + p01.c[k] * a1;
        const int h1 = p10.c[k] * a0 + p11.c[k] * a1;
        o[2 - k] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
    }
}

// flow_to_image at full resolution: RGB [H, W, 3]
__global__ __launch_bounds__(256) void k_vis_flow_rgb(const float* __restrict__ flow, int n, const unsigned* __restrict__ maxrad_bits,
                                                       uint8_t* __restrict__ rgb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Rgb c = wheel_px(flow[i], flow[(size_t)n + i], wheel_den(*maxrad_bits));
    rgb[(size_t)i * 3 + 0] = (uint8_t)c.c[0];
    rgb[(size_t)i * 3 + 1] = (uint8_t)c.c[1];
    rgb[(size_t)i * 3 + 2] = (uint8_t)c.c[2];
}

// ---- maximum radius + unknown count of one flow (flowlib.py:203-209) ---------------------------------------------
// out[0]: bits of the maximum (radii are >= 0, so their bit patterns order as unsigned; any NaN radius becomes the pattern
// above +inf and wins, as np.max propagates it), out[1]: number of unknown pixels.  Zeroed before the launch.
__global__ __launch_bounds__(256) void k_vis_flow_max(const float* __restrict__ flow, int n, unsigned* __restrict__ out) {
    __shared__ unsigned s_max[256], s_unk[256];
    unsigned m = 0, unk = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float u = flow[i], v = flow[(size_t)n + i];
        if (flow_unknown(u, v)) {
            u = v = 0.f;
            ++unk;
        }
        const float s = __fadd_rn(__fmul_rn(u, u), __fmul_rn(v, v));
        const float r = (float)sqrt((double)s);  // correctly rounded float32 sqrt (53 >= 2 * 24 + 2 bits)
        const unsigned b = isnan(r) ? NAN_BITS : __float_as_uint(r);
        m = b > m ? b : m;
    }
    s_max[threadIdx.x] = m;
    s_unk[threadIdx.x] = unk;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_max[threadIdx.x] = s_max[threadIdx.x] > s_max[threadIdx.x + w] ? s_max[threadIdx.x] : s_max[threadIdx.x + w];
            s_unk[threadIdx.x] += s_unk[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMax(&out[0], s_max[0]);
        if (s_unk[0]) atomicAdd(&out[1], s_unk[0]);
    }
}

// ---- exact order statistics of the disparity: radix select ------------------------------------------------------
// Keys order as the values do (sign flip; -0 counts as +0; NaN sorts last, as np.partition places it).
template <class T>
struct SelKey;
template <>
struct SelKey<float> {
    static constexpr int BITS = 32, PASSES = 3;
    __device__ static unsigned long long key(float x) {
        if (isnan(x)) return 0xffffffffull;
        if (x == 0.f) x = 0.f;
        const unsigned b = __float_as_uint(x);
        return (b & 0x80000000u) ? (unsigned)~b : (b | 0x80000000u);
    }
    __device__ static float value(unsigned long long k) {
        const unsigned b = (unsigned)k;
        return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
    }
};
template <>
struct SelKey<double> {
    static constexpr int BITS = 64, PASSES = 6;
    __device__ static unsigned long long key(double x) {
        if (isnan(x)) return ~0ull;
        if (x == 0.0) x = 0.0;
        const unsigned long long b = (unsigned long long)__double_as_longlong(x);
        return (b >> 63) ? ~b : (b | (1ull << 63));
    }
    __device__ static double value(unsigned long long k) {
        return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
    }
};

__device__ __forceinline__ float rn_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float rn_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float rn_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double rn_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double rn_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double rn_mul(double a, double b) { return __dmul_rn(a, b); }

template <int BITS>
__device__ __forceinline__ int sel_shift(int pass) {
    const int s = BITS - 11 * (pass + 1);
    return s < 0 ? 0 : s;
}
template <int BITS, int PASSES>
__device__ __forceinline__ int sel_width(int pass) {
    return pass == PASSES - 1 ? BITS - 11 * (PASSES - 1) : 11;
}

struct SelState {
    unsigned long long prefix;  // the digits chosen so far, in place
    unsigned rank;              // rank of the wanted element among those that share the prefix
    unsigned count;             // how many elements fell into the last chosen bin
};

// Every block walks the finished histograms itself (npass of them): no kernel in between, no state to race on.
// lds: SEL_BINS words.  Wave 0 scans: each lane sums 32 bins, a shuffle scan finds the lane, the lane finds the bin.
template <int BITS, int PASSES>
__device__ SelState sel_resolve(const unsigned* __restrict__ hist, int npass, unsigned k, unsigned* lds) {
    __shared__ SelState st;
    if (threadIdx.x == 0) st = SelState{0ull, k, 0u};
    __syncthreads();
    for (int q = 0; q < npass; ++q) {
        for (int i = threadIdx.x; i < SEL_BINS; i += blockDim.x) lds[i] = hist[q * SEL_BINS + i];
        __syncthreads();
        if (threadIdx.x < 64) {
            const int lane = threadIdx.x;
            const unsigned r = st.rank;
            unsigned sum = 0;
            for (int j = 0; j < 32; ++j) sum += lds[lane * 32 + j];
            unsigned incl = sum;
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(incl, d, 64);
                if (lane >= d) incl += t;
            }
            const unsigned excl = incl - sum;
            if (r >= excl && r < incl) {  // exactly one lane: r < number of elements under the prefix
                unsigned acc = excl;
                int b = lane * 32;
                for (int j = 0; j < 31 && r >= acc + lds[b]; ++j) acc += lds[b++];
                st.prefix |= (unsigned long long)b << sel_shift<BITS>(q);
                st.rank = r - acc;
                st.count = lds[b];
            }
        }
        __syncthreads();
    }
    const SelState out = st;
    __syncthreads();
    return out;
}

// pass `pass` of the select: histogram of its digit over the elements that share the digits chosen so far.
// hist [SEL_MAX_PASSES][SEL_BINS] (zeroed before pass 0), extra[0] = NaN count (pass 0 counts).
template <class T>
__global__ __launch_bounds__(256) void k_sel_hist(const T* __restrict__ depth, int n, int pass, unsigned k, unsigned* __restrict__ hist,
                                                   unsigned* __restrict__ extra) {
    using K = SelKey<T>;
    __shared__ unsigned lds[SEL_BINS];
    __shared__ unsigned s_nan;
    const SelState st = sel_resolve<K::BITS, K::PASSES>(hist, pass, k, lds);
    for (int i = threadIdx.x; i < SEL_BINS; i += blockDim.x) lds[i] = 0;
    if (threadIdx.x == 0) s_nan = 0;
    __syncthreads();
    const int shift = sel_shift<K::BITS>(pass), width = sel_width<K::BITS, K::PASSES>(pass);
    const int above = shift + width;  // bits above this digit: must equal the prefix (none in pass 0)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const T x = disparity<T>(depth[i]);
        if (pass == 0 && isnan(x)) atomicAdd(&s_nan, 1u);
        const unsigned long long key = K::key(x);
        if (above >= K::BITS || (key >> above) == (st.prefix >> above)) atomicAdd(&lds[(unsigned)(key >> shift) & ((1u << width) - 1u)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SEL_BINS; i += blockDim.x)
        if (lds[i]) atomicAdd(&hist[pass * SEL_BINS + i], lds[i]);
    if (threadIdx.x == 0 && s_nan) atomicAdd(&extra[0], s_nan);
}

// the next order statistic when the element of rank k is the last of its value: the smallest key above it.
// inv_min: ~key, maximised (zeroed before the launch).
template <class T>
__global__ __launch_bounds__(256) void k_sel_next(const T* __restrict__ depth, int n, unsigned k, const unsigned* __restrict__ hist,
                                                   unsigned long long* __restrict__ inv_min) {
    using K = SelKey<T>;
    __shared__ unsigned lds[SEL_BINS];
    __shared__ unsigned long long s_best[256];
    const SelState st = sel_resolve<K::BITS, K::PASSES>(hist, K::PASSES, k, lds);
    if (st.rank + 1 < st.count) return;  // the next one has the same value (uniform over the grid)
    unsigned long long best = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned long long key = K::key(disparity<T>(depth[i]));
        if (key > st.prefix && ~key > best) best = ~key;
    }
    s_best[threadIdx.x] = best;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w && s_best[threadIdx.x + w] > s_best[threadIdx.x]) s_best[threadIdx.x] = s_best[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_best[0]) atomicMax(inv_min, s_best[0]);
}

// numpy's _lerp(previous, next, gamma) in T; *vmax = the percentile as a double (Normalize subtracts vmin = 0.0 in float64)
template <class T>
__global__ __launch_bounds__(256) void k_sel_finish(unsigned k, int same_index, T gamma, const unsigned* __restrict__ hist,
                                                     const unsigned* __restrict__ extra, const unsigned long long* __restrict__ inv_min,
                                                     double* __restrict__ vmax) {
    using K = SelKey<T>;
    __shared__ unsigned lds[SEL_BINS];
    const SelState st = sel_resolve<K::BITS, K::PASSES>(hist, K::PASSES, k, lds);
    if (threadIdx.x != 0) return;
    if (extra[0]) {  // a NaN sorts last and np.percentile hands it out
        *vmax = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const T a = K::value(st.prefix);
    T b = a;
    if (!same_index && st.rank + 1 >= st.count) b = K::value(~*inv_min);
    const T diff = rn_sub(b, a);
    T r = rn_add(a, rn_mul(diff, gamma));
    if (gamma >= (T)0.5) r = rn_sub(b, rn_mul(diff, rn_sub((T)1, gamma)));
    *vmax = (double)r;
}

int sel_blocks(int n) {
    const int b = cdiv(n, 256 * 8);
    return b < 1 ? 1 : (b > 512 ? 512 : b);
}

}  // namespace

// ----------------------------------------------------------------------------------------------------------------------
struct dfvo_vis {
    int win_h = 0, win_w = 0;
    int cell[DFVO_VIS_CELLS][4] = {};  // y0, x0, y1, x1
    DevArr<uint8_t> canvas;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DevArr<unsigned char> stage[2];  // uploaded maps (bytes), grown on demand
    DevArr<uint8_t> rgb;             // dfvo_vis_flow_rgb, grown on demand
    // scratch: [0..1] flow 0 (max bits, unknown), [2..3] flow 1, [4] NaN count, [6..7] ~min key above, then the histograms
    DevArr<unsigned> scratch;
    DevArr<double> d_vmax;
    long long counters[DFVO_VIS_COUNTERS] = {};
    float last_ms = 0.f;
};

namespace {

constexpr size_t SCRATCH_WORDS = 8 + (size_t)SEL_MAX_PASSES * SEL_BINS;

// the tables go into the constant memory of each device once per process (drawers may be created from several threads)
int tables_to_device() {
    static std::mutex mu;
    static std::set<int> done;
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    DFVO_HIP_CHECK(hipGetDevice(&dev));
    if (done.count(dev)) return DFVO_OK;
    DFVO_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_magma), VIS_TAB_MAGMA, sizeof(VIS_TAB_MAGMA)));
    DFVO_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_jet), VIS_TAB_JET, sizeof(VIS_TAB_JET)));
    DFVO_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_wheel), VIS_TAB_WHEEL, sizeof(VIS_TAB_WHEEL)));
    done.insert(dev);
    return DFVO_OK;
}

// geometry of one cell for a map of H x W: cv::resize's scales and its exact-half test (enqueue_resize_linear_u8)
int fill_geometry(const dfvo_vis* v, int cell, int H, int W, VisPanel* p) {
    DFVO_ARG_CHECK(cell >= 0 && cell < DFVO_VIS_CELLS, "dfvo_vis: no such cell");
    DFVO_ARG_CHECK(H > 0 && W > 0 && (long long)H * W <= 1280ll * 1920ll, "dfvo_vis: map size out of range (up to 1280 x 1920)");
    p->H = H, p->W = W;
    p->y0 = v->cell[cell][0], p->x0 = v->cell[cell][1];
    p->ch = v->cell[cell][2] - v->cell[cell][0], p->cw = v->cell[cell][3] - v->cell[cell][1];
    DFVO_ARG_CHECK(p->ch > 0 && p->cw > 0, "dfvo_vis: empty cell");
    volatile double inv_x = (double)p->cw / (double)W, inv_y = (double)p->ch / (double)H;
    p->scale_x = 1.0 / inv_x, p->scale_y = 1.0 / inv_y;
    p->area2 = (std::fabs(p->scale_x - 2.0) < 2.220446049250313e-16 && std::fabs(p->scale_y - 2.0) < 2.220446049250313e-16) ? 1 : 0;
    return DFVO_OK;
}

int enqueue_flow_max(dfvo_vis* v, const float* d_flow, int n, int slot) {
    hipLaunchKernelGGL(k_vis_flow_max, dim3(sel_blocks(n)), dim3(256), 0, v->stream, d_flow, n, v->scratch + 2 * slot);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

// np.percentile(1 / (d + 1e-3), 90) -> v->d_vmax.  The indices and gamma are numpy's, in the map's dtype (q = 90 / dtype(100)).
template <class T>
int enqueue_percentile(dfvo_vis* v, const T* d_depth, int n) {
    using K = SelKey<T>;
    volatile T q = (T)90 / (T)100;
    volatile T vi = (T)(n - 1) * q;
    long long prev = (long long)std::floor((double)vi);
    int same = 0;
    T gamma;
    if ((double)vi >= (double)(n - 1)) {  // _get_indexes: both indices -1, gamma = vi - (-1)
        volatile T g = vi + (T)1;
        gamma = g;
        prev = n - 1;
        same = 1;
    } else {
        volatile T g = vi - (T)prev;
        gamma = g;
    }
    const unsigned k = (unsigned)prev;
    const int blocks = sel_blocks(n);
    for (int pass = 0; pass < K::PASSES; ++pass)
        hipLaunchKernelGGL(k_sel_hist<T>, dim3(blocks), dim3(256), 0, v->stream, d_depth, n, pass, k, v->scratch + 8, v->scratch + 4);
    unsigned long long* inv_min = (unsigned long long*)(v->scratch + 6);
    if (!same) hipLaunchKernelGGL(k_sel_next<T>, dim3(blocks), dim3(256), 0, v->stream, d_depth, n, k, v->scratch + 8, inv_min);
    hipLaunchKernelGGL(k_sel_finish<T>, dim3(1), dim3(256), 0, v->stream, k, same, gamma, v->scratch + 8, v->scratch + 4, inv_min, v->d_vmax);
    DFVO_HIP_CHECK(hipGetLastError());
    v->counters[3] += 1;
    return DFVO_OK;
}

int enqueue_panels(dfvo_vis* v, const VisPanels& ps, int n) {
    int ch = 1, cw = 1;
    for (int i = 0; i < n; ++i) ch = std::max(ch, ps.p[i].ch), cw = std::max(cw, ps.p[i].cw);
    hipLaunchKernelGGL(k_vis_panels, dim3(cdiv(cw, 64), cdiv(ch, 4), n), dim3(64, 4), 0, v->stream, ps, v->canvas, v->win_h, v->win_w);
    DFVO_HIP_CHECK(hipGetLastError());
    v->counters[2] += 1;
    return DFVO_OK;
}

int begin_draw(dfvo_vis* v) {
    DFVO_HIP_CHECK(hipMemsetAsync(v->scratch, 0, SCRATCH_WORDS * sizeof(unsigned), v->stream));
    DFVO_HIP_CHECK(hipEventRecord(v->e0, v->stream));
    return DFVO_OK;
}

int end_draw(dfvo_vis* v) {
    DFVO_HIP_CHECK(hipEventRecord(v->e1, v->stream));
    DFVO_HIP_CHECK(hipStreamSynchronize(v->stream));
    DFVO_HIP_CHECK(hipEventElapsedTime(&v->last_ms, v->e0, v->e1));
    return DFVO_OK;
}

int upload(dfvo_vis* v, int slot, const void* h_src, size_t bytes) {
    int rc = v->stage[slot].grow(bytes);
    if (rc != DFVO_OK) return rc;
    DFVO_HIP_CHECK(hipMemcpyAsync(v->stage[slot], h_src, bytes, hipMemcpyHostToDevice, v->stream));
    v->counters[5] += (long long)bytes;
    return DFVO_OK;
}

int read_unknown(dfvo_vis* v, int slot, long long* n_unknown) {
    unsigned u = 0;
    DFVO_HIP_CHECK(hipMemcpy(&u, v->scratch + 2 * slot + 1, sizeof(u), hipMemcpyDeviceToHost));
    if (n_unknown) *n_unknown = (long long)u;
    return DFVO_OK;
}

}  // namespace

#define V_TRY(expr)                     \
    do {                                \
        int _rc = (expr);               \
        if (_rc != DFVO_OK) return _rc; \
    } while (0)

extern "C" {

int dfvo_vis_create(int window_h, int window_w, dfvo_vis** out) {
    DFVO_ARG_CHECK(out && window_h >= 4 && window_w >= 4 && window_h <= 16384 && window_w <= 16384, "dfvo_vis_create: bad argument");
    V_TRY(tables_to_device());
    dfvo_vis* v = new dfvo_vis();
    v->win_h = window_h, v->win_w = window_w;
    // initialize_drawer's quarter grid, int(h / 4 * k): depth | flow1 // flow2 (= rigid_flow_diff = warp_diff) | opt_flow_diff
    auto q = [](int extent, int k) { return (int)((double)extent / 4 * k); };
    const int rows[DFVO_VIS_CELLS] = {2, 2, 3, 3}, cols[DFVO_VIS_CELLS] = {2, 3, 2, 3};
    for (int c = 0; c < DFVO_VIS_CELLS; ++c) {
        v->cell[c][0] = q(window_h, rows[c]), v->cell[c][1] = q(window_w, cols[c]);
        v->cell[c][2] = q(window_h, rows[c] + 1), v->cell[c][3] = q(window_w, cols[c] + 1);
    }
    const size_t bytes = (size_t)window_h * window_w * 3;
    bool ok = hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) == hipSuccess && hipEventCreate(&v->e0) == hipSuccess &&
              hipEventCreate(&v->e1) == hipSuccess && v->canvas.alloc(bytes) == DFVO_OK &&
              v->scratch.alloc(SCRATCH_WORDS) == DFVO_OK && v->d_vmax.alloc(1) == DFVO_OK;
    ok = ok && hipMemsetAsync(v->canvas, 0, bytes, v->stream) == hipSuccess && hipStreamSynchronize(v->stream) == hipSuccess;
    if (!ok) {
        dfvo_vis_destroy(v);
        dfvo::set_last_error("dfvo_vis_create: allocation failed");
        return DFVO_ERR_HIP;
    }
    *out = v;
    return DFVO_OK;
}

void dfvo_vis_destroy(dfvo_vis* v) {
    if (!v) return;
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    if (v->e0) (void)hipEventDestroy(v->e0);
    if (v->e1) (void)hipEventDestroy(v->e1);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;  // (the arrays)
}

int dfvo_vis_cell_rect(const dfvo_vis* v, int cell, int* y0x0y1x1) {
    DFVO_ARG_CHECK(v && y0x0y1x1 && cell >= 0 && cell < DFVO_VIS_CELLS, "dfvo_vis_cell_rect: bad argument");
    for (int i = 0; i < 4; ++i) y0x0y1x1[i] = v->cell[cell][i];
    return DFVO_OK;
}

int dfvo_vis_draw_flow(dfvo_vis* v, int cell, const float* h_flow, int H, int W, long long* n_unknown) {
    DFVO_ARG_CHECK(v && h_flow, "dfvo_vis_draw_flow: bad argument");
    VisPanels ps = {};
    V_TRY(fill_geometry(v, cell, H, W, &ps.p[0]));
    const int n = H * W;
    V_TRY(upload(v, 0, h_flow, sizeof(float) * 2 * n));
    V_TRY(begin_draw(v));
    V_TRY(enqueue_flow_max(v, (const float*)v->stage[0].p, n, 0));
    ps.p[0].kind = VIS_WHEEL;
    ps.p[0].src = v->stage[0];
    ps.p[0].maxrad_bits = v->scratch;
    V_TRY(enqueue_panels(v, ps, 1));
    V_TRY(end_draw(v));
    v->counters[1] += 1;
    return read_unknown(v, 0, n_unknown);
}

int dfvo_vis_draw_map(dfvo_vis* v, int cell, const void* h_map, int is_f64, int H, int W, int kind, int cmap, double vmax_in,
                      double* vmax_out) {
    DFVO_ARG_CHECK(v && h_map && (kind == DFVO_VIS_MAP_VALUE || kind == DFVO_VIS_MAP_DISPARITY) &&
                       (cmap == DFVO_VIS_MAGMA || cmap == DFVO_VIS_JET),
                   "dfvo_vis_draw_map: bad argument");
    DFVO_ARG_CHECK(kind == DFVO_VIS_MAP_DISPARITY || !(vmax_in < 0.0), "dfvo_vis_draw_map: minvalue must be less than or equal to maxvalue");
    VisPanels ps = {};
    V_TRY(fill_geometry(v, cell, H, W, &ps.p[0]));
    const int n = H * W;
    V_TRY(upload(v, 0, h_map, (is_f64 ? sizeof(double) : sizeof(float)) * (size_t)n));
    V_TRY(begin_draw(v));
    VisPanel& p = ps.p[0];
    p.kind = kind == DFVO_VIS_MAP_DISPARITY ? VIS_DISP : VIS_CMAP;
    p.f64 = is_f64 ? 1 : 0;
    p.cmap = cmap == DFVO_VIS_JET ? VIS_CMAP_JET : VIS_CMAP_MAGMA;
    p.src = v->stage[0];
    p.vmax = vmax_in;
    if (p.kind == VIS_DISP) {
        V_TRY(is_f64 ? enqueue_percentile<double>(v, (const double*)v->stage[0].p, n) : enqueue_percentile<float>(v, (const float*)v->stage[0].p, n));
        p.vmax_dev = v->d_vmax;
    }
    V_TRY(enqueue_panels(v, ps, 1));
    V_TRY(end_draw(v));
    v->counters[1] += 1;
    double vm = vmax_in;
    if (p.kind == VIS_DISP) DFVO_HIP_CHECK(hipMemcpy(&vm, v->d_vmax, sizeof(double), hipMemcpyDeviceToHost));
    if (vmax_out) *vmax_out = vm;
    return DFVO_OK;
}

int dfvo_vis_draw_session(dfvo_vis* v, dfvo_session* s, long long generation, int cells, double diff_vmax, int depth_kind,
                          double depth_vmax, long long* n_unknown2, double* depth_vmax_out) {
    DFVO_ARG_CHECK(v && s && cells > 0 && cells < (1 << DFVO_VIS_CELLS), "dfvo_vis_draw_session: bad argument");
    VisSessionSources src;
    V_TRY(dfvo_session_vis_sources(s, generation, &src));
    const bool flows = cells & ((1 << DFVO_VIS_CELL_FLOW1) | (1 << DFVO_VIS_CELL_FLOW2) | (1 << DFVO_VIS_CELL_OPT_FLOW_DIFF));
    if (flows && !src.have_flow) {
        dfvo::set_last_error("dfvo_vis_draw_session: the session holds no flow pass of that generation on the device (none ran, or another "
                             "pass of the flow net overwrote its outputs)");
        return DFVO_ERR_STATE;
    }
    const bool depth = cells & (1 << DFVO_VIS_CELL_DEPTH);
    DFVO_ARG_CHECK(!depth || depth_kind == DFVO_VIS_MAP_VALUE || depth_kind == DFVO_VIS_MAP_DISPARITY, "dfvo_vis_draw_session: bad depth kind");
    if (depth && !src.have_depth) {
        dfvo::set_last_error("dfvo_vis_draw_session: another pass of the depth net overwrote the session's depth buffer");
        return DFVO_ERR_STATE;
    }
    DFVO_ARG_CHECK(!(diff_vmax < 0.0) && !(depth && depth_kind == DFVO_VIS_MAP_VALUE && depth_vmax < 0.0),
                   "dfvo_vis_draw_session: minvalue must be less than or equal to maxvalue");
    // the session's buffers are read behind the events that guard them, and this call returns when the reads are done
    if (flows) DFVO_HIP_CHECK(hipStreamWaitEvent(v->stream, src.e_net, 0));
    if (depth) DFVO_HIP_CHECK(hipStreamWaitEvent(v->stream, src.e_depth, 0));
    V_TRY(begin_draw(v));
    VisPanels ps = {};
    int np = 0;
    const int n = src.H * src.W;
    if (depth) {
        VisPanel& p = ps.p[np];
        V_TRY(fill_geometry(v, DFVO_VIS_CELL_DEPTH, src.depth_h, src.depth_w, &p));
        p.kind = depth_kind == DFVO_VIS_MAP_DISPARITY ? VIS_DISP : VIS_CMAP;
        p.cmap = VIS_CMAP_MAGMA;
        p.src = src.depth;
        p.vmax = depth_vmax;
        if (p.kind == VIS_DISP) {
            V_TRY(enqueue_percentile<float>(v, src.depth, src.depth_h * src.depth_w));
            p.vmax_dev = v->d_vmax;
        }
        ++np;
    }
    const float* fl[2] = {src.fwd, src.bwd};
    const int fcell[2] = {DFVO_VIS_CELL_FLOW1, DFVO_VIS_CELL_FLOW2};
    for (int i = 0; i < 2; ++i) {
        if (!(cells & (1 << fcell[i]))) continue;
        VisPanel& p = ps.p[np];
        V_TRY(fill_geometry(v, fcell[i], src.H, src.W, &p));
        V_TRY(enqueue_flow_max(v, fl[i], n, i));
        p.kind = VIS_WHEEL;
        p.src = fl[i];
        p.maxrad_bits = v->scratch + 2 * i;
        ++np;
    }
    if (cells & (1 << DFVO_VIS_CELL_OPT_FLOW_DIFF)) {
        VisPanel& p = ps.p[np];
        V_TRY(fill_geometry(v, DFVO_VIS_CELL_OPT_FLOW_DIFF, src.H, src.W, &p));
        p.kind = VIS_CMAP;
        p.cmap = VIS_CMAP_JET;
        p.src = src.diff;
        p.vmax = diff_vmax;
        ++np;
    }
    V_TRY(enqueue_panels(v, ps, np));
    V_TRY(end_draw(v));
    v->counters[0] += np;
    for (int i = 0; i < 2; ++i) {
        long long u = 0;
        if (cells & (1 << fcell[i])) V_TRY(read_unknown(v, i, &u));
        if (n_unknown2) n_unknown2[i] = u;
    }
    if (depth_vmax_out) {
        *depth_vmax_out = depth_vmax;
        if (depth && depth_kind == DFVO_VIS_MAP_DISPARITY) DFVO_HIP_CHECK(hipMemcpy(depth_vmax_out, v->d_vmax, sizeof(double), hipMemcpyDeviceToHost));
    }
    return DFVO_OK;
}

int dfvo_vis_session_cells(dfvo_session* s, long long generation, int* cells) {
    DFVO_ARG_CHECK(s && cells, "dfvo_vis_session_cells: bad argument");
    VisSessionSources src;
    V_TRY(dfvo_session_vis_sources(s, generation, &src));
    *cells = (src.have_flow ? (1 << DFVO_VIS_CELL_FLOW1) | (1 << DFVO_VIS_CELL_FLOW2) | (1 << DFVO_VIS_CELL_OPT_FLOW_DIFF) : 0) |
             (src.have_depth ? (1 << DFVO_VIS_CELL_DEPTH) : 0);
    return DFVO_OK;
}

int dfvo_vis_clear_cell(dfvo_vis* v, int cell) {
    DFVO_ARG_CHECK(v && cell >= 0 && cell < DFVO_VIS_CELLS, "dfvo_vis_clear_cell: bad argument");
    const int* r = v->cell[cell];
    DFVO_HIP_CHECK(hipMemset2DAsync(v->canvas + ((size_t)r[0] * v->win_w + r[1]) * 3, (size_t)v->win_w * 3, 0, (size_t)(r[3] - r[1]) * 3,
                                    (size_t)(r[2] - r[0]), v->stream));
    DFVO_HIP_CHECK(hipStreamSynchronize(v->stream));
    v->counters[4] += 1;
    return DFVO_OK;
}

int dfvo_vis_fetch(dfvo_vis* v, int cell, uint8_t* h_dst) {
    DFVO_ARG_CHECK(v && h_dst && cell >= -1 && cell < DFVO_VIS_CELLS, "dfvo_vis_fetch: bad argument");
    if (cell < 0) {
        const size_t bytes = (size_t)v->win_h * v->win_w * 3;
        DFVO_HIP_CHECK(hipMemcpyAsync(h_dst, v->canvas, bytes, hipMemcpyDeviceToHost, v->stream));
        v->counters[6] += (long long)bytes;
    } else {
        const int* r = v->cell[cell];
        const size_t row = (size_t)(r[3] - r[1]) * 3, rows = (size_t)(r[2] - r[0]);
        DFVO_HIP_CHECK(hipMemcpy2DAsync(h_dst, row, v->canvas + ((size_t)r[0] * v->win_w + r[1]) * 3, (size_t)v->win_w * 3, row, rows,
                                        hipMemcpyDeviceToHost, v->stream));
        v->counters[6] += (long long)(row * rows);
    }
    DFVO_HIP_CHECK(hipStreamSynchronize(v->stream));
    return DFVO_OK;
}

int dfvo_vis_counters(const dfvo_vis* v, long long* out) {
    DFVO_ARG_CHECK(v && out, "dfvo_vis_counters: bad argument");
    memcpy(out, v->counters, sizeof(v->counters));
    return DFVO_OK;
}

int dfvo_vis_device_ms(const dfvo_vis* v, float* ms) {
    DFVO_ARG_CHECK(v && ms, "dfvo_vis_device_ms: bad argument");
    *ms = v->last_ms;
    return DFVO_OK;
}

int dfvo_vis_flow_rgb(dfvo_vis* v, const float* h_flow, int H, int W, uint8_t* h_rgb, long long* n_unknown) {
    DFVO_ARG_CHECK(v && h_flow && h_rgb && H > 0 && W > 0 && (long long)H * W <= 1280ll * 1920ll, "dfvo_vis_flow_rgb: bad argument");
    const int n = H * W;
    V_TRY(upload(v, 0, h_flow, sizeof(float) * 2 * n));
    V_TRY(v->rgb.grow((size_t)n * 3));
    V_TRY(begin_draw(v));
    V_TRY(enqueue_flow_max(v, (const float*)v->stage[0].p, n, 0));
    hipLaunchKernelGGL(k_vis_flow_rgb, dim3(cdiv(n, 256)), dim3(256), 0, v->stream, (const float*)v->stage[0].p, n, v->scratch, v->rgb);
    DFVO_HIP_CHECK(hipGetLastError());
    DFVO_HIP_CHECK(hipMemcpyAsync(h_rgb, v->rgb, (size_t)n * 3, hipMemcpyDeviceToHost, v->stream));
    V_TRY(end_draw(v));
    return read_unknown(v, 0, n_unknown);
}

int dfvo_vis_disparity_percentile90(dfvo_vis* v, const void* h_depth, int is_f64, int n, double* out) {
    DFVO_ARG_CHECK(v && h_depth && out && n > 0 && n <= 1280 * 1920, "dfvo_vis_disparity_percentile90: bad argument");
    V_TRY(upload(v, 0, h_depth, (is_f64 ? sizeof(double) : sizeof(float)) * (size_t)n));
    V_TRY(begin_draw(v));
    V_TRY(is_f64 ? enqueue_percentile<double>(v, (const double*)v->stage[0].p, n) : enqueue_percentile<float>(v, (const float*)v->stage[0].p, n));
    V_TRY(end_draw(v));
    DFVO_HIP_CHECK(hipMemcpy(out, v->d_vmax, sizeof(double), hipMemcpyDeviceToHost));
    return DFVO_OK;
}

}  // extern "C"
