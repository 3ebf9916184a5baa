// Input stage on the device (include/dfvo_hip.h, dfvo_undistort_*): what the RobotCar SDK does to a raw camera frame on the host
// (sdk_python/image.py load_image: demosaicing_CFA_Bayer_bilinear, then camera_model.py undistort: scipy.ndimage.map_coordinates
// of order 1 through the per-pixel table, then astype(uint8)), one launch, only inside the box the read-image tail will read.
//   demosaic: plane P_c = the mosaic where the site's colour is c, 0 elsewhere, extended over the border (reflect: -1 -> 0,
//             n -> n - 1; mirror: -1 -> 1, n -> n - 2); R, B = P * [[1,2,1],[2,4,2],[1,2,1]] / 4, G = P * [[0,1,0],[1,4,1],[0,1,0]] / 4.
//             Every value is a multiple of 1/4: summed as integers, exact.
//   remap:    (cx, cy) outside [0, w - 1] x [0, h - 1]: 0.  Else fy = floor(cy), ty = cy - fy, wy = {1 - ty, ty} (x alike) and
//             t = 0; for a, b in (0, 1): c = V[min(fy + a, h - 1)][min(fx + b, w - 1)]; c = c * wy[a]; c = c * wx[b]; t = t + c --
//             float64, one rounding per operation (ud_mul below); the byte is t truncated.
// Under `reflect` the one-pixel frame of a plane can exceed 255 (a site counted twice); the byte is then the truncated value's
// low 8 bits, as the x86 conversion numpy compiles to gives.
// HBM-bound gather: 16 B of table and 3 B written per pixel; the mosaic's neighbourhood (4 x 4 sites) comes from cache.
#include "undistort.h"

namespace dfvo {

// colour (0 R, 1 G, 2 B) of site (y & 1) * 2 + (x & 1), two bits each, by DFVO_BAYER_* code
static const unsigned kBayerSites[4] = {
    0u | 1u << 2 | 1u << 4 | 2u << 6,  // rggb
    2u | 1u << 2 | 1u << 4 | 0u << 6,  // bggr
    1u | 0u << 2 | 2u << 4 | 1u << 6,  // grbg
    1u | 2u << 2 | 0u << 4 | 1u << 6,  // gbrg
};

struct UdBox {
    int y0, y1, x0, x1;
};
struct alignas(16) UdXY {
    double x, y;
};
struct alignas(4) UdQuad {
    uint32_t v[3];
};

// index i in [-1, n] extended over the border, clamped into the plane whatever i is
__device__ __forceinline__ int ud_border(int i, int n, int mirror) {
    if (i < 0) i = mirror ? -i : -i - 1;
    if (i >= n) i = mirror ? 2 * n - 2 - i : 2 * n - 1 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// four times the demosaiced (R, G, B) of site (y, x)
__device__ __forceinline__ void ud_demosaic4(const uint8_t* __restrict__ m, int h, int w, unsigned sites, int mirror, int y, int x,
                                             int num[3]) {
    num[0] = num[1] = num[2] = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int ny = ud_border(y + dy, h, mirror);
        const uint8_t* row = m + (size_t)ny * w;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int nx = ud_border(x + dx, w, mirror);
            const int v = row[nx];
            const int c = (int)(sites >> (2 * ((ny & 1) * 2 + (nx & 1)))) & 3;
            const int ring = (dy != 0) + (dx != 0);                                 // 0 centre, 1 edge, 2 corner
            const int w_rb = 4 >> ring, w_g = ring == 0 ? 4 : (ring == 1 ? 1 : 0);  // the two kernels, times 4
            num[0] += c == 0 ? v * w_rb : 0;
            num[1] += c == 1 ? v * w_g : 0;
            num[2] += c == 2 ? v * w_rb : 0;
        }
    }
}

// V[y][x][0..2] as float64: the demosaiced mosaic, or the distorted RGB frame
template <bool MOSAIC>
__device__ __forceinline__ void ud_value(const uint8_t* __restrict__ src, int h, int w, unsigned sites, int mirror, int y, int x,
                                         double v[3]) {
    if (MOSAIC) {
        int num[3];
        ud_demosaic4(src, h, w, sites, mirror, y, x, num);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (double)num[c] * 0.25;  // exact
    } else {
        const uint8_t* p = src + ((size_t)y * w + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (double)p[c];
    }
}

// A product rounded on its own.  The build's -ffp-contract=fast lets the backend fuse any multiply with the add that follows it,
// whatever `#pragma clang fp contract(off)` says and through __dmul_rn / __dadd_rn, which are plain operators (measured: 120
// v_fmac_f64 in this unit with both in place, and a byte off at 2 x 2); a value that went through an asm statement is no
// multiply the add can be fused with.
__device__ __forceinline__ double ud_mul(double a, double b) {
    double r = a * b;
    asm volatile("" : "+v"(r));
    return r;
}

__device__ __forceinline__ uint32_t ud_byte(double t) { return (uint32_t)t & 255u; }  // 0 <= t < 2^10

template <bool MOSAIC, bool MAP>
__device__ __forceinline__ void ud_pixel(const uint8_t* __restrict__ src, const UdXY* __restrict__ map, int h, int w, unsigned sites,
                                         int mirror, int y, int x, uint32_t out[3]) {
    if (!MAP) {
        int num[3];
        ud_demosaic4(src, h, w, sites, mirror, y, x, num);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (uint32_t)(num[c] >> 2) & 255u;  // the value truncated
        return;
    }
    const UdXY q = map[(size_t)y * w + x];
    out[0] = out[1] = out[2] = 0;
    if (!(q.y >= 0.0 && q.y <= (double)(h - 1) && q.x >= 0.0 && q.x <= (double)(w - 1))) return;
    const double fyd = floor(q.y), fxd = floor(q.x);
    const int fy = (int)fyd, fx = (int)fxd;
    const double ty = q.y - fyd, tx = q.x - fxd;
    const double wy[2] = {1.0 - ty, ty}, wx[2] = {1.0 - tx, tx};
    double t[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int yy = fy + a < h - 1 ? fy + a : h - 1;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int xx = fx + b < w - 1 ? fx + b : w - 1;
            double v[3];
            ud_value<MOSAIC>(src, h, w, sites, mirror, yy, xx, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c] = t[c] + ud_mul(ud_mul(v[c], wy[a]), wx[b]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = ud_byte(t[c]);
}

// A lane owns one quad of four consecutive pixels of the flat plane, aligned to four pixels (12 bytes, so 4-byte aligned) and
// clipped to the box's span of ONE row (depth_consistency.hip's scheme): a whole quad goes out as three 4-byte words, a clipped
// one -- the head or tail of a row's span -- byte by byte.  G: quads a row's span can touch.
template <bool MOSAIC, bool MAP>
__global__ void __launch_bounds__(256) k_undistort(const uint8_t* __restrict__ src, const UdXY* __restrict__ map, int h, int w,
                                                   unsigned sites, int mirror, UdBox box, int G, uint8_t* __restrict__ dst) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)(box.y1 - box.y0) * G) return;
    const int y = box.y0 + (int)(t / G), g = (int)(t % G);
    const long long r0 = (long long)y * w + box.x0, r1 = (long long)y * w + box.x1;
    const long long q0 = ((r0 >> 2) + g) << 2;
    const long long lo = q0 > r0 ? q0 : r0, hi = q0 + 4 < r1 ? q0 + 4 : r1;
    if (lo >= hi) return;
    const int n = (int)(hi - lo), xa = (int)(lo - (long long)y * w);
    if (n == 4) {
        uint32_t px[4][3];
#pragma unroll
        for (int i = 0; i < 4; ++i) ud_pixel<MOSAIC, MAP>(src, map, h, w, sites, mirror, y, xa + i, px[i]);
        UdQuad o;  // bytes R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3, little endian
        o.v[0] = px[0][0] | px[0][1] << 8 | px[0][2] << 16 | px[1][0] << 24;
        o.v[1] = px[1][1] | px[1][2] << 8 | px[2][0] << 16 | px[2][1] << 24;
        o.v[2] = px[2][2] | px[3][0] << 8 | px[3][1] << 16 | px[3][2] << 24;
        *reinterpret_cast<UdQuad*>(dst + lo * 3) = o;
    } else {
        for (int i = 0; i < n; ++i) {
            uint32_t px[3];
            ud_pixel<MOSAIC, MAP>(src, map, h, w, sites, mirror, y, xa + i, px);
            for (int c = 0; c < 3; ++c) dst[(lo + i) * 3 + c] = (uint8_t)px[c];
        }
    }
}

template <bool MOSAIC, bool MAP>
static int launch_undistort(const uint8_t* src, const double* map, int h, int w, unsigned sites, int mirror, UdBox box, uint8_t* dst,
                            hipStream_t s) {
    const int G = (box.x1 - box.x0 + 3) / 4 + 1;
    const long long lanes = (long long)(box.y1 - box.y0) * G;
    hipLaunchKernelGGL((k_undistort<MOSAIC, MAP>), dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, src,
                       reinterpret_cast<const UdXY*>(map), h, w, sites, mirror, box, G, dst);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

static int check_box(const char* fn, int h, int w, int y0, int y1, int x0, int x1) {
    DFVO_ARG_CHECK(h >= 1 && w >= 1 && (long long)h * w < (1ll << 29), std::string(fn) + ": frame size outside 1 .. 2^29 pixels");
    DFVO_ARG_CHECK(0 <= y0 && y0 < y1 && y1 <= h && 0 <= x0 && x0 < x1 && x1 <= w, std::string(fn) + ": box outside the frame");
    return DFVO_OK;
}

int check_undistort_mosaic(const char* fn, const dfvo_undistort_map* map, int img_h, int img_w, int pattern, int border, int y0, int y1,
                           int x0, int x1) {
    const std::string f(fn);
    DFVO_ARG_CHECK(pattern >= 0 && pattern <= 3, f + ": pattern is DFVO_BAYER_RGGB, _BGGR, _GRBG or _GBRG (0 .. 3)");
    DFVO_ARG_CHECK(border == DFVO_BORDER_REFLECT || border == DFVO_BORDER_MIRROR, f + ": border is DFVO_BORDER_REFLECT or _MIRROR");
    const int rc = check_box(fn, img_h, img_w, y0, y1, x0, x1);
    if (rc != DFVO_OK) return rc;
    DFVO_ARG_CHECK(border != DFVO_BORDER_MIRROR || (img_h >= 2 && img_w >= 2), f + ": the mirror border needs a frame of 2 x 2 or more");
    DFVO_ARG_CHECK(!map || (map->h == img_h && map->w == img_w), f + ": the map is of another frame size");
    return DFVO_OK;
}

int enqueue_undistort_mosaic(const dfvo_undistort_map* map, const uint8_t* d_mosaic, int img_h, int img_w, int pattern, int border,
                             int y0, int y1, int x0, int x1, uint8_t* d_rgb, hipStream_t s) {
    const UdBox box = {y0, y1, x0, x1};
    const unsigned sites = kBayerSites[pattern];
    const int mirror = border == DFVO_BORDER_MIRROR;
    if (map) return launch_undistort<true, true>(d_mosaic, map->xy.p, img_h, img_w, sites, mirror, box, d_rgb, s);
    return launch_undistort<true, false>(d_mosaic, nullptr, img_h, img_w, sites, mirror, box, d_rgb, s);
}

}  // namespace dfvo

using namespace dfvo;

extern "C" {

int dfvo_undistort_create(int h, int w, const double* map_xy, dfvo_undistort_map** out) {
    DFVO_ARG_CHECK(out, "dfvo_undistort_create: null out");
    *out = nullptr;
    DFVO_ARG_CHECK(map_xy, "dfvo_undistort_create: null map");
    DFVO_ARG_CHECK(h >= 1 && w >= 1 && (long long)h * w < (1ll << 29), "dfvo_undistort_create: frame size outside 1 .. 2^29 pixels");
    const size_t n = (size_t)h * w;
    std::vector<double> xy(2 * n);
    for (size_t i = 0; i < n; ++i) {
        const double x = map_xy[i], y = map_xy[n + i];
        // (x - x is NaN for NaN and the infinities alike)
        DFVO_ARG_CHECK(x - x == 0.0 && y - y == 0.0, "dfvo_undistort_create: the map has a non-finite entry (pixel " + std::to_string(i) + ")");
        xy[2 * i] = x, xy[2 * i + 1] = y;
    }
    dfvo_undistort_map* m = new dfvo_undistort_map();
    m->h = h, m->w = w;
    int rc = m->xy.alloc(2 * n);
    if (rc == DFVO_OK && hipMemcpy(m->xy.p, xy.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice) != hipSuccess) {
        set_last_error("dfvo_undistort_create: the upload of the map failed");
        rc = DFVO_ERR_HIP;
    }
    if (rc != DFVO_OK) {
        delete m;
        return rc;
    }
    *out = m;
    return DFVO_OK;
}

void dfvo_undistort_destroy(dfvo_undistort_map* map) { delete map; }

int dfvo_undistort_mosaic_u8(const dfvo_undistort_map* map, const uint8_t* d_mosaic, int img_h, int img_w, int pattern, int border,
                             int y0, int y1, int x0, int x1, uint8_t* d_rgb, void* stream) {
    DFVO_ARG_CHECK(d_mosaic && d_rgb, "dfvo_undistort_mosaic_u8: null frame");
    DFVO_ARG_CHECK(((uintptr_t)d_rgb & 3) == 0, "dfvo_undistort_mosaic_u8: d_rgb must be 4-byte aligned");
    const int rc = check_undistort_mosaic("dfvo_undistort_mosaic_u8", map, img_h, img_w, pattern, border, y0, y1, x0, x1);
    if (rc != DFVO_OK) return rc;
    return enqueue_undistort_mosaic(map, d_mosaic, img_h, img_w, pattern, border, y0, y1, x0, x1, d_rgb, (hipStream_t)stream);
}

int dfvo_undistort_rgb_u8(const dfvo_undistort_map* map, const uint8_t* d_src, int y0, int y1, int x0, int x1, uint8_t* d_rgb,
                          void* stream) {
    DFVO_ARG_CHECK(map, "dfvo_undistort_rgb_u8: null map");
    DFVO_ARG_CHECK(d_src && d_rgb, "dfvo_undistort_rgb_u8: null frame");
    DFVO_ARG_CHECK(((uintptr_t)d_rgb & 3) == 0, "dfvo_undistort_rgb_u8: d_rgb must be 4-byte aligned");
    DFVO_ARG_CHECK(d_src != d_rgb, "dfvo_undistort_rgb_u8: the remap is not done in place");
    const int rc = check_box("dfvo_undistort_rgb_u8", map->h, map->w, y0, y1, x0, x1);
    if (rc != DFVO_OK) return rc;
    const UdBox box = {y0, y1, x0, x1};
    return launch_undistort<false, true>(d_src, map->xy.p, map->h, map->w, 0u, 0, box, d_rgb, (hipStream_t)stream);
}

}  // extern "C"
