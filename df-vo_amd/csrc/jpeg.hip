// Device half of the baseline JPEG decode (include/dfvo_hip.h, dfvo_jpeg_*): dequantisation, 8 x 8 inverse DCT, chroma
// upsampling and YCbCr -> RGB of the coefficients the host entropy pass (jpeg_entropy.h) staged, restating libjpeg-turbo's
// default decompression path -- the one Pillow's pixels come from -- operation by operation:
//   IDCT      jidctint.c "slow integer": 13-bit constants, the column pass descaled by 11 into a workspace, then the row pass
//             descaled by 18, + 128, clamped to 0 .. 255 (the rounding between the passes makes the order part of the result);
//   upsample  jdsample.c "fancy" triangle filters over the component's own downsampled width and height, the edge sample
//             replicated at every border: h2v1 (3 near + far + {1, 2}) >> 2, h2v2 3 near + far per column, then
//             (3 this + neighbour + {8, 7}) >> 4;
//   colour    jdcolor.c's 16-bit fixed-point tables, written out as the products they hold.
// Arithmetic width: the IDCT runs in uint32_t, whose overflow wraps, and is reinterpreted as int32_t only for the arithmetic
// right shifts of the two descales -- for the coefficients of a conforming encoder nothing overflows and the values are
// libjpeg's; for any other coefficient data the result is deterministic and clamped (libjpeg looks such samples up in a masked
// table, so parity ends there), and no index depends on a sample.  Upsampling and colour work on bytes in int32_t and cannot
// overflow.
// Two launches for a colour file: k_jpeg_idct over every block of every component (8 lanes per block: lane c does column c,
// then, through an LDS workspace, row c), the samples written over the first 64 bytes of the block's own coefficients (the
// buffer is the operator's workspace); k_jpeg_colour, one lane per output pixel.  A grey file is the first launch alone,
// writing the clipped plane.
#include "../../include/dfvo_hip.h"

#include <stddef.h>

#include "dfvo_common.h"
#include "jpeg_entropy.h"

using namespace dfvo;

namespace {

struct JpegGeom {
    int w, h, ncomp, hs, vs;
    int bw[3], nblk[3];  // blocks per row, blocks in all
    int cw[3], ch[3];    // downsampled size
    unsigned long long off[3];
};

typedef uint32_t u32;

__device__ __forceinline__ int descale(u32 x, int n) { return (int)(x + (1u << (n - 1))) >> n; }

// one 8-point pass of jidctint.c's jpeg_idct_islow on dequantised inputs i[0..7]; o[0..7] before the descale
__device__ __forceinline__ void idct8(const u32* i, u32* o) {
    u32 z2 = i[2], z3 = i[6];
    u32 z1 = (z2 + z3) * 4433u;
    u32 tmp2 = z1 + z3 * (u32)-15137;
    u32 tmp3 = z1 + z2 * 6270u;
    z2 = i[0];
    z3 = i[4];
    u32 tmp0 = (z2 + z3) << 13;
    u32 tmp1 = (z2 - z3) << 13;
    const u32 tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = i[7];
    tmp1 = i[5];
    tmp2 = i[3];
    tmp3 = i[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    u32 z4 = tmp1 + tmp3;
    const u32 z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u;
    tmp1 *= 16819u;
    tmp2 *= 25172u;
    tmp3 *= 12299u;
    z1 *= (u32)-7373;
    z2 *= (u32)-20995;
    z3 *= (u32)-16069;
    z4 *= (u32)-3196;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    o[0] = tmp10 + tmp3;
    o[7] = tmp10 - tmp3;
    o[1] = tmp11 + tmp2;
    o[6] = tmp11 - tmp2;
    o[2] = tmp12 + tmp1;
    o[5] = tmp12 - tmp1;
    o[3] = tmp13 + tmp0;
    o[4] = tmp13 - tmp0;
}

enum { IDCT_BLOCKS = 32 };  // 8 x 8 blocks per 256-lane workgroup

// buf: the device copy of the entropy pass's buffer (header, then coefficients).  gray_dst != null: the one component's
// samples go to gray_dst [h, w], clipped; else over the block's own first 64 bytes as uint8 [8][8].
__global__ void __launch_bounds__(256) k_jpeg_idct(uint8_t* __restrict__ buf, JpegGeom g, uint8_t* __restrict__ gray_dst) {
    __shared__ int ws[IDCT_BLOCKS][8][9];
    const int lb = threadIdx.x >> 3, lane = threadIdx.x & 7;
    long long b = (long long)blockIdx.x * IDCT_BLOCKS + lb;
    int c = 0;
    if (b >= g.nblk[0] && g.ncomp == 3) {
        b -= g.nblk[0];
        c = 1;
        if (b >= g.nblk[1]) {
            b -= g.nblk[1];
            c = 2;
        }
    }
    const bool active = b < g.nblk[c];
    uint8_t* blk = buf + g.off[c] + (unsigned long long)(active ? b : 0) * 128u;
    if (active) {
        const int16_t* coef = reinterpret_cast<const int16_t*>(blk);
        const uint16_t* q = reinterpret_cast<const uint16_t*>(buf + offsetof(dfvo_jpeg_info, quant)) + c * 64;
        u32 in[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; r++) in[r] = (u32)(int)coef[r * 8 + lane] * (u32)q[r * 8 + lane];
        idct8(in, o);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[lb][r][lane] = descale(o[r], 11);
    }
    __syncthreads();  // (also orders every lane's coefficient reads before the block's bytes are overwritten)
    if (!active) return;
    u32 in[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = (u32)ws[lb][lane][k];
    idct8(in, o);
    uint8_t px[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int v = descale(o[k], 18) + 128;
        px[k] = (uint8_t)min(max(v, 0), 255);
    }
    if (gray_dst) {
        const int y = (int)(b / g.bw[0]) * 8 + lane, x0 = (int)(b % g.bw[0]) * 8;
        if (y < g.h)
            for (int k = 0; k < 8; k++)
                if (x0 + k < g.w) gray_dst[(size_t)y * g.w + x0 + k] = px[k];
    } else {
        uint2 v;
        v.x = px[0] | (px[1] << 8) | (px[2] << 16) | ((u32)px[3] << 24);
        v.y = px[4] | (px[5] << 8) | (px[6] << 16) | ((u32)px[7] << 24);
        *reinterpret_cast<uint2*>(blk + lane * 8) = v;
    }
}

__device__ __forceinline__ int jsample(const uint8_t* __restrict__ buf, const JpegGeom& g, int c, int y, int x) {
    return buf[g.off[c] + ((unsigned long long)(y >> 3) * g.bw[c] + (x >> 3)) * 128u + (y & 7) * 8 + (x & 7)];
}

__device__ __forceinline__ int jchroma(const uint8_t* __restrict__ buf, const JpegGeom& g, int c, int y, int x) {
    if (g.hs == 1) return jsample(buf, g, c, y, x);
    const int cx = x >> 1, ox = (x & 1) ? min(cx + 1, g.cw[c] - 1) : max(cx - 1, 0);
    if (g.vs == 1) return (3 * jsample(buf, g, c, y, cx) + jsample(buf, g, c, y, ox) + ((x & 1) ? 2 : 1)) >> 2;
    const int cy = y >> 1, oy = (y & 1) ? min(cy + 1, g.ch[c] - 1) : max(cy - 1, 0);
    const int cur = 3 * jsample(buf, g, c, cy, cx) + jsample(buf, g, c, oy, cx);
    const int oth = 3 * jsample(buf, g, c, cy, ox) + jsample(buf, g, c, oy, ox);
    return (3 * cur + oth + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ void __launch_bounds__(256) k_jpeg_colour(const uint8_t* __restrict__ buf, JpegGeom g, uint8_t* __restrict__ dst) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)g.h * g.w) return;
    const int y = (int)(t / g.w), x = (int)(t % g.w);
    const int Y = jsample(buf, g, 0, y, x);
    const int cb = jchroma(buf, g, 1, y, x) - 128, cr = jchroma(buf, g, 2, y, x) - 128;
    const int r = Y + ((91881 * cr + 32768) >> 16);
    const int gg = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    const int bl = Y + ((116130 * cb + 32768) >> 16);
    uint8_t* o = dst + (size_t)t * 3;
    o[0] = (uint8_t)min(max(r, 0), 255);
    o[1] = (uint8_t)min(max(gg, 0), 255);
    o[2] = (uint8_t)min(max(bl, 0), 255);
}

// the layout the entropy pass derives from size, component count and sampling; DFVO_ERR_ARG when `info` is not that
int jpeg_geom(const char* fn, const dfvo_jpeg_info* info, JpegGeom* g) {
    DFVO_ARG_CHECK(info, std::string(fn) + ": null info");
    const int w = info->width, h = info->height, nc = info->components, H = info->h_samp, V = info->v_samp;
    DFVO_ARG_CHECK(w >= 1 && w <= 65535 && h >= 1 && h <= 65535 && (nc == 1 || nc == 3), std::string(fn) + ": info: size or component count");
    DFVO_ARG_CHECK(nc == 3 ? ((H == 1 && V == 1) || (H == 2 && V == 1) || (H == 2 && V == 2)) : (H == 1 && V == 1),
                   std::string(fn) + ": info: sampling is not 1x1, 2x1 or 2x2");
    const int mx = (w + 8 * H - 1) / (8 * H), my = (h + 8 * V - 1) / (8 * V);
    unsigned long long off = DFVO_JPEG_HEADER_BYTES;
    g->w = w, g->h = h, g->ncomp = nc, g->hs = H, g->vs = V;
    for (int c = 0; c < 3; c++) g->bw[c] = g->nblk[c] = g->cw[c] = g->ch[c] = 0, g->off[c] = 0;
    for (int c = 0; c < nc; c++) {
        const int ch = c == 0 ? H : 1, cv = c == 0 ? V : 1;
        const long long nblk = (long long)(mx * ch) * (my * cv);
        DFVO_ARG_CHECK(nblk <= (1ll << 24), std::string(fn) + ": more than 2^24 blocks in a component");
        g->bw[c] = mx * ch;
        g->nblk[c] = (int)nblk;
        g->cw[c] = (w * ch + H - 1) / H;
        g->ch[c] = (h * cv + V - 1) / V;
        g->off[c] = off;
        DFVO_ARG_CHECK(info->blocks_w[c] == g->bw[c] && info->blocks_h[c] == my * cv && info->comp_w[c] == g->cw[c] &&
                           info->comp_h[c] == g->ch[c] && info->plane_offset[c] == off,
                       std::string(fn) + ": info: not the layout of its size and sampling");
        off += (unsigned long long)nblk * 128u;
    }
    DFVO_ARG_CHECK(info->bytes == off, std::string(fn) + ": info: not the layout of its size and sampling");
    return DFVO_OK;
}

}  // namespace

namespace dfvo {

int enqueue_jpeg_decode(uint8_t* d_coeffs, const dfvo_jpeg_info* info, uint8_t* d_dst, hipStream_t s, const char* fn) {
    JpegGeom g;
    const int rc = jpeg_geom(fn, info, &g);
    if (rc != DFVO_OK) return rc;
    const long long nblk = (long long)g.nblk[0] + g.nblk[1] + g.nblk[2];
    hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)((nblk + IDCT_BLOCKS - 1) / IDCT_BLOCKS)), dim3(256), 0, s, d_coeffs, g,
                       g.ncomp == 1 ? d_dst : (uint8_t*)nullptr);
    DFVO_HIP_CHECK(hipGetLastError());
    if (g.ncomp == 3) {
        const long long px = (long long)g.h * g.w;
        hipLaunchKernelGGL(k_jpeg_colour, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, (const uint8_t*)d_coeffs, g, d_dst);
        DFVO_HIP_CHECK(hipGetLastError());
    }
    return DFVO_OK;
}

}  // namespace dfvo

extern "C" {

int dfvo_jpeg_probe(const uint8_t* h_bytes, size_t n, dfvo_jpeg_info* info) {
    const char* why = "?";
    const int rc = jpeg::probe(h_bytes, n, info, &why);
    if (rc != DFVO_OK) set_last_error(std::string("dfvo_jpeg_probe: ") + why);
    return rc;
}

int dfvo_jpeg_entropy_decode(const uint8_t* h_bytes, size_t n, void* h_dst, size_t capacity_bytes, dfvo_jpeg_info* info) {
    const char* why = "?";
    const int rc = jpeg::entropy_decode(h_bytes, n, h_dst, capacity_bytes, info, &why);
    if (rc != DFVO_OK) set_last_error(std::string("dfvo_jpeg_entropy_decode: ") + why);
    return rc;
}

int dfvo_jpeg_decode_u8(uint8_t* d_coeffs, const dfvo_jpeg_info* info, uint8_t* d_dst, void* stream) {
    DFVO_ARG_CHECK(d_coeffs && d_dst, "dfvo_jpeg_decode_u8: null buffer");
    DFVO_ARG_CHECK(((uintptr_t)d_coeffs & 7u) == 0, "dfvo_jpeg_decode_u8: d_coeffs is not 8-byte aligned");
    return enqueue_jpeg_decode(d_coeffs, info, d_dst, (hipStream_t)stream, "dfvo_jpeg_decode_u8");
}

}  // extern "C"
