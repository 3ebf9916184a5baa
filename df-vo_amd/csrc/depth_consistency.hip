// DepthConsistency.warp_and_reproj_depth + compute_depth_diff, method depth_ratio (libs/matching/depth_consistency.py:69-151
// over libs/geometry/{backprojection, transformation3d, projection}.py), one launch, float32 throughout:
//   P = K^-1 (x, y, 1) d_cur,  P' = T[:3, :] (P, 1),  reproj = P'_z,
//   pixel = (K P')_xy / ((K P')_z + 1e-7), normalised /(W - 1), /(H - 1), (. - 0.5) * 2,
//   warp = grid_sample(d_ref, pixel, bilinear, border padding, corners aligned -- torch 1.1's default),
//   out = clamp(|warp - reproj| / reproj, 0, 1), NaN passed through as torch.clamp passes it.
// HBM-bound: 4 B read + 4 B written per pixel and a four-point gather from the reference depth.
#include "ops.h"

namespace dfvo {

struct DcCam {
    float K[9], Kinv[9], T[12];
};
struct alignas(16) DcF4 {
    float v[4];
};

__device__ __forceinline__ float dc_pixel(const DcCam& c, const float* __restrict__ ref, int H, int W, int x, int y, float d) {
    const float fx = (float)x, fy = (float)y;
    // backprojection.py:61-62
    const float px = (c.Kinv[0] * fx + c.Kinv[1] * fy + c.Kinv[2]) * d;
    const float py = (c.Kinv[3] * fx + c.Kinv[4] * fy + c.Kinv[5]) * d;
    const float pz = (c.Kinv[6] * fx + c.Kinv[7] * fy + c.Kinv[8]) * d;
    // depth_consistency.py:112 / transformation3d.py:31
    const float qx = c.T[0] * px + c.T[1] * py + c.T[2] * pz + c.T[3];
    const float qy = c.T[4] * px + c.T[5] * py + c.T[6] * pz + c.T[7];
    const float qz = c.T[8] * px + c.T[9] * py + c.T[10] * pz + c.T[11];
    const float reproj = qz;
    // projection.py:46-57
    const float u = c.K[0] * qx + c.K[1] * qy + c.K[2] * qz;
    const float v = c.K[3] * qx + c.K[4] * qy + c.K[5] * qz;
    const float wz = (c.K[6] * qx + c.K[7] * qy + c.K[8] * qz) + 1e-7f;
    const float gx = ((u / wz) / (float)(W - 1) - 0.5f) * 2.f;
    const float gy = ((v / wz) / (float)(H - 1) - 0.5f) * 2.f;
    // grid_sample: unnormalise with the corners aligned, clip to the border, bilinear
    float ix = ((gx + 1.f) / 2.f) * (float)(W - 1);
    float iy = ((gy + 1.f) / 2.f) * (float)(H - 1);
    float warp;
    if (ix != ix || iy != iy) {
        warp = ix + iy;  // a NaN coordinate: NaN weights on every corner
    } else {
        ix = ix < 0.f ? 0.f : (ix > (float)(W - 1) ? (float)(W - 1) : ix);
        iy = iy < 0.f ? 0.f : (iy > (float)(H - 1) ? (float)(H - 1) : iy);
        const float xw = floorf(ix), yn = floorf(iy);
        const int x0 = (int)xw, y0 = (int)yn;  // in [0, W - 1] x [0, H - 1] after the clip
        const float tw = ix - xw, te = 1.f - tw, tn = iy - yn, ts = 1.f - tn;
        const bool x1in = x0 + 1 < W, y1in = y0 + 1 < H;  // a corner beyond the border contributes nothing (its weight is 0)
        const float* r0 = ref + (size_t)y0 * W;
        const float* r1 = ref + (size_t)(y1in ? y0 + 1 : y0) * W;
        const int x1 = x1in ? x0 + 1 : x0;
        const float nw = r0[x0], ne = r0[x1], sw = r1[x0], se = r1[x1];
        warp = nw * (ts * te);
        if (x1in) warp += ne * (ts * tw);
        if (y1in) warp += sw * (tn * te);
        if (x1in && y1in) warp += se * (tn * tw);
    }
    const float r = fabsf(warp - reproj) / reproj;
    return r < 0.f ? 0.f : (r > 1.f ? 1.f : r);  // (comparisons, not fminf / fmaxf: NaN goes through)
}

// A lane owns one 16-byte-aligned quad of the flat output, clipped to ONE row (k_read_depth_u16's scheme: row starts are
// unaligned when W is no multiple of 4): four consecutive pixels of a row go out as one 16-byte store, a clipped quad -- a row's
// head or tail -- element by element.  G: quads a row can touch.
__global__ void __launch_bounds__(256) k_depth_consistency(const float* __restrict__ cur, const float* __restrict__ ref, int H, int W,
                                                           int G, DcCam cam, float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)H * G) return;
    const int y = (int)(t / G), g = (int)(t - (long long)y * G);
    const long long r0 = (long long)y * W;
    const long long q0 = ((r0 >> 2) + g) << 2;
    const long long lo = q0 > r0 ? q0 : r0, hi = q0 + 4 < r0 + W ? q0 + 4 : r0 + W;
    if (lo >= hi) return;
    const int n = (int)(hi - lo), xa = (int)(lo - r0);
    if (n == 4) {
        const DcF4 d = *reinterpret_cast<const DcF4*>(cur + lo);
        DcF4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o.v[i] = dc_pixel(cam, ref, H, W, xa + i, y, d.v[i]);
        *reinterpret_cast<DcF4*>(out + lo) = o;
    } else {
        for (int i = 0; i < n; ++i) out[lo + i] = dc_pixel(cam, ref, H, W, xa + i, y, cur[lo + i]);
    }
}

// The same lanes and stores with the pose in device memory (PoseNet's 4x4, written by k_pose_head earlier on the stream).  Every
// workgroup assembles the camera in LDS -- K and K^-1 from the kernel argument, whose T comes in unset, and the twelve pose values
// from T16 -- and every lane copies that struct whole before it does anything else.  The pose is another kernel's output and no
// launch constant: twelve lanes read it with relaxed atomic loads, which the compiler lowers to per-lane vector loads of global
// memory and never to the scalar-cache loads it selects for a uniform address behind a plain or `const __restrict__` pointer.
// The whole-struct copy is what keeps the arithmetic that of k_depth_consistency: under -ffp-contract=fast the compiler decides
// which product of a sum goes into an fma from how it packs the operands, and it packs a camera it copied as one aggregate as it
// packs the kernel argument, but not one whose T was assigned element by element (measured: identical on every pixel against
// one pixel in five off by an ulp or two; tests/test_pipeline_posenet_gpu.py holds it bit for bit).
__global__ void __launch_bounds__(256) k_depth_consistency_dev(const float* __restrict__ cur, const float* __restrict__ ref, int H, int W,
                                                               int G, DcCam cam, const float* T16, float* __restrict__ out) {
    __shared__ DcCam sc;
    if (threadIdx.x < 12)
        sc.T[threadIdx.x] = __hip_atomic_load(T16 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else if (threadIdx.x < 21)
        sc.K[threadIdx.x - 12] = cam.K[threadIdx.x - 12];
    else if (threadIdx.x < 30)
        sc.Kinv[threadIdx.x - 21] = cam.Kinv[threadIdx.x - 21];
    __syncthreads();  // (ahead of every return: all 256 lanes of the workgroup reach it)
    const DcCam c = sc;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)H * G) return;
    const int y = (int)(t / G), g = (int)(t - (long long)y * G);
    const long long r0 = (long long)y * W;
    const long long q0 = ((r0 >> 2) + g) << 2;
    const long long lo = q0 > r0 ? q0 : r0, hi = q0 + 4 < r0 + W ? q0 + 4 : r0 + W;
    if (lo >= hi) return;
    const int n = (int)(hi - lo), xa = (int)(lo - r0);
    if (n == 4) {
        const DcF4 d = *reinterpret_cast<const DcF4*>(cur + lo);
        DcF4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o.v[i] = dc_pixel(c, ref, H, W, xa + i, y, d.v[i]);
        *reinterpret_cast<DcF4*>(out + lo) = o;
    } else {
        for (int i = 0; i < n; ++i) out[lo + i] = dc_pixel(c, ref, H, W, xa + i, y, cur[lo + i]);
    }
}

int launch_depth_consistency_dev(const float* cur, const float* ref, int H, int W, const float* K9, const float* Kinv9,
                                 const float* d_T16, float* out, hipStream_t s) {
    DFVO_ARG_CHECK(cur && ref && out && K9 && Kinv9 && d_T16, "depth_consistency_dev: null argument");
    DFVO_ARG_CHECK(H >= 2 && W >= 2 && (long long)H * W < (1ll << 31), "depth_consistency_dev: the map must be at least 2 x 2");
    DFVO_ARG_CHECK(((uintptr_t)cur & 15) == 0 && ((uintptr_t)out & 15) == 0, "depth_consistency_dev: maps must be 16-byte aligned");
    DFVO_ARG_CHECK(((uintptr_t)d_T16 & 3) == 0, "depth_consistency_dev: the pose must be 4-byte aligned");
    DcCam cam;
    for (int i = 0; i < 9; ++i) cam.K[i] = K9[i], cam.Kinv[i] = Kinv9[i];
    for (int i = 0; i < 12; ++i) cam.T[i] = 0.f;
    const int G = (W + 3) / 4 + 1;
    const long long lanes = (long long)H * G;
    hipLaunchKernelGGL(k_depth_consistency_dev, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, cur, ref, H, W, G, cam, d_T16,
                       out);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

int launch_depth_consistency(const float* cur, const float* ref, int H, int W, const float* K9, const float* Kinv9, const float* T16,
                             float* out, hipStream_t s) {
    DFVO_ARG_CHECK(cur && ref && out && K9 && Kinv9 && T16, "depth_consistency: null argument");
    DFVO_ARG_CHECK(H >= 2 && W >= 2 && (long long)H * W < (1ll << 31), "depth_consistency: the map must be at least 2 x 2");
    DFVO_ARG_CHECK(((uintptr_t)cur & 15) == 0 && ((uintptr_t)out & 15) == 0, "depth_consistency: maps must be 16-byte aligned");
    DcCam cam;
    for (int i = 0; i < 9; ++i) cam.K[i] = K9[i], cam.Kinv[i] = Kinv9[i];
    for (int i = 0; i < 12; ++i) cam.T[i] = T16[i];
    const int G = (W + 3) / 4 + 1;
    const long long lanes = (long long)H * G;
    hipLaunchKernelGGL(k_depth_consistency, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, cur, ref, H, W, G, cam, out);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

}  // namespace dfvo
