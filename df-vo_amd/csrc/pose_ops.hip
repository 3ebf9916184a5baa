// The pose net's two operators that are not convolutions: the two-frame input and the head behind PoseDecoder's last layer.
#include "ops.h"
#include "pose_math.h"

namespace dfvo {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// forward_pose (deep_models.py:217-225) + resnet_encoder.py:89: ToTensor of both frames, concatenated on the channel axis
// (image 0's RGB, then image 1's), every channel (v - 0.45) / 0.225; channels 6 and 7 are the zero padding of the NHWC8 input
__global__ void k_img2_u8_to_pose_input(const uint8_t* __restrict__ img0, const uint8_t* __restrict__ img1, int n,
                                        float* __restrict__ dst) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    float v[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c] = ((float)img0[(size_t)idx * 3 + c] / 255.f - 0.45f) / 0.225f;
        v[3 + c] = ((float)img1[(size_t)idx * 3 + c] / 255.f - 0.45f) / 0.225f;
    }
    f32x4* o = reinterpret_cast<f32x4*>(dst + (size_t)idx * 8);
    o[0] = f32x4{v[0], v[1], v[2], v[3]};
    o[1] = f32x4{v[4], v[5], 0.f, 0.f};
}

int launch_img2_u8_to_pose_input(const uint8_t* img0, const uint8_t* img1, int H, int W, float* dst, hipStream_t s) {
    const int n = H * W;
    hipLaunchKernelGGL(k_img2_u8_to_pose_input, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, img0, img1, n, dst);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

// pose_decoder.py:47-52 + monodepth2.py:97,118 in one workgroup of 16 rows x 16 channel lanes (12 used):
// out.mean(3).mean(2) -- every row's mean over the width first, then the mean of the row means over the height, both summed
// in index order --, x 0.01, frame 0's six values through pose_from_parameters.  map: [h, w, cs] floats, 12 channels used.
__global__ void __launch_bounds__(256) k_pose_head(const float* __restrict__ map, int h, int w, int cs, float mult,
                                                   float* __restrict__ pose16, float* __restrict__ params6) {
    __shared__ float row_mean[16][16];
    __shared__ float par[16];
    const int c = threadIdx.x & 15, r = threadIdx.x >> 4;
    float acc = 0.f;  // lanes r == 0: the sum of the row means
    for (int y0 = 0; y0 < h; y0 += 16) {
        const int y = y0 + r;
        float sum = 0.f;
        if (c < 12 && y < h) {
            const float* p = map + (size_t)y * w * cs + c;
            for (int x = 0; x < w; ++x) sum += p[(size_t)x * cs];
        }
        row_mean[r][c] = sum / (float)w;
        __syncthreads();
        if (r == 0) {
            const int rows = min(16, h - y0);
            for (int i = 0; i < rows; ++i) acc += row_mean[i][c];
        }
        __syncthreads();
    }
    if (r == 0) par[c] = 0.01f * (acc / (float)h);
    __syncthreads();
    if (threadIdx.x == 0) {
        float p[6], M[16];
        for (int i = 0; i < 6; ++i) p[i] = par[i];
        pose_from_parameters(p, mult, M);
        for (int i = 0; i < 16; ++i) pose16[i] = M[i];
        if (params6)
            for (int i = 0; i < 6; ++i) params6[i] = p[i];
    }
}

int launch_pose_head(const float* map, int h, int w, int cs, float mult, float* pose16, float* params6, hipStream_t s) {
    DFVO_ARG_CHECK(map && pose16 && h >= 1 && w >= 1 && cs >= 12, "pose_head: bad argument");
    hipLaunchKernelGGL(k_pose_head, dim3(1), dim3(256), 0, s, map, h, w, cs, mult, pose16, params6);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

}  // namespace dfvo
