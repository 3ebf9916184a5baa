// The pose net's 6 -> 4x4 arithmetic: monodepth2's transformation_from_parameters(axisangle, translation, invert=True)
// (layers.py:28-104) in float32, operation by operation.  Host and device: k_pose_head (pose_ops.hip) runs it on one lane,
// tests/host_harness/pose_math_check.cpp on the CPU.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define DFVO_POSE_HD __host__ __device__
#else
#define DFVO_POSE_HD
#endif

namespace dfvo {

// p: axis-angle (3), translation (3); M: row-major 4x4 = R^T . T(-t); the translation column is multiplied by `mult`
// (Monodepth2PoseNet.inference_pose: pose[:, :3, 3] *= stereo_baseline_multiplier)
DFVO_POSE_HD inline void pose_from_parameters(const float p[6], float mult, float M[16]) {
    // rot_from_axisangle: axis = vec / (angle + 1e-7) -- the zero vector gives the zero axis and R = I
    const float angle = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    const float d = angle + 1e-7f;
    const float x = p[0] / d, y = p[1] / d, z = p[2] / d;
    const float ca = cosf(angle), sa = sinf(angle);
    const float C = 1.f - ca;
    const float xs = x * sa, ys = y * sa, zs = z * sa;
    const float xC = x * C, yC = y * C, zC = z * C;
    const float xyC = x * yC, yzC = y * zC, zxC = z * xC;
    float R[9];
    R[0] = x * xC + ca;
    R[1] = xyC - zs;
    R[2] = zxC + ys;
    R[3] = xyC + zs;
    R[4] = y * yC + ca;
    R[5] = yzC - xs;
    R[6] = zxC - ys;
    R[7] = yzC + xs;
    R[8] = z * zC + ca;
    const float t[3] = {-p[3], -p[4], -p[5]};
    for (int i = 0; i < 3; ++i) {
        // row i of R^T is column i of R; the matmul's fourth term is R^T[i][3] * 1 = 0
        const float r0 = R[i], r1 = R[3 + i], r2 = R[6 + i];
        M[4 * i + 0] = r0;
        M[4 * i + 1] = r1;
        M[4 * i + 2] = r2;
        M[4 * i + 3] = (r0 * t[0] + r1 * t[1] + r2 * t[2]) * mult;
    }
    M[12] = M[13] = M[14] = 0.f;
    M[15] = 1.f;
}

}  // namespace dfvo
