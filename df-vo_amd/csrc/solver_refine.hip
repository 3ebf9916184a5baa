// The trackers' iterative keypoint refinement: the device-side hand-over between a first pass and the second pass on kp_depth.
// Reference call sites (paths relative to /root/reference):
//   libs/dfvo.py:194-222, 236-244                 the second E pass / scale stage / PnP pass
//   libs/tracker/E_tracker.py:422-440             compute_rigid_flow_kp: rigid_flow_pose = inv(hybrid_pose)
//   libs/tracker/pnp_tracker.py:112-118, 127-145  pose = inv([Rodrigues(r) | t]); rigid_flow_pose = inv(pose)
// One-lane kernels: each reads the first pass's results where the chain left them, so no host wait sits between a pass and the
// selection behind it.  See tracker.h on sequential semantics.  Built with -ffp-contract=off.
#include "np_legacy.h"  // sm::rigid_pose_inv_f32, sm::rigid_pose_f32
#include "tracker.h"

namespace dfvo {

struct RefineMats {
    float Kinv[9], K[9];
};

__device__ void refine_begin(IterCtl* __restrict__ ctl, bool gated, int* __restrict__ kp_info2) {
    *ctl = IterCtl();
    ctl->done = gated ? 1 : 0;
    ctl->status = gated ? ITER_NOT_RUN : ITER_RUNNING;
    ctl->sel_round = -1;
    if (gated) kp_info2[0] = kp_info2[1] = kp_info2[2] = 0;
}

// dfvo.py:195-200: hybrid_pose = [R_E | t_E * scale], its translation left zero when the scale is -1
__global__ void k_refine_e_mats(const PoseState* __restrict__ ps, const ScaleResult* __restrict__ sr, RefineMats m,
                                float* __restrict__ mats /*Kinv[9] | T[16] | K[9]*/, IterCtl* __restrict__ ctl,
                                int* __restrict__ kp_info2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool gated = ps->t[0] == 0 && ps->t[1] == 0 && ps->t[2] == 0;
    refine_begin(ctl, gated, kp_info2);
    if (gated) return;
    double E[16];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) E[r * 4 + c] = ps->R[r * 3 + c];
        E[r * 4 + 3] = ps->t[r];
    }
    E[12] = E[13] = E[14] = 0.0;
    E[15] = 1.0;
    const double scale = sr->scale;
    ctl->scale = scale;
    for (int i = 0; i < 9; ++i) {
        mats[i] = m.Kinv[i];
        mats[25 + i] = m.K[i];
    }
    sm::rigid_pose_inv_f32(E, scale == -1.0 ? 0.0 : scale, mats + 9);
}

__global__ void k_refine_pnp_mats(const PnpResult* __restrict__ pr, RefineMats m, float* __restrict__ mats, IterCtl* __restrict__ ctl,
                                  int* __restrict__ kp_info2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    refine_begin(ctl, false, kp_info2);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0};
    for (int i = 0; i < 9; ++i) {
        mats[i] = m.Kinv[i];
        mats[25 + i] = m.K[i];
    }
    if (pr->found)
        sm::rigid_pose_f32(pr->R, pr->tvec, mats + 9);
    else
        sm::rigid_pose_f32(I, z, mats + 9);
}

__global__ void k_refine_final(const PoseState* __restrict__ p1, const ScaleResult* __restrict__ s1, const PoseState* __restrict__ p2,
                               const ScaleResult* __restrict__ s2, int scale_enable, RefineFinal* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    (void)p1;
    for (int i = 0; i < 9; ++i) out->R[i] = p2->R[i];
    for (int i = 0; i < 3; ++i) out->t[i] = p2->t[i];
    const bool t2_zero = p2->t[0] == 0 && p2->t[1] == 0 && p2->t[2] == 0;
    double scale = s1->scale;
    const bool scale_ran = scale_enable && !t2_zero;
    out->scale2 = 0.0;
    if (scale_ran) scale = out->scale2 = s2->scale;
    out->scale = scale;
    out->t2_zero = t2_zero ? 1 : 0;
    out->scale_ran = scale_ran ? 1 : 0;
    out->needs_pnp = (t2_zero || scale == -1.0) ? 1 : 0;
    out->pad = 0;
}

static RefineMats refine_mats(const RigidKpConfig& cfg) {
    RefineMats m;
    for (int i = 0; i < 9; ++i) m.Kinv[i] = cfg.Kinv[i], m.K[i] = cfg.K[i];
    return m;
}

int enqueue_refine_e_mats(RigidKpBuffers& rb, const PoseState* d_pose, const ScaleResult* d_scale, const RigidKpConfig& cfg,
                          int* d_kp_info2, hipStream_t s) {
    DFVO_ARG_CHECK(rb.mats && rb.ctl && d_pose && d_scale && d_kp_info2, "refine_e_mats: bad argument");
    hipLaunchKernelGGL(k_refine_e_mats, dim3(1), dim3(64), 0, s, d_pose, d_scale, refine_mats(cfg), rb.mats.p, rb.ctl.p, d_kp_info2);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

int enqueue_refine_pnp_mats(RigidKpBuffers& rb, const PnpResult* d_pnp, const RigidKpConfig& cfg, int* d_kp_info2, hipStream_t s) {
    DFVO_ARG_CHECK(rb.mats && rb.ctl && d_pnp && d_kp_info2, "refine_pnp_mats: bad argument");
    hipLaunchKernelGGL(k_refine_pnp_mats, dim3(1), dim3(64), 0, s, d_pnp, refine_mats(cfg), rb.mats.p, rb.ctl.p, d_kp_info2);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

int enqueue_refine_final(const PoseState* d_pose1, const ScaleResult* d_scale1, const PoseState* d_pose2, const ScaleResult* d_scale2,
                         int scale_enable, RefineFinal* d_out, hipStream_t s) {
    DFVO_ARG_CHECK(d_pose1 && d_scale1 && d_pose2 && d_scale2 && d_out, "refine_final: bad argument");
    hipLaunchKernelGGL(k_refine_final, dim3(1), dim3(64), 0, s, d_pose1, d_scale1, d_pose2, d_scale2, scale_enable, d_out);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

}  // namespace dfvo
