// The opaque handle types of include/dfvo_hip.h, shared by the translation units of the extern "C" surface
// (capi.hip: nets and operators, capi_tracker.hip: solvers, session.hip: the frame session under the drop-in classes).
#pragma once
#include "../../include/dfvo_hip.h"
#include "nets.h"
#include "resize_lanczos.h"
#include "solver.h"
#include "tracker.h"

struct dfvo_flownet {
    dfvo::FlowNet net;
};
struct dfvo_depthnet {
    dfvo::DepthNet net;
    dfvo::LanczosResizer resize;  // dfvo_depthnet_forward_image_host / the session: tables for the last image size seen
    dfvo::DevArr<uint8_t> img_full;  // the full-size frame of dfvo_depthnet_forward_image_host, grown on demand
};
struct dfvo_posenet {
    dfvo::PoseNet net;
    dfvo::LanczosResizer resize;     // dfvo_posenet_forward_images_host: tables for the last image size seen
    dfvo::DevArr<uint8_t> img_full;  // its two full-size frames, grown on demand
};
struct dfvo_tracker {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    dfvo::TrackerBuffers tb;
    dfvo::RigidKpBuffers rigid;
    dfvo::BestNBuffers bestn;
    dfvo::RansacWorkspace& ws = tb.ws_e;
    // staging of the host-array entry points, grown on demand (capi_tracker.hip: stage_flow, stage_depth)
    dfvo::DevArr<float> d_flow, d_diff;  // [2][px], [px]
    dfvo::DevArr<float> d_depth_diff;    // [px], dfvo_kp_local_bestn_depth
    dfvo::DevArr<double> d_depth;
    dfvo::DevArr<double> d_small;        // 64 doubles
    dfvo::DevArr<double> d_x1, d_x2, d_X4;
    hipEvent_t ev_iter[2] = {nullptr, nullptr};  // around the rounds of dfvo_scale_recovery_iterative (created on first use)
    dfvo::PinnedArr<unsigned char> h_iter;  // results of dfvo_scale_recovery_iterative: IterCtl | RandomState | keypoints
    dfvo::PnpBuffers pnp;
};


// internal helpers of capi_tracker.hip used by session.hip
int dfvo_pose_config_from(const dfvo_pose2d2d_cfg* cfg, dfvo::PoseConfig* pc);
int dfvo_pose_fetch(dfvo_tracker* t, int n, const dfvo_pose2d2d_cfg* cfg, dfvo_pose2d2d_out* out, uint8_t* h_inliers);
