// Host-only pieces of dfvo_pipeline_set_iterative (pipeline.hip): what the option block may hold, the keypoint counts the
// loop's scale stage can meet, the rigid-flow keypoint configuration built from the pipeline's intrinsics, and the record a
// pair leaves whose loop did not run.  No HIP call in here: tests/host_harness/pipeline_iter_check.cpp runs it on the CPU.
#pragma once
#include "../../include/dfvo_hip.h"
#include "tracker.h"

namespace dfvo {

// keypoints the pipeline's source hands to the trackers, at most
inline int tracked_kp_max(int kp_source, int kp_sampled_num, int kp_num_bestN, int kp_num_row, int kp_num_col) {
    if (kp_source == DFVO_KP_SOURCE_SAMPLED) return kp_sampled_num;
    if (kp_source == DFVO_KP_SOURCE_BESTN) return kp_num_bestN;
    const long long cells = (long long)kp_num_row * kp_num_col;
    return cells > 0 ? (int)((kp_num_bestN / cells) * cells) : 0;  // math.floor(N / (rows * cols)) per cell
}

// nullptr, or why dfvo_pipeline_set_iterative refuses the block (the launcher's own refusals come from rigid_flow_kp_geometry)
inline const char* iter_opts_refusal(const dfvo_pipeline_iter_opts& o, int scale_min_samples) {
    if (o.kp_src != DFVO_ITER_KP_DEPTH && o.kp_src != DFVO_ITER_KP_BEST)
        return "dfvo_pipeline_set_iterative: kp_src is DFVO_ITER_KP_DEPTH or DFVO_ITER_KP_BEST";
    if (!(o.num_row > 0 && o.num_col > 0 && o.num_bestN > 0))
        return "dfvo_pipeline_set_iterative: num_row, num_col, num_bestN are positive";
    if (o.rigid_flow_thre != o.rigid_flow_thre || o.optical_flow_thre != o.optical_flow_thre)
        return "dfvo_pipeline_set_iterative: a threshold is NaN";
    if (!(scale_min_samples >= 1 && scale_min_samples <= 8)) return "dfvo_pipeline_set_iterative: scale_min_samples in [1,8]";
    return nullptr;
}

// keypoints the scale stage of a round reads: that round's uniform set (at most n_sel) or the tracked set (at most n_trk)
inline bool iter_kp_count_ok(int kp_src, int n_sel, int n_trk) { return (kp_src == DFVO_ITER_KP_DEPTH ? n_sel : n_trk) <= ITER_MAX_KP; }

// kp_selection.rigid_flow_kp as the launchers take it: float32 thresholds and intrinsics (K from fx fy cx cy, its inverse as
// the caller computed it in float64 and cast, as the reference's RigidFlow layer receives them); T is not read by the loop
inline RigidKpConfig iter_rigid_config(const dfvo_pipeline_iter_opts& o, double fx, double fy, double cx, double cy, const double* Kinv) {
    RigidKpConfig rc = {};
    rc.num_row = o.num_row;
    rc.num_col = o.num_col;
    rc.num_bestN = o.num_bestN;
    rc.rigid_thre = (float)o.rigid_flow_thre;
    rc.opt_thre = (float)o.optical_flow_thre;
    rc.score_rigid = 0;  // (the loop reads the uniform set alone, which no score touches)
    const double K[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
    for (int i = 0; i < 9; i++) {
        rc.K[i] = (float)K[i];
        rc.Kinv[i] = (float)Kinv[i];
    }
    return rc;
}

// what dfvo_pipeline_get_iterative reports for a pair whose loop did not run
inline void iter_record_reset(IterCtl* ctl) {
    *ctl = IterCtl();
    ctl->done = 1;
    ctl->status = ITER_NOT_RUN;
    ctl->sel_round = -1;
    for (int r = 0; r < ITER_ROUNDS; ++r) ctl->n_kp[r] = -1;
}

}  // namespace dfvo
