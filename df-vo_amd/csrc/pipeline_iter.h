// Host-only pieces of dfvo_pipeline_set_iterative (pipeline_options.hip) beside pipeline_setup.h's rules: the rigid-flow keypoint
// configuration built from the pipeline's intrinsics, and the record a pair leaves whose loop did not run.  No HIP call in here:
// tests/host_harness/pipeline_iter_check.cpp runs it on the CPU.
#pragma once
#include "pipeline_setup.h"
#include "tracker.h"

namespace dfvo {

static_assert(SETUP_ITER_MAX_KP == ITER_MAX_KP, "pipeline_setup.h states the bound of k_scale_ratios");

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
