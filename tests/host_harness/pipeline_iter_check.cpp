// Stand-alone check of the host-only half of dfvo_pipeline_set_iterative (df-vo_amd/csrc/pipeline_iter.h and, through it,
// pipeline_setup.h): the option block's refusals, the keypoint counts of the loop's scale stage, the rigid-flow keypoint
// configuration and the "not run" record.
// No HIP library: hip_stub.h stands in for the entry points the included headers name.  Built with
// -fsanitize=address,undefined and run by tests/test_pipeline_iter_host_cpu.py; exit status 0 = every check holds.
#include "hip_stub.h"

#include "../../df-vo_amd/csrc/pipeline_iter.h"

static dfvo_pipeline_iter_opts opts(int kp_src, int rows, int cols, int n, double rt, double ot) {
    dfvo_pipeline_iter_opts o = {};
    o.enable = 1, o.kp_src = kp_src, o.num_row = rows, o.num_col = cols, o.num_bestN = n, o.rigid_flow_thre = rt, o.optical_flow_thre = ot;
    return o;
}
static bool has(const char* msg, const char* word) { return msg && strstr(msg, word); }

int main() {
    arm(-1);  // (no allocation in here; none may fail)
    // tracked keypoints by source: local_bestN rounds down per cell, the others hand out their count
    CHECK(tracked_kp_max(DFVO_KP_SOURCE_LOCAL_BESTN, 1999, 2000, 10, 10) == 2000);
    CHECK(tracked_kp_max(DFVO_KP_SOURCE_LOCAL_BESTN, 1999, 2050, 10, 10) == 2000);
    CHECK(tracked_kp_max(DFVO_KP_SOURCE_LOCAL_BESTN, 1999, 777, 7, 9) == 12 * 63);
    CHECK(tracked_kp_max(DFVO_KP_SOURCE_LOCAL_BESTN, 1999, 99, 10, 10) == 0);
    CHECK(tracked_kp_max(DFVO_KP_SOURCE_LOCAL_BESTN, 1999, 2000, 0, 10) == 0);
    CHECK(tracked_kp_max(DFVO_KP_SOURCE_LOCAL_BESTN, 0, 2000000000, 40000, 40000) == 1600000000);  // (no int overflow in the cell count)
    CHECK(tracked_kp_max(DFVO_KP_SOURCE_BESTN, 1999, 777, 10, 10) == 777);
    CHECK(tracked_kp_max(DFVO_KP_SOURCE_SAMPLED, 1999, 777, 10, 10) == 1999);
    // the option block
    const double nan = std::nan("");
    CHECK(iter_opts_refusal(opts(DFVO_ITER_KP_DEPTH, 10, 10, 2000, 5, 0.1), 3) == nullptr);
    CHECK(iter_opts_refusal(opts(DFVO_ITER_KP_BEST, 1, 1, 1, -1, 0), 8) == nullptr);
    CHECK(has(iter_opts_refusal(opts(2, 10, 10, 2000, 5, 0.1), 3), "kp_src"));
    CHECK(has(iter_opts_refusal(opts(-1, 10, 10, 2000, 5, 0.1), 3), "kp_src"));
    CHECK(has(iter_opts_refusal(opts(0, 0, 10, 2000, 5, 0.1), 3), "positive"));
    CHECK(has(iter_opts_refusal(opts(0, 10, -3, 2000, 5, 0.1), 3), "positive"));
    CHECK(has(iter_opts_refusal(opts(0, 10, 10, 0, 5, 0.1), 3), "positive"));
    CHECK(has(iter_opts_refusal(opts(0, 10, 10, 2000, nan, 0.1), 3), "NaN"));
    CHECK(has(iter_opts_refusal(opts(0, 10, 10, 2000, 5, nan), 3), "NaN"));
    CHECK(has(iter_opts_refusal(opts(0, 10, 10, 2000, 5, 0.1), 0), "scale_min_samples"));
    CHECK(has(iter_opts_refusal(opts(0, 10, 10, 2000, 5, 0.1), 9), "scale_min_samples"));
    // the bound of the scale stage: the uniform set under kp_depth, the tracked set under kp_best
    CHECK(iter_kp_count_ok(DFVO_ITER_KP_DEPTH, ITER_MAX_KP, 1 << 30) && !iter_kp_count_ok(DFVO_ITER_KP_DEPTH, ITER_MAX_KP + 1, 0));
    CHECK(iter_kp_count_ok(DFVO_ITER_KP_BEST, 1 << 30, ITER_MAX_KP) && !iter_kp_count_ok(DFVO_ITER_KP_BEST, 0, ITER_MAX_KP + 1));
    // the launcher's configuration: float32 casts, K laid out row-major from fx fy cx cy, the inverse as given
    const double Kinv[9] = {1.0 / 3, 0, -0.1, 0, 1.0 / 7, -0.2, 0, 0, 1};
    const RigidKpConfig rc = iter_rigid_config(opts(DFVO_ITER_KP_BEST, 4, 6, 500, 0.1, 1e-6), 718.856, 719.5, 607.1928, 185.2157, Kinv);
    CHECK(rc.num_row == 4 && rc.num_col == 6 && rc.num_bestN == 500 && rc.score_rigid == 0);
    CHECK(rc.rigid_thre == (float)0.1 && rc.opt_thre == (float)1e-6);
    const float K[9] = {(float)718.856, 0, (float)607.1928, 0, (float)719.5, (float)185.2157, 0, 0, 1};
    for (int i = 0; i < 9; i++) CHECK(rc.K[i] == K[i] && rc.Kinv[i] == (float)Kinv[i]);
    for (int i = 0; i < 16; i++) CHECK(rc.T[i] == 0.f);
    // the record of a pair whose loop did not run
    IterCtl ctl;
    memset(&ctl, 0x5a, sizeof(ctl));
    iter_record_reset(&ctl);
    CHECK(ctl.status == ITER_NOT_RUN && ctl.done == 1 && ctl.n_iter == 0 && ctl.sel_round == -1 && ctl.scale == 0.0 && ctl.pad == 0);
    for (int r = 0; r < ITER_ROUNDS; r++) CHECK(ctl.n_kp[r] == -1 && ctl.scale_in[r] == 0.0 && ctl.scale_out[r] == 0.0);
    if (g_failed || g_allocs || g_hip_calls) return 1;
    printf("pipeline_iter: ok\n");
    return 0;
}
