// Fused pipeline (pipeline_state.h): a pair's solver stage (pre-part, track_begin's chain, track_end) and the slot getters.
#include "pipeline_state.h"

// DFVO_TRACK_TRACE (tuning aid): per 20 pairs, the device time of the chain's three segments and track_end's host-side phases
struct TrackTrace {
    using Clock = std::chrono::steady_clock;
    static double ms_since(Clock::time_point a) { return std::chrono::duration<double, std::milli>(Clock::now() - a).count(); }
    static TrackTrace& get() { static TrackTrace t; return t; }
    const bool on = getenv("DFVO_TRACK_TRACE") != nullptr;
    double acc[2] = {0, 0}, dev[3] = {0, 0, 0};
    int dev_n = 0, n = 0;

    // track_begin: the events the chain's launchers record between its segments
    int begin(TrackerBuffers& tb) const {
        if (on && !tb.ev_t[0])
            for (int i = 0; i < 4; i++) DFVO_HIP_CHECK(hipEventCreate(&tb.ev_t[i]));
        return DFVO_OK;
    }
    // track_end of a pair with n_kp keypoints that took the E path: entered at t0, waited wait_ms for the chain
    void end_pair(const TrackerBuffers& tb, int n_kp, Clock::time_point t0, double wait_ms) {
        if (!on) return;
        float d[3] = {0, 0, 0};  // device time of the chain's three segments (valid when the pair took the E path)
        bool ok = n_kp > 10;
        for (int i = 0; i < 3 && ok; i++) ok = hipEventElapsedTime(&d[i], tb.ev_t[i], tb.ev_t[i + 1]) == hipSuccess;
        for (int i = 0; i < 3 && ok; i++) dev[i] += d[i];
        dev_n += ok;
        if (dev_n == 20) {
            fprintf(stderr, "track device ms: shuffles + five-point batch %.3f | bookkeeping + recoverPose %.3f | scale %.3f\n",
                    dev[0] / 20, dev[1] / 20, dev[2] / 20);
            dev[0] = dev[1] = dev[2] = 0;
            dev_n = 0;
        }
        acc[0] += wait_ms;
        acc[1] += ms_since(t0);
        if (++n % 20 == 0) {
            fprintf(stderr, "track_end host ms: waited for the chain %.3f | total %.3f\n", acc[0] / 20, acc[1] / 20);
            acc[0] = acc[1] = 0;
        }
    }
};

static void fill_pnp_out(const PnpResult& pr, dfvo_track_out* out) {
    for (int i = 0; i < 9; i++) out->R[i] = pr.R[i];
    for (int i = 0; i < 3; i++) out->t[i] = pr.tvec[i];
    out->scale = 1.0;
    out->pnp_found = pr.found;
    out->pnp_inliers = pr.best_inliers;
    out->pnp_n_filtered = pr.n_filtered;
    out->status = DFVO_TRACK_PNP;
}

// dfvo.py:225-250: PnP on (ref keypoints + ref depth) -> cur keypoints, on the chain's stream; p->pnp.result behind it.  The
// reference depth is ordered on that stream by set_ref_depth / the previous pair's roll-over
static int enqueue_pnp(dfvo_pipeline* p, Slot& sl, int n) {
    TrackerBuffers& tb = sl.tb;
    return enqueue_compute_pose_3d2d(p->pnp, tb.mt_state, tb.kp_ref, tb.kp_cur, tb.kp_info, n, p->ref_depth, p->H, p->W, p->pnp_cfg, p->s_trk());
}

// RNG-independent half of the solver stage of `slot` (keypoint selection, homography RANSAC + refinement, GRIC-H):
// waits on the device for the slot's flow outputs and runs on a stream of its own, so it executes as soon as those
// nets are done -- typically while dfvo_pipeline_track of the previous pair is still blocking the host.  The numpy
// RandomState is not touched here; all RNG consumers stay in dfvo_pipeline_track, in pair order.
static int enqueue_pre_part(dfvo_pipeline* p, int slot, const float* d_flow_override, const float* d_diff_override,
                            hipStream_t sp) {
    const dfvo_pipeline_cfg& c = p->cfg;
    const dfvo_pipeline_opts& o = p->opts;
    Slot& sl = p->slots[slot];
    TrackerBuffers& tb = sl.tb;
    DFVO_HIP_CHECK(hipStreamWaitEvent(sp, sl.e_flow, 0));
    const float* flow = d_flow_override ? d_flow_override : sl.fwd.p;
    const float* diff = d_diff_override ? d_diff_override : sl.diff.p;
    sl.flow_in = flow;
    sl.diff_in = diff;
    // the keypoint stage by source; each leaves tb.kp_ref / tb.kp_cur / tb.kp_info = [n, good_kp_found, ..] behind on sp
    if (o.kp_source == DFVO_KP_SOURCE_BESTN) {
        DFVO_TRY(enqueue_bestn_flow_kp(sl.bestn, flow, diff, p->H, p->W, c.kp_num_bestN, sp, tb.kp_ref, tb.kp_cur, tb.kp_info));
    } else if (o.kp_source == DFVO_KP_SOURCE_SAMPLED) {
        DFVO_TRY(enqueue_kp_sampled(flow, p->H, p->W, p->sample_crop[0], p->sample_crop[1], p->sample_crop[2], p->sample_crop[3],
                                 p->d_samples, o.kp_sampled_num, tb.kp_ref, tb.kp_cur, sp, tb.kp_info));
    } else {
        // the depth mask (kp_selection.py:118-119,145-148): the slot's map, written by the pose lane ahead of e_depth
        const bool mask = p->pose.depth_consistency != 0;
        if (mask) DFVO_HIP_CHECK(hipStreamWaitEvent(sp, sl.e_depth, 0));
        DFVO_TRY(enqueue_local_bestn(tb, flow, diff, p->H, p->W, c.kp_num_row, c.kp_num_col, c.kp_num_bestN, (float)c.kp_thre, sp,
                                  o.kp_score_method, mask ? sl.depth_diff.p : nullptr, mask ? p->pose.depth_thre : 0.f));
    }
    DFVO_HIP_CHECK(hipMemcpyAsync(sl.h_info, tb.kp_info, 3 * sizeof(int), hipMemcpyDeviceToHost, sp));
    DFVO_HIP_CHECK(hipEventRecord(sl.e_pre, sp));  // the host only needs the keypoint count; tb.ev_h orders the rest
    if (o.tracking_method == DFVO_TRACKING_PNP) {
        // dfvo.py:165: no E-tracker at all.  The inlier mask stays what dfvo_pipeline_get_keypoints documents for a pair
        // the E-tracker did not see: all ones
        DFVO_HIP_CHECK(hipMemsetAsync(tb.best_inliers, 1, (size_t)tb.kp_cap, sp));
        return DFVO_OK;
    }
    return enqueue_pose_h_part(tb, tb.kp_cap, p->pose_cfg, sp);  // keypoint count read on the device; kp_cap bounds the launches
}

extern "C" {

int dfvo_pipeline_prefetch_track(dfvo_pipeline* p, int slot, const float* d_flow_override, const float* d_diff_override) {
    DFVO_ARG_CHECK(p && slot_ok(slot), "dfvo_pipeline_prefetch_track: bad argument");
    if (deep_pose_tracking(p)) return DFVO_OK;  // no keypoint stage: nothing to run ahead
    DFVO_ARG_CHECK(!p->slots[slot].prefetched, "dfvo_pipeline_prefetch_track: slot already prefetched and not yet tracked");
    DFVO_TRY(enqueue_pre_part(p, slot, d_flow_override, d_diff_override, p->s_pre(slot)));
    p->slots[slot].prefetched = true;
    return DFVO_OK;
}

// First half of dfvo_pipeline_track: waits for the slot's keypoint stage, enqueues the RandomState-ordered chain (shuffles,
// 5 x five-point RANSAC, GRIC, recoverPose, scale recovery) and the copy of its results into pinned host memory, returns.
// The host is then free to enqueue the next pairs' nets while the chain runs (dfvo_pipeline_track_end collects).
int dfvo_pipeline_track_begin(dfvo_pipeline* p, int slot, const float* d_flow_override, const float* d_diff_override,
                              const double* d_depth_override) {
    DFVO_ARG_CHECK(p && slot_ok(slot), "dfvo_pipeline_track_begin: bad argument");
    DFVO_ARG_CHECK(p->slots[slot].begun == IDLE, "dfvo_pipeline_track_begin: the slot's previous pair was not collected (track_end)");
    DFVO_ARG_CHECK(p->pending_slot == -1, "dfvo_pipeline_track_begin: another pair is begun and not yet collected -- the PnP decision "
                                          "of track_end (RandomState draws) comes before the next pair's chain");
    hipStream_t s = p->s_trk();
    Slot& sl = p->slots[slot];
    TrackerBuffers& tb = sl.tb;
    DFVO_TRY(TrackTrace::get().begin(tb));
    auto begun = [&](Begun b) {  // the pair is pending from here on
        sl.begun = b;
        p->pending_slot = slot;
        return DFVO_OK;
    };
    if (deep_pose_tracking(p)) {
        // dfvo.py:252-255: the pair's motion is the pose net's matrix.  No keypoints, no RandomState draw; the 16 floats go to
        // pinned memory behind the pose lane
        DFVO_HIP_CHECK(hipStreamWaitEvent(s, sl.e_depth, 0));
        DFVO_HIP_CHECK(hipMemcpyAsync(sl.h_pose.p, sl.pose16, 16 * sizeof(float), hipMemcpyDeviceToHost, s));
        DFVO_HIP_CHECK(hipEventRecord(sl.e_res, s));
        sl.depth_override = nullptr;
        sl.n = 0;
        return begun(CHAIN_ENQUEUED);
    }
    const bool pnp_only = p->opts.tracking_method == DFVO_TRACKING_PNP;
    const bool iterative = p->iter.enable && !pnp_only;
    // side stream: the scale stage's fills leave the dependent chain (the iterative loop clears the map itself, every round)
    if (!pnp_only && !iterative) DFVO_TRY(enqueue_scale_prepare(tb, p->H, p->W));
    if (iterative) iter_record_reset(sl.h_iter);  // (the slot is idle: its last record was copied long ago)
    // A pre-part nobody prefetched: in the lane layout it goes onto the chain's lane (s), whose next work needs it anyway --
    // the depth lane may already hold later pairs' nets, and it would run behind them
    if (!sl.prefetched)
        DFVO_TRY(enqueue_pre_part(p, slot, d_flow_override, d_diff_override, p->plan.layout == LAYOUT_LANES ? s : p->s_pre(slot)));
    sl.prefetched = false;
    DFVO_HIP_CHECK(hipEventSynchronize(sl.e_pre));  // keypoint info is in pinned host memory now
    const int* info = sl.h_info;
    sl.depth_override = d_depth_override;
    if (!info[1]) return begun(NO_KEYPOINTS);
    const int n = sl.n = info[0];
    if (pnp_only) {
        // dfvo.py:225-250 on every pair: E_pose stays SE3(), so the only RandomState draws of the pair are PnP's shuffles.
        // The keypoint stage is complete (the host waited for e_pre above)
        if (!p->has_ref_depth) return begun(NO_REF_DEPTH);
        DFVO_TRY(enqueue_pnp(p, sl, n));
        DFVO_HIP_CHECK(hipMemcpyAsync(&sl.h_res.p->pnp, p->pnp.result, sizeof(PnpResult), hipMemcpyDeviceToHost, s));
        DFVO_HIP_CHECK(hipEventRecord(sl.e_res, s));
        return begun(CHAIN_ENQUEUED);
    }
    // waits for tb.ev_h (the prefetched half) on the device
    DFVO_TRY(enqueue_pose_e_part(tb, n, p->pose_cfg, s, p->d_T21, iterative ? p->d_E_pose.p : nullptr));
    DFVO_HIP_CHECK(hipStreamWaitEvent(s, sl.e_depth, 0));
    const double* depth = d_depth_override ? d_depth_override : sl.proc_depth.p;
    if (iterative) {
        // E_tracker.py:509-569, all rounds, gated and started from prev_scale on the device; p->ref_raw is ordered on s by
        // set_ref_* / the previous pair's roll-over, like the reference depth
        IterDevice dev;
        dev.prev_scale = p->d_prev_scale;
        dev.gate = tb.pose;
        DFVO_TRY(enqueue_scale_recovery_iterative(tb, sl.rigid, sl.flow_in, sl.diff_in, p->ref_raw, depth, p->H, p->W, p->iter_cfg,
                                               p->scale_cfg, p->d_E_pose, p->d_T21, 0.0, p->iter.kp_src, n, s, &dev));
        DFVO_HIP_CHECK(hipMemcpyAsync(sl.h_iter.p, sl.rigid.ctl, sizeof(IterCtl), hipMemcpyDeviceToHost, s));
    } else {
        DFVO_TRY(enqueue_find_scale(tb, n, p->d_T21, depth, p->H, p->W, p->scale_cfg, s, tb.pose, true));
    }
    if (tb.ev_t[3]) DFVO_HIP_CHECK(hipEventRecord(tb.ev_t[3], s));
    DFVO_HIP_CHECK(hipMemcpyAsync(&sl.h_res.p->pose, tb.pose, sizeof(PoseState), hipMemcpyDeviceToHost, s));
    DFVO_HIP_CHECK(hipMemcpyAsync(&sl.h_res.p->scale, tb.scale_out, sizeof(ScaleResult), hipMemcpyDeviceToHost, s));
    DFVO_HIP_CHECK(hipEventRecord(sl.e_res, s));
    return begun(CHAIN_ENQUEUED);
}

// Second half: waits for the chain's results, runs the PnP fallback where the reference takes it (dfvo.py:225-250; decided
// on the host, so the NEXT pair's chain must not be begun before this returns -- it consumes the same RandomState), rolls
// the reference depth over.
int dfvo_pipeline_track_end(dfvo_pipeline* p, int slot, dfvo_track_out* out) {
    DFVO_ARG_CHECK(p && out && slot_ok(slot), "dfvo_pipeline_track_end: bad argument");
    DFVO_ARG_CHECK(p->slots[slot].begun != IDLE, "dfvo_pipeline_track_end: no pair pending in this slot (track_begin)");
    hipStream_t s = p->s_trk();
    Slot& sl = p->slots[slot];
    const auto t0 = TrackTrace::Clock::now();
    const Begun begun = sl.begun;
    const int n = sl.n;
    const double* d_depth_override = sl.depth_override;
    sl.begun = IDLE;
    p->pending_slot = -1;
    sl.pose_override = nullptr;  // (held for the pair that ends here)
    memset(out, 0, sizeof(*out));
    for (int i = 0; i < 3; i++) out->R[i * 4] = 1.0;
    if (deep_pose_tracking(p)) {
        DFVO_HIP_CHECK(hipEventSynchronize(sl.e_res));
        const float* T = sl.h_pose.p;  // row-major 4x4; float32 -> double is exact
        for (int r = 0; r < 3; r++) {
            for (int q = 0; q < 3; q++) out->R[r * 3 + q] = (double)T[r * 4 + q];
            out->t[r] = (double)T[r * 4 + 3];
        }
        out->scale = 1.0;
        out->status = DFVO_TRACK_DEEP_POSE;
        return DFVO_OK;  // (no depth to roll over: none was computed)
    }
    const int* info = sl.h_info;
    out->n_kp = info[0];
    out->good_kp_found = info[1];
    if (begun == NO_KEYPOINTS) {
        out->status = DFVO_TRACK_CONSTANT_MOTION;
        DFVO_TRY(roll_ref_depth(p, slot, d_depth_override));
        DFVO_HIP_CHECK(hipStreamSynchronize(s));
        return DFVO_OK;
    }
    if (p->opts.tracking_method == DFVO_TRACKING_PNP) {
        // the PnP chain was enqueued by track_begin: nothing to decide here, only its result to wait for
        out->status = DFVO_TRACK_NEEDS_PNP;
        if (begun != NO_REF_DEPTH) {
            DFVO_HIP_CHECK(hipEventSynchronize(sl.e_res));
            const PnpResult pr = sl.h_res.p->pnp;
            DFVO_ARG_CHECK(pr.status >= 0, "dfvo_pipeline_track: the PnP tracker reported an internal error");
            fill_pnp_out(pr, out);
        }
        return roll_ref_depth(p, slot, d_depth_override);
    }
    DFVO_HIP_CHECK(hipEventSynchronize(sl.e_res));
    const double wait_ms = TrackTrace::ms_since(t0);
    const PoseState ps = sl.h_res.p->pose;
    const ScaleResult sr = sl.h_res.p->scale;
    for (int i = 0; i < 9; i++) out->R[i] = ps.R[i];
    for (int i = 0; i < 3; i++) out->t[i] = ps.t[i];
    out->best_inlier_cnt = ps.best_cnt;
    out->num_valid = ps.num_valid;
    out->cheirality = ps.cheirality;
    const bool t_zero = ps.t[0] == 0 && ps.t[1] == 0 && ps.t[2] == 0;
    double scale = sr.scale;
    if (p->iter.enable) {
        const IterCtl ctl = *sl.h_iter.p;
        scale = ctl.scale;  // the last completed round's
        if (!t_zero && (ctl.status == ITER_EMPTY || ctl.status == ITER_NO_CONSENSUS)) {
            // where the reference raises: the pair is over (the slot idle, nothing pending, the depths rolled over), the
            // RandomState and prev_scale hold what the reference had at the raise, `out` the E-tracker's pose
            out->scale = ctl.n_iter > 0 ? scale : 0.0;
            out->status = DFVO_TRACK_E;
            DFVO_TRY(roll_ref_depth(p, slot, d_depth_override));
            if (ctl.status == ITER_EMPTY) {
                dfvo::set_last_error("dfvo_pipeline_track_end: sampling threshold is too small (no rigid-flow keypoint selected)");
                return DFVO_ERR_EMPTY_SELECTION;
            }
            dfvo::set_last_error("dfvo_pipeline_track_end: RANSAC could not find a valid consensus set");
            return DFVO_ERR_NO_CONSENSUS;
        }
    }
    out->scale = t_zero ? 0.0 : scale;  // dfvo.py:198: scale recovery only when ||t|| != 0
    out->scale_n_valid = sr.n_valid;
    out->scale_n_trials = sr.n_trials;
    out->scale_n_inliers = sr.n_inliers;
    if (t_zero || scale == -1.0) {  // the PnP fallback
        out->status = DFVO_TRACK_NEEDS_PNP;
        if (p->has_ref_depth) {
            DFVO_TRY(enqueue_pnp(p, sl, n));
            PnpResult pr;
            DFVO_HIP_CHECK(hipMemcpyAsync(&pr, p->pnp.result, sizeof(pr), hipMemcpyDeviceToHost, s));
            DFVO_HIP_CHECK(hipStreamSynchronize(s));
            DFVO_ARG_CHECK(pr.status >= 0, "dfvo_pipeline_track: the PnP fallback reported an internal error");
            fill_pnp_out(pr, out);
        }
    } else {
        out->status = DFVO_TRACK_E;
    }
    // the roll-over copy is ordered on s_trk ahead of anything the next pair enqueues there: no host wait needed
    DFVO_TRY(roll_ref_depth(p, slot, d_depth_override));
    TrackTrace::get().end_pair(sl.tb, n, t0, wait_ms);
    return DFVO_OK;
}

int dfvo_pipeline_track(dfvo_pipeline* p, int slot, const float* d_flow_override, const float* d_diff_override,
                        const double* d_depth_override, dfvo_track_out* out) {
    DFVO_ARG_CHECK(p && out && slot_ok(slot), "dfvo_pipeline_track: bad argument");
    DFVO_TRY(dfvo_pipeline_track_begin(p, slot, d_flow_override, d_diff_override, d_depth_override));
    const int rc_end = dfvo_pipeline_track_end(p, slot, out);
    if (rc_end != DFVO_OK && rc_end != DFVO_ERR_EMPTY_SELECTION && rc_end != DFVO_ERR_NO_CONSENSUS) return rc_end;
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk()));  // (synchronous, as documented: the roll-over copy included)
    return rc_end;
}

int dfvo_pipeline_get_flow(dfvo_pipeline* p, int slot, float* h_fwd, float* h_bwd, float* h_diff, float* h_raw_depth,
                           double* h_depth) {
    DFVO_ARG_CHECK(p && slot_ok(slot), "dfvo_pipeline_get_flow: bad argument");
    DFVO_ARG_CHECK(!deep_pose_tracking(p), "dfvo_pipeline_get_flow: tracking_method DFVO_TRACKING_DEEP_POSE runs neither the flow net "
                                           "nor the depth net: there are no outputs");
    const size_t px = (size_t)p->H * p->W;
    const Slot& sl = p->slots[slot];
    DFVO_HIP_CHECK(hipDeviceSynchronize());
    if (h_fwd) DFVO_HIP_CHECK(hipMemcpy(h_fwd, sl.fwd, 2 * px * sizeof(float), hipMemcpyDeviceToHost));
    if (h_bwd) DFVO_HIP_CHECK(hipMemcpy(h_bwd, sl.bwd, 2 * px * sizeof(float), hipMemcpyDeviceToHost));
    if (h_diff) DFVO_HIP_CHECK(hipMemcpy(h_diff, sl.diff, px * sizeof(float), hipMemcpyDeviceToHost));
    if (h_raw_depth) DFVO_HIP_CHECK(hipMemcpy(h_raw_depth, sl.raw_depth, px * sizeof(float), hipMemcpyDeviceToHost));
    if (h_depth) DFVO_HIP_CHECK(hipMemcpy(h_depth, sl.proc_depth, px * sizeof(double), hipMemcpyDeviceToHost));
    return DFVO_OK;
}

int dfvo_pipeline_get_ref_depth(dfvo_pipeline* p, float* h_raw_depth, double* h_depth) {
    DFVO_ARG_CHECK(p, "dfvo_pipeline_get_ref_depth: null pipeline");
    const size_t px = (size_t)p->H * p->W;
    DFVO_HIP_CHECK(hipDeviceSynchronize());
    if (h_raw_depth) DFVO_HIP_CHECK(hipMemcpy(h_raw_depth, p->ref_raw, px * sizeof(float), hipMemcpyDeviceToHost));
    if (h_depth) DFVO_HIP_CHECK(hipMemcpy(h_depth, p->ref_depth, px * sizeof(double), hipMemcpyDeviceToHost));
    return DFVO_OK;
}

int dfvo_pipeline_get_keypoints(dfvo_pipeline* p, int slot, int cap, double* h_kp_ref, double* h_kp_cur,
                                uint8_t* h_inliers, int* n_out) {
    DFVO_ARG_CHECK(p && n_out && slot_ok(slot) && cap >= 0, "dfvo_pipeline_get_keypoints: bad argument");
    DFVO_ARG_CHECK(!deep_pose_tracking(p), "dfvo_pipeline_get_keypoints: tracking_method DFVO_TRACKING_DEEP_POSE selects no keypoints");
    TrackerBuffers& tb = p->slots[slot].tb;
    DFVO_HIP_CHECK(hipDeviceSynchronize());
    int info[3] = {0, 0, 0};
    DFVO_HIP_CHECK(hipMemcpy(info, tb.kp_info, sizeof(info), hipMemcpyDeviceToHost));
    *n_out = info[0];
    const int n = info[0] < cap ? info[0] : cap;
    if (n > 0 && h_kp_ref) DFVO_HIP_CHECK(hipMemcpy(h_kp_ref, tb.kp_ref, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
    if (n > 0 && h_kp_cur) DFVO_HIP_CHECK(hipMemcpy(h_kp_cur, tb.kp_cur, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
    if (n > 0 && h_inliers) DFVO_HIP_CHECK(hipMemcpy(h_inliers, tb.best_inliers, n, hipMemcpyDeviceToHost));
    return DFVO_OK;
}

int dfvo_pipeline_get_iterative(dfvo_pipeline* p, int slot, dfvo_scale_iter_out* out, int cap, double* h_kp_ref, double* h_kp_cur,
                                float* h_rigid_flow_diff) {
    DFVO_ARG_CHECK(p && out && slot_ok(slot) && cap >= 0, "dfvo_pipeline_get_iterative: bad argument");
    DFVO_ARG_CHECK(p->iter.enable, "dfvo_pipeline_get_iterative: the iterative scale recovery is not on (dfvo_pipeline_set_iterative)");
    Slot& sl = p->slots[slot];
    DFVO_ARG_CHECK(sl.begun == IDLE, "dfvo_pipeline_get_iterative: the slot's pair is not collected yet (track_end)");
    DFVO_HIP_CHECK(hipDeviceSynchronize());
    const IterCtl ctl = *sl.h_iter.p;
    const int n = ctl.sel_round >= 0 ? ctl.n_kp[ctl.sel_round] : 0;
    out->scale = ctl.scale;
    out->n_iter = ctl.n_iter;
    out->n_kp = n;
    out->kp_round = ctl.sel_round;
    out->status = ctl.status;
    out->device_ms = 0.f;
    for (int r = 0; r < ITER_ROUNDS; r++) {
        out->scale_in[r] = ctl.scale_in[r];
        out->scale_out[r] = ctl.scale_out[r];
        out->n_kp_round[r] = ctl.n_kp[r];
    }
    const int m = n < cap ? n : cap;
    const size_t sc = (size_t)sl.rigid.sel_cap * 2;  // rigid.kp: [best ref | best cur | uniform ref | uniform cur], sel_cap x 2 each
    if (m > 0 && h_kp_ref) DFVO_HIP_CHECK(hipMemcpy(h_kp_ref, sl.rigid.kp + 2 * sc, sizeof(double) * 2 * m, hipMemcpyDeviceToHost));
    if (m > 0 && h_kp_cur) DFVO_HIP_CHECK(hipMemcpy(h_kp_cur, sl.rigid.kp + 3 * sc, sizeof(double) * 2 * m, hipMemcpyDeviceToHost));
    if (ctl.sel_round >= 0 && h_rigid_flow_diff)
        DFVO_HIP_CHECK(hipMemcpy(h_rigid_flow_diff, sl.rigid.rdiff_of(ctl.sel_round, p->H, p->W), sizeof(float) * (size_t)p->H * p->W,
                                 hipMemcpyDeviceToHost));
    return DFVO_OK;
}

int dfvo_pipeline_get_pose_net(dfvo_pipeline* p, int slot, float* h_pose16, float* h_depth_diff) {
    DFVO_ARG_CHECK(p && slot_ok(slot), "dfvo_pipeline_get_pose_net: bad argument");
    DFVO_ARG_CHECK(p->pose.enable, "dfvo_pipeline_get_pose_net: the pose net is not on (dfvo_pipeline_set_pose_net)");
    DFVO_ARG_CHECK(!h_depth_diff || p->pose.depth_consistency, "dfvo_pipeline_get_pose_net: no depth-difference map without depth_consistency");
    const Slot& sl = p->slots[slot];
    DFVO_HIP_CHECK(hipDeviceSynchronize());
    if (h_pose16) DFVO_HIP_CHECK(hipMemcpy(h_pose16, sl.pose16, 16 * sizeof(float), hipMemcpyDeviceToHost));
    if (h_depth_diff) DFVO_HIP_CHECK(hipMemcpy(h_depth_diff, sl.depth_diff, (size_t)p->H * p->W * sizeof(float), hipMemcpyDeviceToHost));
    return DFVO_OK;
}

}  // extern "C"
