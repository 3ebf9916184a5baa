// Fused pipeline (pipeline_state.h): a pair's solver stage (pre-part, track_begin's chain, track_end) and the slot getters.
#include "pipeline_state.h"

// DFVO_TRACK_TRACE (tuning aid): per 20 pairs, the device time of the chain's three segments and track_end's host-side phases
struct TrackTrace {
    using Clock = std::chrono::steady_clock;
    static double ms_since(Clock::time_point a) { return std::chrono::duration<double, std::milli>(Clock::now() - a).count(); }
    static TrackTrace& get() { static TrackTrace t; return t; }
    const bool on = getenv("DFVO_TRACK_TRACE") != nullptr;
    double acc[2] = {0, 0}, dev[3] = {0, 0, 0}, lead[3] = {0, 0, 0};
    int dev_n = 0, lead_n = 0, n = 0;

    // track_begin: the events the chain's launchers record between its segments, and the homography half on its stream
    int begin(TrackerBuffers& tb) const {
        if (on && !tb.ev_t[0])
            for (int i = 0; i < TrackerBuffers::N_EV_T; i++) DFVO_HIP_CHECK(hipEventCreate(&tb.ev_t[i]));
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
        // how long before the chain's marks the run-ahead half had passed its own (negative: the chain waited for it)
        float l[3] = {0, 0, 0};
        const int from[3] = {4, 5, 5}, to[3] = {0, 0, 1};
        bool okl = ok && tb.ev_t_half;
        for (int i = 0; i < 3 && okl; i++) okl = hipEventElapsedTime(&l[i], tb.ev_t[from[i]], tb.ev_t[to[i]]) == hipSuccess;
        for (int i = 0; i < 3 && okl; i++) lead[i] += l[i];
        lead_n += okl;
        if (lead_n == 20) {
            fprintf(stderr, "run-ahead half, ms ahead: ev_start before the shuffles %.3f | ev_h before the shuffles %.3f | ev_h before the "
                            "end of the five-point batch %.3f\n", lead[0] / 20, lead[1] / 20, lead[2] / 20);
            lead[0] = lead[1] = lead[2] = 0;
            lead_n = 0;
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
static int enqueue_pnp(dfvo_pipeline* p, TrackerBuffers& tb, int n, const PnpConfig& cfg) {
    return enqueue_compute_pose_3d2d(p->pnp, tb.mt_state, tb.kp_ref, tb.kp_cur, tb.kp_info, n, p->ref_depth, p->H, p->W, cfg, p->s_trk());
}
// the first PnP pass of a pair: 3 repeats when a second one follows (pnp_tracker.py:87)
static int enqueue_pnp_first(dfvo_pipeline* p, Slot& sl, int n) {
    return enqueue_pnp(p, sl.tb, n, p->refine.pnp_enable ? p->pnp_cfg1 : p->pnp_cfg);
}

// dfvo_pipeline_set_refine: what dfvo_pipeline_get_refine reports for a pair that ran no refinement
static void refine_record_reset(RefineHost* h) {
    *h = RefineHost();
    h->ctl.done = 1;
    h->ctl.status = ITER_NOT_RUN;
    for (int i = 0; i < 3; i++) h->rec.R1[i * 4] = h->rec.pnp_R1[i * 4] = 1.0;
}

// The hand-over behind a first pass, on the chain's stream and gated there: the rigid-flow pose from the pass's device result
// (E: inv([R | t * scale]), skipped without a translation; PnP: [Rodrigues(r) | t]), kp_selection_good_depth on the reference
// frame's raw depth, the best set kp_depth into the second buffer set, its count and the gate into pinned memory
static int enqueue_refine_select(dfvo_pipeline* p, Slot& sl, bool pnp) {
    hipStream_t s = p->s_trk();
    TrackerBuffers& t2 = sl.tb2;
    RigidKpConfig rc = p->refine_cfg;
    rc.score_rigid = pnp ? p->refine.pnp_score_rigid : p->refine.e_score_rigid;
    if (pnp)
        DFVO_TRY(enqueue_refine_pnp_mats(sl.rigid, p->pnp.result, rc, t2.kp_info, s));
    else
        DFVO_TRY(enqueue_refine_e_mats(sl.rigid, sl.tb.pose, sl.tb.scale_out, rc, t2.kp_info, s));
    DFVO_TRY(enqueue_rigid_flow_kp_dev(sl.rigid, sl.flow_in, sl.diff_in, p->ref_raw, p->H, p->W, rc, &sl.rigid.ctl.p->done, t2.kp_ref,
                                       t2.kp_cur, t2.kp_info, s));
    DFVO_HIP_CHECK(hipMemcpyAsync(sl.h_refine.p->info2, t2.kp_info, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    DFVO_HIP_CHECK(hipMemcpyAsync(&sl.h_refine.p->ctl, sl.rigid.ctl, sizeof(IterCtl), hipMemcpyDeviceToHost, s));
    return DFVO_OK;
}

// where the reference's "sampling threshold is too small." assertion fires: the pair is over, as the iterative loop ends it
static int refine_empty_selection(dfvo_pipeline* p, int slot, const double* d_depth_override, RefineHost* h) {
    h->rec.empty = 1;
    DFVO_TRY(roll_ref_depth(p, slot, d_depth_override));
    dfvo::set_last_error("dfvo_pipeline_track_end: sampling threshold is too small (no rigid-flow keypoint selected)");
    return DFVO_ERR_EMPTY_SELECTION;
}

// the PnP branch of dfvo.py:225-250 with pnp_tracker.iterative_kp: `pr1` is pass one's result and the selection behind it has
// arrived in pinned memory; the second pass on kp_depth with the configured repeats, waited for here
static int refine_pnp_second(dfvo_pipeline* p, int slot, const PnpResult& pr1, const double* d_depth_override, dfvo_track_out* out) {
    hipStream_t s = p->s_trk();
    Slot& sl = p->slots[slot];
    RefineHost* h = sl.h_refine.p;
    h->rec.pnp_ran = 1;
    h->rec.pnp_found1 = pr1.found;
    if (pr1.found) {
        for (int i = 0; i < 9; i++) h->rec.pnp_R1[i] = pr1.R[i];
        for (int i = 0; i < 3; i++) h->rec.pnp_t1[i] = pr1.tvec[i];
    }
    const int n3 = h->rec.n_kp = h->info2[0];
    fill_pnp_out(pr1, out);
    if (n3 == 0) return refine_empty_selection(p, slot, d_depth_override, h);
    DFVO_TRY(enqueue_pnp(p, sl.tb2, n3, p->pnp_cfg));
    PnpResult pr;
    DFVO_HIP_CHECK(hipMemcpyAsync(&pr, p->pnp.result, sizeof(pr), hipMemcpyDeviceToHost, s));
    DFVO_HIP_CHECK(hipStreamSynchronize(s));
    DFVO_ARG_CHECK(pr.status >= 0, "dfvo_pipeline_track: the PnP tracker's second pass reported an internal error");
    fill_pnp_out(pr, out);
    return DFVO_OK;
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
    if (refine_on(p->refine)) refine_record_reset(sl.h_refine);
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
        DFVO_TRY(enqueue_pnp_first(p, sl, n));
        DFVO_HIP_CHECK(hipMemcpyAsync(&sl.h_res.p->pnp, p->pnp.result, sizeof(PnpResult), hipMemcpyDeviceToHost, s));
        if (p->refine.pnp_enable) DFVO_TRY(enqueue_refine_select(p, sl, true));
        DFVO_HIP_CHECK(hipEventRecord(sl.e_res, s));
        return begun(CHAIN_ENQUEUED);
    }
    // the shuffles and the five-point batch start behind tb.ev_start; s waits for tb.ev_h (the prefetched half) on the device
    // only in front of the validity bookkeeping, the first kernel that reads the homography
    DFVO_TRY(enqueue_pose_e_part(tb, n, p->refine.e_enable ? p->pose_cfg1 : p->pose_cfg, s, p->d_T21, iterative ? p->d_E_pose.p : nullptr));
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
        // e_tracker.iterative_kp: the kp_depth selection behind pass one, so that its count arrives with pass one's results
        if (p->refine.e_enable) DFVO_TRY(enqueue_refine_select(p, sl, false));
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
            if (p->refine.pnp_enable) {
                const int rc_ref = refine_pnp_second(p, slot, pr, d_depth_override, out);
                if (rc_ref != DFVO_OK) return rc_ref;  // (an empty selection: the depths are rolled)
            }
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
    bool t_zero = ps.t[0] == 0 && ps.t[1] == 0 && ps.t[2] == 0;
    double scale = sr.scale;
    ScaleResult sr_last = sr;  // the counts of the last scale stage that ran
    if (p->refine.e_enable) {
        // dfvo.py:194-222.  Pass one and the selection behind it are in pinned memory; the second pass needs the kp_depth count
        // on the host (launch geometry, the "more than 10 keypoints" rule), so it is enqueued here, ahead of the PnP decision
        RefineHost* h = sl.h_refine.p;
        for (int i = 0; i < 9; i++) h->rec.R1[i] = ps.R[i];
        for (int i = 0; i < 3; i++) h->rec.t1[i] = ps.t[i];
        h->rec.scale1 = t_zero ? 0.0 : sr.scale;
        if (!t_zero) {
            TrackerBuffers& t2 = sl.tb2;
            const int n2 = h->info2[0];
            h->rec.e_ran = 1;
            h->rec.n_kp = h->rec.n_inliers = n2;
            if (n2 == 0) {
                h->rec.n_inliers = 0;
                out->scale = scale;
                out->status = DFVO_TRACK_E;
                return refine_empty_selection(p, slot, d_depth_override, h);
            }
            DFVO_TRY(enqueue_compute_pose_2d2d(t2, n2, p->pose_cfg, s, p->d_T21));
            if (p->refine.scale_enable)  // gated on the device by the second pass's translation
                DFVO_TRY(enqueue_find_scale(t2, n2, p->d_T21, d_depth_override ? d_depth_override : sl.proc_depth.p, p->H, p->W,
                                            p->scale_cfg, s, t2.pose, false));
            DFVO_TRY(enqueue_refine_final(sl.tb.pose, sl.tb.scale_out, t2.pose, t2.scale_out, p->refine.scale_enable, sl.refine_final, s));
            DFVO_HIP_CHECK(hipMemcpyAsync(&h->pose2, t2.pose, sizeof(PoseState), hipMemcpyDeviceToHost, s));
            DFVO_HIP_CHECK(hipMemcpyAsync(&h->scale2, t2.scale_out, sizeof(ScaleResult), hipMemcpyDeviceToHost, s));
            DFVO_HIP_CHECK(hipMemcpyAsync(&h->fin, sl.refine_final, sizeof(RefineFinal), hipMemcpyDeviceToHost, s));
            DFVO_HIP_CHECK(hipStreamSynchronize(s));
            const RefineFinal& fin = h->fin;
            for (int i = 0; i < 9; i++) out->R[i] = fin.R[i];
            for (int i = 0; i < 3; i++) out->t[i] = fin.t[i];
            out->best_inlier_cnt = h->pose2.best_cnt;
            out->num_valid = h->pose2.num_valid;
            out->cheirality = h->pose2.cheirality;
            t_zero = fin.t2_zero != 0;
            scale = fin.scale;
            h->rec.scale_ran = fin.scale_ran;
            h->rec.scale2 = fin.scale2;
            if (fin.scale_ran) sr_last = h->scale2;
        }
    }
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
    out->scale_n_valid = sr_last.n_valid;
    out->scale_n_trials = sr_last.n_trials;
    out->scale_n_inliers = sr_last.n_inliers;
    if (t_zero || scale == -1.0) {  // the PnP fallback
        out->status = DFVO_TRACK_NEEDS_PNP;
        if (p->has_ref_depth) {
            DFVO_TRY(enqueue_pnp_first(p, sl, n));
            PnpResult pr;
            DFVO_HIP_CHECK(hipMemcpyAsync(&pr, p->pnp.result, sizeof(pr), hipMemcpyDeviceToHost, s));
            if (p->refine.pnp_enable) DFVO_TRY(enqueue_refine_select(p, sl, true));
            DFVO_HIP_CHECK(hipStreamSynchronize(s));
            DFVO_ARG_CHECK(pr.status >= 0, "dfvo_pipeline_track: the PnP fallback reported an internal error");
            fill_pnp_out(pr, out);
            if (p->refine.pnp_enable) {
                const int rc_ref = refine_pnp_second(p, slot, pr, d_depth_override, out);
                if (rc_ref != DFVO_OK) return rc_ref;  // (an empty selection: the depths are rolled)
            }
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

int dfvo_pipeline_get_refine(dfvo_pipeline* p, int slot, dfvo_refine_out* out, int cap, double* h_kp_ref, double* h_kp_cur,
                             uint8_t* h_inliers, float* h_rigid_flow_diff) {
    DFVO_ARG_CHECK(p && out && slot_ok(slot) && cap >= 0, "dfvo_pipeline_get_refine: bad argument");
    DFVO_ARG_CHECK(refine_on(p->refine), "dfvo_pipeline_get_refine: no keypoint refinement is on (dfvo_pipeline_set_refine)");
    Slot& sl = p->slots[slot];
    DFVO_ARG_CHECK(sl.begun == IDLE, "dfvo_pipeline_get_refine: the slot's pair is not collected yet (track_end)");
    DFVO_HIP_CHECK(hipDeviceSynchronize());
    *out = sl.h_refine.p->rec;
    const int m = out->n_kp < cap ? out->n_kp : cap, mi = out->n_inliers < cap ? out->n_inliers : cap;
    if (m > 0 && h_kp_ref) DFVO_HIP_CHECK(hipMemcpy(h_kp_ref, sl.tb2.kp_ref, sizeof(double) * 2 * m, hipMemcpyDeviceToHost));
    if (m > 0 && h_kp_cur) DFVO_HIP_CHECK(hipMemcpy(h_kp_cur, sl.tb2.kp_cur, sizeof(double) * 2 * m, hipMemcpyDeviceToHost));
    if (mi > 0 && h_inliers) DFVO_HIP_CHECK(hipMemcpy(h_inliers, sl.tb2.best_inliers, mi, hipMemcpyDeviceToHost));
    if ((out->e_ran || out->pnp_ran) && h_rigid_flow_diff)
        DFVO_HIP_CHECK(hipMemcpy(h_rigid_flow_diff, sl.rigid.rdiff, sizeof(float) * (size_t)p->H * p->W, hipMemcpyDeviceToHost));
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
