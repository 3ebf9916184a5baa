// Fused pipeline (pipeline_state.h): the option setters.  Each asks pipeline_setup.h before it allocates and commits afterwards.
#include "pipeline_state.h"

static int refuse(const char* why) { return dfvo::set_last_error(why), DFVO_ERR_ARG; }

// the solvers' configurations, each in its members' order (tracker.h)
void fill_solver_cfgs(dfvo_pipeline* p) {
    const dfvo_pipeline_cfg& c = p->cfg;
    const dfvo_pipeline_opts& o = p->opts;
    p->pose_cfg = {c.fx, c.cx, c.cy, c.e_reproj_thre, c.e_repeat, c.e_max_iters, {}, {}, o.validity_method,
                   o.validity_method == DFVO_VALIDITY_GRIC ? 0.0 : o.validity_thre};
    p->pnp_cfg = {c.fx, c.fy, c.cx, c.cy, {}, c.min_depth, c.max_depth, c.pnp_repeat, c.pnp_iters, c.pnp_reproj_thre};
    p->scale_cfg = {c.cx, c.cy, c.fx, c.fy, c.scale_min_samples, c.scale_max_trials, c.scale_stop_prob, c.scale_thre, o.scale_method};
    for (int i = 0; i < 9; i++) {
        p->pose_cfg.KinvT[i] = c.KinvT[i];
        p->pose_cfg.Kinv[i] = p->pnp_cfg.inv_K[i] = c.Kinv[i];
    }
    // a first pass of the keypoint refinement: max_ransac_iter = 3 (E_tracker.py:207, pnp_tracker.py:87, is_iterative False)
    p->pose_cfg1 = p->pose_cfg;
    p->pnp_cfg1 = p->pnp_cfg;
    p->pose_cfg1.repeat = p->pnp_cfg1.repeat = 3;
}

extern "C" {

int dfvo_pipeline_set_options(dfvo_pipeline* p, const dfvo_pipeline_opts* o) {
    DFVO_ARG_CHECK(p && o, "dfvo_pipeline_set_options: null argument");
    DFVO_ARG_CHECK(!p->started, "dfvo_pipeline_set_options: comes before the first dfvo_pipeline_enqueue_nets / _set_ref_*");
    const dfvo_pipeline_cfg& c = p->cfg;
    if (const char* why = options_refusal(c, *o, p->iter, p->pose)) return refuse(why);
    if (const char* why = options_refine_refusal(*o, p->refine)) return refuse(why);
    // every buffer the chosen source needs at its final size, here: nothing on the per-pair path allocates (hipFree waits
    // for the whole device).  kp_count stays 0 for local_bestN, whose launcher sizes its own buffers as before
    const int kp_count = options_kp_count(c, *o);
    int crop[4] = {0, 0, 0, 0};
    DevArr<int> d_samples;  // (p->d_samples keeps the committed list until nothing below can fail any more)
    if (o->kp_source == DFVO_KP_SOURCE_SAMPLED) {
        flow_crop_px(c, *o, crop);
        std::vector<int> samples(kp_count);
        generate_kp_samples(crop[0], crop[1], crop[2], crop[3], kp_count, samples.data());
        DFVO_TRY(d_samples.alloc(samples.size()));
        DFVO_HIP_CHECK(hipMemcpy(d_samples, samples.data(), sizeof(int) * samples.size(), hipMemcpyHostToDevice));
    }
    if (kp_count > 0) {
        for (int i = 0; i < DFVO_PIPELINE_SLOTS; i++) {
            DFVO_TRY(p->slots[i].tb.ensure_kp(kp_count, 1, 1));
            if (o->kp_source == DFVO_KP_SOURCE_BESTN) DFVO_TRY(p->slots[i].bestn.ensure((size_t)p->H * p->W, 0));
        }
        if (c.pnp_iters > 0) DFVO_TRY(p->pnp.ensure(kp_count + 8, c.pnp_iters));
    }
    p->d_samples = std::move(d_samples);
    for (int i = 0; i < 4; ++i) p->sample_crop[i] = crop[i];
    p->opts = *o;
    fill_solver_cfgs(p);
    return DFVO_OK;
}

int dfvo_pipeline_set_depth_source(dfvo_pipeline* p, const dfvo_pipeline_depth_src* d) {
    DFVO_ARG_CHECK(p && d, "dfvo_pipeline_set_depth_source: null argument");
    DFVO_ARG_CHECK(!p->started && !p->nets_ready,
                   "dfvo_pipeline_set_depth_source: comes before dfvo_pipeline_finalize and the first dfvo_pipeline_enqueue_nets / _set_ref_*");
    if (const char* why = depth_source_refusal(*d)) return refuse(why);
    p->dsrc = d->source == DFVO_DEPTH_NET ? dfvo_pipeline_depth_src{} : *d;
    return DFVO_OK;
}

int dfvo_pipeline_set_iterative(dfvo_pipeline* p, const dfvo_pipeline_iter_opts* o) {
    DFVO_ARG_CHECK(p && o, "dfvo_pipeline_set_iterative: null argument");
    DFVO_ARG_CHECK(!p->started, "dfvo_pipeline_set_iterative: comes before the first dfvo_pipeline_enqueue_nets / _set_ref_*");
    if (!o->enable) {
        p->iter = {};
        return DFVO_OK;
    }
    const dfvo_pipeline_cfg& c = p->cfg;
    if (const char* why = iter_opts_refusal(*o, c.scale_min_samples)) return refuse(why);
    if (const char* why = iter_refine_refusal(*o, p->refine)) return refuse(why);
    const RigidKpConfig rc = iter_rigid_config(*o, c.fx, c.fy, c.cx, c.cy, c.Kinv);
    int cells, n_best, cap, par;
    size_t lds;
    DFVO_TRY(rigid_flow_kp_geometry(p->H, p->W, rc, &cells, &n_best, &cap, &lds, &par));  // the launcher's refusals
    const int n_sel = cells * n_best, n_trk = tracked_kp_max(p->opts.kp_source, p->opts.kp_sampled_num, c.kp_num_bestN, c.kp_num_row, c.kp_num_col);
    DFVO_ARG_CHECK(iter_kp_count_ok(o->kp_src, n_sel, n_trk),
                   "dfvo_pipeline_set_iterative: more keypoints than the depth-ratio kernel holds in 64 KB of LDS (16384)");
    // every buffer of the loop at its final size, here: nothing on the per-pair path allocates.  The scale stage's
    // keypoint-sized buffers hold a round's uniform set as well as the tracked set; local_bestN keeps its selection lists
    const int kp_need = std::max(std::max(n_sel, n_trk), 16);
    const bool lb = p->opts.kp_source == DFVO_KP_SOURCE_LOCAL_BESTN;
    const int lb_cells = lb ? c.kp_num_row * c.kp_num_col : 1, lb_best = lb && lb_cells > 0 ? c.kp_num_bestN / lb_cells : 1;
    for (Slot& sl : p->slots) {
        DFVO_TRY(sl.rigid.ensure(p->H, p->W, cells, n_best, cap));
        DFVO_TRY(sl.tb.ensure_kp(kp_need, lb_cells > 0 ? lb_cells : 1, lb_best > 0 ? lb_best : 1));
        DFVO_TRY(sl.tb.grow_winner(p->H, p->W));
        if (!sl.h_iter && sl.h_iter.alloc(1)) return DFVO_ERR_HIP;
        iter_record_reset(sl.h_iter);
    }
    p->iter = *o;
    p->iter_cfg = rc;
    return DFVO_OK;
}

int dfvo_pipeline_set_refine(dfvo_pipeline* p, const dfvo_pipeline_refine_opts* o) {
    DFVO_ARG_CHECK(p && o, "dfvo_pipeline_set_refine: null argument");
    DFVO_ARG_CHECK(!p->started, "dfvo_pipeline_set_refine: comes before the first dfvo_pipeline_enqueue_nets / _set_ref_*");
    if (const char* why = refine_opts_refusal(*o, p->opts, p->iter)) return refuse(why);
    if (!refine_on(*o)) {
        p->refine = {};
        return DFVO_OK;
    }
    const dfvo_pipeline_cfg& c = p->cfg;
    dfvo_pipeline_iter_opts grid = {};  // (the rigid-flow keypoint configuration is the iterative loop's: one builder)
    grid.num_row = o->num_row, grid.num_col = o->num_col, grid.num_bestN = o->num_bestN;
    grid.rigid_flow_thre = o->rigid_flow_thre, grid.optical_flow_thre = o->optical_flow_thre;
    const RigidKpConfig rc = iter_rigid_config(grid, c.fx, c.fy, c.cx, c.cy, c.Kinv);
    int cells, n_best, cap, par;
    size_t lds;
    DFVO_TRY(rigid_flow_kp_geometry(p->H, p->W, rc, &cells, &n_best, &cap, &lds, &par));  // the launcher's refusals
    const int n_sel = cells * n_best;
    DFVO_ARG_CHECK(refine_kp_count_ok(*o, n_sel),
                   "dfvo_pipeline_set_refine: more kp_depth keypoints than the depth-ratio kernel holds in 64 KB of LDS (16384)");
    // every buffer of the second passes at its final size, here: nothing on the per-pair path allocates.  The second buffer set
    // gets the intrinsics now, so its first homography part finds them in place
    const int kp_need = std::max(n_sel, 16);
    double hk[18];
    for (int i = 0; i < 9; i++) hk[i] = c.KinvT[i], hk[9 + i] = c.Kinv[i];
    for (Slot& sl : p->slots) {
        DFVO_TRY(sl.rigid.ensure(p->H, p->W, cells, n_best, cap));
        if (!sl.tb2.kp_info) DFVO_TRY(sl.tb2.init_shared(p->slots[0].tb));
        DFVO_TRY(sl.tb2.ensure_kp(kp_need, 1, 1));
        DFVO_TRY(sl.tb2.grow_winner(p->H, p->W));
        DFVO_HIP_CHECK(hipMemcpy(sl.tb2.small, hk, sizeof(hk), hipMemcpyHostToDevice));
        memcpy(sl.tb2.h_small, hk, sizeof(hk));
        sl.tb2.small_valid = true;
        if (!sl.refine_final && sl.refine_final.alloc_zeroed(1)) return DFVO_ERR_HIP;
        if (!sl.h_refine && sl.h_refine.alloc(1)) return DFVO_ERR_HIP;
        *sl.h_refine.p = RefineHost();
    }
    if (o->pnp_enable && c.pnp_iters > 0) DFVO_TRY(p->pnp.ensure(std::max(p->pnp.cap, n_sel + 8), c.pnp_iters));
    p->refine = *o;
    p->refine_cfg = rc;
    return DFVO_OK;
}

int dfvo_pipeline_set_pose_net(dfvo_pipeline* p, const dfvo_pipeline_pose_opts* o) {
    DFVO_ARG_CHECK(p && o, "dfvo_pipeline_set_pose_net: null argument");
    DFVO_ARG_CHECK(!p->started, "dfvo_pipeline_set_pose_net: comes before the first dfvo_pipeline_enqueue_nets / _set_ref_*");
    if (const char* why = pose_net_refusal(p->opts, *o)) return refuse(why);
    if (!o->enable) {
        p->pose = {};
        return DFVO_OK;
    }
    // every buffer of the lane at its final size, here: nothing on the per-pair path allocates
    const size_t px = (size_t)p->H * p->W;
    p->pose_feed_pitch = ((size_t)p->feedH * p->feedW * 3 + 15) / 16 * 16;
    if (!p->pose_feed && p->pose_feed.alloc_zeroed(2 * p->pose_feed_pitch)) return DFVO_ERR_HIP;
    if (!p->pose_out && p->pose_out.alloc_zeroed(16)) return DFVO_ERR_HIP;
    for (Slot& sl : p->slots) {
        if (!sl.pose16 && sl.pose16.alloc_zeroed(16)) return DFVO_ERR_HIP;
        if (!sl.h_pose && sl.h_pose.alloc(16)) return DFVO_ERR_HIP;
        if (o->depth_consistency && !sl.depth_diff && sl.depth_diff.alloc_zeroed(px)) return DFVO_ERR_HIP;
    }
    if (p->nets_ready) DFVO_TRY(finalize_pose_net(p));
    p->pose = *o;
    return DFVO_OK;
}

int dfvo_pipeline_set_pose_override(dfvo_pipeline* p, int slot, const float* d_pose16) {
    DFVO_ARG_CHECK(p && slot_ok(slot), "dfvo_pipeline_set_pose_override: bad argument");
    DFVO_ARG_CHECK(p->pose.enable, "dfvo_pipeline_set_pose_override: the pose net is not on (dfvo_pipeline_set_pose_net)");
    p->slots[slot].pose_override = d_pose16;
    return DFVO_OK;
}

int dfvo_pipeline_set_raw_depth_override(dfvo_pipeline* p, int slot, const float* d_raw) {
    DFVO_ARG_CHECK(p && slot_ok(slot), "dfvo_pipeline_set_raw_depth_override: bad argument");
    p->slots[slot].raw_override = d_raw;
    return DFVO_OK;
}

int dfvo_pipeline_get_prev_scale(dfvo_pipeline* p, double* h_scale) {
    DFVO_ARG_CHECK(p && h_scale, "dfvo_pipeline_get_prev_scale: null argument");
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk()));
    DFVO_HIP_CHECK(hipMemcpy(h_scale, p->d_prev_scale, sizeof(double), hipMemcpyDeviceToHost));
    return DFVO_OK;
}

int dfvo_pipeline_set_prev_scale(dfvo_pipeline* p, double scale) {
    DFVO_ARG_CHECK(p, "dfvo_pipeline_set_prev_scale: null pipeline");
    DFVO_ARG_CHECK(p->pending_slot == -1, "dfvo_pipeline_set_prev_scale: a pair is begun and not yet collected");
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk()));
    DFVO_HIP_CHECK(hipMemcpy(p->d_prev_scale, &scale, sizeof(double), hipMemcpyHostToDevice));
    return DFVO_OK;
}

}  // extern "C"
