// Fused pipeline (pipeline_state.h): create / destroy, the roles' streams, the nets' parameters, the RandomState, the reports.
#include "pipeline_state.h"

extern "C" {

int dfvo_pipeline_create(const dfvo_pipeline_cfg* cfg, dfvo_pipeline** out) {
    DFVO_ARG_CHECK(cfg && out, "dfvo_pipeline_create: null argument");
    dfvo_pipeline* p = new dfvo_pipeline();
    p->cfg = *cfg;
    p->H = cfg->img_h;
    p->W = cfg->img_w;
    p->feedH = cfg->feed_h;
    p->feedW = cfg->feed_w;
    auto fail = [&](int rc) {
        dfvo_pipeline_destroy(p);  // (tolerates a half-built pipeline)
        return rc;
    };
    auto create_owned = [&](hipStream_t* s, bool solver) -> int {
        DFVO_HIP_CHECK(solver ? create_solver_stream(s) : create_net_stream(s));
        p->owned.push_back(*s);
        return DFVO_OK;
    };
    // two LiteFlowNet instances on two pipes, alternating pairs (measured 1 / 2 / 3: 217 / 287 / 272 pairs/s, profiles/
    // r3ag_flow_instances_ab.txt).  DFVO_FLOW_INSTANCES=1 is a test hook: the carry-over from a pass of the SAME instance
    p->flow_instances = getenv("DFVO_FLOW_INSTANCES") && atoi(getenv("DFVO_FLOW_INSTANCES")) == 1 ? 1 : 2;
    // The streams of the roles by measurement (stream_pool.hip, stream_layout.h): twelve candidates, classified by dispatch pipe
    // and by hardware queue.  Eight or more queues: the wide layout, a stream per role -- pipe A / B: one flow-net instance each,
    // pipe C: the depth net + the two run-ahead homography chains, pipe D: the RandomState-ordered chain and its two side streams,
    // alone.  Four to seven queues (GPU_MAX_HW_QUEUES at the runtime's default of 4): eight busy streams would share queues,
    // and streams of one queue execute in host enqueue order -- a wait enqueued for one of them holds up the others' work;
    // the lane layout takes one stream from each of four queues and puts the roles of a lane on that one stream (flow |
    // flow_x | depth + pre-parts | chain + side streams), so which roles share a queue is decided here and not by the runtime.
    // DFVO_STREAM_LAYOUT=auto|wide|lanes forces one (A/B runs, tests).  Falls back to creation order when the probe does
    // not settle or finds too few groups / queues for the layout: the roles the pool did not fill stay null here and get
    // streams created below, in the order the pair rate was measured with (TrackerBuffers::init).
    int choice = LAYOUT_CHOICE_AUTO;
    if (const char* e = getenv("DFVO_STREAM_LAYOUT")) {
        if (!strcmp(e, "wide"))
            choice = LAYOUT_CHOICE_WIDE;
        else if (!strcmp(e, "lanes"))
            choice = LAYOUT_CHOICE_LANES;
        else if (strcmp(e, "auto")) {
            dfvo::set_last_error("dfvo_pipeline_create: DFVO_STREAM_LAYOUT is auto, wide or lanes");
            return fail(DFVO_ERR_ARG);
        }
    }
    auto own = [&](hipStream_t s) {  // a stream taken from the pool
        if (s) p->owned.push_back(s);
        return s;
    };
    auto wanted = [&](int r) { return r != ROLE_FLOW_X || p->flow_instances > 1; };
    StreamPool pool;
    if (pool.create(12) == DFVO_OK && pool.ngroups > 0) {
        p->pool_groups = pool.ngroups;
        p->pool_queues = pool.nqueues;
    }
    const StreamPlan plan = plan_stream_layout(p->pool_groups, p->pool_queues, choice);
    if (plan.layout == LAYOUT_LANES) {
        const PoolClasses c = {pool.group, pool.queue_group, pool.ngroups, pool.nqueues};
        int pick[4];
        if (pick_lane_candidates(c, pick)) {
            for (int l = 0; l < 4; ++l) p->lane[l] = own(pool.take_index(pick[l]));
            for (int r = 0; r < ROLE_COUNT; ++r)
                if (wanted(r)) p->role[r] = p->lane[plan.lane[r]];
            p->plan = plan;
        }
    } else if (plan.layout == LAYOUT_WIDE) {
        int g[4] = {-1, -1, -1, -1}, ng = 0;  // the four largest groups, largest first
        std::vector<int> order;
        for (int i = 0; i < pool.ngroups; ++i) order.push_back(i);
        std::sort(order.begin(), order.end(), [&](int a, int b) { return pool.count(a) > pool.count(b); });
        for (int i = 0; i < 4; ++i) g[ng++] = order[i];
        // role -> pipe: trk rep0 rep1 | depth pre0 pre1 | flow | flow_x (plan.lane).  Other placements were measured
        // (profiles/r3k_layouts.txt): a run-ahead homography chain on a flow net's pipe 178-194 pairs/s against 266 -- its
        // long single-workgroup kernels hold up the dispatch of the flow net's hundred short launches per pass.
        // Per role, the pipe group its stream comes from: by the plan's rank (0 = largest), or, with two small groups,
        // chain and depth roles on the two large ones
        int from[ROLE_COUNT] = {g[0], g[0], g[0], g[1], g[1], g[1], g[2], g[3]};
        const bool full = pool.count(g[0]) >= 3 && pool.count(g[1]) >= 3 && pool.count(g[2]) >= 3 && pool.count(g[3]) >= 3;
        if (full)
            for (int r = 0; r < ROLE_COUNT; ++r) from[r] = g[plan.lane[r]];
        if (full || (pool.count(g[0]) >= 3 && pool.count(g[1]) >= 3 && pool.count(g[2]) >= 1 && pool.count(g[3]) >= 1))
            for (int r = 0; r < ROLE_COUNT; ++r)
                if (wanted(r)) p->role[r] = own(pool.take(from[r]));
        if (p->s_trk()) p->plan = plan;
    }
    pool.release();
    if (!p->s_trk() && (create_owned(&p->role[ROLE_FLOW], false) || create_owned(&p->role[ROLE_DEPTH], false) ||
                        create_owned(&p->role[ROLE_TRK], true))) {
        dfvo::set_last_error("dfvo_pipeline_create: hipStreamCreate failed (no GPU?)");
        return fail(DFVO_ERR_HIP);
    }
    for (hipEvent_t* e : {&p->e_ref, &p->e_roll})
        if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return fail(DFVO_ERR_HIP);
    for (Slot& sl : p->slots)
        for (hipEvent_t* e : {&sl.e_flow, &sl.e_depth, &sl.e_pre, &sl.e_res})
            if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) {
                dfvo::set_last_error("dfvo_pipeline_create: hipEventCreate failed");
                return fail(DFVO_ERR_HIP);
            }
    for (int i = 0; i < p->flow_instances; ++i) {
        hipStream_t* sf = &p->role[ROLE_FLOW + i];
        if (!*sf && create_owned(sf, false)) return fail(DFVO_ERR_HIP);
        if (int rc = p->flow[i].init(p->H, p->W, *sf)) return fail(rc);
    }
    if (int rc = p->depth.init(p->feedH, p->feedW, p->s_depth())) return fail(rc);
    p->depth.min_depth = cfg->net_min_depth;
    p->depth.max_depth = cfg->net_max_depth;
    p->depth.baseline_mult = cfg->baseline_mult;
    // (lanes: the chain's side streams are the chain's own stream)
    if (int rc = p->role[ROLE_REP0] ? p->slots[0].tb.init(p->role[ROLE_REP0], p->role[ROLE_REP1], true) : p->slots[0].tb.init()) return fail(rc);
    for (int i = 1; i < DFVO_PIPELINE_SLOTS; i++)
        if (int rc = p->slots[i].tb.init_shared(p->slots[0].tb)) return fail(rc);
    // the PnP fallback's buffers at their final size: grown lazily they would be freed and re-allocated (hipFree waits for
    // the whole device) whenever a pair with more keypoints than any before takes the fallback
    if (cfg->kp_num_bestN > 0 && cfg->pnp_iters > 0)
        if (int rc = p->pnp.ensure(cfg->kp_num_bestN + 8, cfg->pnp_iters)) return fail(rc);
    for (int r : {ROLE_PRE0, ROLE_PRE1})
        if (!p->role[r] && create_owned(&p->role[r], true)) return fail(DFVO_ERR_HIP);
    const size_t px = (size_t)p->H * p->W, feed_px = (size_t)p->feedH * p->feedW;
    for (Slot& sl : p->slots)
        if (sl.h_info.alloc(4) || sl.h_res.alloc(1) || sl.fwd.alloc(2 * px) || sl.bwd.alloc(2 * px) || sl.diff.alloc(px) ||
            sl.raw_depth.alloc(px) || sl.proc_depth.alloc(px))
            return fail(DFVO_ERR_HIP);
    if (p->depth_small.alloc(feed_px) || p->ref_depth.alloc(px) || p->ref_raw.alloc(px) || p->d_T21.alloc(16) ||
        p->feed_buf.alloc(feed_px * 3) || p->d_E_pose.alloc(16) || p->d_prev_scale.alloc(1))
        return fail(DFVO_ERR_HIP);
    if (hipMemset(p->d_prev_scale, 0, sizeof(double)) != hipSuccess) return fail(DFVO_ERR_HIP);  // EssTracker.prev_scale = 0
    if (p->feed_resize.init(p->H, p->W, p->feedH, p->feedW) != DFVO_OK) return fail(DFVO_ERR_HIP);
    enqueue_mt_seed(p->slots[0].tb, cfg->seed, p->s_trk());
    (void)hipStreamSynchronize(p->s_trk());
    fill_solver_cfgs(p);
    if (getenv("DFVO_STREAM_PROBE_VERBOSE")) {
        char line[256];
        if (dfvo_pipeline_stream_layout(p, line, sizeof(line)) == DFVO_OK) fprintf(stderr, "dfvo pipeline streams: %s\n", line);
    }
    *out = p;
    return DFVO_OK;
}

// also the failure path of dfvo_pipeline_create: every member may be in its initial state
void dfvo_pipeline_destroy(dfvo_pipeline* p) {
    if (!p) return;
    (void)hipDeviceSynchronize();
    for (int i = DFVO_PIPELINE_SLOTS - 1; i >= 0; i--) {
        Slot& sl = p->slots[i];
        sl.tb2.release();
        sl.tb.release();  // (the sharing sets before slots[0].tb, whose RandomState and events they borrow)
        for (hipEvent_t e : {sl.e_flow, sl.e_depth, sl.e_pre, sl.e_res})
            if (e) (void)hipEventDestroy(e);
    }
    for (hipEvent_t e : {p->e_ref, p->e_roll})
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : p->owned) (void)hipStreamDestroy(s);
    delete p;  // (device and pinned memory: DevArr / PinnedArr members, here, in the nets and in the buffer sets; the nets' graphs)
}

static int pipe_store(ParamStore* ps, const char* name, const float* h, int ndim, const int* shape) {
    DFVO_ARG_CHECK(name && h && ndim >= 0 && ndim <= 8, "set_param: bad argument");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign(h, h + n);
    ps->t[name] = std::move(t);
    return DFVO_OK;
}

int dfvo_pipeline_set_flow_param(dfvo_pipeline* p, const char* name, const float* h, int ndim, const int* shape) {
    DFVO_ARG_CHECK(p && !p->nets_ready, "dfvo_pipeline_set_flow_param: bad state");
    for (int i = 0; i < p->flow_instances; ++i) DFVO_TRY(pipe_store(&p->flow[i].params, name, h, ndim, shape));
    return DFVO_OK;
}
int dfvo_pipeline_set_depth_param(dfvo_pipeline* p, const char* name, const float* h, int ndim, const int* shape) {
    DFVO_ARG_CHECK(p && !p->nets_ready, "dfvo_pipeline_set_depth_param: bad state");
    return pipe_store(&p->depth.params, name, h, ndim, shape);
}
int dfvo_pipeline_set_pose_param(dfvo_pipeline* p, const char* name, const float* h, int ndim, const int* shape) {
    DFVO_ARG_CHECK(p && !p->pose_net.finalized, "dfvo_pipeline_set_pose_param: bad state");
    return pipe_store(&p->pose_net.params, name, h, ndim, shape);
}
int dfvo_pipeline_finalize(dfvo_pipeline* p) {
    DFVO_ARG_CHECK(p, "null pipeline");
    for (int i = 0; i < p->flow_instances; ++i) DFVO_TRY(p->flow[i].finalize());
    if (p->dsrc.source != DFVO_DEPTH_EXTERNAL) DFVO_TRY(p->depth.finalize());  // (external depth: no parameters, no graph)
    if (p->pose.enable) DFVO_TRY(finalize_pose_net(p));
    p->nets_ready = true;
    return DFVO_OK;
}
int dfvo_pipeline_set_graph(dfvo_pipeline* p, int enable) {
    DFVO_ARG_CHECK(p, "null pipeline");
    for (int i = 0; i < p->flow_instances; ++i) p->flow[i].use_graph = enable != 0;
    p->depth.use_graph = enable != 0;
    p->pose_net.use_graph = enable != 0;
    return DFVO_OK;
}

int dfvo_pipeline_seed(dfvo_pipeline* p, uint32_t seed) {
    DFVO_ARG_CHECK(p, "null pipeline");
    // synchronous: the first RandomState consumer of the next pair (the keypoint shuffles) runs on tb.s_rep[0], which is
    // ordered after the keypoint stage but not after s_trk -- the new key must be in place before track() is called
    DFVO_TRY(enqueue_mt_seed(p->slots[0].tb, seed, p->s_trk()));
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk()));
    return DFVO_OK;
}

int dfvo_pipeline_get_rng_state(dfvo_pipeline* p, uint32_t* h_state) {
    DFVO_ARG_CHECK(p && h_state, "dfvo_pipeline_get_rng_state: null argument");
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk()));
    DFVO_HIP_CHECK(hipMemcpy(h_state, p->slots[0].tb.mt_state, 625 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DFVO_OK;
}

int dfvo_pipeline_set_rng_state(dfvo_pipeline* p, const uint32_t* h_state) {
    DFVO_ARG_CHECK(p && h_state, "dfvo_pipeline_set_rng_state: null argument");
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk()));
    DFVO_HIP_CHECK(hipMemcpy(p->slots[0].tb.mt_state, h_state, 625 * sizeof(uint32_t), hipMemcpyHostToDevice));
    return DFVO_OK;
}

int dfvo_pipeline_sync(dfvo_pipeline* p) {
    DFVO_ARG_CHECK(p, "null pipeline");
    for (int i = 0; i < p->flow_instances; ++i) DFVO_HIP_CHECK(hipStreamSynchronize(p->role[ROLE_FLOW + i]));
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_depth()));
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk()));
    return DFVO_OK;
}

int dfvo_pipeline_stream_layout(dfvo_pipeline* p, char* buf, int n) {
    DFVO_ARG_CHECK(p && buf && n > 0, "dfvo_pipeline_stream_layout: bad argument");
    // "layout=lanes groups=4 queues=4 streams=4 trk=3 rep0=3 ... flow_x=1": per role the index of its stream among the
    // pipeline's distinct streams (lanes: the lane), so equal numbers mean one stream.  (The side streams are slots[0].tb's:
    // its own in the creation-order fallback)
    std::vector<hipStream_t> role(p->role, p->role + ROLE_COUNT);
    role[ROLE_REP0] = p->slots[0].tb.s_rep[0];
    role[ROLE_REP1] = p->slots[0].tb.s_rep[1];
    std::vector<hipStream_t> distinct;
    if (p->plan.layout == LAYOUT_LANES) distinct.assign(p->lane, p->lane + 4);
    int idx[ROLE_COUNT];
    for (int r = 0; r < ROLE_COUNT; ++r) {
        idx[r] = -1;
        if (!role[r]) continue;
        auto it = std::find(distinct.begin(), distinct.end(), role[r]);
        idx[r] = (int)(it - distinct.begin());
        if (it == distinct.end()) distinct.push_back(role[r]);
    }
    int w = snprintf(buf, n, "layout=%s groups=%d queues=%d streams=%d", stream_layout_name(p->plan.layout), p->pool_groups,
                     p->pool_queues, (int)distinct.size());
    for (int r = 0; r < ROLE_COUNT && w > 0 && w < n; ++r) w += snprintf(buf + w, n - w, " %s=%d", stream_role_name(r), idx[r]);
    DFVO_ARG_CHECK(w > 0 && w < n, "dfvo_pipeline_stream_layout: the buffer is too small");
    return DFVO_OK;
}

double dfvo_pipeline_net_flops(const dfvo_pipeline* p) {
    if (!p) return 0.0;
    const double pose = p->pose.enable ? p->pose_net.flops_last : 0.0;
    if (deep_pose_tracking(p)) return pose;
    return pose + (p->dsrc.source == DFVO_DEPTH_EXTERNAL ? p->flow[0].flops_last : p->flow[0].flops_last + p->depth.flops_last);
}

}  // extern "C"

// the pose net on the depth stream (stream order is the whole synchronisation of the pose lane), built once
int finalize_pose_net(dfvo_pipeline* p) {
    if (!p->pose_net.stream) DFVO_TRY(p->pose_net.init(p->feedH, p->feedW, p->s_depth()));
    p->pose_net.baseline_mult = p->cfg.baseline_mult;
    return p->pose_net.finalize();
}
