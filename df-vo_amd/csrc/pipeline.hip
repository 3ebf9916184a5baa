// Fused per-pair tracking pipeline: both CNNs, keypoint selection, E-tracker and scale recovery chained
// on the device (three HIP streams), with two host round trips per pair (keypoint count, final pose).
// Orchestration follows /root/reference/libs/dfvo.py:299-345 (deep_model_inference) and :121-262
// (tracking): the host-side glue of the reference (cv2.resize nearest, preprocess_depth, dict passing)
// becomes device kernels; the pose composition stays on the host (dfvo.py:109-119).
// dfvo_pipeline_set_options selects the keypoint source (local_bestN | bestN | sampled), the validity and scale-RANSAC methods
// and hybrid | PnP-only tracking; dfvo_pipeline_set_iterative puts scale_recovery.method "iterative" (the one-call device loop
// of solver_scale.hip) in the place of find_scale_from_depth; dfvo_pipeline_set_depth_source puts a 16-bit depth image per
// frame (depth.depth_src gt, dfvo.py:296-319) in the place of the depth net; dfvo_pipeline_set_pose_net adds the pose lane
// (monodepth2's pose net, the depth-consistency keypoint mask, tracking_method deep_pose); without them the pipeline runs
// default_configuration.yml.
#include "../../include/dfvo_hip.h"
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nets.h"
#include "ops.h"
#include "pipeline_iter.h"
#include "resize_lanczos.h"
#include "stream_layout.h"
#include "tracker.h"

using namespace dfvo;

// what the RandomState-ordered chain of a pair leaves in pinned host memory behind Slot::e_res
struct ChainResult {
    PoseState pose;
    ScaleResult scale;
    PnpResult pnp;  // tracking_method PnP
};
static_assert(offsetof(ChainResult, scale) == sizeof(PoseState) && offsetof(ChainResult, pnp) == sizeof(PoseState) + sizeof(ScaleResult) &&
                  sizeof(ChainResult) == sizeof(PoseState) + sizeof(ScaleResult) + sizeof(PnpResult),
              "ChainResult is the three results back to back");

// a pair between dfvo_pipeline_track_begin and _end
enum Begun {
    IDLE,            // no chain pending
    NO_KEYPOINTS,    // the pending pair had no good keypoints
    NO_REF_DEPTH,    // PnP-only pair without a reference depth
    CHAIN_ENQUEUED,  // Slot::n keypoints went into the chain
};

// what each of the pairs in flight has of its own
struct Slot {
    TrackerBuffers tb;   // [0] owns the numpy RandomState and the RNG-side events, the others share them
    BestNBuffers bestn;  // kp_source bestN: the whole-image selection's workspace
    hipEvent_t e_flow = nullptr, e_depth = nullptr;
    // RNG-independent half of the solver stage (keypoint selection, homography chain) enqueued ahead of time
    // (dfvo_pipeline_prefetch_track): completion event and pinned keypoint info [n, good_kp_found, regions, -]
    hipEvent_t e_pre = nullptr;
    PinnedArr<int> h_info;
    bool prefetched = false;
    // dfvo_pipeline_track_begin / _end
    PinnedArr<ChainResult> h_res;
    hipEvent_t e_res = nullptr;
    Begun begun = IDLE;
    int n = 0;
    const double* depth_override = nullptr;
    // dfvo_pipeline_set_iterative: the loop's buffers and its record in pinned memory (copied ahead of e_res), the maps the
    // keypoint stage of the pending pair read, the caller's raw depth for the roll-over (until track_end)
    RigidKpBuffers rigid;
    PinnedArr<IterCtl> h_iter;
    const float* flow_in = nullptr;
    const float* diff_in = nullptr;
    const float* raw_override = nullptr;
    // outputs of the nets
    DevArr<float> fwd, bwd, diff, raw_depth;
    DevArr<double> proc_depth;
    // dfvo_pipeline_set_pose_net: the 4x4 the slot's pair uses (the net's, or the override's copy), the depth-difference map of
    // the mask, the caller's pose for the next pair enqueued here (until track_end), deep_pose tracking's pinned result
    DevArr<float> pose16, depth_diff;
    const float* pose_override = nullptr;
    PinnedArr<float> h_pose;
};

struct dfvo_pipeline {
    int H = 0, W = 0, feedH = 0, feedW = 0;
    FlowNet flow;
    // further flow-net instances, each on its own stream (DFVO_FLOW_INSTANCES, default 2): consecutive pairs rotate
    // over the instances, so the latency-bound coarse pyramid levels of one pass overlap the throughput-bound fine
    // levels of another (8.7 -> 7.1 ms per pair with two); costs one set of activations (~1.3 GB) per instance
    FlowNet flow_x[DFVO_PIPELINE_SLOTS - 1];
    int flow_instances = 1;
    DepthNet depth;
    Slot slots[DFVO_PIPELINE_SLOTS];
    int pending_slot = -1;  // the one pair begun and not yet collected (the chains consume ONE RandomState, in pair order)
    hipEvent_t e_ref = nullptr;  // reference depth of the first frame written (dfvo_pipeline_set_ref_image / _set_ref_depth)
    // the roll-over copy ref_depth <- proc_depth[slot] (s_trk) has read its source / written its target: the depth stream's
    // next writers of either wait for it on the device (recorded by roll_ref_depth, waited for once roll_pending)
    hipEvent_t e_roll = nullptr;
    bool roll_pending = false;
    DevArr<float> depth_small;
    LanczosResizer feed_resize;  // current frame -> depth-net feed size (when the caller passes no resized frame)
    DevArr<uint8_t> feed_buf;
    DevArr<double> d_T21;
    // scale_recovery.method iterative: the E-tracker's pose (cur -> ref, unit translation) beside its inverse, and
    // EssTracker.prev_scale, carried from pair to pair on the device (s_trk orders its readers and writers)
    DevArr<double> d_E_pose, d_prev_scale;
    dfvo_pipeline_iter_opts iter = {};
    RigidKpConfig iter_cfg = {};
    // PnP fallback: processed depth of the reference frame (= the previous pair's current frame)
    PnpBuffers pnp;
    DevArr<double> ref_depth;
    DevArr<float> ref_raw;
    bool has_ref_depth = false;
    dfvo_pipeline_cfg cfg;
    // dfvo_pipeline_set_options: the tracking configuration beyond default_configuration.yml (all zero = that configuration)
    dfvo_pipeline_opts opts = {};
    // dfvo_pipeline_set_depth_source: all zero = the depth net; EXTERNAL = 16-bit depth images (depth.depth_src gt), no depth net
    dfvo_pipeline_depth_src dsrc = {};
    // dfvo_pipeline_set_pose_net: all zero = no pose lane.  The net replays a captured graph, so its addresses are fixed: two
    // staging frames (pose_feed: reference | current, the current copied to the reference's behind the net) and one output
    // (pose_out, copied into the slot).  pose_ref_raw: the reference frame's raw depth as the NEXT pair's mask reads it -- the
    // raw depth of the slot the last enqueue_nets* call filled, or ref_raw after a set_ref_* call (null: neither came yet)
    dfvo_pipeline_pose_opts pose = {};
    PoseNet pose_net;
    DevArr<uint8_t> pose_feed;
    size_t pose_feed_pitch = 0;
    DevArr<float> pose_out;
    bool pose_ref_feed = false;  // pose_feed's reference half holds the previous call's current feed
    const float* pose_ref_raw = nullptr;
    bool started = false;                   // a pair or a reference depth was enqueued: the options are final
    DevArr<int> d_samples;                  // kp_source sampled: generate_kp_samples' index list, uploaded once
    int sample_crop[4] = {0, 0, 0, 0};      // y0 y1 x0 x1 [px] of cfg.crop.flow_crop
    bool nets_ready = false;
    const FlowNet* last_flow = nullptr;  // the instance that ran the previous pair (carry source of a d_ref == NULL call)
    // Streams.  `owned` is every stream the pipeline created or took from the pool, destroyed once by dfvo_pipeline_destroy;
    // the handles below it are the roles, plain copies.  s_pre: the two streams the run-ahead halves alternate on; s_rep: the
    // chain's side streams, lent to slots[0].tb (null: that object created its own, the creation-order fallback).
    // Stream layout (stream_layout.h).  LAYOUT_LANES: lane[0 .. 3] are the pipeline's only streams, one per hardware queue,
    // and every role's stream is one of them (s_flow, s_flow_x[0], s_depth = s_pre[0] = s_pre[1], s_trk = s_rep[0] = s_rep[1]);
    // otherwise every role has a stream to itself and lane[] is null.
    std::vector<hipStream_t> owned;
    hipStream_t s_flow = nullptr, s_depth = nullptr, s_trk = nullptr;
    hipStream_t s_flow_x[DFVO_PIPELINE_SLOTS - 1] = {};
    hipStream_t s_pre[2] = {nullptr, nullptr}, s_rep[2] = {nullptr, nullptr};
    hipStream_t lane[4] = {nullptr, nullptr, nullptr, nullptr};
    StreamPlan plan;
    int pool_groups = 0, pool_queues = 0;  // what the pool measured (0: no measurement)
};

#define P_TRY(expr)                     \
    do {                                \
        int _rc = (expr);               \
        if (_rc != DFVO_OK) return _rc; \
    } while (0)

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
    auto own = [&](hipStream_t s) {  // a stream taken from the pool
        if (s) p->owned.push_back(s);
        return s;
    };
    auto create_owned = [&](hipStream_t* s, bool solver) -> int {
        DFVO_HIP_CHECK(solver ? create_solver_stream(s) : create_net_stream(s));
        p->owned.push_back(*s);
        return DFVO_OK;
    };
    // two LiteFlowNet instances on two pipes, alternating pairs (measured 1 / 2 / 3: 217 / 287 / 272 pairs/s, profiles/
    // r3ag_flow_instances_ab.txt).  DFVO_FLOW_INSTANCES=1 is a test hook: the carry-over from a pass of the SAME instance
    p->flow_instances = getenv("DFVO_FLOW_INSTANCES") && atoi(getenv("DFVO_FLOW_INSTANCES")) == 1 ? 1 : 2;
    const bool fx = p->flow_instances > 1;
    // Streams by measurement (stream_pool.hip, stream_layout.h): twelve candidates, classified by dispatch pipe and by
    // hardware queue.  Eight or more queues: the wide layout, a stream per role -- pipe A / B: one flow-net instance each, pipe
    // C: the depth net + the two run-ahead homography chains, pipe D: the RandomState-ordered chain and its two side streams,
    // alone.  Four to seven queues (GPU_MAX_HW_QUEUES at the runtime's default of 4): eight busy streams would share queues,
    // and streams of one queue execute in host enqueue order -- a wait enqueued for one of them holds up the others' work;
    // the lane layout takes one stream from each of four queues and puts the roles of a lane on that one stream (flow |
    // flow_x | depth + pre-parts | chain + side streams), so which roles share a queue is decided here and not by the runtime.
    // DFVO_STREAM_LAYOUT=auto|wide|lanes forces one (A/B runs, tests).  Falls back to creation order when the probe does
    // not settle or finds too few groups / queues for the layout: the roles the pool did not fill stay null here and get
    // streams created below, in the order the pair rate was measured with (TrackerBuffers::init).
    {
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
        StreamPool pool;
        if (pool.create(12) == DFVO_OK && pool.ngroups > 0) {
            p->pool_groups = pool.ngroups;
            p->pool_queues = pool.nqueues;
        }
        StreamPlan plan = plan_stream_layout(p->pool_groups, p->pool_queues, choice);
        if (plan.layout == LAYOUT_LANES) {
            PoolClasses c;
            c.group = pool.group;
            c.queue_group = pool.queue_group;
            c.ngroups = pool.ngroups;
            c.nqueues = pool.nqueues;
            int pick[4];
            if (pick_lane_candidates(c, pick)) {
                for (int l = 0; l < 4; ++l) p->lane[l] = own(pool.take_index(pick[l]));
                auto of = [&](int role) { return p->lane[plan.lane[role]]; };
                p->s_trk = of(ROLE_TRK), p->s_rep[0] = of(ROLE_REP0), p->s_rep[1] = of(ROLE_REP1);
                p->s_depth = of(ROLE_DEPTH), p->s_pre[0] = of(ROLE_PRE0), p->s_pre[1] = of(ROLE_PRE1);
                p->s_flow = of(ROLE_FLOW);
                if (fx) p->s_flow_x[0] = of(ROLE_FLOW_X);
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
            if (full || (pool.count(g[0]) >= 3 && pool.count(g[1]) >= 3 && pool.count(g[2]) >= 1 && pool.count(g[3]) >= 1)) {
                p->s_trk = own(pool.take(from[ROLE_TRK]));
                p->s_rep[0] = own(pool.take(from[ROLE_REP0]));
                p->s_rep[1] = own(pool.take(from[ROLE_REP1]));
                p->s_depth = own(pool.take(from[ROLE_DEPTH]));
                p->s_pre[0] = own(pool.take(from[ROLE_PRE0]));
                p->s_pre[1] = own(pool.take(from[ROLE_PRE1]));
                p->s_flow = own(pool.take(from[ROLE_FLOW]));
                if (fx) p->s_flow_x[0] = own(pool.take(from[ROLE_FLOW_X]));
            }
            if (p->s_trk) p->plan = plan;
        }
        pool.release();
    }
    if (!p->s_trk && (create_owned(&p->s_flow, false) || create_owned(&p->s_depth, false) || create_owned(&p->s_trk, true))) {
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
    int rc = p->flow.init(p->H, p->W, p->s_flow);
    if (rc != DFVO_OK) return fail(rc);
    for (int i = 0; i + 1 < p->flow_instances; ++i) {
        if (!p->s_flow_x[i] && create_owned(&p->s_flow_x[i], false)) return fail(DFVO_ERR_HIP);
        rc = p->flow_x[i].init(p->H, p->W, p->s_flow_x[i]);
        if (rc != DFVO_OK) return fail(rc);
    }
    rc = p->depth.init(p->feedH, p->feedW, p->s_depth);
    if (rc != DFVO_OK) return fail(rc);
    p->depth.min_depth = cfg->net_min_depth;
    p->depth.max_depth = cfg->net_max_depth;
    p->depth.baseline_mult = cfg->baseline_mult;
    // (lanes: the chain's side streams are the chain's own stream)
    rc = p->s_rep[0] ? p->slots[0].tb.init(p->s_rep[0], p->s_rep[1], true) : p->slots[0].tb.init();
    if (rc != DFVO_OK) return fail(rc);
    for (int i = 1; i < DFVO_PIPELINE_SLOTS; i++) {
        rc = p->slots[i].tb.init_shared(p->slots[0].tb);
        if (rc != DFVO_OK) return fail(rc);
    }
    // the PnP fallback's buffers at their final size: grown lazily they would be freed and re-allocated (hipFree waits for
    // the whole device) whenever a pair with more keypoints than any before takes the fallback
    if (cfg->kp_num_bestN > 0 && cfg->pnp_iters > 0) {
        rc = p->pnp.ensure(cfg->kp_num_bestN + 8, cfg->pnp_iters);
        if (rc != DFVO_OK) return fail(rc);
    }
    for (int i = 0; i < 2; i++)
        if (!p->s_pre[i] && create_owned(&p->s_pre[i], true)) return fail(DFVO_ERR_HIP);
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
    enqueue_mt_seed(p->slots[0].tb, cfg->seed, p->s_trk);
    (void)hipStreamSynchronize(p->s_trk);
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
    for (int i = 0; i + 1 < p->flow_instances; ++i) P_TRY(pipe_store(&p->flow_x[i].params, name, h, ndim, shape));
    return pipe_store(&p->flow.params, name, h, ndim, shape);
}
int dfvo_pipeline_set_depth_param(dfvo_pipeline* p, const char* name, const float* h, int ndim, const int* shape) {
    DFVO_ARG_CHECK(p && !p->nets_ready, "dfvo_pipeline_set_depth_param: bad state");
    return pipe_store(&p->depth.params, name, h, ndim, shape);
}
int dfvo_pipeline_set_pose_param(dfvo_pipeline* p, const char* name, const float* h, int ndim, const int* shape) {
    DFVO_ARG_CHECK(p && !p->pose_net.finalized, "dfvo_pipeline_set_pose_param: bad state");
    return pipe_store(&p->pose_net.params, name, h, ndim, shape);
}
// the pose net on the depth stream (stream order is the whole synchronisation of the pose lane), built once
static int finalize_pose_net(dfvo_pipeline* p) {
    if (!p->pose_net.stream) P_TRY(p->pose_net.init(p->feedH, p->feedW, p->s_depth));
    p->pose_net.baseline_mult = p->cfg.baseline_mult;
    return p->pose_net.finalize();
}
int dfvo_pipeline_finalize(dfvo_pipeline* p) {
    DFVO_ARG_CHECK(p, "null pipeline");
    P_TRY(p->flow.finalize());
    for (int i = 0; i + 1 < p->flow_instances; ++i) P_TRY(p->flow_x[i].finalize());
    if (p->dsrc.source != DFVO_DEPTH_EXTERNAL) P_TRY(p->depth.finalize());  // (external depth: no parameters, no graph)
    if (p->pose.enable) P_TRY(finalize_pose_net(p));
    p->nets_ready = true;
    return DFVO_OK;
}
int dfvo_pipeline_set_graph(dfvo_pipeline* p, int enable) {
    DFVO_ARG_CHECK(p, "null pipeline");
    p->flow.use_graph = enable != 0;
    for (int i = 0; i + 1 < p->flow_instances; ++i) p->flow_x[i].use_graph = enable != 0;
    p->depth.use_graph = enable != 0;
    p->pose_net.use_graph = enable != 0;
    return DFVO_OK;
}

int dfvo_pipeline_set_pose_net(dfvo_pipeline* p, const dfvo_pipeline_pose_opts* o) {
    DFVO_ARG_CHECK(p && o, "dfvo_pipeline_set_pose_net: null argument");
    DFVO_ARG_CHECK(!p->started, "dfvo_pipeline_set_pose_net: comes before the first dfvo_pipeline_enqueue_nets / _set_ref_*");
    const bool deep = p->opts.tracking_method == DFVO_TRACKING_DEEP_POSE;
    if (!o->enable) {
        DFVO_ARG_CHECK(!o->depth_consistency, "dfvo_pipeline_set_pose_net: depth_consistency needs enable (the mask reads the net's pose)");
        DFVO_ARG_CHECK(!deep, "dfvo_pipeline_set_pose_net: tracking_method DFVO_TRACKING_DEEP_POSE needs the pose net");
        p->pose = {};
        return DFVO_OK;
    }
    if (o->depth_consistency) {
        DFVO_ARG_CHECK(p->opts.kp_source == DFVO_KP_SOURCE_LOCAL_BESTN,
                       "dfvo_pipeline_set_pose_net: depth_consistency masks kp_source DFVO_KP_SOURCE_LOCAL_BESTN only (kp_selection.py:118-148)");
        DFVO_ARG_CHECK(!deep, "dfvo_pipeline_set_pose_net: depth_consistency under tracking_method DFVO_TRACKING_DEEP_POSE: nothing "
                              "selects keypoints");
        DFVO_ARG_CHECK(o->depth_thre == o->depth_thre, "dfvo_pipeline_set_pose_net: depth_thre is NaN");
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
    if (p->nets_ready) P_TRY(finalize_pose_net(p));
    p->pose = *o;
    return DFVO_OK;
}

int dfvo_pipeline_set_pose_override(dfvo_pipeline* p, int slot, const float* d_pose16) {
    DFVO_ARG_CHECK(p && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS), "dfvo_pipeline_set_pose_override: bad argument");
    DFVO_ARG_CHECK(p->pose.enable, "dfvo_pipeline_set_pose_override: the pose net is not on (dfvo_pipeline_set_pose_net)");
    p->slots[slot].pose_override = d_pose16;
    return DFVO_OK;
}

int dfvo_pipeline_get_pose_net(dfvo_pipeline* p, int slot, float* h_pose16, float* h_depth_diff) {
    DFVO_ARG_CHECK(p && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS), "dfvo_pipeline_get_pose_net: bad argument");
    DFVO_ARG_CHECK(p->pose.enable, "dfvo_pipeline_get_pose_net: the pose net is not on (dfvo_pipeline_set_pose_net)");
    DFVO_ARG_CHECK(!h_depth_diff || p->pose.depth_consistency, "dfvo_pipeline_get_pose_net: no depth-difference map without depth_consistency");
    const Slot& sl = p->slots[slot];
    DFVO_HIP_CHECK(hipDeviceSynchronize());
    if (h_pose16) DFVO_HIP_CHECK(hipMemcpy(h_pose16, sl.pose16, 16 * sizeof(float), hipMemcpyDeviceToHost));
    if (h_depth_diff) DFVO_HIP_CHECK(hipMemcpy(h_depth_diff, sl.depth_diff, (size_t)p->H * p->W * sizeof(float), hipMemcpyDeviceToHost));
    return DFVO_OK;
}
int dfvo_pipeline_seed(dfvo_pipeline* p, uint32_t seed) {
    DFVO_ARG_CHECK(p, "null pipeline");
    // synchronous: the first RandomState consumer of the next pair (the keypoint shuffles) runs on tb.s_rep[0], which is
    // ordered after the keypoint stage but not after s_trk -- the new key must be in place before track() is called
    P_TRY(enqueue_mt_seed(p->slots[0].tb, seed, p->s_trk));
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk));
    return DFVO_OK;
}

int dfvo_pipeline_set_options(dfvo_pipeline* p, const dfvo_pipeline_opts* o) {
    DFVO_ARG_CHECK(p && o, "dfvo_pipeline_set_options: null argument");
    DFVO_ARG_CHECK(!p->started, "dfvo_pipeline_set_options: comes before the first dfvo_pipeline_enqueue_nets / _set_ref_*");
    DFVO_ARG_CHECK(o->kp_source >= DFVO_KP_SOURCE_LOCAL_BESTN && o->kp_source <= DFVO_KP_SOURCE_SAMPLED,
                   "dfvo_pipeline_set_options: kp_source is DFVO_KP_SOURCE_LOCAL_BESTN, _BESTN or _SAMPLED");
    DFVO_ARG_CHECK(o->kp_score_method == DFVO_KP_SCORE_FLOW || o->kp_score_method == DFVO_KP_SCORE_FLOW_RATIO,
                   "dfvo_pipeline_set_options: kp_score_method is DFVO_KP_SCORE_FLOW or DFVO_KP_SCORE_FLOW_RATIO");
    DFVO_ARG_CHECK(o->validity_method >= DFVO_VALIDITY_GRIC && o->validity_method <= DFVO_VALIDITY_HOMO_RATIO,
                   "dfvo_pipeline_set_options: validity_method is DFVO_VALIDITY_GRIC, _FLOW or _HOMO_RATIO");
    DFVO_ARG_CHECK(o->validity_method == DFVO_VALIDITY_GRIC || o->validity_thre == o->validity_thre,
                   "dfvo_pipeline_set_options: validity_thre is NaN");
    DFVO_ARG_CHECK(o->scale_method == DFVO_SCALE_DEPTH_RATIO || o->scale_method == DFVO_SCALE_ABS_DIFF,
                   "dfvo_pipeline_set_options: scale_method is DFVO_SCALE_DEPTH_RATIO or DFVO_SCALE_ABS_DIFF");
    DFVO_ARG_CHECK(o->tracking_method == DFVO_TRACKING_HYBRID || o->tracking_method == DFVO_TRACKING_PNP ||
                       (o->tracking_method == DFVO_TRACKING_DEEP_POSE && p->pose.enable && !p->pose.depth_consistency),
                   "dfvo_pipeline_set_options: tracking_method is DFVO_TRACKING_HYBRID, DFVO_TRACKING_PNP or, behind "
                   "dfvo_pipeline_set_pose_net with enable and without depth_consistency, DFVO_TRACKING_DEEP_POSE");
    DFVO_ARG_CHECK(!p->pose.depth_consistency || o->kp_source == DFVO_KP_SOURCE_LOCAL_BESTN,
                   "dfvo_pipeline_set_options: kp_source with dfvo_pipeline_set_pose_net's depth_consistency is DFVO_KP_SOURCE_LOCAL_BESTN, "
                   "the only source the reference masks");
    const dfvo_pipeline_cfg& c = p->cfg;
    // every buffer the chosen source needs at its final size, here: nothing on the per-pair path allocates (hipFree waits
    // for the whole device).  kp_count stays 0 for local_bestN, whose launcher sizes its own buffers as before
    int kp_count = 0;
    int crop[4] = {0, 0, 0, 0};
    std::vector<int> samples;
    if (o->kp_source == DFVO_KP_SOURCE_BESTN) {
        DFVO_ARG_CHECK(c.kp_num_bestN >= 1, "dfvo_pipeline_set_options: bestN needs kp_num_bestN >= 1");
        kp_count = c.kp_num_bestN;
    } else if (o->kp_source == DFVO_KP_SOURCE_SAMPLED) {
        DFVO_ARG_CHECK(o->kp_sampled_num >= 1, "dfvo_pipeline_set_options: sampled needs kp_sampled_num >= 1");
        for (int i = 0; i < 4; ++i)
            DFVO_ARG_CHECK(o->flow_crop[i] >= 0.0 && o->flow_crop[i] <= 1.0, "dfvo_pipeline_set_options: flow_crop fractions lie in [0, 1]");
        crop[0] = (int)(o->flow_crop[0] * p->H);
        crop[1] = (int)(o->flow_crop[1] * p->H);
        crop[2] = (int)(o->flow_crop[2] * p->W);
        crop[3] = (int)(o->flow_crop[3] * p->W);
        DFVO_ARG_CHECK(crop[0] < crop[1] && crop[2] < crop[3], "dfvo_pipeline_set_options: flow_crop is empty");
        kp_count = o->kp_sampled_num;
        samples.resize(kp_count);
        generate_kp_samples(crop[0], crop[1], crop[2], crop[3], kp_count, samples.data());
    }
    DFVO_ARG_CHECK(!(p->iter.enable && p->iter.kp_src == DFVO_ITER_KP_BEST && kp_count > ITER_MAX_KP),
                   "dfvo_pipeline_set_options: more tracked keypoints than the iterative scale loop takes (16384)");
    p->d_samples.release();
    if (!samples.empty()) {
        P_TRY(p->d_samples.alloc(samples.size()));
        DFVO_HIP_CHECK(hipMemcpy(p->d_samples, samples.data(), sizeof(int) * samples.size(), hipMemcpyHostToDevice));
    }
    if (kp_count > 0) {
        for (int i = 0; i < DFVO_PIPELINE_SLOTS; i++) {
            P_TRY(p->slots[i].tb.ensure_kp(kp_count, 1, 1));
            if (o->kp_source == DFVO_KP_SOURCE_BESTN) P_TRY(p->slots[i].bestn.ensure((size_t)p->H * p->W, 0));
        }
        if (c.pnp_iters > 0) P_TRY(p->pnp.ensure(kp_count + 8, c.pnp_iters));
    }
    for (int i = 0; i < 4; ++i) p->sample_crop[i] = crop[i];
    p->opts = *o;
    return DFVO_OK;
}

int dfvo_pipeline_set_depth_source(dfvo_pipeline* p, const dfvo_pipeline_depth_src* d) {
    DFVO_ARG_CHECK(p && d, "dfvo_pipeline_set_depth_source: null argument");
    DFVO_ARG_CHECK(!p->started && !p->nets_ready,
                   "dfvo_pipeline_set_depth_source: comes before dfvo_pipeline_finalize and the first dfvo_pipeline_enqueue_nets / _set_ref_*");
    DFVO_ARG_CHECK(d->source == DFVO_DEPTH_NET || d->source == DFVO_DEPTH_EXTERNAL,
                   "dfvo_pipeline_set_depth_source: source is DFVO_DEPTH_NET or DFVO_DEPTH_EXTERNAL");
    if (d->source == DFVO_DEPTH_NET) {
        p->dsrc = {};
        return DFVO_OK;
    }
    DFVO_ARG_CHECK(d->scale > 0.0 && d->scale <= 1.7976931348623157e308, "dfvo_pipeline_set_depth_source: scale must be finite and > 0");
    DFVO_ARG_CHECK(d->src_h >= 1 && d->src_w >= 1, "dfvo_pipeline_set_depth_source: src_h, src_w >= 1");
    p->dsrc = *d;
    return DFVO_OK;
}

static int pipeline_kp_max(const dfvo_pipeline* p) {
    const dfvo_pipeline_cfg& c = p->cfg;
    return tracked_kp_max(p->opts.kp_source, p->opts.kp_sampled_num, c.kp_num_bestN, c.kp_num_row, c.kp_num_col);
}

int dfvo_pipeline_set_iterative(dfvo_pipeline* p, const dfvo_pipeline_iter_opts* o) {
    DFVO_ARG_CHECK(p && o, "dfvo_pipeline_set_iterative: null argument");
    DFVO_ARG_CHECK(!p->started, "dfvo_pipeline_set_iterative: comes before the first dfvo_pipeline_enqueue_nets / _set_ref_*");
    if (!o->enable) {
        p->iter = {};
        return DFVO_OK;
    }
    const dfvo_pipeline_cfg& c = p->cfg;
    if (const char* why = iter_opts_refusal(*o, c.scale_min_samples)) {
        dfvo::set_last_error(why);
        return DFVO_ERR_ARG;
    }
    const RigidKpConfig rc = iter_rigid_config(*o, c.fx, c.fy, c.cx, c.cy, c.Kinv);
    int cells, n_best, cap, par;
    size_t lds;
    P_TRY(rigid_flow_kp_geometry(p->H, p->W, rc, &cells, &n_best, &cap, &lds, &par));  // the launcher's refusals
    const int n_sel = cells * n_best, n_trk = pipeline_kp_max(p);
    DFVO_ARG_CHECK(iter_kp_count_ok(o->kp_src, n_sel, n_trk),
                   "dfvo_pipeline_set_iterative: more keypoints than the depth-ratio kernel holds in 64 KB of LDS (16384)");
    // every buffer of the loop at its final size, here: nothing on the per-pair path allocates.  The scale stage's
    // keypoint-sized buffers hold a round's uniform set as well as the tracked set; local_bestN keeps its selection lists
    const int kp_need = std::max(std::max(n_sel, n_trk), 16);
    const bool lb = p->opts.kp_source == DFVO_KP_SOURCE_LOCAL_BESTN;
    const int lb_cells = lb ? c.kp_num_row * c.kp_num_col : 1, lb_best = lb && lb_cells > 0 ? c.kp_num_bestN / lb_cells : 1;
    for (Slot& sl : p->slots) {
        P_TRY(sl.rigid.ensure(p->H, p->W, cells, n_best, cap));
        P_TRY(sl.tb.ensure_kp(kp_need, lb_cells > 0 ? lb_cells : 1, lb_best > 0 ? lb_best : 1));
        P_TRY(sl.tb.grow_winner(p->H, p->W));
        if (!sl.h_iter && sl.h_iter.alloc(1)) return DFVO_ERR_HIP;
        iter_record_reset(sl.h_iter);
    }
    p->iter = *o;
    p->iter_cfg = rc;
    return DFVO_OK;
}

int dfvo_pipeline_get_prev_scale(dfvo_pipeline* p, double* h_scale) {
    DFVO_ARG_CHECK(p && h_scale, "dfvo_pipeline_get_prev_scale: null argument");
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk));
    DFVO_HIP_CHECK(hipMemcpy(h_scale, p->d_prev_scale, sizeof(double), hipMemcpyDeviceToHost));
    return DFVO_OK;
}

int dfvo_pipeline_set_prev_scale(dfvo_pipeline* p, double scale) {
    DFVO_ARG_CHECK(p, "dfvo_pipeline_set_prev_scale: null pipeline");
    DFVO_ARG_CHECK(p->pending_slot == -1, "dfvo_pipeline_set_prev_scale: a pair is begun and not yet collected");
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk));
    DFVO_HIP_CHECK(hipMemcpy(p->d_prev_scale, &scale, sizeof(double), hipMemcpyHostToDevice));
    return DFVO_OK;
}

// preprocess_depth of the depth net's output (crop, clamp, nearest resize to the image size) into a raw / processed pair, on
// the depth stream.  Either target may still be read or written by the last roll-over copy on s_trk (proc_depth[slot] is its
// source, ref_depth its target; track_end does not wait for it on the host): ordered behind it.  Placed after the net, so
// nothing stalls in practice.
static int enqueue_depth_post(dfvo_pipeline* p, float* raw, double* proc) {
    const dfvo_pipeline_cfg& c = p->cfg;
    const int y0 = (int)(p->H * c.depth_crop[0]), y1 = (int)(p->H * c.depth_crop[1]);
    const int x0 = (int)(p->W * c.depth_crop[2]), x1 = (int)(p->W * c.depth_crop[3]);
    if (p->roll_pending) DFVO_HIP_CHECK(hipStreamWaitEvent(p->s_depth, p->e_roll, 0));
    return launch_depth_post(p->depth_small, p->feedH, p->feedW, p->H, p->W, y0, y1, x0, x1, (float)c.min_depth, (float)c.max_depth,
                             raw, proc, p->s_depth);
}

// the same pair from a 16-bit depth image (read_depth + preprocess_depth, dfvo_read_depth_u16), under the same ordering
static int enqueue_read_depth(dfvo_pipeline* p, const uint16_t* d_u16, float* raw, double* proc) {
    const dfvo_pipeline_cfg& c = p->cfg;
    const int y0 = (int)(p->H * c.depth_crop[0]), y1 = (int)(p->H * c.depth_crop[1]);
    const int x0 = (int)(p->W * c.depth_crop[2]), x1 = (int)(p->W * c.depth_crop[3]);
    if (p->roll_pending) DFVO_HIP_CHECK(hipStreamWaitEvent(p->s_depth, p->e_roll, 0));
    return dfvo_read_depth_u16(d_u16, p->dsrc.src_h, p->dsrc.src_w, p->dsrc.scale, p->H, p->W, y0, y1, x0, x1, c.min_depth, c.max_depth, raw,
                               proc, p->s_depth);
}

static int enqueue_flow_half(dfvo_pipeline* p, int slot, const uint8_t* d_ref, const uint8_t* d_cur);

static bool deep_pose_tracking(const dfvo_pipeline* p) { return p->opts.tracking_method == DFVO_TRACKING_DEEP_POSE; }

// what a pair's pose lane needs from earlier calls, checked before anything of the pair is enqueued
static int check_pose_lane(const dfvo_pipeline* p, const uint8_t* d_ref, const char* who) {
    if (!d_ref && !p->pose_ref_feed) {
        dfvo::set_last_error(std::string(who) + ": d_ref == NULL (reference frame = the previous call's current frame) needs a previous call");
        return DFVO_ERR_ARG;
    }
    if (p->pose.depth_consistency && !p->pose_ref_raw) {
        dfvo::set_last_error(std::string(who) + ": the depth-consistency mask needs the reference frame's raw depth: "
                             "dfvo_pipeline_set_ref_image / _set_ref_depth (d_feed) / _set_ref_depth_u16 / _set_ref_raw_depth first");
        return DFVO_ERR_ARG;
    }
    return DFVO_OK;
}

// A pair enqueued into the slot the previous pair used: the slot's raw depth is the mask's reference depth and is about to be
// overwritten with the current frame's, so it moves to ref_raw first (on the depth stream, behind a pending roll-over, which is
// ref_raw's other writer)
static int keep_ref_raw(dfvo_pipeline* p, Slot& sl) {
    if (!p->pose.depth_consistency || p->pose_ref_raw != sl.raw_depth.p) return DFVO_OK;
    if (p->roll_pending) DFVO_HIP_CHECK(hipStreamWaitEvent(p->s_depth, p->e_roll, 0));
    DFVO_HIP_CHECK(hipMemcpyAsync(p->ref_raw, sl.raw_depth, (size_t)p->H * p->W * sizeof(float), hipMemcpyDeviceToDevice, p->s_depth));
    p->pose_ref_raw = p->ref_raw.p;
    return DFVO_OK;
}

// The pose lane of a pair, on the depth stream behind the slot's raw depth (deep_models.py:217-230, depth_consistency.py:69-151):
// both feed images into the net's fixed staging frames, the net, its 4x4 (or the caller's) into the slot, the current feed kept as
// the next pair's reference feed, and with the mask on the depth-difference map from the pose where it lies, in device memory.
// d_cur_feed: the current frame at feed size (the caller's or the depth net's), or null to resize d_cur here.
// Stream order is all the synchronisation there is: the previous slot's raw depth was written on this stream, and is overwritten
// on it three pairs later.  ref_raw's other writer is the iterative loop's roll-over on s_trk, under the e_roll rule.
static int enqueue_pose_lane(dfvo_pipeline* p, int slot, const uint8_t* d_ref, const uint8_t* d_cur, const uint8_t* d_cur_feed) {
    Slot& sl = p->slots[slot];
    hipStream_t s = p->s_depth;
    const size_t feed_bytes = (size_t)p->feedH * p->feedW * 3;
    uint8_t* feed_ref = p->pose_feed.p;
    uint8_t* feed_cur = p->pose_feed.p + p->pose_feed_pitch;
    if (d_cur_feed)
        DFVO_HIP_CHECK(hipMemcpyAsync(feed_cur, d_cur_feed, feed_bytes, hipMemcpyDeviceToDevice, s));
    else
        P_TRY(p->feed_resize.enqueue(d_cur, feed_cur, s));
    if (d_ref) P_TRY(p->feed_resize.enqueue(d_ref, feed_ref, s));
    P_TRY(p->pose_net.forward(feed_ref, feed_cur, p->pose_out, nullptr));
    const float* pose = sl.pose_override ? sl.pose_override : p->pose_out.p;
    DFVO_HIP_CHECK(hipMemcpyAsync(sl.pose16, pose, 16 * sizeof(float), hipMemcpyDeviceToDevice, s));
    DFVO_HIP_CHECK(hipMemcpyAsync(feed_ref, feed_cur, feed_bytes, hipMemcpyDeviceToDevice, s));
    p->pose_ref_feed = true;
    if (p->pose.depth_consistency) {
        const dfvo_pipeline_cfg& c = p->cfg;
        const float K[9] = {(float)c.fx, 0.f, (float)c.cx, 0.f, (float)c.fy, (float)c.cy, 0.f, 0.f, 1.f};
        float Kinv[9];
        for (int i = 0; i < 9; ++i) Kinv[i] = (float)c.Kinv[i];
        if (p->pose_ref_raw == p->ref_raw.p && p->roll_pending) DFVO_HIP_CHECK(hipStreamWaitEvent(s, p->e_roll, 0));
        P_TRY(launch_depth_consistency_dev(sl.raw_depth, p->pose_ref_raw, p->H, p->W, K, Kinv, sl.pose16, sl.depth_diff, s));
        p->pose_ref_raw = sl.raw_depth.p;
    }
    return DFVO_OK;
}

int dfvo_pipeline_enqueue_nets(dfvo_pipeline* p, int slot, const uint8_t* d_ref, const uint8_t* d_cur,
                               const uint8_t* d_cur_feed) {
    DFVO_ARG_CHECK(p && p->nets_ready && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS) && d_cur,
                   "dfvo_pipeline_enqueue_nets: bad argument");
    DFVO_ARG_CHECK(p->dsrc.source == DFVO_DEPTH_NET, "dfvo_pipeline_enqueue_nets: the depth source is DFVO_DEPTH_EXTERNAL (no depth net): "
                                                     "dfvo_pipeline_enqueue_nets_depth takes the pair's depth image");
    if (p->pose.enable) P_TRY(check_pose_lane(p, d_ref, "dfvo_pipeline_enqueue_nets"));
    if (deep_pose_tracking(p)) {  // dfvo.py:302: neither the depth net nor the flow net
        p->started = true;
        P_TRY(enqueue_pose_lane(p, slot, d_ref, d_cur, d_cur_feed));
        DFVO_HIP_CHECK(hipEventRecord(p->slots[slot].e_depth, p->s_depth));
        return DFVO_OK;
    }
    DFVO_ARG_CHECK(d_ref || p->last_flow, "dfvo_pipeline_enqueue_nets: d_ref == NULL (reference frame = the previous call's "
                                          "current frame) needs a previous call");
    p->started = true;
    Slot& sl = p->slots[slot];
    P_TRY(keep_ref_raw(p, sl));
    // depth of the current frame (dfvo.py:305-319); without a caller-resized frame the LANCZOS resize of
    // deep_models.py:195-199 runs here, ahead of the net on its stream
    if (!d_cur_feed) {
        P_TRY(p->feed_resize.enqueue(d_cur, p->feed_buf, p->s_depth));
        d_cur_feed = p->feed_buf;
    }
    P_TRY(p->depth.forward(d_cur_feed, p->depth_small));
    P_TRY(enqueue_depth_post(p, sl.raw_depth, sl.proc_depth));
    if (p->pose.enable) P_TRY(enqueue_pose_lane(p, slot, d_ref, d_cur, d_cur_feed));
    DFVO_HIP_CHECK(hipEventRecord(sl.e_depth, p->s_depth));
    return enqueue_flow_half(p, slot, d_ref, d_cur);
}

int dfvo_pipeline_enqueue_nets_depth(dfvo_pipeline* p, int slot, const uint8_t* d_ref, const uint8_t* d_cur, const uint16_t* d_depth_u16) {
    DFVO_ARG_CHECK(p && p->nets_ready && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS) && d_cur && d_depth_u16,
                   "dfvo_pipeline_enqueue_nets_depth: bad argument");
    DFVO_ARG_CHECK(p->dsrc.source == DFVO_DEPTH_EXTERNAL, "dfvo_pipeline_enqueue_nets_depth: the depth source is DFVO_DEPTH_NET "
                                                          "(dfvo_pipeline_set_depth_source): dfvo_pipeline_enqueue_nets runs the depth net");
    if (p->pose.enable) P_TRY(check_pose_lane(p, d_ref, "dfvo_pipeline_enqueue_nets_depth"));
    if (deep_pose_tracking(p)) {  // (the depth image has no reader)
        p->started = true;
        P_TRY(enqueue_pose_lane(p, slot, d_ref, d_cur, nullptr));
        DFVO_HIP_CHECK(hipEventRecord(p->slots[slot].e_depth, p->s_depth));
        return DFVO_OK;
    }
    DFVO_ARG_CHECK(d_ref || p->last_flow, "dfvo_pipeline_enqueue_nets_depth: d_ref == NULL (reference frame = the previous call's "
                                          "current frame) needs a previous call");
    p->started = true;
    Slot& sl = p->slots[slot];
    P_TRY(keep_ref_raw(p, sl));
    // depth of the current frame: the sensor's image where dfvo.py:305-319 runs the depth net
    P_TRY(enqueue_read_depth(p, d_depth_u16, sl.raw_depth, sl.proc_depth));
    if (p->pose.enable) P_TRY(enqueue_pose_lane(p, slot, d_ref, d_cur, nullptr));  // (the LANCZOS feed for the pose net alone)
    DFVO_HIP_CHECK(hipEventRecord(sl.e_depth, p->s_depth));
    return enqueue_flow_half(p, slot, d_ref, d_cur);
}

static int enqueue_flow_half(dfvo_pipeline* p, int slot, const uint8_t* d_ref, const uint8_t* d_cur) {
    Slot& sl = p->slots[slot];
    const size_t px = (size_t)p->H * p->W;
    // forward/backward flow (dfvo.py:321-335)
    const int inst = slot % p->flow_instances;
    FlowNet& fn = inst == 0 ? p->flow : p->flow_x[inst - 1];
    hipStream_t sf = fn.stream;
    // frame pointers may change per pair (not captured).  d_ref == NULL: the image / feature pyramids of the reference frame
    // are carried over from the pass that saw it as its current frame (the other flow-net instance, normally)
    // Whatever this pass is (carried or not), it overwrites this instance's pyramids: the previous pass -- normally on the
    // OTHER instance -- may still be copying them (its carry-over reads this instance's current-frame pyramids), so this
    // stream is ordered behind that pass's feature stage.  A carried pass waits for the same event anyway; a full pass
    // enqueued right behind a carried one without a sync in between would otherwise race with that copy.
    if (p->last_flow && p->last_flow != &fn && p->last_flow->e_feat) DFVO_HIP_CHECK(hipStreamWaitEvent(sf, p->last_flow->e_feat, 0));
    // (the net writing the slot's buffers itself, one levels graph per slot, was measured: no gain -- profiles/r3x_copy_ab.txt)
    P_TRY(fn.forward(d_ref, d_cur, fn.out_fwd.p, fn.out_bwd.p, fn.out_diff.p, d_ref ? nullptr : p->last_flow));
    DFVO_HIP_CHECK(hipMemcpyAsync(sl.fwd, fn.out_fwd.p, 2 * px * sizeof(float), hipMemcpyDeviceToDevice, sf));
    DFVO_HIP_CHECK(hipMemcpyAsync(sl.bwd, fn.out_bwd.p, 2 * px * sizeof(float), hipMemcpyDeviceToDevice, sf));
    DFVO_HIP_CHECK(hipMemcpyAsync(sl.diff, fn.out_diff.p, px * sizeof(float), hipMemcpyDeviceToDevice, sf));
    p->last_flow = &fn;
    DFVO_HIP_CHECK(hipEventRecord(sl.e_flow, sf));
    return DFVO_OK;
}

int dfvo_pipeline_set_ref_depth(dfvo_pipeline* p, const uint8_t* d_feed, const double* d_depth_override) {
    DFVO_ARG_CHECK(p && p->nets_ready && ((d_feed != nullptr) != (d_depth_override != nullptr)),
                   "dfvo_pipeline_set_ref_depth: exactly one of d_feed / d_depth_override");
    DFVO_ARG_CHECK(!d_feed || p->dsrc.source == DFVO_DEPTH_NET, "dfvo_pipeline_set_ref_depth: d_feed with the depth source DFVO_DEPTH_EXTERNAL "
                                                                "(no depth net): dfvo_pipeline_set_ref_depth_u16 or d_depth_override");
    p->started = true;
    const size_t px = (size_t)p->H * p->W;
    if (d_depth_override) {
        DFVO_HIP_CHECK(hipMemcpyAsync(p->ref_depth, d_depth_override, px * sizeof(double), hipMemcpyDeviceToDevice, p->s_trk));
        DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk));
    } else {
        P_TRY(p->depth.forward(d_feed, p->depth_small));
        P_TRY(enqueue_depth_post(p, p->ref_raw, p->ref_depth));
        // not waited for on the host: the solver stream (PnP fallback reads the reference depth, the roll-over writes it)
        // is ordered behind it on the device, the depth stream runs its later passes in order anyway
        DFVO_HIP_CHECK(hipEventRecord(p->e_ref, p->s_depth));
        DFVO_HIP_CHECK(hipStreamWaitEvent(p->s_trk, p->e_ref, 0));
        p->pose_ref_raw = p->ref_raw.p;  // (written on the depth stream: the mask's read is in stream order)
    }
    p->has_ref_depth = true;
    return DFVO_OK;
}

int dfvo_pipeline_set_ref_image(dfvo_pipeline* p, const uint8_t* d_img) {
    DFVO_ARG_CHECK(p && p->nets_ready && d_img, "dfvo_pipeline_set_ref_image: bad argument");
    DFVO_ARG_CHECK(p->dsrc.source == DFVO_DEPTH_NET, "dfvo_pipeline_set_ref_image: the depth source is DFVO_DEPTH_EXTERNAL (no depth net): "
                                                     "dfvo_pipeline_set_ref_depth_u16 takes the first frame's depth image");
    P_TRY(p->feed_resize.enqueue(d_img, p->feed_buf, p->s_depth));
    return dfvo_pipeline_set_ref_depth(p, p->feed_buf, nullptr);
}

int dfvo_pipeline_set_ref_depth_u16(dfvo_pipeline* p, const uint16_t* d_depth_u16) {
    DFVO_ARG_CHECK(p && p->nets_ready && d_depth_u16, "dfvo_pipeline_set_ref_depth_u16: bad argument");
    DFVO_ARG_CHECK(p->dsrc.source == DFVO_DEPTH_EXTERNAL, "dfvo_pipeline_set_ref_depth_u16: the depth source is DFVO_DEPTH_NET "
                                                          "(dfvo_pipeline_set_depth_source): dfvo_pipeline_set_ref_image / _set_ref_depth");
    p->started = true;
    P_TRY(enqueue_read_depth(p, d_depth_u16, p->ref_raw, p->ref_depth));
    // (ordered as the depth net's reference depth is: the solver stream behind it on the device, no host wait)
    DFVO_HIP_CHECK(hipEventRecord(p->e_ref, p->s_depth));
    DFVO_HIP_CHECK(hipStreamWaitEvent(p->s_trk, p->e_ref, 0));
    p->pose_ref_raw = p->ref_raw.p;
    p->has_ref_depth = true;
    return DFVO_OK;
}

int dfvo_pipeline_set_ref_raw_depth(dfvo_pipeline* p, const float* d_raw) {
    DFVO_ARG_CHECK(p && d_raw, "dfvo_pipeline_set_ref_raw_depth: null argument");
    p->started = true;
    DFVO_HIP_CHECK(hipMemcpyAsync(p->ref_raw, d_raw, (size_t)p->H * p->W * sizeof(float), hipMemcpyDeviceToDevice, p->s_trk));
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk));
    p->pose_ref_raw = p->ref_raw.p;  // (complete: the host waited)
    return DFVO_OK;
}

int dfvo_pipeline_set_raw_depth_override(dfvo_pipeline* p, int slot, const float* d_raw) {
    DFVO_ARG_CHECK(p && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS), "dfvo_pipeline_set_raw_depth_override: bad argument");
    p->slots[slot].raw_override = d_raw;
    return DFVO_OK;
}

// the current frame's depth becomes the reference depth of the next pair (dfvo.py:  ref_data <- cur_data); with the iterative
// scale loop on, its raw depth becomes ref_data['raw_depth'] as well, under the same e_roll ordering
static int roll_ref_depth(dfvo_pipeline* p, int slot, const double* d_depth_override) {
    const size_t px = (size_t)p->H * p->W;
    Slot& sl = p->slots[slot];
    DFVO_HIP_CHECK(hipStreamWaitEvent(p->s_trk, sl.e_depth, 0));
    const double* depth = d_depth_override ? d_depth_override : sl.proc_depth.p;
    DFVO_HIP_CHECK(hipMemcpyAsync(p->ref_depth, depth, px * sizeof(double), hipMemcpyDeviceToDevice, p->s_trk));
    if (p->iter.enable) {
        const float* raw = sl.raw_override ? sl.raw_override : sl.raw_depth.p;
        DFVO_HIP_CHECK(hipMemcpyAsync(p->ref_raw, raw, px * sizeof(float), hipMemcpyDeviceToDevice, p->s_trk));
    }
    sl.raw_override = nullptr;
    DFVO_HIP_CHECK(hipEventRecord(p->e_roll, p->s_trk));
    p->roll_pending = true;
    p->has_ref_depth = true;
    return DFVO_OK;
}

static void fill_pose_cfg(const dfvo_pipeline_cfg& c, const dfvo_pipeline_opts& o, PoseConfig* pc) {
    pc->validity = o.validity_method;
    pc->validity_thre = o.validity_method == DFVO_VALIDITY_GRIC ? 0.0 : o.validity_thre;
    pc->fx = c.fx;
    pc->cx = c.cx;
    pc->cy = c.cy;
    pc->reproj_thre = c.e_reproj_thre;
    pc->repeat = c.e_repeat;
    pc->max_iters = c.e_max_iters;
    for (int i = 0; i < 9; i++) {
        pc->KinvT[i] = c.KinvT[i];
        pc->Kinv[i] = c.Kinv[i];
    }
}

static void fill_pnp_cfg(const dfvo_pipeline_cfg& c, PnpConfig* pc3) {
    pc3->fx = c.fx;
    pc3->fy = c.fy;
    pc3->cx = c.cx;
    pc3->cy = c.cy;
    for (int i = 0; i < 9; i++) pc3->inv_K[i] = c.Kinv[i];
    pc3->min_depth = c.min_depth;
    pc3->max_depth = c.max_depth;
    pc3->repeat = c.pnp_repeat;
    pc3->iters = c.pnp_iters;
    pc3->reproj_thre = c.pnp_reproj_thre;
}

static void fill_scale_cfg(const dfvo_pipeline_cfg& c, const dfvo_pipeline_opts& o, ScaleConfig* sc) {
    sc->cx = c.cx;
    sc->cy = c.cy;
    sc->fx = c.fx;
    sc->fy = c.fy;
    sc->min_samples = c.scale_min_samples;
    sc->max_trials = c.scale_max_trials;
    sc->stop_prob = c.scale_stop_prob;
    sc->thre = c.scale_thre;
    sc->method = o.scale_method;
}

static void fill_pnp_out(const PnpResult& pr, dfvo_track_out* out) {
    for (int i = 0; i < 9; i++) out->R[i] = pr.R[i];
    for (int i = 0; i < 3; i++) out->t[i] = pr.tvec[i];
    out->scale = 1.0;
    out->pnp_found = pr.found;
    out->pnp_inliers = pr.best_inliers;
    out->pnp_n_filtered = pr.n_filtered;
    out->status = DFVO_TRACK_PNP;
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
        P_TRY(enqueue_bestn_flow_kp(sl.bestn, flow, diff, p->H, p->W, c.kp_num_bestN, sp, tb.kp_ref, tb.kp_cur, tb.kp_info));
    } else if (o.kp_source == DFVO_KP_SOURCE_SAMPLED) {
        P_TRY(enqueue_kp_sampled(flow, p->H, p->W, p->sample_crop[0], p->sample_crop[1], p->sample_crop[2], p->sample_crop[3],
                                 p->d_samples, o.kp_sampled_num, tb.kp_ref, tb.kp_cur, sp, tb.kp_info));
    } else {
        // the depth mask (kp_selection.py:118-119,145-148): the slot's map, written by the pose lane ahead of e_depth
        const bool mask = p->pose.depth_consistency != 0;
        if (mask) DFVO_HIP_CHECK(hipStreamWaitEvent(sp, sl.e_depth, 0));
        P_TRY(enqueue_local_bestn(tb, flow, diff, p->H, p->W, c.kp_num_row, c.kp_num_col, c.kp_num_bestN, (float)c.kp_thre, sp,
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
    PoseConfig pc;
    fill_pose_cfg(c, p->opts, &pc);
    P_TRY(enqueue_pose_h_part(tb, tb.kp_cap, pc, sp));  // keypoint count read on the device; kp_cap bounds the launches
    return DFVO_OK;
}

int dfvo_pipeline_prefetch_track(dfvo_pipeline* p, int slot, const float* d_flow_override, const float* d_diff_override) {
    DFVO_ARG_CHECK(p && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS), "dfvo_pipeline_prefetch_track: bad argument");
    if (deep_pose_tracking(p)) return DFVO_OK;  // no keypoint stage: nothing to run ahead
    DFVO_ARG_CHECK(!p->slots[slot].prefetched, "dfvo_pipeline_prefetch_track: slot already prefetched and not yet tracked");
    P_TRY(enqueue_pre_part(p, slot, d_flow_override, d_diff_override, p->s_pre[slot & 1]));
    p->slots[slot].prefetched = true;
    return DFVO_OK;
}

// First half of dfvo_pipeline_track: waits for the slot's keypoint stage, enqueues the RandomState-ordered chain (shuffles,
// 5 x five-point RANSAC, GRIC, recoverPose, scale recovery) and the copy of its results into pinned host memory, returns.
// The host is then free to enqueue the next pairs' nets while the chain runs (dfvo_pipeline_track_end collects).
int dfvo_pipeline_track_begin(dfvo_pipeline* p, int slot, const float* d_flow_override, const float* d_diff_override,
                              const double* d_depth_override) {
    DFVO_ARG_CHECK(p && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS), "dfvo_pipeline_track_begin: bad argument");
    DFVO_ARG_CHECK(p->slots[slot].begun == IDLE, "dfvo_pipeline_track_begin: the slot's previous pair was not collected (track_end)");
    DFVO_ARG_CHECK(p->pending_slot == -1, "dfvo_pipeline_track_begin: another pair is begun and not yet collected -- the PnP decision "
                                          "of track_end (RandomState draws) comes before the next pair's chain");
    const dfvo_pipeline_cfg& c = p->cfg;
    hipStream_t s = p->s_trk;
    Slot& sl = p->slots[slot];
    TrackerBuffers& tb = sl.tb;
    static const bool trace = getenv("DFVO_TRACK_TRACE") != nullptr;
    if (trace && !tb.ev_t[0])
        for (int i = 0; i < 4; i++) DFVO_HIP_CHECK(hipEventCreate(&tb.ev_t[i]));
    if (deep_pose_tracking(p)) {
        // dfvo.py:252-255: the pair's motion is the pose net's matrix.  No keypoints, no RandomState draw; the 16 floats go to
        // pinned memory behind the pose lane
        DFVO_HIP_CHECK(hipStreamWaitEvent(s, sl.e_depth, 0));
        DFVO_HIP_CHECK(hipMemcpyAsync(sl.h_pose.p, sl.pose16, 16 * sizeof(float), hipMemcpyDeviceToHost, s));
        DFVO_HIP_CHECK(hipEventRecord(sl.e_res, s));
        sl.depth_override = nullptr;
        sl.n = 0;
        sl.begun = CHAIN_ENQUEUED;
        p->pending_slot = slot;
        return DFVO_OK;
    }
    const bool pnp_only = p->opts.tracking_method == DFVO_TRACKING_PNP;
    const bool iterative = p->iter.enable && !pnp_only;
    // side stream: the scale stage's fills leave the dependent chain (the iterative loop clears the map itself, every round)
    if (!pnp_only && !iterative) P_TRY(enqueue_scale_prepare(tb, p->H, p->W));
    if (iterative) iter_record_reset(sl.h_iter);  // (the slot is idle: its last record was copied long ago)
    // A pre-part nobody prefetched: in the lane layout it goes onto the chain's lane (s), whose next work needs it anyway --
    // the depth lane may already hold later pairs' nets, and it would run behind them
    if (!sl.prefetched)
        P_TRY(enqueue_pre_part(p, slot, d_flow_override, d_diff_override, p->plan.layout == LAYOUT_LANES ? s : p->s_pre[slot & 1]));
    sl.prefetched = false;
    DFVO_HIP_CHECK(hipEventSynchronize(sl.e_pre));  // keypoint info is in pinned host memory now
    const int* info = sl.h_info;
    sl.depth_override = d_depth_override;
    auto begun = [&](Begun b) {  // the pair is pending from here on
        sl.begun = b;
        p->pending_slot = slot;
        return DFVO_OK;
    };
    if (!info[1]) return begun(NO_KEYPOINTS);
    const int n = sl.n = info[0];
    if (pnp_only) {
        // dfvo.py:225-250 on every pair: E_pose stays SE3(), so the only RandomState draws of the pair are PnP's shuffles.
        // The keypoint stage is complete (the host waited for e_pre above); the reference depth is ordered on s by
        // set_ref_depth / the previous pair's roll-over
        if (!p->has_ref_depth) return begun(NO_REF_DEPTH);
        PnpConfig pc3;
        fill_pnp_cfg(c, &pc3);
        P_TRY(enqueue_compute_pose_3d2d(p->pnp, tb.mt_state, tb.kp_ref, tb.kp_cur, tb.kp_info, n, p->ref_depth, p->H, p->W, pc3, s));
        DFVO_HIP_CHECK(hipMemcpyAsync(&sl.h_res.p->pnp, p->pnp.result, sizeof(PnpResult), hipMemcpyDeviceToHost, s));
        DFVO_HIP_CHECK(hipEventRecord(sl.e_res, s));
        return begun(CHAIN_ENQUEUED);
    }
    PoseConfig pc;
    fill_pose_cfg(c, p->opts, &pc);
    // waits for tb.ev_h (the prefetched half) on the device
    P_TRY(enqueue_pose_e_part(tb, n, pc, s, p->d_T21, iterative ? p->d_E_pose.p : nullptr));
    DFVO_HIP_CHECK(hipStreamWaitEvent(s, sl.e_depth, 0));
    ScaleConfig sc;
    fill_scale_cfg(c, p->opts, &sc);
    const double* depth = d_depth_override ? d_depth_override : sl.proc_depth.p;
    if (iterative) {
        // E_tracker.py:509-569, all rounds, gated and started from prev_scale on the device; p->ref_raw is ordered on s by
        // set_ref_* / the previous pair's roll-over, like the reference depth
        IterDevice dev;
        dev.prev_scale = p->d_prev_scale;
        dev.gate = tb.pose;
        P_TRY(enqueue_scale_recovery_iterative(tb, sl.rigid, sl.flow_in, sl.diff_in, p->ref_raw, depth, p->H, p->W, p->iter_cfg, sc,
                                               p->d_E_pose, p->d_T21, 0.0, p->iter.kp_src, n, s, &dev));
        DFVO_HIP_CHECK(hipMemcpyAsync(sl.h_iter.p, sl.rigid.ctl, sizeof(IterCtl), hipMemcpyDeviceToHost, s));
    } else {
        P_TRY(enqueue_find_scale(tb, n, p->d_T21, depth, p->H, p->W, sc, s, tb.pose, true));
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
    DFVO_ARG_CHECK(p && out && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS), "dfvo_pipeline_track_end: bad argument");
    DFVO_ARG_CHECK(p->slots[slot].begun != IDLE, "dfvo_pipeline_track_end: no pair pending in this slot (track_begin)");
    const dfvo_pipeline_cfg& c = p->cfg;
    hipStream_t s = p->s_trk;
    Slot& sl = p->slots[slot];
    TrackerBuffers& tb = sl.tb;
    static const bool trace = getenv("DFVO_TRACK_TRACE") != nullptr;  // host-side phase timing (tuning aid)
    static double tr_acc[2] = {0, 0}, tr_dev[3] = {0, 0, 0};
    static int tr_dev_n = 0, tr_n = 0;
    const auto tr0 = std::chrono::steady_clock::now();
    auto tr_ms = [&](std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    };
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
        P_TRY(roll_ref_depth(p, slot, d_depth_override));
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
    const double tr_wait = tr_ms(tr0);
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
            P_TRY(roll_ref_depth(p, slot, d_depth_override));
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
    if (t_zero || scale == -1.0) {  // dfvo.py:225-250: PnP on (ref keypoints + ref depth) -> cur keypoints
        out->status = DFVO_TRACK_NEEDS_PNP;
        if (p->has_ref_depth) {
            PnpConfig pc3;
            fill_pnp_cfg(c, &pc3);
            P_TRY(enqueue_compute_pose_3d2d(p->pnp, tb.mt_state, tb.kp_ref, tb.kp_cur, tb.kp_info, n,
                                            p->ref_depth, p->H, p->W, pc3, s));
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
    P_TRY(roll_ref_depth(p, slot, d_depth_override));
    if (trace) {
        float d01 = 0, d12 = 0, d23 = 0;  // device time of the chain's three segments (valid when the pair took the E path)
        if (n > 10 && hipEventElapsedTime(&d01, tb.ev_t[0], tb.ev_t[1]) == hipSuccess &&
            hipEventElapsedTime(&d12, tb.ev_t[1], tb.ev_t[2]) == hipSuccess &&
            hipEventElapsedTime(&d23, tb.ev_t[2], tb.ev_t[3]) == hipSuccess) {
            tr_dev[0] += d01;
            tr_dev[1] += d12;
            tr_dev[2] += d23;
            tr_dev_n++;
        }
        if (tr_dev_n == 20) {
            fprintf(stderr, "track device ms: shuffles + five-point batch %.3f | bookkeeping + recoverPose %.3f | scale %.3f\n",
                    tr_dev[0] / 20, tr_dev[1] / 20, tr_dev[2] / 20);
            tr_dev[0] = tr_dev[1] = tr_dev[2] = 0;
            tr_dev_n = 0;
        }
        tr_acc[0] += tr_wait;
        tr_acc[1] += tr_ms(tr0);
        if (++tr_n % 20 == 0) {
            fprintf(stderr, "track_end host ms: waited for the chain %.3f | total %.3f\n", tr_acc[0] / 20, tr_acc[1] / 20);
            tr_acc[0] = tr_acc[1] = 0;
        }
    }
    return DFVO_OK;
}

int dfvo_pipeline_track(dfvo_pipeline* p, int slot, const float* d_flow_override, const float* d_diff_override,
                        const double* d_depth_override, dfvo_track_out* out) {
    DFVO_ARG_CHECK(p && out && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS), "dfvo_pipeline_track: bad argument");
    P_TRY(dfvo_pipeline_track_begin(p, slot, d_flow_override, d_diff_override, d_depth_override));
    const int rc_end = dfvo_pipeline_track_end(p, slot, out);
    if (rc_end != DFVO_OK && rc_end != DFVO_ERR_EMPTY_SELECTION && rc_end != DFVO_ERR_NO_CONSENSUS) return rc_end;
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk));  // (synchronous, as documented: the roll-over copy included)
    return rc_end;
}

int dfvo_pipeline_get_flow(dfvo_pipeline* p, int slot, float* h_fwd, float* h_bwd, float* h_diff, float* h_raw_depth,
                           double* h_depth) {
    DFVO_ARG_CHECK(p && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS), "dfvo_pipeline_get_flow: bad argument");
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
    DFVO_ARG_CHECK(p && n_out && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS) && cap >= 0,
                   "dfvo_pipeline_get_keypoints: bad argument");
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
    DFVO_ARG_CHECK(p && out && (slot >= 0 && slot < DFVO_PIPELINE_SLOTS) && cap >= 0, "dfvo_pipeline_get_iterative: bad argument");
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

int dfvo_pipeline_get_rng_state(dfvo_pipeline* p, uint32_t* h_state) {
    DFVO_ARG_CHECK(p && h_state, "dfvo_pipeline_get_rng_state: null argument");
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk));
    DFVO_HIP_CHECK(hipMemcpy(h_state, p->slots[0].tb.mt_state, 625 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DFVO_OK;
}

int dfvo_pipeline_set_rng_state(dfvo_pipeline* p, const uint32_t* h_state) {
    DFVO_ARG_CHECK(p && h_state, "dfvo_pipeline_set_rng_state: null argument");
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk));
    DFVO_HIP_CHECK(hipMemcpy(p->slots[0].tb.mt_state, h_state, 625 * sizeof(uint32_t), hipMemcpyHostToDevice));
    return DFVO_OK;
}

int dfvo_pipeline_sync(dfvo_pipeline* p) {
    DFVO_ARG_CHECK(p, "null pipeline");
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_flow));
    for (int i = 0; i + 1 < p->flow_instances; ++i) DFVO_HIP_CHECK(hipStreamSynchronize(p->s_flow_x[i]));
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_depth));
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk));
    return DFVO_OK;
}

int dfvo_pipeline_stream_layout(dfvo_pipeline* p, char* buf, int n) {
    DFVO_ARG_CHECK(p && buf && n > 0, "dfvo_pipeline_stream_layout: bad argument");
    // "layout=lanes groups=4 queues=4 streams=4 trk=3 rep0=3 ... flow_x=1": per role the index of its stream among the
    // pipeline's distinct streams (lanes: the lane), so equal numbers mean one stream
    hipStream_t role[ROLE_COUNT] = {p->s_trk, p->slots[0].tb.s_rep[0], p->slots[0].tb.s_rep[1], p->s_depth, p->s_pre[0], p->s_pre[1], p->s_flow,
                                    p->flow_instances > 1 ? p->s_flow_x[0] : nullptr};
    std::vector<hipStream_t> distinct;
    const bool lanes = p->plan.layout == LAYOUT_LANES;
    if (lanes) distinct.assign(p->lane, p->lane + 4);
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
    if (p->opts.tracking_method == DFVO_TRACKING_DEEP_POSE) return pose;
    return pose + (p->dsrc.source == DFVO_DEPTH_EXTERNAL ? p->flow.flops_last : p->flow.flops_last + p->depth.flops_last);
}

}  // extern "C"
