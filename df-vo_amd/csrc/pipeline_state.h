// Fused per-pair tracking pipeline: both CNNs, keypoint selection, E-tracker and scale recovery chained
// on the device (three HIP streams), with two host round trips per pair (keypoint count, final pose).
// Orchestration follows the reference's libs/dfvo.py:299-345 (deep_model_inference) and :121-262
// (tracking): the host-side glue of the reference (cv2.resize nearest, preprocess_depth, dict passing)
// becomes device kernels; the pose composition stays on the host (dfvo.py:109-119).
// dfvo_pipeline_set_options selects the keypoint source (local_bestN | bestN | sampled), the validity and scale-RANSAC methods
// and hybrid | PnP-only tracking; dfvo_pipeline_set_iterative puts scale_recovery.method "iterative" (the one-call device loop
// of solver_scale.hip) in the place of find_scale_from_depth; dfvo_pipeline_set_depth_source puts a 16-bit depth image per
// frame (depth.depth_src gt, dfvo.py:296-319) in the place of the depth net; dfvo_pipeline_set_pose_net adds the pose lane
// (monodepth2's pose net, the depth-consistency keypoint mask, tracking_method deep_pose); without them the pipeline runs
// default_configuration.yml.
// This header: the state, for the units pipeline_create / _options (its rules: pipeline_setup.h) / _nets / _track .hip.
#pragma once
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

// dfvo_pipeline_set_refine: what a pair's refinement leaves in pinned host memory.  info2 / ctl arrive behind Slot::e_res with
// pass one (the E selection is enqueued behind it); the rest is filled in by track_end as the second passes complete
struct RefineHost {
    int info2[4];  // the second pass's kp_info triple as the last selection wrote it
    IterCtl ctl;   // the hand-over's gate: status ITER_NOT_RUN = the selection did not run
    PoseState pose2;
    ScaleResult scale2;
    RefineFinal fin;
    dfvo_refine_out rec;  // dfvo_pipeline_get_refine's record of the pair last collected
};

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
    // dfvo_pipeline_set_refine: the second passes' buffer set (own keypoint and RANSAC workspaces, slots[0].tb's RandomState), the
    // device bookkeeping behind the second E pass, and what the pair's refinement left in pinned memory (RefineHost)
    TrackerBuffers tb2;
    DevArr<RefineFinal> refine_final;
    PinnedArr<RefineHost> h_refine;
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
    // flow[0 .. flow_instances): the flow-net instances, each on its own stream (DFVO_FLOW_INSTANCES, default 2): consecutive
    // pairs rotate over the instances, so the latency-bound coarse pyramid levels of one pass overlap the throughput-bound fine
    // levels of another (8.7 -> 7.1 ms per pair with two); costs one set of activations (~1.3 GB) per instance
    FlowNet flow[DFVO_PIPELINE_SLOTS];
    int flow_instances = 1;
    DepthNet depth;
    Slot slots[DFVO_PIPELINE_SLOTS];
    int pending_slot = -1;  // the one pair begun and not yet collected (the chains consume ONE RandomState, in pair order)
    hipEvent_t e_ref = nullptr;  // reference depth of the first frame written (dfvo_pipeline_set_ref_image / _set_ref_depth)
    hipEvent_t e_roll = nullptr;  // recorded by roll_ref_depth behind the roll-over copies, waited for by wait_roll
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
    // dfvo_pipeline_set_refine: all zero = no refinement.  refine_cfg: the rigid-flow keypoint configuration (score_rigid set per
    // selection); pose_cfg1 / pnp_cfg1: pose_cfg / pnp_cfg with the 3 repeats of a first pass (is_iterative False)
    dfvo_pipeline_refine_opts refine = {};
    RigidKpConfig refine_cfg = {};
    PoseConfig pose_cfg1;
    PnpConfig pnp_cfg1;
    // PnP fallback: processed depth of the reference frame (= the previous pair's current frame)
    PnpBuffers pnp;
    DevArr<double> ref_depth;
    DevArr<float> ref_raw;
    bool has_ref_depth = false;
    dfvo_pipeline_cfg cfg;
    // dfvo_pipeline_set_options: the tracking configuration beyond default_configuration.yml (all zero = that configuration)
    dfvo_pipeline_opts opts = {};
    // the solvers' configurations as cfg and opts give them (fill_solver_cfgs: dfvo_pipeline_create, dfvo_pipeline_set_options)
    PoseConfig pose_cfg;
    PnpConfig pnp_cfg;
    ScaleConfig scale_cfg;
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
    // role[] below it is the stream of each role of stream_layout.h, plain copies.  ROLE_PRE0 / 1: the two streams the run-ahead
    // halves alternate on; ROLE_REP0 / 1: the chain's side streams, lent to slots[0].tb (null: that object created its own, the
    // creation-order fallback); ROLE_FLOW + i: flow[i]'s.
    // Stream layout (stream_layout.h).  LAYOUT_LANES: lane[0 .. 3] are the pipeline's only streams, one per hardware queue,
    // and every role's stream is one of them (flow, flow_x, depth = pre0 = pre1, trk = rep0 = rep1);
    // otherwise every role has a stream to itself and lane[] is null.
    std::vector<hipStream_t> owned;
    hipStream_t role[ROLE_COUNT] = {};
    hipStream_t lane[4] = {nullptr, nullptr, nullptr, nullptr};
    StreamPlan plan;
    int pool_groups = 0, pool_queues = 0;  // what the pool measured (0: no measurement)

    hipStream_t s_trk() const { return role[ROLE_TRK]; }
    hipStream_t s_depth() const { return role[ROLE_DEPTH]; }
    hipStream_t s_pre(int slot) const { return role[ROLE_PRE0 + (slot & 1)]; }
};
static_assert(ROLE_FLOW_X == ROLE_FLOW + 1 && ROLE_COUNT == ROLE_FLOW + 2 && ROLE_PRE1 == ROLE_PRE0 + 1,
              "role[ROLE_FLOW + i] for the at most two flow-net instances, role[ROLE_PRE0 + i]");

inline bool slot_ok(int slot) { return slot >= 0 && slot < DFVO_PIPELINE_SLOTS; }
inline bool deep_pose_tracking(const dfvo_pipeline* p) { return p->opts.tracking_method == DFVO_TRACKING_DEEP_POSE; }

// The e_roll rule.  The roll-over copies ref_depth <- proc_depth[slot] and ref_raw <- raw_depth[slot] run on s_trk, and
// track_end does not wait for them on the host: the next writer of ref_depth, ref_raw or proc_depth[slot] on another stream
// (the depth stream's preprocess_depth, the move of the mask's reference depth) waits for the pending roll-over on the device.
// Its callers sit behind the net on their stream, so nothing stalls in practice.
inline int wait_roll(dfvo_pipeline* p, hipStream_t s) {
    if (p->roll_pending) DFVO_HIP_CHECK(hipStreamWaitEvent(s, p->e_roll, 0));
    return DFVO_OK;
}

inline bool refine_rolls_raw(const dfvo_pipeline* p) { return p->refine.e_enable || p->refine.pnp_enable; }
void fill_solver_cfgs(dfvo_pipeline* p);                                         // pipeline_options.hip
int finalize_pose_net(dfvo_pipeline* p);                                          // pipeline_create.hip
int roll_ref_depth(dfvo_pipeline* p, int slot, const double* d_depth_override);  // pipeline_nets.hip
