// Fused pipeline (pipeline_state.h): a pair's depth, pose lane and flow ahead of its solver stage; the reference depth.
#include "pipeline_state.h"

// where a frame's depth comes from, one of: the frame at feed size for the depth net | the sensor's 16-bit image (read_depth)
struct DepthInput { const uint8_t* feed; const uint16_t* u16; };

// A raw / processed depth pair on the depth stream: the depth net and preprocess_depth of its output (crop, clamp, nearest
// resize to the image size), or both in one launch from a depth image.  The targets are written under the e_roll rule.
static int enqueue_depth(dfvo_pipeline* p, DepthInput in, float* raw, double* proc) {
    const dfvo_pipeline_cfg& c = p->cfg;
    const int y0 = (int)(p->H * c.depth_crop[0]), y1 = (int)(p->H * c.depth_crop[1]);
    const int x0 = (int)(p->W * c.depth_crop[2]), x1 = (int)(p->W * c.depth_crop[3]);
    if (in.feed) DFVO_TRY(p->depth.forward(in.feed, p->depth_small));
    DFVO_TRY(wait_roll(p, p->s_depth()));
    if (in.feed)
        return launch_depth_post(p->depth_small, p->feedH, p->feedW, p->H, p->W, y0, y1, x0, x1, (float)c.min_depth, (float)c.max_depth,
                                 raw, proc, p->s_depth());
    return dfvo_read_depth_u16(in.u16, p->dsrc.src_h, p->dsrc.src_w, p->dsrc.scale, p->H, p->W, y0, y1, x0, x1, c.min_depth, c.max_depth, raw,
                               proc, p->s_depth());
}

static int need_previous_call(const char* who) {
    dfvo::set_last_error(std::string(who) + ": d_ref == NULL (reference frame = the previous call's current frame) needs a previous call");
    return DFVO_ERR_ARG;
}

// what a pair's pose lane needs from earlier calls, checked before anything of the pair is enqueued
static int check_pose_lane(const dfvo_pipeline* p, const uint8_t* d_ref, const char* who) {
    if (!d_ref && !p->pose_ref_feed) return need_previous_call(who);
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
    DFVO_TRY(wait_roll(p, p->s_depth()));
    DFVO_HIP_CHECK(hipMemcpyAsync(p->ref_raw, sl.raw_depth, (size_t)p->H * p->W * sizeof(float), hipMemcpyDeviceToDevice, p->s_depth()));
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
    hipStream_t s = p->s_depth();
    const size_t feed_bytes = (size_t)p->feedH * p->feedW * 3;
    uint8_t* feed_ref = p->pose_feed.p;
    uint8_t* feed_cur = p->pose_feed.p + p->pose_feed_pitch;
    if (d_cur_feed)
        DFVO_HIP_CHECK(hipMemcpyAsync(feed_cur, d_cur_feed, feed_bytes, hipMemcpyDeviceToDevice, s));
    else
        DFVO_TRY(p->feed_resize.enqueue(d_cur, feed_cur, s));
    if (d_ref) DFVO_TRY(p->feed_resize.enqueue(d_ref, feed_ref, s));
    DFVO_TRY(p->pose_net.forward(feed_ref, feed_cur, p->pose_out, nullptr));
    const float* pose = sl.pose_override ? sl.pose_override : p->pose_out.p;
    DFVO_HIP_CHECK(hipMemcpyAsync(sl.pose16, pose, 16 * sizeof(float), hipMemcpyDeviceToDevice, s));
    DFVO_HIP_CHECK(hipMemcpyAsync(feed_ref, feed_cur, feed_bytes, hipMemcpyDeviceToDevice, s));
    p->pose_ref_feed = true;
    if (p->pose.depth_consistency) {
        const dfvo_pipeline_cfg& c = p->cfg;
        const float K[9] = {(float)c.fx, 0.f, (float)c.cx, 0.f, (float)c.fy, (float)c.cy, 0.f, 0.f, 1.f};
        float Kinv[9];
        for (int i = 0; i < 9; ++i) Kinv[i] = (float)c.Kinv[i];
        if (p->pose_ref_raw == p->ref_raw.p) DFVO_TRY(wait_roll(p, s));
        DFVO_TRY(launch_depth_consistency_dev(sl.raw_depth, p->pose_ref_raw, p->H, p->W, K, Kinv, sl.pose16, sl.depth_diff, s));
        p->pose_ref_raw = sl.raw_depth.p;
    }
    return DFVO_OK;
}

static int enqueue_flow_half(dfvo_pipeline* p, int slot, const uint8_t* d_ref, const uint8_t* d_cur) {
    Slot& sl = p->slots[slot];
    const size_t px = (size_t)p->H * p->W;
    // forward/backward flow (dfvo.py:321-335)
    FlowNet& fn = p->flow[slot % p->flow_instances];
    hipStream_t sf = fn.stream;
    // frame pointers may change per pair (not captured).  d_ref == NULL: the image / feature pyramids of the reference frame
    // are carried over from the pass that saw it as its current frame (the other flow-net instance, normally)
    // Whatever this pass is (carried or not), it overwrites this instance's pyramids: the previous pass -- normally on the
    // OTHER instance -- may still be copying them (its carry-over reads this instance's current-frame pyramids), so this
    // stream is ordered behind that pass's feature stage.  A carried pass waits for the same event anyway; a full pass
    // enqueued right behind a carried one without a sync in between would otherwise race with that copy.
    if (p->last_flow && p->last_flow != &fn && p->last_flow->e_feat) DFVO_HIP_CHECK(hipStreamWaitEvent(sf, p->last_flow->e_feat, 0));
    // (the net writing the slot's buffers itself, one levels graph per slot, was measured: no gain -- profiles/r3x_copy_ab.txt)
    DFVO_TRY(fn.forward(d_ref, d_cur, fn.out_fwd.p, fn.out_bwd.p, fn.out_diff.p, d_ref ? nullptr : p->last_flow));
    DFVO_HIP_CHECK(hipMemcpyAsync(sl.fwd, fn.out_fwd.p, 2 * px * sizeof(float), hipMemcpyDeviceToDevice, sf));
    DFVO_HIP_CHECK(hipMemcpyAsync(sl.bwd, fn.out_bwd.p, 2 * px * sizeof(float), hipMemcpyDeviceToDevice, sf));
    DFVO_HIP_CHECK(hipMemcpyAsync(sl.diff, fn.out_diff.p, px * sizeof(float), hipMemcpyDeviceToDevice, sf));
    p->last_flow = &fn;
    DFVO_HIP_CHECK(hipEventRecord(sl.e_flow, sf));
    return DFVO_OK;
}

// One pair into `slot`, for both entry points.  in.feed and in.u16 both null: the current frame is resized for the depth net
static int enqueue_pair(dfvo_pipeline* p, int slot, const uint8_t* d_ref, const uint8_t* d_cur, DepthInput in, const char* who) {
    Slot& sl = p->slots[slot];
    if (p->pose.enable) DFVO_TRY(check_pose_lane(p, d_ref, who));
    if (deep_pose_tracking(p)) {  // dfvo.py:302: neither the depth net nor the flow net (a depth image has no reader)
        p->started = true;
        DFVO_TRY(enqueue_pose_lane(p, slot, d_ref, d_cur, in.feed));
        DFVO_HIP_CHECK(hipEventRecord(sl.e_depth, p->s_depth()));
        return DFVO_OK;
    }
    if (!d_ref && !p->last_flow) return need_previous_call(who);
    p->started = true;
    DFVO_TRY(keep_ref_raw(p, sl));
    // depth of the current frame (dfvo.py:305-319), the sensor's image where the reference runs the depth net; without a
    // caller-resized frame the LANCZOS resize of deep_models.py:195-199 runs here, ahead of the net on its stream
    if (!in.u16 && !in.feed) {
        DFVO_TRY(p->feed_resize.enqueue(d_cur, p->feed_buf, p->s_depth()));
        in.feed = p->feed_buf;
    }
    DFVO_TRY(enqueue_depth(p, in, sl.raw_depth, sl.proc_depth));
    if (p->pose.enable) DFVO_TRY(enqueue_pose_lane(p, slot, d_ref, d_cur, in.feed));  // (in.feed null: its own LANCZOS feed)
    DFVO_HIP_CHECK(hipEventRecord(sl.e_depth, p->s_depth()));
    return enqueue_flow_half(p, slot, d_ref, d_cur);
}

// The first reference frame's depths.  Not waited for on the host: the solver stream (PnP fallback reads the reference depth,
// the roll-over writes it) is ordered behind it on the device, the depth stream runs its later passes in order anyway
static int enqueue_ref_depth(dfvo_pipeline* p, DepthInput in) {
    p->started = true;
    DFVO_TRY(enqueue_depth(p, in, p->ref_raw, p->ref_depth));
    DFVO_HIP_CHECK(hipEventRecord(p->e_ref, p->s_depth()));
    DFVO_HIP_CHECK(hipStreamWaitEvent(p->s_trk(), p->e_ref, 0));
    p->pose_ref_raw = p->ref_raw.p;  // (written on the depth stream: the mask's read is in stream order)
    p->has_ref_depth = true;
    return DFVO_OK;
}

// the current frame's depth becomes the reference depth of the next pair (dfvo.py:  ref_data <- cur_data); with the iterative
// scale loop on, its raw depth becomes ref_data['raw_depth'] as well, under the same e_roll ordering
int roll_ref_depth(dfvo_pipeline* p, int slot, const double* d_depth_override) {
    const size_t px = (size_t)p->H * p->W;
    Slot& sl = p->slots[slot];
    DFVO_HIP_CHECK(hipStreamWaitEvent(p->s_trk(), sl.e_depth, 0));
    const double* depth = d_depth_override ? d_depth_override : sl.proc_depth.p;
    DFVO_HIP_CHECK(hipMemcpyAsync(p->ref_depth, depth, px * sizeof(double), hipMemcpyDeviceToDevice, p->s_trk()));
    if (p->iter.enable || refine_rolls_raw(p)) {
        const float* raw = sl.raw_override ? sl.raw_override : sl.raw_depth.p;
        DFVO_HIP_CHECK(hipMemcpyAsync(p->ref_raw, raw, px * sizeof(float), hipMemcpyDeviceToDevice, p->s_trk()));
    }
    sl.raw_override = nullptr;
    DFVO_HIP_CHECK(hipEventRecord(p->e_roll, p->s_trk()));
    p->roll_pending = true;
    p->has_ref_depth = true;
    return DFVO_OK;
}

extern "C" {

int dfvo_pipeline_enqueue_nets(dfvo_pipeline* p, int slot, const uint8_t* d_ref, const uint8_t* d_cur,
                               const uint8_t* d_cur_feed) {
    DFVO_ARG_CHECK(p && p->nets_ready && slot_ok(slot) && d_cur, "dfvo_pipeline_enqueue_nets: bad argument");
    DFVO_ARG_CHECK(p->dsrc.source == DFVO_DEPTH_NET, "dfvo_pipeline_enqueue_nets: the depth source is DFVO_DEPTH_EXTERNAL (no depth net): "
                                                     "dfvo_pipeline_enqueue_nets_depth takes the pair's depth image");
    return enqueue_pair(p, slot, d_ref, d_cur, {d_cur_feed, nullptr}, "dfvo_pipeline_enqueue_nets");
}

int dfvo_pipeline_enqueue_nets_depth(dfvo_pipeline* p, int slot, const uint8_t* d_ref, const uint8_t* d_cur, const uint16_t* d_depth_u16) {
    DFVO_ARG_CHECK(p && p->nets_ready && slot_ok(slot) && d_cur && d_depth_u16, "dfvo_pipeline_enqueue_nets_depth: bad argument");
    DFVO_ARG_CHECK(p->dsrc.source == DFVO_DEPTH_EXTERNAL, "dfvo_pipeline_enqueue_nets_depth: the depth source is DFVO_DEPTH_NET "
                                                          "(dfvo_pipeline_set_depth_source): dfvo_pipeline_enqueue_nets runs the depth net");
    return enqueue_pair(p, slot, d_ref, d_cur, {nullptr, d_depth_u16}, "dfvo_pipeline_enqueue_nets_depth");
}

int dfvo_pipeline_set_ref_depth(dfvo_pipeline* p, const uint8_t* d_feed, const double* d_depth_override) {
    DFVO_ARG_CHECK(p && p->nets_ready && ((d_feed != nullptr) != (d_depth_override != nullptr)),
                   "dfvo_pipeline_set_ref_depth: exactly one of d_feed / d_depth_override");
    DFVO_ARG_CHECK(!d_feed || p->dsrc.source == DFVO_DEPTH_NET, "dfvo_pipeline_set_ref_depth: d_feed with the depth source DFVO_DEPTH_EXTERNAL "
                                                                "(no depth net): dfvo_pipeline_set_ref_depth_u16 or d_depth_override");
    if (d_feed) return enqueue_ref_depth(p, {d_feed, nullptr});
    p->started = true;
    DFVO_HIP_CHECK(hipMemcpyAsync(p->ref_depth, d_depth_override, (size_t)p->H * p->W * sizeof(double), hipMemcpyDeviceToDevice, p->s_trk()));
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk()));
    p->has_ref_depth = true;
    return DFVO_OK;
}

int dfvo_pipeline_set_ref_image(dfvo_pipeline* p, const uint8_t* d_img) {
    DFVO_ARG_CHECK(p && p->nets_ready && d_img, "dfvo_pipeline_set_ref_image: bad argument");
    DFVO_ARG_CHECK(p->dsrc.source == DFVO_DEPTH_NET, "dfvo_pipeline_set_ref_image: the depth source is DFVO_DEPTH_EXTERNAL (no depth net): "
                                                     "dfvo_pipeline_set_ref_depth_u16 takes the first frame's depth image");
    DFVO_TRY(p->feed_resize.enqueue(d_img, p->feed_buf, p->s_depth()));
    return enqueue_ref_depth(p, {p->feed_buf, nullptr});
}

int dfvo_pipeline_set_ref_depth_u16(dfvo_pipeline* p, const uint16_t* d_depth_u16) {
    DFVO_ARG_CHECK(p && p->nets_ready && d_depth_u16, "dfvo_pipeline_set_ref_depth_u16: bad argument");
    DFVO_ARG_CHECK(p->dsrc.source == DFVO_DEPTH_EXTERNAL, "dfvo_pipeline_set_ref_depth_u16: the depth source is DFVO_DEPTH_NET "
                                                          "(dfvo_pipeline_set_depth_source): dfvo_pipeline_set_ref_image / _set_ref_depth");
    return enqueue_ref_depth(p, {nullptr, d_depth_u16});
}

int dfvo_pipeline_set_ref_raw_depth(dfvo_pipeline* p, const float* d_raw) {
    DFVO_ARG_CHECK(p && d_raw, "dfvo_pipeline_set_ref_raw_depth: null argument");
    p->started = true;
    DFVO_HIP_CHECK(hipMemcpyAsync(p->ref_raw, d_raw, (size_t)p->H * p->W * sizeof(float), hipMemcpyDeviceToDevice, p->s_trk()));
    DFVO_HIP_CHECK(hipStreamSynchronize(p->s_trk()));
    p->pose_ref_raw = p->ref_raw.p;  // (complete: the host waited)
    return DFVO_OK;
}

}  // extern "C"
