// Host-only: what the fused pipeline's option setters (pipeline_options.hip) refuse, each rule written once.  Either of two
// setters may come first, so a rule that spans two blocks is a predicate both ask, each beside the other's committed block and
// in its own words.  No HIP call: tests/host_harness/pipeline_setup_check.cpp walks the combinations on the CPU.
#pragma once
#include "../../include/dfvo_hip.h"
#include <initializer_list>

namespace dfvo {

// k_scale_ratios keeps one int per keypoint in 64 KB of dynamic LDS.  The bound's second statement, beside tracker.h's
// ITER_MAX_KP (this header includes dfvo_hip.h alone); pipeline_iter.h holds the two equal
constexpr int SETUP_ITER_MAX_KP = 16384;

// keypoints the pipeline's source hands to the trackers, at most
inline int tracked_kp_max(int kp_source, int kp_sampled_num, int kp_num_bestN, int kp_num_row, int kp_num_col) {
    if (kp_source == DFVO_KP_SOURCE_SAMPLED) return kp_sampled_num;
    if (kp_source == DFVO_KP_SOURCE_BESTN) return kp_num_bestN;
    const long long cells = (long long)kp_num_row * kp_num_col;
    return cells > 0 ? (int)((kp_num_bestN / cells) * cells) : 0;  // math.floor(N / (rows * cols)) per cell
}

// keypoints dfvo_pipeline_set_options sizes the source's buffers for; 0 for local_bestN, whose launcher sizes its own
inline int options_kp_count(const dfvo_pipeline_cfg& c, const dfvo_pipeline_opts& o) {
    return o.kp_source == DFVO_KP_SOURCE_BESTN ? c.kp_num_bestN : o.kp_source == DFVO_KP_SOURCE_SAMPLED ? o.kp_sampled_num : 0;
}

// y0 y1 x0 x1 [px] of cfg.crop.flow_crop (kp_source sampled)
inline void flow_crop_px(const dfvo_pipeline_cfg& c, const dfvo_pipeline_opts& o, int crop[4]) {
    for (int i = 0; i < 4; ++i) crop[i] = (int)(o.flow_crop[i] * (i < 2 ? c.img_h : c.img_w));
}

// dfvo_pipeline_set_iterative's block (the launcher's own refusals come from rigid_flow_kp_geometry)
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
inline bool iter_kp_count_ok(int kp_src, int n_sel, int n_trk) { return (kp_src == DFVO_ITER_KP_DEPTH ? n_sel : n_trk) <= SETUP_ITER_MAX_KP; }

// The three rules between the option block and the pose block
inline bool deep_pose_without_net(const dfvo_pipeline_opts& o, const dfvo_pipeline_pose_opts& po) {
    return o.tracking_method == DFVO_TRACKING_DEEP_POSE && !po.enable;
}
inline bool deep_pose_with_mask(const dfvo_pipeline_opts& o, const dfvo_pipeline_pose_opts& po) {  // nothing selects keypoints
    return o.tracking_method == DFVO_TRACKING_DEEP_POSE && po.depth_consistency;
}
inline bool mask_off_local_bestn(const dfvo_pipeline_opts& o, const dfvo_pipeline_pose_opts& po) {  // the only source the reference masks
    return po.depth_consistency && o.kp_source != DFVO_KP_SOURCE_LOCAL_BESTN;
}

// dfvo_pipeline_set_options: the candidate block `o` beside the committed iterative and pose blocks
inline const char* options_refusal(const dfvo_pipeline_cfg& c, const dfvo_pipeline_opts& o, const dfvo_pipeline_iter_opts& it,
                                   const dfvo_pipeline_pose_opts& po) {
    if (!(o.kp_source >= DFVO_KP_SOURCE_LOCAL_BESTN && o.kp_source <= DFVO_KP_SOURCE_SAMPLED))
        return "dfvo_pipeline_set_options: kp_source is DFVO_KP_SOURCE_LOCAL_BESTN, _BESTN or _SAMPLED";
    if (!(o.kp_score_method == DFVO_KP_SCORE_FLOW || o.kp_score_method == DFVO_KP_SCORE_FLOW_RATIO))
        return "dfvo_pipeline_set_options: kp_score_method is DFVO_KP_SCORE_FLOW or DFVO_KP_SCORE_FLOW_RATIO";
    if (!(o.validity_method >= DFVO_VALIDITY_GRIC && o.validity_method <= DFVO_VALIDITY_HOMO_RATIO))
        return "dfvo_pipeline_set_options: validity_method is DFVO_VALIDITY_GRIC, _FLOW or _HOMO_RATIO";
    if (!(o.validity_method == DFVO_VALIDITY_GRIC || o.validity_thre == o.validity_thre)) return "dfvo_pipeline_set_options: validity_thre is NaN";
    if (!(o.scale_method == DFVO_SCALE_DEPTH_RATIO || o.scale_method == DFVO_SCALE_ABS_DIFF))
        return "dfvo_pipeline_set_options: scale_method is DFVO_SCALE_DEPTH_RATIO or DFVO_SCALE_ABS_DIFF";
    if (!(o.tracking_method >= DFVO_TRACKING_HYBRID && o.tracking_method <= DFVO_TRACKING_DEEP_POSE) || deep_pose_without_net(o, po) ||
        deep_pose_with_mask(o, po))
        return "dfvo_pipeline_set_options: tracking_method is DFVO_TRACKING_HYBRID, DFVO_TRACKING_PNP or, behind "
               "dfvo_pipeline_set_pose_net with enable and without depth_consistency, DFVO_TRACKING_DEEP_POSE";
    if (mask_off_local_bestn(o, po))
        return "dfvo_pipeline_set_options: kp_source with dfvo_pipeline_set_pose_net's depth_consistency is DFVO_KP_SOURCE_LOCAL_BESTN, "
               "the only source the reference masks";
    if (o.kp_source == DFVO_KP_SOURCE_BESTN && !(c.kp_num_bestN >= 1)) return "dfvo_pipeline_set_options: bestN needs kp_num_bestN >= 1";
    if (o.kp_source == DFVO_KP_SOURCE_SAMPLED) {
        if (!(o.kp_sampled_num >= 1)) return "dfvo_pipeline_set_options: sampled needs kp_sampled_num >= 1";
        for (int i = 0; i < 4; ++i)
            if (!(o.flow_crop[i] >= 0.0 && o.flow_crop[i] <= 1.0)) return "dfvo_pipeline_set_options: flow_crop fractions lie in [0, 1]";
        int crop[4];
        flow_crop_px(c, o, crop);
        if (!(crop[0] < crop[1] && crop[2] < crop[3])) return "dfvo_pipeline_set_options: flow_crop is empty";
    }
    if (it.enable && !iter_kp_count_ok(it.kp_src, 0, options_kp_count(c, o)))
        return "dfvo_pipeline_set_options: more tracked keypoints than the iterative scale loop takes (16384)";
    return nullptr;
}

// dfvo_pipeline_set_refine.  An all-zero block is "off"; a block that enables nothing but is not all zero is a mistake
inline bool refine_on(const dfvo_pipeline_refine_opts& r) { return r.e_enable || r.scale_enable || r.pnp_enable; }
inline bool refine_all_zero(const dfvo_pipeline_refine_opts& r) {
    return !refine_on(r) && !r.e_score_rigid && !r.pnp_score_rigid && !r.num_row && !r.num_col && !r.num_bestN &&
           r.rigid_flow_thre == 0.0 && r.optical_flow_thre == 0.0;
}
// The rules between the refinement block and the iterative / option blocks, each asked by both setters
inline bool refine_with_iterative(const dfvo_pipeline_refine_opts& r, const dfvo_pipeline_iter_opts& it) { return refine_on(r) && it.enable; }
inline bool refine_with_deep_pose(const dfvo_pipeline_refine_opts& r, const dfvo_pipeline_opts& o) {
    return refine_on(r) && o.tracking_method == DFVO_TRACKING_DEEP_POSE;
}
inline bool e_refine_without_e_tracker(const dfvo_pipeline_refine_opts& r, const dfvo_pipeline_opts& o) {  // dfvo.py:165
    return r.e_enable && o.tracking_method == DFVO_TRACKING_PNP;
}
// the second scale stage shares k_scale_ratios' LDS layout: n_sel = the most kp_depth keypoints a selection returns
inline bool refine_kp_count_ok(const dfvo_pipeline_refine_opts& r, int n_sel) { return !r.scale_enable || n_sel <= SETUP_ITER_MAX_KP; }

// dfvo_pipeline_set_refine: the candidate block `r` beside the committed option and iterative blocks (the launcher's own
// refusals come from rigid_flow_kp_geometry)
inline const char* refine_opts_refusal(const dfvo_pipeline_refine_opts& r, const dfvo_pipeline_opts& o, const dfvo_pipeline_iter_opts& it) {
    for (int v : {r.e_enable, r.scale_enable, r.pnp_enable, r.e_score_rigid, r.pnp_score_rigid})
        if (v != 0 && v != 1) return "dfvo_pipeline_set_refine: the enables are 0 or 1, the scores DFVO_REFINE_SCORE_OPT_FLOW or _RIGID_FLOW";
    if (!refine_on(r)) return refine_all_zero(r) ? nullptr : "dfvo_pipeline_set_refine: nothing enabled: the block is all zero then";
    if (r.scale_enable && !r.e_enable)
        return "dfvo_pipeline_set_refine: scale_enable without e_enable: the second scale stage runs behind the second E pass only";
    if (!(r.num_row > 0 && r.num_col > 0 && r.num_bestN > 0)) return "dfvo_pipeline_set_refine: num_row, num_col, num_bestN are positive";
    if (r.rigid_flow_thre != r.rigid_flow_thre || r.optical_flow_thre != r.optical_flow_thre)
        return "dfvo_pipeline_set_refine: a threshold is NaN";
    if (refine_with_iterative(r, it))
        return "dfvo_pipeline_set_refine: not beside dfvo_pipeline_set_iterative's method (scale_recovery.method iterative)";
    if (refine_with_deep_pose(r, o)) return "dfvo_pipeline_set_refine: tracking_method DFVO_TRACKING_DEEP_POSE runs no tracker to refine";
    if (e_refine_without_e_tracker(r, o)) return "dfvo_pipeline_set_refine: e_enable under tracking_method DFVO_TRACKING_PNP: no E-tracker runs";
    return nullptr;
}
// dfvo_pipeline_set_options / _set_iterative, behind their own rules: the candidate block beside the committed refinement block
inline const char* options_refine_refusal(const dfvo_pipeline_opts& o, const dfvo_pipeline_refine_opts& r) {
    if (refine_with_deep_pose(r, o)) return "dfvo_pipeline_set_options: tracking_method DFVO_TRACKING_DEEP_POSE beside dfvo_pipeline_set_refine";
    if (e_refine_without_e_tracker(r, o))
        return "dfvo_pipeline_set_options: tracking_method DFVO_TRACKING_PNP beside dfvo_pipeline_set_refine's e_enable: no E-tracker runs";
    return nullptr;
}
inline const char* iter_refine_refusal(const dfvo_pipeline_iter_opts& it, const dfvo_pipeline_refine_opts& r) {
    return refine_with_iterative(r, it) ? "dfvo_pipeline_set_iterative: not beside dfvo_pipeline_set_refine (the keypoint refinement runs under "
                                          "scale_recovery.method simple)"
                                        : nullptr;
}

inline const char* depth_source_refusal(const dfvo_pipeline_depth_src& d) {
    if (!(d.source == DFVO_DEPTH_NET || d.source == DFVO_DEPTH_EXTERNAL))
        return "dfvo_pipeline_set_depth_source: source is DFVO_DEPTH_NET or DFVO_DEPTH_EXTERNAL";
    if (d.source == DFVO_DEPTH_NET) return nullptr;
    if (!(d.scale > 0.0 && d.scale <= 1.7976931348623157e308)) return "dfvo_pipeline_set_depth_source: scale must be finite and > 0";
    if (!(d.src_h >= 1 && d.src_w >= 1)) return "dfvo_pipeline_set_depth_source: src_h, src_w >= 1";
    return nullptr;
}

// dfvo_pipeline_set_pose_net: the candidate block `po` beside the committed option block
inline const char* pose_net_refusal(const dfvo_pipeline_opts& o, const dfvo_pipeline_pose_opts& po) {
    if (!po.enable) {
        if (po.depth_consistency) return "dfvo_pipeline_set_pose_net: depth_consistency needs enable (the mask reads the net's pose)";
        if (deep_pose_without_net(o, po)) return "dfvo_pipeline_set_pose_net: tracking_method DFVO_TRACKING_DEEP_POSE needs the pose net";
    } else if (po.depth_consistency) {
        if (mask_off_local_bestn(o, po))
            return "dfvo_pipeline_set_pose_net: depth_consistency masks kp_source DFVO_KP_SOURCE_LOCAL_BESTN only (kp_selection.py:118-148)";
        if (deep_pose_with_mask(o, po))
            return "dfvo_pipeline_set_pose_net: depth_consistency under tracking_method DFVO_TRACKING_DEEP_POSE: nothing "
                   "selects keypoints";
        if (po.depth_thre != po.depth_thre) return "dfvo_pipeline_set_pose_net: depth_thre is NaN";
    }
    return nullptr;
}

}  // namespace dfvo
