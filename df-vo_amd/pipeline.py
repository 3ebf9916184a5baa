"""Host driver of the fused per-pair pipeline (dfvo_pipeline_*): configuration marshalling, the
double-buffered net/solver software pipeline, and pose accumulation as in
the reference's libs/dfvo.py:109-119 (update_global_pose) and :121-262 (tracking: the hybrid path of
default_configuration.yml, and through the option keys below the keypoint sources, validity / scale methods, the
PnP-only tracking and the iterative scale recovery of the shipped ablation files, depth.depth_src gt: 16-bit depth images in
the place of the depth net, and the pose net with its two consumers, the kp_selection.depth_consistency mask and tracking_method
deep_pose; options_from_cfg maps the reference's configuration object to them)."""
import ctypes as C

import numpy as np
import torch

from . import capi

DEFAULTS = dict(  # options/examples/default_configuration.yml
    net_min_depth=0.1, net_max_depth=100.0, baseline_mult=5.4, min_depth=0.0, max_depth=50.0,
    depth_crop=((0.3, 1.0), (0.0, 1.0)), kp_num_row=10, kp_num_col=10, kp_num_bestN=2000, kp_thre=0.1,
    e_reproj_thre=0.2, e_repeat=5, e_max_iters=1000, scale_min_samples=3, scale_max_trials=100,
    scale_stop_prob=0.99, scale_thre=0.1, seed=4869, pnp_repeat=5, pnp_iters=100, pnp_reproj_thre=1.0)

STATUS = {0: "E", 1: "constant_motion", 2: "needs_pnp", 3: "PnP", 4: "DeepPose"}

# dfvo_pipeline_set_options: the tracking configurations beyond default_configuration.yml.  Every key defaults to that
# configuration; the values are the reference's own spellings (options/examples/ablation_*.yml)
OPTION_DEFAULTS = dict(kp_source="local_bestN", kp_score_method="flow", kp_sampled_num=2000, flow_crop=((0.0, 1.0), (0.0, 1.0)),
                       validity="GRIC", validity_thre=None, scale_method="depth_ratio", tracking_method="hybrid")
_KP_SOURCE = {"local_bestN": 0, "bestN": 1, "sampled": 2}
_KP_SCORE = {"flow": 0, "flow_ratio": 1}
_VALIDITY = {"GRIC": 0, "flow": 1, "homo_ratio": 2}
_SCALE_METHOD = {"depth_ratio": 0, "abs_diff": 1}
_TRACKING = {"hybrid": 0, "PnP": 1, "deep_pose": 2}

# dfvo_pipeline_set_iterative: scale_recovery.method and the kp_selection.rigid_flow_kp block (ablation_scale_iterative.yml).
# One table per option block of the library (_split_options deals an override dict out to them)
ITER_DEFAULTS = dict(scale_recovery="simple", iter_kp_src="kp_best", rigid_num_bestN=2000, rigid_num_row=10, rigid_num_col=10,
                     rigid_flow_thre=5.0, optical_flow_thre=0.1)
_SCALE_RECOVERY = {"simple": 0, "iterative": 1}
_ITER_KP_SRC = {"kp_depth": 0, "kp_best": 1}
ITER_STATUS = {0: "finished", 1: "empty_selection", 2: "no_consensus", 3: "not_run"}

# dfvo_pipeline_set_refine: the iterative_kp blocks of e_tracker / scale_recovery / pnp_tracker under scale_recovery.method simple
# (a second tracker pass on the rigid-flow keypoints kp_depth, dfvo.py:194-222, 236-244).  The grid and the thresholds are
# ITER_DEFAULTS' rigid_* / *_flow_thre keys (kp_selection.rigid_flow_kp), shared with the iterative scale loop
REFINE_DEFAULTS = dict(e_iterative_kp=False, scale_iterative_kp=False, pnp_iterative_kp=False, e_iterative_score="opt_flow",
                       pnp_iterative_score="rigid_flow")
_REFINE_SCORE = {"opt_flow": 0, "rigid_flow": 1}

# dfvo_pipeline_set_depth_source: depth.depth_src.  "external" (depth_src: gt) tracks on a 16-bit depth image per frame in the
# place of the depth net; depth_scale is the loader's scale_factor of read_depth (500 kitti.py, 5000 tum.py / kinect.py: not in
# the reference's YAML), depth_size the (height, width) of those images, None = the image size
DEPTH_DEFAULTS = dict(depth_source="net", depth_scale=None, depth_size=None)
_DEPTH_SOURCE = {"net": capi.DEPTH_NET, "external": capi.DEPTH_EXTERNAL}


# dfvo_pipeline_set_pose_net: deep_pose.enable (monodepth2's two-frame pose net on the depth stream) and what reads its pose --
# kp_selection.depth_consistency (enable, thre) here, tracking_method "deep_pose" among the option keys
POSE_DEFAULTS = dict(pose_net=False, depth_consistency=False, depth_consistency_thre=0.05)

_NUMBER = (int, float, np.integer, np.floating)


def _ptr(t):
    """the device (or host) pointer of a tensor for the C ABI; None stays NULL"""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _split_options(overrides):
    """an override dict as the five blocks (DEFAULTS + OPTION_DEFAULTS, ITER_DEFAULTS, DEPTH_DEFAULTS, POSE_DEFAULTS,
    REFINE_DEFAULTS), each with its defaults filled in; a key of none of the last four goes to the first"""
    blocks = [dict(DEFAULTS, **OPTION_DEFAULTS), dict(ITER_DEFAULTS), dict(DEPTH_DEFAULTS), dict(POSE_DEFAULTS), dict(REFINE_DEFAULTS)]
    for k, v in overrides.items():
        next((b for b in blocks[1:] if k in b), blocks[0])[k] = v
    return blocks


def _choice(o, key, table):
    v = o[key]
    if v not in table:
        raise ValueError("%s = %r: one of %s" % (key, v, ", ".join(repr(k) for k in table)))
    return table[v]


def _positive_int(key, v, numbers_only=True):
    """`v` as an int; ValueError naming `key` unless it is a whole number >= 1 (numbers_only=False: whatever int() takes)"""
    if isinstance(v, bool) or (numbers_only and not isinstance(v, _NUMBER)) or int(v) != v or v < 1:
        raise ValueError("%s = %r: a positive integer" % (key, v))
    return int(v)


def _finite(key, v, what="a finite threshold", refused=(bool, str), numbers_only=False):
    """`v` as a float; ValueError naming `key` for None, the `refused` types, with numbers_only anything but a number, and what
    float() does not make finite"""
    if v is None or isinstance(v, refused) or (numbers_only and not isinstance(v, _NUMBER)) or not np.isfinite(float(v)):
        raise ValueError("%s = %r: %s" % (key, v, what))
    return float(v)


def check_options(o):
    """the option keys of `o` (OPTION_DEFAULTS filled in) as the fields of capi.PipelineOpts; ValueError on a bad value"""
    f = dict(kp_source=_choice(o, "kp_source", _KP_SOURCE), kp_score_method=_choice(o, "kp_score_method", _KP_SCORE),
             validity_method=_choice(o, "validity", _VALIDITY), scale_method=_choice(o, "scale_method", _SCALE_METHOD),
             tracking_method=_choice(o, "tracking_method", _TRACKING))
    f["kp_sampled_num"] = _positive_int("kp_sampled_num", o["kp_sampled_num"], numbers_only=False)
    try:
        (y0, y1), (x0, x1) = o["flow_crop"]
        crop = [float(v) for v in (y0, y1, x0, x1)]
    except (TypeError, ValueError):
        raise ValueError("flow_crop = %r: [[y0, y1], [x0, x1]] fractions" % (o["flow_crop"],))
    if not (0.0 <= crop[0] < crop[1] <= 1.0 and 0.0 <= crop[2] < crop[3] <= 1.0):
        raise ValueError("flow_crop = %r: 0 <= y0 < y1 <= 1 and 0 <= x0 < x1 <= 1" % (o["flow_crop"],))
    f["flow_crop"] = crop
    f["validity_thre"] = 0.0  # (unused under GRIC: E_tracker.py:196-205)
    if o["validity"] != "GRIC":
        f["validity_thre"] = _finite("validity_thre", o["validity_thre"], "validity %r needs a finite threshold" % (o["validity"],), refused=bool)
    return f


def check_iter_options(o):
    """the iterative-scale keys of `o` (ITER_DEFAULTS filled in) as the fields of capi.PipelineIterOpts; ValueError on a bad value"""
    f = dict(enable=_choice(o, "scale_recovery", _SCALE_RECOVERY), kp_src=_choice(o, "iter_kp_src", _ITER_KP_SRC))
    for key, field in (("rigid_num_bestN", "num_bestN"), ("rigid_num_row", "num_row"), ("rigid_num_col", "num_col")):
        f[field] = _positive_int(key, o[key])
    for key in ("rigid_flow_thre", "optical_flow_thre"):
        f[key] = _finite(key, o[key])
    if f["num_bestN"] < f["num_row"] * f["num_col"]:
        raise ValueError("rigid_num_bestN = %r: fewer than one keypoint per cell of the %d x %d grid (rigid_num_row, rigid_num_col)"
                         % (o["rigid_num_bestN"], f["num_row"], f["num_col"]))
    return f


def check_refine_options(o, io=None, tracking_method="hybrid"):
    """the refinement keys of `o` (REFINE_DEFAULTS filled in) beside the iterative block `io` (ITER_DEFAULTS filled in: the grid,
    the thresholds, the scale method) as the fields of capi.PipelineRefineOpts, None when no refinement is on; ValueError on a
    bad value"""
    io = dict(ITER_DEFAULTS) if io is None else io
    for key in ("e_iterative_kp", "scale_iterative_kp", "pnp_iterative_kp"):
        if not isinstance(o[key], (bool, np.bool_)):
            raise ValueError("%s = %r: True or False" % (key, o[key]))
    f = dict(e_enable=int(o["e_iterative_kp"]), scale_enable=int(o["scale_iterative_kp"]), pnp_enable=int(o["pnp_iterative_kp"]),
             e_score_rigid=_choice(o, "e_iterative_score", _REFINE_SCORE), pnp_score_rigid=_choice(o, "pnp_iterative_score", _REFINE_SCORE))
    if not (f["e_enable"] or f["scale_enable"] or f["pnp_enable"]):
        return None
    if f["scale_enable"] and not f["e_enable"]:
        raise ValueError("scale_iterative_kp = True without e_iterative_kp: the second scale stage runs behind the second E pass")
    if io["scale_recovery"] != "simple":
        raise ValueError("the keypoint refinement (e_ / scale_ / pnp_iterative_kp) runs under scale_recovery 'simple', not %r"
                         % (io["scale_recovery"],))
    if tracking_method == "deep_pose":
        raise ValueError("the keypoint refinement under tracking_method 'deep_pose': no tracker runs")
    if tracking_method == "PnP" and f["e_enable"]:
        raise ValueError("e_iterative_kp = True under tracking_method 'PnP': no E-tracker runs")
    g = check_iter_options(dict(io, scale_recovery="simple"))
    f.update({k: g[k] for k in ("num_row", "num_col", "num_bestN", "rigid_flow_thre", "optical_flow_thre")})
    return f


def check_depth_options(o, img_h=None, img_w=None):
    """the depth-source keys of `o` (DEPTH_DEFAULTS filled in) as the fields of capi.PipelineDepthSrc; ValueError on a bad value"""
    f = dict(source=_choice(o, "depth_source", _DEPTH_SOURCE), scale=0.0, src_h=0, src_w=0)
    size = o["depth_size"]
    if size is not None:
        try:
            sh, sw = size
        except (TypeError, ValueError):
            raise ValueError("depth_size = %r: (height, width) of the depth images, or None for the image size" % (size,))
        try:
            f["src_h"], f["src_w"] = _positive_int("depth_size", sh), _positive_int("depth_size", sw)
        except ValueError:
            raise ValueError("depth_size = %r: two positive integers" % (size,)) from None
    elif img_h is not None:
        f["src_h"], f["src_w"] = int(img_h), int(img_w)
    if o["depth_source"] == "external":
        what = "depth_source 'external' needs the depth images' scale factor, finite and > 0 (read_depth: 500 for KITTI, 5000 for TUM)"
        f["scale"] = _finite("depth_scale", o["depth_scale"], what, numbers_only=True)
        if f["scale"] <= 0:
            raise ValueError("depth_scale = %r: %s" % (o["depth_scale"], what))
    return f


def check_pose_options(o, kp_source="local_bestN"):
    """the pose-lane keys of `o` (POSE_DEFAULTS filled in) as the fields of capi.PipelinePoseOpts; ValueError on a bad value"""
    for key in ("pose_net", "depth_consistency"):
        if not isinstance(o[key], (bool, np.bool_)):
            raise ValueError("%s = %r: True or False" % (key, o[key]))
    thre = _finite("depth_consistency_thre", o["depth_consistency_thre"], numbers_only=True)
    if o["depth_consistency"] and not o["pose_net"]:
        raise ValueError("depth_consistency = True without pose_net: the mask is computed from the pose net's pose")
    if o["depth_consistency"] and kp_source != "local_bestN":
        raise ValueError("depth_consistency = True with kp_source = %r: the reference masks local_bestN only" % (kp_source,))
    return dict(enable=int(o["pose_net"]), depth_consistency=int(o["depth_consistency"]), depth_thre=thre)


def options_from_cfg(cfg):
    """The reference's configuration object (default_cfg.Cfg / EasyDict of options/examples/*.yml) as the override dict of
    TrackingPipeline -- only the keys that differ from DEFAULTS / OPTION_DEFAULTS, so default_configuration.yml maps to {}.
    NotImplementedError, naming the key, for what the fused pipeline does not run."""
    def get(path, default=None):
        node = cfg
        for k in path.split("."):
            if node is None or k not in node:
                return default
            node = node[k]
        return node

    method = get("scale_recovery.method", "simple")
    if method not in _SCALE_RECOVERY:
        raise NotImplementedError("scale_recovery.method: %s: not run by the fused pipeline" % method)
    iterative = method == "iterative"
    if get("online_finetune.enable", False):
        raise NotImplementedError("online_finetune.enable: not run by the fused pipeline")
    # the trackers' iterative keypoint refinement (dfvo.py:194-222, 236-244): under the simple scale method, on kp_depth
    refine = {k: bool(get(k + ".iterative_kp.enable", False)) for k in ("e_tracker", "scale_recovery", "pnp_tracker")}
    rigid_kp = bool(get("kp_selection.rigid_flow_kp.enable", False))
    for k, on in refine.items():
        if on and iterative:
            raise NotImplementedError("%s.iterative_kp.enable: under scale_recovery.method: iterative: not run by the fused pipeline" % k)
        if on and not rigid_kp:  # (kp_selection_good_depth returns nothing then: the reference dies on the missing key)
            raise NotImplementedError("%s.iterative_kp.enable: without kp_selection.rigid_flow_kp.enable nothing selects kp_depth" % k)
        if on and get(k + ".iterative_kp.kp_src", "kp_depth") != "kp_depth":
            raise NotImplementedError("%s.iterative_kp.kp_src: %s: the second pass runs on kp_depth"
                                      % (k, get(k + ".iterative_kp.kp_src")))
    if rigid_kp and not iterative and not any(refine.values()):
        raise NotImplementedError("kp_selection.rigid_flow_kp.enable: nothing reads the rigid-flow keypoints (no iterative_kp block "
                                  "is enabled, scale_recovery.method is simple)")
    if refine["scale_recovery"] and not refine["e_tracker"]:
        raise NotImplementedError("scale_recovery.iterative_kp.enable: without e_tracker.iterative_kp.enable nothing reads it")
    # the pose net runs for a consumer: tracking_method deep_pose (dfvo.py:252-255) or the depth mask of hybrid / PnP tracking
    tracking = get("tracking_method", "hybrid")
    deep, mask = bool(get("deep_pose.enable", False)), bool(get("kp_selection.depth_consistency.enable", False))
    if mask and not deep:  # (DepthConsistency.compute dies on the missing ref_data['deep_pose'])
        raise NotImplementedError("kp_selection.depth_consistency.enable: without deep_pose.enable the mask has no pose to warp with")
    if tracking == "deep_pose" and not deep:
        raise NotImplementedError("tracking_method: deep_pose without deep_pose.enable: there is no pose net to track with")
    if tracking == "deep_pose":
        mask = False  # (dfvo.py:139-143: the map is computed in the hybrid / PnP branch only)
        for k, on in refine.items():
            if on:
                raise NotImplementedError("%s.iterative_kp.enable: under tracking_method: deep_pose no tracker runs" % k)
    if tracking == "PnP":  # (dfvo.py:165: the E-tracker's blocks are not read)
        refine["e_tracker"] = refine["scale_recovery"] = False
        if rigid_kp and not iterative and not refine["pnp_tracker"]:
            raise NotImplementedError("kp_selection.rigid_flow_kp.enable: nothing reads the rigid-flow keypoints under "
                                      "tracking_method: PnP without pnp_tracker.iterative_kp.enable")
    if deep and not mask and tracking != "deep_pose":
        raise NotImplementedError("deep_pose.enable: nothing reads the pose (tracking_method is not deep_pose, "
                                  "kp_selection.depth_consistency is off): the fused pipeline does not run the net")
    if iterative and not get("kp_selection.rigid_flow_kp.enable", False):
        # (kp_selection_good_depth returns nothing then, and the loop dies on its missing key: E_tracker.py:541,671)
        raise NotImplementedError("kp_selection.rigid_flow_kp.enable: False under scale_recovery.method: iterative: the loop "
                                  "selects its keypoints there")
    srcs = {k: get(k + ".kp_src", "kp_best") for k in ("e_tracker", "scale_recovery", "pnp_tracker")}
    iter_kp_src = "kp_best"
    if iterative and srcs["scale_recovery"] == "kp_depth":  # each round's scale from that round's rigid-flow keypoints
        iter_kp_src = "kp_depth"
        srcs["scale_recovery"] = srcs["e_tracker"]
    for k, v in srcs.items():
        if v == "kp_depth":
            raise NotImplementedError("%s.kp_src: kp_depth: not run by the fused pipeline" % k)
        if v not in ("kp_best", "kp_list"):
            raise NotImplementedError("%s.kp_src: %s: unknown keypoint source" % (k, v))
    if len(set(srcs.values())) != 1:
        raise NotImplementedError("kp_src: %s disagree; the fused pipeline tracks one keypoint set" % ", ".join(
            "%s.kp_src = %s" % kv for kv in sorted(srcs.items())))
    src = srcs["e_tracker"]
    if tracking == "deep_pose":
        # nothing selects keypoints: the source keys are not read
        return {"tracking_method": "deep_pose", "pose_net": True}
    if src == "kp_best":  # keypoint_sampler.py:108-129: local_bestN, else bestN
        if get("kp_selection.local_bestN.enable", False):
            source = "local_bestN"
        elif get("kp_selection.bestN.enable", False):
            source = "bestN"
        else:
            raise NotImplementedError("kp_src: kp_best, but neither kp_selection.local_bestN nor kp_selection.bestN is enabled")
    else:
        if not get("kp_selection.sampled_kp.enable", False):
            raise NotImplementedError("kp_src: kp_list, but kp_selection.sampled_kp is not enabled")
        source = "sampled"
    if mask and source != "local_bestN":
        raise NotImplementedError("kp_selection.depth_consistency.enable: with keypoint source %s: the reference masks "
                                  "kp_selection.local_bestN only" % source)
    full = dict(kp_source=source, tracking_method=tracking,
                validity=get("e_tracker.validity.method", "GRIC"),
                scale_method=get("scale_recovery.ransac.method", "depth_ratio"),
                seed=get("seed", 4869), min_depth=get("depth.min_depth", 0.0), max_depth=get("depth.max_depth", 50.0),
                e_reproj_thre=get("e_tracker.ransac.reproj_thre", 0.2), e_repeat=get("e_tracker.ransac.repeat", 5),
                scale_min_samples=get("scale_recovery.ransac.min_samples", 3),
                scale_max_trials=get("scale_recovery.ransac.max_trials", 100),
                scale_stop_prob=get("scale_recovery.ransac.stop_prob", 0.99), scale_thre=get("scale_recovery.ransac.thre", 0.1),
                pnp_repeat=get("pnp_tracker.ransac.repeat", 5), pnp_iters=get("pnp_tracker.ransac.iter", 100),
                pnp_reproj_thre=get("pnp_tracker.ransac.reproj_thre", 1.0))
    crop = get("crop.depth_crop")
    if crop is not None:
        full["depth_crop"] = tuple(tuple(float(v) for v in r) for r in crop)
    if full["validity"] != "GRIC":
        full["validity_thre"] = get("e_tracker.validity.thre")
    if source == "local_bestN":
        full.update(kp_num_bestN=get("kp_selection.local_bestN.num_bestN", 2000), kp_num_row=get("kp_selection.local_bestN.num_row", 10),
                    kp_num_col=get("kp_selection.local_bestN.num_col", 10), kp_thre=get("kp_selection.local_bestN.thre", 0.1),
                    kp_score_method=get("kp_selection.local_bestN.score_method", "flow"))
    elif source == "bestN":
        full["kp_num_bestN"] = get("kp_selection.bestN.num_bestN", 2000)
    else:
        full["kp_sampled_num"] = get("kp_selection.sampled_kp.num_kp", 2000)
        fc = get("crop.flow_crop")
        if fc is not None:
            full["flow_crop"] = tuple(tuple(float(v) for v in r) for r in fc)
    if iterative or any(refine.values()):
        rk = "kp_selection.rigid_flow_kp."
        full.update(rigid_num_bestN=get(rk + "num_bestN", 2000),
                    rigid_num_row=get(rk + "num_row", 10), rigid_num_col=get(rk + "num_col", 10),
                    rigid_flow_thre=get(rk + "rigid_flow_thre", 5), optical_flow_thre=get(rk + "optical_flow_thre", 0.1))
    if iterative:
        full.update(scale_recovery="iterative", iter_kp_src=iter_kp_src)
    if any(refine.values()):
        full.update(e_iterative_kp=refine["e_tracker"], scale_iterative_kp=refine["scale_recovery"],
                    pnp_iterative_kp=refine["pnp_tracker"])
        if refine["e_tracker"]:
            full["e_iterative_score"] = get("e_tracker.iterative_kp.score_method", "opt_flow")
        if refine["pnp_tracker"]:
            full["pnp_iterative_score"] = get("pnp_tracker.iterative_kp.score_method", "rigid_flow")
    depth_src = get("depth.depth_src")
    if depth_src == "gt":  # dfvo.py:296-319: read_depth's image in the place of the depth net (depth_scale: the loader's, an override)
        full["depth_source"] = "external"
    elif depth_src is not None:
        raise NotImplementedError("depth.depth_src: %s: not run by the fused pipeline (None: the depth net, gt: 16-bit depth images)"
                                  % (depth_src,))
    if mask:
        full.update(pose_net=True, depth_consistency=True, depth_consistency_thre=get("kp_selection.depth_consistency.thre", 0.05))
    base = {k: v for block in _split_options({}) for k, v in block.items()}
    out = {k: v for k, v in full.items() if base.get(k) != v}
    o, io, _, po, ro = _split_options(out)
    check_options(o)
    check_iter_options(io)
    check_pose_options(po, source)
    check_refine_options(ro, io, tracking)
    return out


class TrackingPipeline:
    def __init__(self, img_h, img_w, feed_h, feed_w, K, flow_sd, depth_sd, pose_sd=None, **overrides):
        o, io, do, po, ro = _split_options(overrides)
        fields = check_options(o)  # (before anything touches the device: a bad value is a ValueError)
        iter_fields = check_iter_options(io)
        refine_fields = check_refine_options(ro, io, o["tracking_method"])
        depth_fields = check_depth_options(do, img_h, img_w)
        pose_fields = check_pose_options(po, o["kp_source"])
        self.deep_pose = o["tracking_method"] == "deep_pose"
        if self.deep_pose and not po["pose_net"]:
            raise ValueError("tracking_method = 'deep_pose' without pose_net = True: there is no pose net to track with")
        if self.deep_pose and po["depth_consistency"]:
            raise ValueError("depth_consistency = True under tracking_method 'deep_pose': nothing selects keypoints")
        if po["pose_net"] and pose_sd is None:
            raise ValueError("pose_sd = None: pose_net = True runs the pose net and needs its weights")
        self.external_depth = do["depth_source"] == "external"
        if depth_sd is None and not self.external_depth:
            raise ValueError("depth_sd = None: depth_source 'net' runs the depth net and needs its weights (depth_source "
                             "'external' tracks on 16-bit depth images and takes none)")
        capi.require_gpu()
        self.lib = capi.lib()
        self.opts = o
        self.iter_opts = io
        self.depth_opts = do
        self.pose_opts = po
        self.refine_opts = ro
        self.refine = refine_fields is not None
        self.depth_size = (depth_fields["src_h"], depth_fields["src_w"])
        self.iterative = io["scale_recovery"] == "iterative"
        self.H, self.W, self.feed_h, self.feed_w = img_h, img_w, feed_h, feed_w
        K = np.asarray(K, np.float64)
        self.K = K
        cfg = capi.PipelineCfg(img_h=img_h, img_w=img_w, feed_h=feed_h, feed_w=feed_w,
                               net_min_depth=o["net_min_depth"], net_max_depth=o["net_max_depth"],
                               baseline_mult=o["baseline_mult"], min_depth=o["min_depth"], max_depth=o["max_depth"],
                               fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], kp_num_row=o["kp_num_row"],
                               kp_num_col=o["kp_num_col"], kp_num_bestN=o["kp_num_bestN"], kp_thre=o["kp_thre"],
                               e_reproj_thre=o["e_reproj_thre"], e_repeat=o["e_repeat"], e_max_iters=o["e_max_iters"],
                               scale_min_samples=o["scale_min_samples"], scale_max_trials=o["scale_max_trials"],
                               scale_stop_prob=o["scale_stop_prob"], scale_thre=o["scale_thre"], seed=o["seed"],
                               pnp_repeat=o["pnp_repeat"], pnp_iters=o["pnp_iters"],
                               pnp_reproj_thre=o["pnp_reproj_thre"])
        (y0, y1), (x0, x1) = o["depth_crop"]
        for i, v in enumerate((y0, y1, x0, x1)):
            cfg.depth_crop[i] = v
        KinvT, Kinv = np.linalg.inv(K.T), np.linalg.inv(K)
        for i in range(9):
            cfg.KinvT[i] = KinvT.flat[i]
            cfg.Kinv[i] = Kinv.flat[i]
        h = C.c_void_p()
        capi.check(self.lib.dfvo_pipeline_create(C.byref(cfg), C.byref(h)))
        self.h = h
        if self.external_depth:  # (a pipeline of the depth net makes no call here: it enqueues what it always did)
            self._apply(self.lib.dfvo_pipeline_set_depth_source, capi.PipelineDepthSrc(**depth_fields))
        if po["pose_net"]:  # (ahead of set_options, which takes tracking_method deep_pose only behind it)
            self._apply(self.lib.dfvo_pipeline_set_pose_net, capi.PipelinePoseOpts(**pose_fields))
        if any(o[k] != v for k, v in OPTION_DEFAULTS.items()):
            crop = fields.pop("flow_crop")
            popts = capi.PipelineOpts(**fields)
            for i, v in enumerate(crop):
                popts.flow_crop[i] = v
            self._apply(self.lib.dfvo_pipeline_set_options, popts)
        if self.iterative:  # (behind set_options: the bound on the tracked keypoints depends on the keypoint source)
            self._apply(self.lib.dfvo_pipeline_set_iterative, capi.PipelineIterOpts(**iter_fields))
        if self.refine:  # (behind set_options: what it refuses depends on the tracking method)
            self._apply(self.lib.dfvo_pipeline_set_refine, capi.PipelineRefineOpts(**refine_fields))
        # keypoints a pair can have (get_keypoints' default capacity)
        self.kp_max = {"local_bestN": o["kp_num_bestN"], "bestN": o["kp_num_bestN"], "sampled": o["kp_sampled_num"]}[o["kp_source"]]
        nh, nw = self._net_size(img_h, img_w)
        params = {k: (v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, np.float32))
                  for k, v in flow_sd.items()}
        for l in range(1, 7):
            params["aux.linspace_x.%d" % l] = torch.linspace(-1.0, 1.0, nw >> (l - 1)).numpy()
            params["aux.linspace_y.%d" % l] = torch.linspace(-1.0, 1.0, nh >> (l - 1)).numpy()
        capi.set_params(self.lib.dfvo_pipeline_set_flow_param, h, params)
        if not self.external_depth:
            dparams = {k: v.detach().cpu().float().numpy() for k, v in depth_sd.items()
                       if hasattr(v, "detach") and v.dim() > 0 and "num_batches_tracked" not in k}
            capi.set_params(self.lib.dfvo_pipeline_set_depth_param, h, dparams)
        if po["pose_net"]:
            pparams = {k: v.detach().cpu().float().numpy() for k, v in pose_sd.items()
                       if hasattr(v, "detach") and v.dim() > 0 and "num_batches_tracked" not in k and not k.startswith("encoder.fc")}
            capi.set_params(self.lib.dfvo_pipeline_set_pose_param, h, pparams)
        capi.check(self.lib.dfvo_pipeline_finalize(h))

    @classmethod
    def from_cfg(cls, cfg, K, flow_sd, depth_sd, feed_h, feed_w, pose_sd=None, **overrides):
        """a pipeline for the reference's configuration object `cfg` (image size from cfg.image); `overrides` win"""
        o = options_from_cfg(cfg)  # (depth.depth_src gt: depth_scale, the loader's scale factor, comes with `overrides`)
        o.update(overrides)
        return cls(int(cfg["image"]["height"]), int(cfg["image"]["width"]), feed_h, feed_w, K, flow_sd, depth_sd, pose_sd=pose_sd, **o)

    @staticmethod
    def _net_size(h, w):
        from .synthetic import _net_size
        return _net_size(h, w)

    def _apply(self, fn, struct):
        """one of the library's option setters on the new pipeline; a refusal closes it before the DfvoError goes on"""
        try:
            capi.check(fn(self.h, C.byref(struct)))
        except capi.DfvoError:
            self.close()
            raise

    def close(self):
        if self.h is not None:
            self.lib.dfvo_pipeline_destroy(self.h)
            self.h = None

    def seed(self, seed):
        capi.check(self.lib.dfvo_pipeline_seed(self.h, int(seed) & 0xffffffff))

    def set_graph(self, enable):
        capi.check(self.lib.dfvo_pipeline_set_graph(self.h, int(enable)))

    def _depth_image(self, depth, what):
        """host-side check of a 16-bit depth image (contiguous device uint16 [src_h, src_w]); its device pointer.  Which mode
        takes one is the library's decision (DFVO_ERR_ARG naming the call and the mode)"""
        ok = isinstance(depth, torch.Tensor) and depth.dtype == torch.uint16 and tuple(depth.shape) == self.depth_size \
            and depth.is_cuda and depth.is_contiguous()
        if not ok:
            got = "%s %s on %s" % (depth.dtype, list(depth.shape), depth.device) if isinstance(depth, torch.Tensor) else repr(type(depth))
            raise capi.DfvoError("%s: the depth image is a contiguous device uint16 tensor %s, got %s" % (what, list(self.depth_size), got))
        return C.c_void_p(depth.data_ptr())

    def enqueue_nets(self, slot, d_ref, d_cur, d_feed=None, depth=None):
        """device uint8 tensors (torch.cuda): ref/cur [H,W,3]; feed [feed_h,feed_w,3] = the LANCZOS-resized current
        frame, or None to have the pipeline resize d_cur on the device.
        d_ref=None: the reference frame is the current frame of the previous enqueue_nets call -- the flow net carries that
        frame's image / feature pyramids over instead of running Features on it again (sequences).
        depth (depth_source "external": required there, refused otherwise): the current frame's 16-bit depth image, a device
        uint16 tensor [src_h, src_w] (depth_size), under the frames' contract: complete when handed over, unchanged until
        the slot's track / track_end has returned.  d_feed has no reader then and is refused."""
        if depth is not None:
            dp = self._depth_image(depth, "enqueue_nets")
            if d_feed is not None:
                raise capi.DfvoError("enqueue_nets: d_feed beside a depth image: the depth net it would feed does not run")
            capi.check(self.lib.dfvo_pipeline_enqueue_nets_depth(self.h, slot, _ptr(d_ref), _ptr(d_cur), dp))
            return
        capi.check(self.lib.dfvo_pipeline_enqueue_nets(self.h, slot, _ptr(d_ref), _ptr(d_cur), _ptr(d_feed)))

    def prefetch_track(self, slot, flow=None, diff=None):
        """enqueue keypoint selection + the homography chain of `slot` now (call right after enqueue_nets(slot));
        track(slot) then only runs the RandomState consumers"""
        capi.check(self.lib.dfvo_pipeline_prefetch_track(self.h, slot, _ptr(flow), _ptr(diff)))

    def track(self, slot, flow=None, diff=None, depth=None, raw_depth=None):
        """raw_depth (iterative scale recovery, with `depth`): the raw float32 depth of the current frame, which becomes the
        next pair's ref_data['raw_depth'] in place of the depth net's"""
        if raw_depth is not None:
            self.set_raw_depth_override(slot, raw_depth)
        out = capi.TrackOut()
        capi.check(self.lib.dfvo_pipeline_track(self.h, slot, _ptr(flow), _ptr(diff), _ptr(depth), C.byref(out)))
        return out

    def track_begin(self, slot, flow=None, diff=None, depth=None, raw_depth=None):
        """first half of track(): enqueues the RandomState-ordered chain of `slot` and returns; the host can feed the nets of
        the pairs ahead while it runs.  Pair k + 1 must not be begun before track_end(k) returned."""
        if raw_depth is not None:
            self.set_raw_depth_override(slot, raw_depth)
        capi.check(self.lib.dfvo_pipeline_track_begin(self.h, slot, _ptr(flow), _ptr(diff), _ptr(depth)))

    def track_end(self, slot):
        out = capi.TrackOut()
        capi.check(self.lib.dfvo_pipeline_track_end(self.h, slot, C.byref(out)))
        return out

    def set_ref_depth(self, d_feed=None, depth=None, raw_depth=None):
        """depth of the first reference frame: the uint8 feed image (runs the depth net) or a processed depth map; raw_depth
        (with `depth`, iterative scale recovery): its raw float32 depth, ref_data['raw_depth'] of the first pair"""
        capi.check(self.lib.dfvo_pipeline_set_ref_depth(self.h, _ptr(d_feed), _ptr(depth)))
        if raw_depth is not None:
            capi.check(self.lib.dfvo_pipeline_set_ref_raw_depth(self.h, _ptr(raw_depth)))

    def set_raw_depth_override(self, slot, raw_depth):
        """the raw float32 depth [H,W] of `slot`'s current frame for the roll-over, until the slot's track_end (None withdraws)"""
        capi.check(self.lib.dfvo_pipeline_set_raw_depth_override(self.h, slot, _ptr(raw_depth)))

    def set_pose_override(self, slot, pose16):
        """a device float32 4x4 (contiguous) that the pair enqueued into `slot` next uses in the place of the pose net's; set
        before the slot's enqueue_nets, unchanged until its track_end, which withdraws it (as None does)"""
        capi.check(self.lib.dfvo_pipeline_set_pose_override(self.h, slot, _ptr(pose16)))

    def get_pose_net(self, slot):
        """(pose [4,4] f32, depth_diff [H,W] f32 or None without the mask): what the slot's last pair used"""
        pose = np.full((4, 4), np.nan, np.float32)  # (NaN: what the library does not write shows)
        m = np.full((self.H, self.W), np.nan, np.float32) if self.pose_opts["depth_consistency"] else None
        capi.check(self.lib.dfvo_pipeline_get_pose_net(self.h, slot, capi.as_ptr(pose), capi.as_ptr(m)))
        return pose, m

    def get_prev_scale(self):
        """EssTracker.prev_scale as the pipeline carries it on the device (iterative scale recovery)"""
        v = C.c_double(0.0)
        capi.check(self.lib.dfvo_pipeline_get_prev_scale(self.h, C.byref(v)))
        return v.value

    def set_prev_scale(self, scale):
        capi.check(self.lib.dfvo_pipeline_set_prev_scale(self.h, float(scale)))

    def get_iterative(self, slot, want_map=False):
        """the iterative scale loop's record of the pair last collected from `slot`: dict(status "finished" | "empty_selection"
        | "no_consensus" | "not_run", scale, n_iter, kp_round, scale_in [5], scale_out [5], n_kp_round [5], ref_kp / cur_kp [n,2]:
        the uniform keypoints of the last round that selected any, rigid_flow_diff [H,W] f32 with want_map)"""
        cap = max(1, self.iter_opts["rigid_num_bestN"])
        out = capi.ScaleIterOut()
        kr, kc = np.zeros((cap, 2)), np.zeros((cap, 2))
        m = np.zeros((self.H, self.W), np.float32) if want_map else None
        capi.check(self.lib.dfvo_pipeline_get_iterative(self.h, slot, C.byref(out), cap, capi.as_ptr(kr), capi.as_ptr(kc),
                                                        capi.as_ptr(m)))
        assert out.n_kp <= cap
        return dict(status=ITER_STATUS[out.status], scale=out.scale, n_iter=out.n_iter, kp_round=out.kp_round,
                    scale_in=list(out.scale_in), scale_out=list(out.scale_out), n_kp_round=list(out.n_kp_round),
                    ref_kp=kr[:out.n_kp], cur_kp=kc[:out.n_kp], rigid_flow_diff=m if out.kp_round >= 0 else None)

    def get_refine(self, slot, want_map=False):
        """the keypoint refinement's record of the pair last collected from `slot`: dict(e_ran, scale_ran, pnp_ran, empty, R1 [3,3],
        t1 [3], scale1: E pass one; scale2; pnp_found1, pnp_R1, pnp_t1: PnP pass one; ref_kp / cur_kp [n,2]: kp_depth of the pair's
        last selection; inliers [m] bool: the second E pass's mask over ITS kp_depth (m = n unless a PnP selection followed);
        rigid_flow_diff [H,W] f32 with want_map, None when no selection ran)"""
        cap = max(1, self.iter_opts["rigid_num_bestN"])
        out = capi.RefineOut()
        kr, kc, inl = np.zeros((cap, 2)), np.zeros((cap, 2)), np.zeros(cap, np.uint8)
        m = np.zeros((self.H, self.W), np.float32) if want_map else None
        capi.check(self.lib.dfvo_pipeline_get_refine(self.h, slot, C.byref(out), cap, capi.as_ptr(kr), capi.as_ptr(kc),
                                                     capi.as_ptr(inl), capi.as_ptr(m)))
        assert out.n_kp <= cap and out.n_inliers <= cap
        return dict(e_ran=bool(out.e_ran), scale_ran=bool(out.scale_ran), pnp_ran=bool(out.pnp_ran), empty=bool(out.empty),
                    R1=np.array(out.R1[:]).reshape(3, 3), t1=np.array(out.t1[:]), scale1=out.scale1, scale2=out.scale2,
                    pnp_found1=bool(out.pnp_found1), pnp_R1=np.array(out.pnp_R1[:]).reshape(3, 3), pnp_t1=np.array(out.pnp_t1[:]),
                    ref_kp=kr[:out.n_kp], cur_kp=kc[:out.n_kp], inliers=inl[:out.n_inliers].astype(bool),
                    rigid_flow_diff=m if (out.e_ran or out.pnp_ran) else None)

    def set_ref_depth_image(self, d_depth_u16):
        """depth of the first reference frame from its 16-bit depth image (depth_source "external"; device uint16
        [src_h, src_w]): raw and processed reference depth in one launch, nothing else to set for the iterative scale loop"""
        capi.check(self.lib.dfvo_pipeline_set_ref_depth_u16(self.h, self._depth_image(d_depth_u16, "set_ref_depth_image")))

    def set_ref_image(self, d_img):
        """depth of the first reference frame from the full-size uint8 frame (device LANCZOS resize + depth net)"""
        capi.check(self.lib.dfvo_pipeline_set_ref_image(self.h, _ptr(d_img)))

    def sync(self):
        capi.check(self.lib.dfvo_pipeline_sync(self.h))

    def stream_layout(self):
        """the stream layout in use, parsed: {"layout": "lanes" | "wide" | "creation", "groups": n, "queues": n, "streams": n,
        "trk": i, ...} with, per role, the index of its stream (dfvo_pipeline_stream_layout); "text" is the line itself"""
        buf = C.create_string_buffer(256)
        capi.check(self.lib.dfvo_pipeline_stream_layout(self.h, buf, len(buf)))
        text = buf.value.decode()
        d = {"text": text}
        for kv in text.split():
            k, v = kv.split("=")
            d[k] = v if k == "layout" else int(v)
        return d

    def net_flops(self):
        return self.lib.dfvo_pipeline_net_flops(self.h)

    def get_outputs(self, slot):
        px = self.H * self.W
        fwd = np.zeros((2, self.H, self.W), np.float32)
        bwd = np.zeros((2, self.H, self.W), np.float32)
        diff = np.zeros((self.H, self.W), np.float32)
        raw = np.zeros((self.H, self.W), np.float32)
        dep = np.zeros((self.H, self.W), np.float64)
        capi.check(self.lib.dfvo_pipeline_get_flow(self.h, slot, capi.as_ptr(fwd), capi.as_ptr(bwd), capi.as_ptr(diff),
                                                   capi.as_ptr(raw), capi.as_ptr(dep)))
        return fwd, bwd, diff, raw, dep

    def get_ref_depth(self):
        """(raw [H,W] f32, processed [H,W] f64): the reference frame's depths as the next pair will read them"""
        raw = np.zeros((self.H, self.W), np.float32)
        dep = np.zeros((self.H, self.W), np.float64)
        capi.check(self.lib.dfvo_pipeline_get_ref_depth(self.h, capi.as_ptr(raw), capi.as_ptr(dep)))
        return raw, dep

    def get_keypoints(self, slot, cap=None):
        """the tracked keypoints of the reference / current frame [n,2] f64 and the E-tracker's inlier mask [n] bool for `slot`"""
        if cap is None:
            cap = max(4096, int(self.kp_max))
        kr = np.zeros((cap, 2))
        kc = np.zeros((cap, 2))
        inl = np.zeros(cap, np.uint8)
        n = C.c_int(0)
        capi.check(self.lib.dfvo_pipeline_get_keypoints(self.h, slot, cap, capi.as_ptr(kr), capi.as_ptr(kc), capi.as_ptr(inl),
                                                        C.byref(n)))
        assert n.value <= cap
        return kr[:n.value], kc[:n.value], inl[:n.value].astype(bool)

    def get_rng_state(self):
        """the device-resident numpy RandomState as np.random.get_state() would return it"""
        st = np.zeros(625, np.uint32)
        capi.check(self.lib.dfvo_pipeline_get_rng_state(self.h, capi.as_ptr(st)))
        return ("MT19937", st[:624].copy(), int(st[624]), 0, 0.0)

    def set_rng_state(self, state):
        st = np.zeros(625, np.uint32)
        st[:624] = state[1]
        st[624] = state[2]
        capi.check(self.lib.dfvo_pipeline_set_rng_state(self.h, capi.as_ptr(st)))

    # ---- hybrid pose + accumulation (dfvo.py:109-119, 163-262) -------------------------------------------
    @staticmethod
    def hybrid_pose(out, prev_motion):
        """relative pose cur -> ref as a 4x4; `prev_motion` is used for the constant-motion fallback"""
        T = np.eye(4)
        if out.status == 1:
            return prev_motion.copy(), "constant_motion"
        if out.status == 2:
            raise capi.DfvoError("PnP fallback required but no reference depth is known: call set_ref_depth() "
                                 "for the first frame")
        if out.status == 4:  # dfvo.py:252-255: SE3(ref_data['deep_pose'])
            T[:3, :3] = np.array(out.R[:]).reshape(3, 3)
            T[:3, 3] = np.array(out.t[:])
            return T, "DeepPose"
        if out.status == 3:  # pnp_tracker.py:112-118: SE3 from (R, t) of solvePnP, then pose = inv_pose
            T[:3, :3] = np.array(out.R[:]).reshape(3, 3)
            T[:3, 3] = np.array(out.t[:])
            return np.linalg.inv(T), "PnP"
        T[:3, :3] = np.array(out.R[:]).reshape(3, 3)
        T[:3, 3] = np.array(out.t[:]) * out.scale
        return T, "E"

    @staticmethod
    def accumulate(global_pose, rel):
        """update_global_pose (dfvo.py:109-119) with scale 1: t_w += R_w t ; R_w = R_w R"""
        g = global_pose.copy()
        g[:3, 3:] = g[:3, :3] @ rel[:3, 3:] + g[:3, 3:]
        g[:3, :3] = g[:3, :3] @ rel[:3, :3]
        return g
