"""A KITTI odometry folder through the fused pipeline: the dataset layer of the reference (libs/datasets/kitti.py KittiOdom,
libs/general/utils.py load_kitti_odom_intrinsics, libs/general/configuration.py ConfigLoader) as plain functions, and the runner
that puts a FrameStream under sequence.run_sequence.  Host only; the frames' way to the device is frame_stream.py."""
import glob
import os

import numpy as np

from . import sequence
from .default_cfg import Cfg
from .frame_stream import FrameStream
from .pipeline import TrackingPipeline

KITTI_RAW_H, KITTI_RAW_W = 370.0, 1226.0  # the loader's hard-coded raw image size, whatever the files' is
GT_DEPTH_SCALE = 500                      # kitti.py:157-159


def kitti_odom_intrinsics(calib_txt, h, w):
    """K [3,3] for images resized to h x w: load_kitti_odom_intrinsics(calib_txt, h, w)[2] (utils.py:240-262, kitti.py:70-84) --
    the THIRD line of calib.txt (P2), its fx, fy, cx, cy scaled from the hard-coded 1226 x 370 raw size with the loader's own
    operation order (x / raw * new)"""
    with open(calib_txt, "r") as f:
        lines = f.readlines()
    if len(lines) < 3:
        raise ValueError("%s: %d lines; the loader reads the third (P2)" % (calib_txt, len(lines)))
    p = [float(t) for t in lines[2].split(" ")[1:]]
    cx, cy = p[2] / KITTI_RAW_W * w, p[6] / KITTI_RAW_H * h
    fx, fy = p[0] / KITTI_RAW_W * w, p[5] / KITTI_RAW_H * h
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def kitti_odom_paths(img_seq_dir, seq, ext, depth_dir=None):
    """the files KittiOdom reads for sequence `seq` (kitti.py:27-39,86-167): as many frames as <img_seq_dir>/<seq>/image_2 holds
    *.<ext> files, frame i = image_2/%06d.<ext>; with depth_dir (depth.depth_src gt) its depth <depth_dir>/gt/<seq>/%010d.png at
    scale factor 500.  Returns {"calib", "images", "depths" (None without depth_dir), "depth_scale"}."""
    seq = str(seq)
    root = os.path.join(img_seq_dir, seq)
    img_dir = os.path.join(root, "image_2")
    n = len(glob.glob(os.path.join(img_dir, "*.{}".format(ext))))
    images = [os.path.join(img_dir, "{:06d}.{}".format(i, ext)) for i in range(n)]
    depths = None
    if depth_dir is not None:
        d = "{}/gt/{}/".format(depth_dir, seq)
        depths = [os.path.join(d, "{:010d}.png".format(i)) for i in range(n)]
    return dict(calib=os.path.join(root, "calib.txt"), images=images, depths=depths,
                depth_scale=GT_DEPTH_SCALE if depths is not None else None)


def _merge(base, new):
    """ConfigLoader.update_dict (configuration.py:71-89): keys of `new` replace those of `base`, except that a dictionary
    already in `base` is merged into, key by key.  (The loader tells a present key by `get(key, -1) != -1`: a value equal
    to -1 counts as absent -- and is replaced either way.)"""
    for k in new:
        if base.get(k, -1) != -1 and isinstance(base[k], dict):
            base[k] = _merge(base[k], new[k])
        else:
            base[k] = new[k]
    return base


def _as_cfg(node):
    if isinstance(node, dict):
        return Cfg((k, _as_cfg(v)) for k, v in node.items())
    if isinstance(node, (list, tuple)):  # (EasyDict converts dictionaries inside lists too)
        return type(node)(_as_cfg(v) for v in node)
    return node


def cfg_from_yaml(default_yml, overlay_yml=None):
    """ConfigLoader.merge_cfg([default_yml, overlay_yml]) (configuration.py:33-46) as a default_cfg.Cfg"""
    import yaml
    merged = {}
    for path in (default_yml, overlay_yml):
        if path is None:
            continue
        with open(path, "r") as f:
            merged = _merge(merged, yaml.load(f, Loader=yaml.FullLoader))
    return _as_cfg(merged)


def load_weights(cfg):
    """(flow_sd, depth_sd or None, pose_sd or None, feed_h, feed_w) from the files the configuration names: deep_flow.flow_net_weight,
    depth.deep_depth.pretrained_model (encoder.pth with the feed size + depth.pth; not read under depth.depth_src gt) and
    deep_pose.pretrained_model (pose_encoder.pth + pose.pth) when deep_pose.enable"""
    import torch
    flow_sd = torch.load(cfg["deep_flow"]["flow_net_weight"], map_location="cpu")
    depth_sd, feed_h, feed_w = None, 192, 640
    if cfg.get("depth", {}).get("depth_src") is None:
        d = cfg["depth"]["deep_depth"]["pretrained_model"]
        depth_sd = dict(torch.load(os.path.join(d, "encoder.pth"), map_location="cpu"))
        feed_h, feed_w = int(depth_sd["height"]), int(depth_sd["width"])
        depth_sd.update(torch.load(os.path.join(d, "depth.pth"), map_location="cpu"))
    pose_sd = None
    if cfg.get("deep_pose", {}).get("enable"):
        d = cfg["deep_pose"]["pretrained_model"]
        pose_sd = dict(torch.load(os.path.join(d, "pose_encoder.pth"), map_location="cpu"))
        pose_sd.update(torch.load(os.path.join(d, "pose.pth"), map_location="cpu"))
    return flow_sd, depth_sd, pose_sd, feed_h, feed_w


def run_kitti_odom(cfg, flow_sd=None, depth_sd=None, pose_sd=None, seq=None, out_dir=None, gt_poses=None, world=1, rank=0,
                   dist=None, comm=None, feed_h=None, feed_w=None, slots=12, workers=6, ahead=3, carry_features=True, rng_mode=None,
                   compose="host", alignment=None, n_frames=None, jpeg="host", **overrides):
    """DFVO.main over one KITTI odometry sequence (apis/run.py) on the fused pipeline, frames read from disk as it tracks:
      1. TrackingPipeline.from_cfg(cfg, K of <img_seq_dir>/<seq>/calib.txt, weights, **overrides) -- a configuration that
         pipeline.options_from_cfg refuses is refused here with its message;
      2. a FrameStream over image_2/*.<image.ext> (read_image: resize to image.height x image.width) and, under depth.depth_src
         gt, a second one over the 16-bit depth images (their size is the first file's); jpeg ("host" or "device") is the
         image stream's: "device" decodes JPEG frames on the device, to the same frames (frame_stream.py);
      3. sequence.run_sequence (world / rank / dist / comm: its frame-parallel chunking);
      4. out_dir/<seq>.txt through evaluation.save_traj (rank 0);
      5. with gt_poses ([n,4,4] or the path of a KITTI pose file) evaluation.evaluate.
    cfg: a default_cfg.Cfg (cfg_from_yaml); seq defaults to cfg.seq.  Weights: state dicts, or None to load the files cfg names
    (load_weights).  Returns {"poses", "gathered", "metrics"}, one entry of sequence.run_sequences."""
    from . import evaluation as ev
    seq = str(cfg["seq"] if seq is None else seq)
    h, w = int(cfg["image"]["height"]), int(cfg["image"]["width"])
    external = cfg.get("depth", {}).get("depth_src") == "gt"
    d = cfg["directory"]
    files = kitti_odom_paths(d["img_seq_dir"], seq, cfg["image"].get("ext", "png"), d.get("depth_dir") if external else None)
    n = len(files["images"]) if n_frames is None else min(int(n_frames), len(files["images"]))
    if n < 2:
        raise ValueError("%s: %d frames; tracking needs two" % (os.path.dirname(files["calib"]), n))
    K = kitti_odom_intrinsics(files["calib"], h, w)
    if flow_sd is None:
        flow_sd, depth_sd, pose_sd, fh, fw = load_weights(cfg)
        feed_h, feed_w = feed_h or fh, feed_w or fw
    if external:
        from .frame_stream import probe
        overrides.setdefault("depth_scale", files["depth_scale"])
        overrides.setdefault("depth_size", probe(files["depths"][0])[:2])
    pipe = TrackingPipeline.from_cfg(cfg, K, flow_sd, depth_sd, feed_h or 192, feed_w or 640, pose_sd=pose_sd, **overrides)
    frames = depths = None
    try:
        frames = FrameStream(files["images"][:n], h, w, slots=slots, workers=workers, jpeg=jpeg)
        if external:
            depths = FrameStream(files["depths"][:n], pipe.depth_size[0], pipe.depth_size[1], slots=slots, workers=workers,
                                 kind="depth_u16")
        poses, gathered = sequence.run_sequence(pipe, frames, n, world, rank, dist, seed=int(cfg.get("seed", 4869)), rng_mode=rng_mode, ahead=ahead, compose=compose,
                                                carry_features=carry_features, comm=comm, depths=depths)
    finally:
        try:
            pipe.sync()  # the pipeline may still read the streams' frames
        finally:
            for s in (frames, depths):
                if s is not None:
                    s.close()
            pipe.close()
    metrics = None
    if gt_poses is not None:
        gt = ev.load_traj(gt_poses) if isinstance(gt_poses, (str, os.PathLike)) else np.asarray(gt_poses)
        metrics = ev.evaluate(gt[:len(poses)], poses, alignment=alignment)
    if out_dir is not None and rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        ev.save_traj(os.path.join(out_dir, "%s.txt" % seq), poses)
    return {"poses": poses, "gathered": gathered, "metrics": metrics}
