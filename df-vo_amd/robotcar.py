"""An Oxford RobotCar folder through the fused pipeline: the dataset layer of the reference (libs/datasets/oxford_robotcar.py
OxfordRobotCar) as plain functions, and the runner that puts a FrameStream under sequence.run_sequence.
source "raw" (default): the dataset's own stereo/centre/<timestamp>.png Bayer mosaics, demosaiced and undistorted on the device
through the SDK's table (undistort.py) -- the reference's route is offline (SDK load_image -> undistorted_stereo/centre/*.jpg);
source "undistorted": those pre-made files through the plain stream, with frame_stream.py's JPEG caveat.
Ground truth is taken as a KITTI-format pose file only; the SDK's pose interpolation is not restated.  Host only."""
import os

import numpy as np

from . import sequence
from .frame_stream import FrameStream
from .kitti import cfg_from_yaml, load_weights  # noqa: F401  (the configuration and the weights are read the same way)
from .pipeline import TrackingPipeline

RAW_H, RAW_W = 960, 1280           # oxford_robotcar.py:84-85
CROP = [[0.0, 0.8], [0.0, 1.0]]    # y_crop, x_crop (oxford_robotcar.py:102-103): the car's bonnet is cut off
PATTERN = "gbrg"                   # sdk_python/image.py BAYER_STEREO
CAMERA = "stereo_narrow_left"      # the model of stereo/centre frames (camera_model.py __load_intrinsics)
SOURCES = ("raw", "undistorted")


def robotcar_intrinsics(intrinsics_txt, h, w):
    """K [3,3] for frames cropped by CROP and resized to h x w: get_intrinsics_param (oxford_robotcar.py:77-114) with its own
    operations -- the first line of the model file is fx fy cx cy at 960 x 1280"""
    p = np.loadtxt(intrinsics_txt)[0]
    K = np.eye(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = p[0], p[1], p[2], p[3]
    crop_h = int(RAW_H * (CROP[0][1] - CROP[0][0]))
    crop_w = int(RAW_W * (CROP[1][1] - CROP[1][0]))
    K[0, 2] -= int(RAW_W * CROP[1][0])
    K[1, 2] -= int(RAW_H * CROP[0][0])
    K[0] *= (w / crop_w)
    K[1] *= (h / crop_h)
    return K


def robotcar_paths(img_seq_dir, seq, source="raw", ext="png"):
    """the files of sequence `seq`, in the order of stereo.timestamps column 0: raw <seq>/stereo/centre/<timestamp>.png, or
    undistorted <seq>/undistorted_stereo/centre/<timestamp, 16 digits>.<ext> (oxford_robotcar.py:128-148).
    Returns {"images", "timestamps", "intrinsics", "lut"}."""
    if source not in SOURCES:
        raise ValueError("source: %r: one of %s" % (source, ", ".join(SOURCES)))
    seq = str(seq)
    stamps = np.loadtxt(os.path.join(img_seq_dir, seq, "stereo.timestamps"), dtype=np.int64, usecols=(0,), ndmin=1)
    if source == "raw":
        d = os.path.join(img_seq_dir, seq, "stereo", "centre")
        images = [os.path.join(d, "%d.png" % t) for t in stamps]
    else:
        d = os.path.join(img_seq_dir, seq, "undistorted_stereo", "centre")
        images = [os.path.join(d, "{:016d}.{}".format(int(t), ext)) for t in stamps]
    models = os.path.join(img_seq_dir, "robotcar-dataset-sdk", "models")
    return dict(images=images, timestamps=stamps, intrinsics=os.path.join(models, CAMERA + ".txt"),
                lut=os.path.join(models, CAMERA + "_distortion_lut.bin"))


def run_robotcar(cfg, flow_sd=None, depth_sd=None, pose_sd=None, seq=None, source="raw", out_dir=None, gt_poses=None, feed_h=None,
                 feed_w=None, slots=12, workers=6, ahead=3, carry_features=True, compose="host", alignment=None, n_frames=None,
                 border="reflect", raw_size=(RAW_H, RAW_W), jpeg="host", **overrides):
    """DFVO.main over one RobotCar sequence on the fused pipeline, frames read from disk as it tracks (kitti.run_kitti_odom's
    shape): K of the model file, a FrameStream over the mosaics with the SDK's table (raw_size: the files' size, which the table
    is for) or over the pre-made undistorted files, sequence.run_sequence, out_dir/<seq>.txt, evaluation against gt_poses
    ([n,4,4] or a KITTI pose file).  jpeg ("host" or "device"; source "undistorted" only, a mosaic is no JPEG): the stream's, "device"
    decodes JPEG frames on the device to the same frames (frame_stream.py).  Returns {"poses", "gathered", "metrics"}."""
    from . import evaluation as ev
    from .undistort import UndistortMap
    seq = str(cfg["seq"] if seq is None else seq)
    h, w = int(cfg["image"]["height"]), int(cfg["image"]["width"])
    files = robotcar_paths(cfg["directory"]["img_seq_dir"], seq, source, cfg["image"].get("ext", "jpg"))
    n = len(files["images"]) if n_frames is None else min(int(n_frames), len(files["images"]))
    if n < 2:
        raise ValueError("%s: %d frames; tracking needs two" % (seq, n))
    K = robotcar_intrinsics(files["intrinsics"], h, w)
    if flow_sd is None:
        flow_sd, depth_sd, pose_sd, fh, fw = load_weights(cfg)
        feed_h, feed_w = feed_h or fh, feed_w or fw
    pipe = TrackingPipeline.from_cfg(cfg, K, flow_sd, depth_sd, feed_h or 192, feed_w or 640, pose_sd=pose_sd, **overrides)
    frames = umap = None
    try:
        if source == "raw" and jpeg != "host":
            raise ValueError("jpeg=%r: for source \"undistorted\" (the raw mosaics are PNG files)" % (jpeg,))
        if source == "raw":
            umap = UndistortMap.from_lut_file(files["lut"], raw_size[0], raw_size[1])
            frames = FrameStream(files["images"][:n], h, w, crop=CROP, slots=slots, workers=workers, mosaic=PATTERN, undistort=umap,
                                 border=border)
        else:
            frames = FrameStream(files["images"][:n], h, w, crop=CROP, slots=slots, workers=workers, jpeg=jpeg)
        poses, gathered = sequence.run_sequence(pipe, frames, n, seed=int(cfg.get("seed", 4869)), ahead=ahead, compose=compose,
                                                carry_features=carry_features)
    finally:
        try:
            pipe.sync()  # the pipeline may still read the stream's frames
        finally:
            if frames is not None:
                frames.close()  # (drains the ring: no kernel reads the table after it)
            if umap is not None:
                umap.close()
            pipe.close()
    metrics = None
    if gt_poses is not None:
        gt = ev.load_traj(gt_poses) if isinstance(gt_poses, (str, os.PathLike)) else np.asarray(gt_poses)
        metrics = ev.evaluate(gt[:len(poses)], poses, alignment=alignment)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        ev.save_traj(os.path.join(out_dir, "%s.txt" % seq), poses)
    return {"poses": poses, "gathered": gathered, "metrics": metrics}
