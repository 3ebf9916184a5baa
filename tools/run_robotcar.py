"""An Oxford RobotCar sequence from disk through the fused pipeline (df-vo_amd/robotcar.py run_robotcar): the reference's
apis/run.py -d <default.yml> -c <overlay.yml> for dataset robotcar, on the dataset's own raw frames.
    python tools/run_robotcar.py -d default_configuration.yml -c oxford_robotcar.yml --seq 2014-05-06-12-54-54 --out result/
--source raw (default): <img_seq_dir>/<seq>/stereo/centre/<timestamp>.png Bayer mosaics, demosaiced and undistorted on the device
through <img_seq_dir>/robotcar-dataset-sdk/models/stereo_narrow_left_distortion_lut.bin; --source undistorted: the files the SDK's
offline tool wrote to <seq>/undistorted_stereo/centre (JPEG: decoder parity with the reference's frames is not established).
Writes <out>/<seq>.txt and prints one JSON line; --gt <poses.txt> (KITTI format) adds the KITTI metrics."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-d", "--default_configuration", required=True, help="default configuration yml")
    ap.add_argument("-c", "--configuration", default=None, help="overlay yml")
    ap.add_argument("--seq", default=None, help="sequence (default: the configuration's seq)")
    ap.add_argument("--source", default="raw", choices=("raw", "undistorted"), help="which files are read")
    ap.add_argument("--border", default="reflect", choices=("reflect", "mirror"), help="the demosaic's border rule")
    ap.add_argument("--out", default=None, help="directory of <seq>.txt (default: the configuration's directory.result_dir)")
    ap.add_argument("--gt", default=None, help="KITTI-format pose file to evaluate against")
    ap.add_argument("--frames", type=int, default=None, help="track the first N frames only")
    ap.add_argument("--slots", type=int, default=12, help="ring slots")
    ap.add_argument("--workers", type=int, default=6, help="decoder threads (at most 16)")
    ap.add_argument("--jpeg", default="host", choices=("host", "device"),
                    help="--source undistorted: device decodes JPEG frames on the device (the same frames)")
    a = ap.parse_args(argv)
    robotcar = importlib.import_module("df-vo_amd.robotcar")
    cfg = robotcar.cfg_from_yaml(a.default_configuration, a.configuration)
    if cfg.get("dataset", "robotcar") != "robotcar":
        raise SystemExit("dataset: %s: this runner reads robotcar folders" % cfg["dataset"])
    out = a.out if a.out is not None else cfg.get("directory", {}).get("result_dir")
    seq = str(cfg["seq"] if a.seq is None else a.seq)
    t0 = time.perf_counter()
    r = robotcar.run_robotcar(cfg, seq=seq, source=a.source, border=a.border, out_dir=out, gt_poses=a.gt, n_frames=a.frames,
                              slots=a.slots, workers=a.workers, jpeg=a.jpeg)
    dt = time.perf_counter() - t0
    print(json.dumps(dict(tool="run_robotcar", seq=seq, source=a.source, frames=len(r["poses"]), seconds_with_setup=dt,
                          trajectory=None if out is None else os.path.join(out, "%s.txt" % seq), metrics=r["metrics"]), default=float))


if __name__ == "__main__":
    main()
