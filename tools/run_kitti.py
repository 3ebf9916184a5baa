"""A KITTI odometry sequence from disk through the fused pipeline (df-vo_amd/kitti.py run_kitti_odom): the reference's
apis/run.py -d <default.yml> -c <overlay.yml> for dataset kitti_odom, frames decoded by worker threads while the device tracks.
    python tools/run_kitti.py -d options/examples/default_configuration.yml -c options/examples/kitti.yml --seq 09 --out result/
The configuration names the data (directory.img_seq_dir, directory.depth_dir, image.ext / height / width) and the weights
(deep_flow.flow_net_weight, depth.deep_depth.pretrained_model, deep_pose.pretrained_model).  Writes <out>/<seq>.txt and prints one
JSON line; --gt <poses.txt> adds the KITTI metrics.  --jpeg device: JPEG frames (image.ext: jpg) are decoded on the device."""
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
    ap.add_argument("--out", default=None, help="directory of <seq>.txt (default: the configuration's directory.result_dir)")
    ap.add_argument("--gt", default=None, help="KITTI pose file to evaluate against")
    ap.add_argument("--frames", type=int, default=None, help="track the first N frames only")
    ap.add_argument("--slots", type=int, default=12, help="ring slots per stream")
    ap.add_argument("--workers", type=int, default=6, help="decoder threads (at most 16)")
    ap.add_argument("--jpeg", default="host", choices=("host", "device"),
                    help="device: JPEG frames are entropy-decoded by the workers and decoded on the device (the same frames)")
    a = ap.parse_args(argv)
    kitti = importlib.import_module("df-vo_amd.kitti")
    cfg = kitti.cfg_from_yaml(a.default_configuration, a.configuration)
    if cfg.get("dataset", "kitti_odom") != "kitti_odom":
        raise SystemExit("dataset: %s: this runner reads kitti_odom folders" % cfg["dataset"])
    out = a.out if a.out is not None else cfg.get("directory", {}).get("result_dir")
    t0 = time.perf_counter()
    r = kitti.run_kitti_odom(cfg, seq=a.seq, out_dir=out, gt_poses=a.gt, n_frames=a.frames, slots=a.slots, workers=a.workers, jpeg=a.jpeg)
    dt = time.perf_counter() - t0
    n = len(r["poses"])
    print(json.dumps(dict(tool="run_kitti", seq=str(cfg["seq"] if a.seq is None else a.seq), frames=n, seconds_with_setup=dt,
                          trajectory=None if out is None else os.path.join(out, "%s.txt" % (cfg["seq"] if a.seq is None else a.seq)),
                          metrics=r["metrics"]), default=float))


if __name__ == "__main__":
    main()
