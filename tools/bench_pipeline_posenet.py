"""Pair rate of the fused pipeline with the pose lane beside the default, in one process:
    python tools/bench_pipeline_posenet.py [--pairs 20] [--warmup 5] [--runs 3] [--thre 1.0] [--configs default,mask,deep_pose]
                                           [--out profiles/pipeline_posenet_rates.json]
Three pipelines on bench.py's workload (the coded tunnel world at 376 x 1241, two frames in turn, images in -> pose out through
sequence.track_chunk), run in turn --runs times each, every run --pairs timed pairs after --warmup untimed ones:
    default    default_configuration.yml
    mask       pose_net + depth_consistency: the pose net and the depth-difference map on the depth stream, local_bestN masked.
               --thre is kp_selection.depth_consistency.thre; the default 1.0 passes every pixel whose map value is below the
               clamp, so the keypoint stage selects what the default selects and the difference in rate is the lane's cost
    deep_pose  tracking_method deep_pose: the pose lane alone
The pose net's last layer is the constant drive of the world (one metre forward), as in the tests.  One JSON line per run on
stdout; with --out the runs and their per-configuration minimum / median / maximum are merged into that file under "rates"."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 376, 1241
CONFIGS = ("default", "mask", "deep_pose")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--thre", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default=",".join(CONFIGS), help="comma list out of default, mask, deep_pose (one alone: a run for DFVO_TRACK_TRACE)")
    a = ap.parse_args()
    configs = tuple(c for c in CONFIGS if c in a.configs.split(","))
    os.environ.setdefault("DFVO_CONV_PRECISION", "f16x3")  # bench.py's headline arithmetic, read when the layers are packed
    capi = importlib.import_module("df-vo_amd.capi")
    syn = importlib.import_module("df-vo_amd.synthetic")
    pmod = importlib.import_module("df-vo_amd.pipeline")
    smod = importlib.import_module("df-vo_amd.sequence")
    import torch
    capi.require_gpu()
    code_mode = "mux" if syn._net_size(H, W) == (H, W) else "pot"
    seq = syn.coded_tunnel_sequence(H, W, 2, mode=code_mode, step=1.0, seed=7,
                                    poses=None if code_mode == "mux" else syn.tunnel_poses_lateral(2, 0.4))
    K = seq["K"]
    fsd, dsd = syn.crafted_liteflownet_state_dict(H, W, code_mode), syn.crafted_monodepth2_state_dict()
    psd = syn.posenet_state_dict(4869)
    psd["net.3.weight"] = torch.zeros_like(psd["net.3.weight"])
    psd["net.3.bias"] = torch.zeros(12)
    psd["net.3.bias"][5] = 100.0 * (-1.0 / 5.4)
    d_frames = smod.frames_to_device([seq["frames"][0], seq["frames"][1]])

    class PingPong:  # the sequence A, B, A, B, ... as an indexable of device frames
        def __getitem__(self, i):
            return d_frames[i % 2]

    kw = {"default": {}, "mask": dict(pose_sd=psd, pose_net=True, depth_consistency=True, depth_consistency_thre=a.thre),
          "deep_pose": dict(pose_sd=psd, pose_net=True, tracking_method="deep_pose")}
    pipes = {c: pmod.TrackingPipeline(H, W, 192, 640, K, fsd, dsd, seed=4869, **kw[c]) for c in configs}
    runs = []
    try:
        for c in configs:
            smod.track_chunk(pipes[c], PingPong(), 0, a.warmup)
        for r in range(a.runs):
            for c in configs:
                pipe = pipes[c]
                smod.track_chunk(pipe, PingPong(), 0, a.warmup)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rel, status = smod.track_chunk(pipe, PingPong(), 0, a.pairs)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                res = dict(tool="bench_pipeline_posenet", config=c, run=r, height=H, width=W, pairs=a.pairs, warmup=a.warmup,
                           conv_precision=os.environ["DFVO_CONV_PRECISION"], frames_per_s=round(a.pairs / dt, 3),
                           ms_per_pair=round(dt / a.pairs * 1e3, 3), status_counts={str(int(s)): int((status == s).sum()) for s in set(status)},
                           net_gflop_per_pair=round(pipe.net_flops() / 1e9, 3))
                if c == "mask":
                    res["depth_consistency_thre"] = a.thre
                runs.append(res)
                print(json.dumps(res), flush=True)
    finally:
        for pipe in pipes.values():
            pipe.close()
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        rates = {c: [r["frames_per_s"] for r in runs if r["config"] == c] for c in configs}
        doc["rates"] = dict(runs=runs, summary={c: dict(min=min(v), median=float(np.median(v)), max=max(v)) for c, v in rates.items()})
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
