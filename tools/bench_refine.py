"""Pair rate of the fused pipeline with the trackers' iterative keypoint refinement (dfvo_pipeline_set_refine) beside the default.
    python tools/bench_refine.py --leg default | e | e_scale [--pairs 20] [--warmup 5]
--leg: images in -> pose out on bench.py's workload (the coded tunnel world at 376 x 1241, two frames in turn, --pairs timed pairs
after --warmup untimed ones, through sequence.track_chunk); one JSON line with frames/s.
    default   the default configuration, for comparison in the same session
    e         e_tracker.iterative_kp: a first E pass with 3 repeats, kp_depth under its pose, a second pass with 5
    e_scale   the same with scale_recovery.iterative_kp: find_scale_from_depth again on kp_depth
The refined legs also count the pairs whose second pass ran and the mean kp_depth count, on a further, untimed walk
(get_refine waits for the device).
One leg per process: a pipeline takes its own streams."""
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
LEGS = {"default": {}, "e": dict(e_iterative_kp=True), "e_scale": dict(e_iterative_kp=True, scale_iterative_kp=True)}


def leg(a):
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
    fsd = syn.crafted_liteflownet_state_dict(H, W, code_mode)
    d_frames = smod.frames_to_device([seq["frames"][0], seq["frames"][1]])
    res = dict(tool="bench_refine", leg=a.leg, height=H, width=W, pairs=a.pairs, warmup=a.warmup,
               conv_precision=os.environ["DFVO_CONV_PRECISION"])
    pipe = pmod.TrackingPipeline(H, W, 192, 640, seq["K"], fsd, syn.crafted_monodepth2_state_dict(), seed=4869, **LEGS[a.leg])

    class PingPong:  # the sequence A, B, A, B, ... as an indexable of device frames
        def __getitem__(self, i):
            return d_frames[i % 2]

    smod.track_chunk(pipe, PingPong(), 0, a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rel, status = smod.track_chunk(pipe, PingPong(), 0, a.pairs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res.update(frames_per_s=round(a.pairs / dt, 3), ms_per_pair=round(dt / a.pairs * 1e3, 3), tracked_by_E=int((status == 0).sum()),
               tracked_by_PnP=int((status == 3).sum()), translation_norm_mean=float(np.mean([np.linalg.norm(r[:3, 3]) for r in rel])))
    if pipe.refine:  # what the refinement did, on a third, untimed walk (get_refine waits for the device)
        recs = []
        smod.track_chunk(pipe, PingPong(), 0, a.pairs, collect=lambda j, out: recs.append(pipe.get_refine(j % smod.SLOTS)))
        res.update(second_e_passes=int(sum(r["e_ran"] for r in recs)), second_scale_stages=int(sum(r["scale_ran"] for r in recs)),
                   kp_depth_mean=float(np.mean([len(r["ref_kp"]) for r in recs])))
    pipe.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=sorted(LEGS))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    leg(ap.parse_args())


if __name__ == "__main__":
    main()
