"""Rate of the fused pipeline under one tracking configuration (dfvo_pipeline_set_options), one JSON line.
Scene, overrides and the unloaded solver-stage loop are those of tools/bench_stages.py (four rigid ramp scenes at 376 x 1241
handed in as flow / consistency / depth overrides); the pair rate comes from the run-ahead loop of sequence.track_chunk (nets
and the RNG-independent half three pairs ahead, track_begin / track_end).

  python tools/bench_pipeline_options.py default|bestN|sampled|flow|PnP [--steps 40]"""
import argparse
import importlib
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "default": {},
    "bestN": {"kp_source": "bestN"},                                   # ablation_correspondences_best_n.yml
    "sampled": {"kp_source": "sampled"},                               # ablation_correspondences_uniform.yml
    "flow": {"validity": "flow", "validity_thre": 5},                  # ablation_model_sel_flow.yml
    "PnP": {"tracking_method": "PnP"},                                 # ablation_tracker_pnp.yml
}
SLOTS, AHEAD = 4, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    from PIL import Image
    syn = importlib.import_module("df-vo_amd.synthetic")
    pmod = importlib.import_module("df-vo_amd.pipeline")
    H, W, n = 376, 1241, args.steps
    scenes = [syn.rigid_scene(H, W, seed=100 + i) for i in range(4)]
    pipe = pmod.TrackingPipeline(H, W, 192, 640, scenes[0]["K"], syn.liteflownet_state_dict(4869),
                                 syn.monodepth2_state_dict(4869), seed=4869, **CONFIGS[args.config])
    ref, cur = syn.image_pair(H, W, seed=1)
    feed = np.asarray(Image.fromarray(cur).resize((640, 192), Image.LANCZOS))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_ref, d_cur, d_feed = dev(ref), dev(cur), dev(feed)
    d_sc = [(dev(s["flow"]), dev(s["diff"]), dev(s["depth_cur"])) for s in scenes]
    pipe.set_ref_depth(depth=dev(scenes[0]["depth_ref"]))
    for k in range(3):
        pipe.enqueue_nets(k % 2, d_ref, d_cur, d_feed)
        pipe.track(k % 2, *d_sc[k % 4])
    pipe.sync()
    torch.cuda.synchronize()

    def feed_pair(j):
        pipe.enqueue_nets(j % SLOTS, d_ref, d_cur, d_feed)
        pipe.prefetch_track(j % SLOTS, d_sc[j % 4][0], d_sc[j % 4][1])

    status = {}
    t0 = time.perf_counter()
    for j in range(min(AHEAD, n)):
        feed_pair(j)
    for j in range(n):
        pipe.track_begin(j % SLOTS, *d_sc[j % 4])
        if j + AHEAD < n:
            feed_pair(j + AHEAD)
        out = pipe.track_end(j % SLOTS)
        status[pmod.STATUS[out.status]] = status.get(pmod.STATUS[out.status], 0) + 1
    pipe.sync()
    t_pair = (time.perf_counter() - t0) / n
    t0 = time.perf_counter()
    for k in range(n):
        pipe.track(1 - (n % 2), *d_sc[k % 4])
    pipe.sync()
    t_track = (time.perf_counter() - t0) / n
    pipe.close()
    print(json.dumps({"config": args.config, "overrides": CONFIGS[args.config], "size": [H, W], "steps": n,
                      "pairs_per_s": round(1.0 / t_pair, 2), "ms_per_pair": round(t_pair * 1e3, 3),
                      "solver_stage_only_ms": round(t_track * 1e3, 3), "status": status}))


if __name__ == "__main__":
    main()
