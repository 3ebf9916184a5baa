"""Pair rate of the fused pipeline under depth.depth_src gt (depth_source "external": 16-bit depth images in the place of the depth
net) beside the default, and the device time of dfvo_read_depth_u16.
    python tools/bench_depth_source.py --leg external | net [--pairs 20] [--warmup 5]
    python tools/bench_depth_source.py --kernel [--reps 200]
--leg: images in -> pose out on bench.py's workload (the coded tunnel world at 376 x 1241, two frames in turn, --pairs timed pairs
after --warmup untimed ones, through sequence.track_chunk); one JSON line with frames/s.
    external  depth_source "external", no depth weights; the depth images are the world's own depth of the two frames, quantised at
              scale 500 (kitti.py's scale_factor), uploaded once
    net       the default configuration (the depth net runs), for comparison in the same session
--kernel: HIP-event time of one dfvo_read_depth_u16 launch to 376 x 1241 from a 376 x 1241 and from a 480 x 640 source, as the
mean over --reps back-to-back launches (what a launch costs a busy stream) and as the smallest single launch between two events
(which includes the launch latency), with the bytes the kernel moves (2 B read per output pixel's source sample at most -- the
source image counted once -- and 12 B written per output pixel) and the bandwidth that makes of them.
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
SCALE = 500
PEAK_TBPS = 8.0  # MI355X HBM3E peak


def quantise(depth):
    return np.clip(np.rint(depth * SCALE), 0, 65535).astype(np.uint16)


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
    K = seq["K"]
    fsd = syn.crafted_liteflownet_state_dict(H, W, code_mode)
    d_frames = smod.frames_to_device([seq["frames"][0], seq["frames"][1]])
    res = dict(tool="bench_depth_source", leg=a.leg, height=H, width=W, pairs=a.pairs, warmup=a.warmup,
               conv_precision=os.environ["DFVO_CONV_PRECISION"])
    kw = {}
    if a.leg == "external":
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        z = [syn.tunnel_flow(K, seq["poses"][i], seq["poses"][1 - i], yy, xx, **seq["world"])[2] for i in range(2)]  # depth of frame i
        d_depths = [smod.depth_to_device(quantise(np.clip(zi, 0, None))) for zi in z]
        pipe = pmod.TrackingPipeline(H, W, 192, 640, K, fsd, None, seed=4869, depth_source="external", depth_scale=SCALE)

        class PingPongDepth:
            def __getitem__(self, i):
                return d_depths[i % 2]
        kw["depths"] = PingPongDepth()
        res.update(depth_scale=SCALE, depth_h2d_bytes_per_frame=2 * H * W)
    else:
        pipe = pmod.TrackingPipeline(H, W, 192, 640, K, fsd, syn.crafted_monodepth2_state_dict(), seed=4869)

    class PingPong:  # the sequence A, B, A, B, ... as an indexable of device frames
        def __getitem__(self, i):
            return d_frames[i % 2]

    smod.track_chunk(pipe, PingPong(), 0, a.warmup, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rel, status = smod.track_chunk(pipe, PingPong(), 0, a.pairs, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res.update(frames_per_s=round(a.pairs / dt, 3), ms_per_pair=round(dt / a.pairs * 1e3, 3), tracked_by_E=int((status == 0).sum()),
               tracked_by_PnP=int((status == 3).sum()), net_gflop_per_pair=round(pipe.net_flops() / 1e9, 3),
               translation_norm_mean=float(np.mean([np.linalg.norm(r[:3, 3]) for r in rel])))
    pipe.close()
    print(json.dumps(res))


def kernel(a):
    capi = importlib.import_module("df-vo_amd.capi")
    import torch
    capi.require_gpu()
    lib = capi.lib()
    stream = torch.cuda.current_stream()
    raw = torch.empty((H, W), dtype=torch.float32, device="cuda")
    proc = torch.empty((H, W), dtype=torch.float64, device="cuda")
    y0 = int(H * 0.3)
    out = []
    for h, w in ((H, W), (480, 640)):
        g = np.random.Generator(np.random.PCG64(3))
        src = torch.from_numpy(g.integers(0, 65536, (h, w), dtype=np.uint16)).cuda()

        def launch():
            capi.check(lib.dfvo_read_depth_u16(src.data_ptr(), h, w, float(SCALE), H, W, y0, H, 0, W, 0.0, 50.0, raw.data_ptr(),
                                               proc.data_ptr(), stream.cuda_stream))
        for _ in range(20):
            launch()
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            launch()
        e1.record(stream)
        e1.synchronize()
        back_to_back_us = e0.elapsed_time(e1) * 1e3 / a.reps
        single = []
        for _ in range(50):
            stream.synchronize()
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            single.append(e0.elapsed_time(e1) * 1e3)
        # the source samples the resize reads: every source pixel at most once from memory (the rest are cache hits)
        read = 2 * min(h * w, H * W)
        moved = read + 12 * H * W
        out.append(dict(src_h=h, src_w=w, bytes_read=read, bytes_written=12 * H * W, bytes_moved=moved,
                        back_to_back_us=round(back_to_back_us, 3), single_launch_us_min=round(min(single), 3),
                        single_launch_us_median=round(float(np.median(single)), 3),
                        back_to_back_tbps=round(moved / back_to_back_us / 1e6, 4),
                        share_of_hbm_peak=round(moved / back_to_back_us / 1e6 / PEAK_TBPS, 4),
                        least_time_at_peak_us=round(moved / (PEAK_TBPS * 1e6), 3)))
    print(json.dumps(dict(tool="bench_depth_source", kernel="k_read_depth_u16", height=H, width=W, reps=a.reps, hbm_peak_tbps=PEAK_TBPS,
                          cases=out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, choices=["external", "net"])
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if a.kernel:
        return kernel(a)
    if not a.leg:
        ap.error("--leg external | net, or --kernel")
    return leg(a)


if __name__ == "__main__":
    main()
