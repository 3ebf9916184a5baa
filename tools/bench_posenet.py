"""What the pose net and the depth-consistency map cost at the KITTI image size (profiles/posenet_rates.json):
    python tools/bench_posenet.py --precision f16x3 | fp32 [--calls 50] [--warmup 10]
One JSON line:
  forward_pose_ms      wall time of one blocking dfvo_posenet_forward_images_host call -- what DeepModel.forward_pose costs the
                       frame loop: two 376 x 1241 frames uploaded, resized to 192 x 640 (LANCZOS), the net (replayed graph), 64
                       bytes back -- as the mean and the median over --calls calls after --warmup untimed ones
  net_device_ms        HIP-event time of dfvo_posenet_forward alone on device-resident feed frames (mean over --calls replays)
  depth_consistency_us HIP-event time of one dfvo_depth_consistency launch at 376 x 1241: mean over 200 back-to-back launches,
                       with the bytes it moves (4 B read of the current depth and 4 B written per pixel; the four-point gather of
                       the reference depth reads every reference pixel about once from memory: 4 B more) and the bandwidth that is
The conv precision is process-wide while the net is packed: one precision per process."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, FEED_H, FEED_W = 376, 1241, 192, 640
PEAK_TBPS = 8.0  # MI355X HBM3E peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "fp32", "f16"])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    capi = importlib.import_module("df-vo_amd.capi")
    syn = importlib.import_module("df-vo_amd.synthetic")
    import torch
    capi.require_gpu()
    lib = capi.lib()
    capi.check(lib.dfvo_set_conv_precision(a.precision.encode()))
    net = C.c_void_p()
    capi.check(lib.dfvo_posenet_create(FEED_H, FEED_W, 5.4, None, C.byref(net)))
    capi.set_params(lib.dfvo_posenet_set_param, net, {k: v.numpy() for k, v in syn.posenet_state_dict(4869).items()})
    capi.check(lib.dfvo_posenet_finalize(net))
    img0, img1 = syn.image_pair(H, W, seed=1001)
    pose = np.zeros((4, 4), np.float32)

    def forward_pose():
        capi.check(lib.dfvo_posenet_forward_images_host(net, capi.as_ptr(img0), capi.as_ptr(img1), H, W, capi.as_ptr(pose)))
    for _ in range(a.warmup):
        forward_pose()
    wall = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        forward_pose()
        wall.append((time.perf_counter() - t0) * 1e3)
    # the net alone, on device-resident feed frames, timed on its own stream
    f0, f1 = (torch.from_numpy(np.ascontiguousarray(i[:FEED_H, :FEED_W])).cuda() for i in (img0, img1))
    out = torch.zeros(24, device="cuda")
    s = torch.cuda.Stream()
    net2 = C.c_void_p()
    capi.check(lib.dfvo_posenet_create(FEED_H, FEED_W, 5.4, C.c_void_p(s.cuda_stream), C.byref(net2)))
    capi.set_params(lib.dfvo_posenet_set_param, net2, {k: v.numpy() for k, v in syn.posenet_state_dict(4869).items()})
    capi.check(lib.dfvo_posenet_finalize(net2))
    torch.cuda.synchronize()

    def forward_net():
        capi.check(lib.dfvo_posenet_forward(net2, C.c_void_p(f0.data_ptr()), C.c_void_p(f1.data_ptr()), C.c_void_p(out.data_ptr()),
                                            C.c_void_p(out.data_ptr() + 64)))
    for _ in range(a.warmup):
        forward_net()
    s.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(a.calls):
        forward_net()
    e1.record(s)
    e1.synchronize()
    net_ms = e0.elapsed_time(e1) / a.calls
    gflop = lib.dfvo_posenet_last_flops(net2) / 1e9
    # the depth-consistency launch
    g = np.random.Generator(np.random.PCG64(5))
    cur = torch.from_numpy((5 + 30 * g.random((H, W), dtype=np.float32))).cuda()
    ref = torch.from_numpy((5 + 30 * g.random((H, W), dtype=np.float32))).cuda()
    dd = torch.empty((H, W), dtype=torch.float32, device="cuda")
    K = syn.kitti_K(H, W)
    mats = [np.ascontiguousarray(m, dtype=np.float32) for m in (K, np.linalg.inv(K), np.eye(4))]
    mats[2][2, 3] = 1.0
    reps = 200

    def launch():
        capi.check(lib.dfvo_depth_consistency(C.c_void_p(cur.data_ptr()), C.c_void_p(ref.data_ptr()), H, W, capi.as_ptr(mats[0]),
                                              capi.as_ptr(mats[1]), capi.as_ptr(mats[2]), C.c_void_p(dd.data_ptr()), C.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize()
    for _ in range(20):
        launch()
    s.synchronize()
    e0.record(s)
    for _ in range(reps):
        launch()
    e1.record(s)
    e1.synchronize()
    dc_us = e0.elapsed_time(e1) * 1e3 / reps
    moved = 12 * H * W
    lib.dfvo_posenet_destroy(net)
    lib.dfvo_posenet_destroy(net2)
    print(json.dumps(dict(tool="bench_posenet", conv_precision=a.precision, height=H, width=W, feed_height=FEED_H, feed_width=FEED_W,
                          calls=a.calls, warmup=a.warmup, forward_pose_ms_mean=round(float(np.mean(wall)), 3),
                          forward_pose_ms_median=round(float(np.median(wall)), 3), forward_pose_ms_min=round(min(wall), 3),
                          net_device_ms=round(net_ms, 3), net_gflop=round(gflop, 3), net_tflops=round(gflop / net_ms, 2),
                          depth_consistency_us=round(dc_us, 3), depth_consistency_bytes_moved=moved,
                          depth_consistency_tbps=round(moved / dc_us / 1e6, 3),
                          depth_consistency_share_of_hbm_peak=round(moved / dc_us / 1e6 / PEAK_TBPS, 4), hbm_peak_tbps=PEAK_TBPS)))


if __name__ == "__main__":
    main()
