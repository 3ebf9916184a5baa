"""Rate of scale_recovery.method "iterative" through the drop-in class: EssTracker.scale_recovery at 376 x 1241 on the rigid
ramp scenes of tools/bench_stages.py (four of them in turn, prev_scale carried from call to call as the tracker does).
    python tools/bench_iterative_scale.py [--pairs 40] [--warmup 5] [--host-loop] [--prev-scale S]
Prints one JSON line: wall time per call (mean, median), the rounds the loop took, and -- where the loop runs as one device call --
the device time of the enqueued rounds from HIP events (per call and per executed round).  --host-loop times the loop of
host calls instead (EssTracker.iterative_on_device = False); a tree without the device loop is timed as it is.
--prev-scale S sets prev_scale to S before every call: the loop then starts away from the answer and takes several rounds (the
first pair of a sequence, or a pair after a rejected one), where the carried scale of the default run mostly takes one."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-loop", action="store_true")
    ap.add_argument("--prev-scale", type=float, default=None)
    a = ap.parse_args()
    capi = importlib.import_module("df-vo_amd.capi")
    syn = importlib.import_module("df-vo_amd.synthetic")
    cfg_mod = importlib.import_module("df-vo_amd.default_cfg")
    cam_mod = importlib.import_module("df-vo_amd.libs.geometry.camera_modules")
    E_mod = importlib.import_module("df-vo_amd.libs.tracker.E_tracker")
    capi.require_gpu()
    H, W = 376, 1241
    scenes = [syn.rigid_scene(H, W, seed=100 + i) for i in range(4)]
    cfg = cfg_mod.default_configuration(H, W, None, None)
    cfg.kp_selection.rigid_flow_kp.enable = True
    cfg.scale_recovery.method = "iterative"
    cfg.scale_recovery.kp_src = "kp_depth"
    K = scenes[0]["K"]
    et = E_mod.EssTracker(cfg, cam_mod.Intrinsics([K[0, 2], K[1, 2], K[0, 0], K[1, 1]]), None)
    on_device = hasattr(et, "iterative_on_device") and not a.host_loop
    if hasattr(et, "iterative_on_device"):
        et.iterative_on_device = on_device
    rounds_now = [0]
    find = et.find_scale_from_depth

    def counted(*args):
        rounds_now[0] += 1
        return find(*args)
    et.find_scale_from_depth = counted  # (the host loop's rounds; the device loop reports its own)
    data = []
    for s in scenes:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = s["R"], s["t"]
        E = np.linalg.inv(T)
        E[:3, 3] /= np.linalg.norm(E[:3, 3])
        data.append((dict(flow=s["flow"], flow_diff=s["diff"][..., None], raw_depth=s["depth_ref"].astype(np.float32)),
                     dict(depth=s["depth_cur"]), E))
    np.random.seed(4869)
    wall, rounds, dev_ms, scales = [], [], [], []
    for k in range(a.warmup + a.pairs):
        ref, cur, E = data[k % 4]
        ref, cur = dict(ref), dict(cur)
        rounds_now[0] = 0
        if a.prev_scale is not None:
            et.prev_scale = a.prev_scale
        t0 = time.perf_counter()
        out = et.scale_recovery(cur, ref, cam_mod.SE3(E.copy()), False)
        dt = time.perf_counter() - t0
        if k < a.warmup:
            continue
        wall.append(dt * 1e3)
        scales.append(float(out["scale"]))
        if on_device:
            rounds.append(int(et.last_iterative.n_iter))
            dev_ms.append(float(et.last_iterative.device_ms))
        else:
            rounds.append(rounds_now[0])
    res = dict(tool="bench_iterative_scale", loop="device" if on_device else "host", height=H, width=W, pairs=a.pairs,
               warmup=a.warmup, prev_scale="carried" if a.prev_scale is None else a.prev_scale, wall_ms_mean=float(np.mean(wall)), wall_ms_median=float(np.median(wall)),
               wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)), rounds_mean=float(np.mean(rounds)),
               rounds=sorted(set(rounds)), scale_mean=float(np.mean(scales)))
    if on_device:
        res["device_ms_mean"] = float(np.mean(dev_ms))
        res["device_ms_per_round"] = float(np.sum(dev_ms) / max(1, np.sum(rounds)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
