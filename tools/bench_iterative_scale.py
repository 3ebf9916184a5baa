"""Rate of scale_recovery.method "iterative" through the drop-in class: EssTracker.scale_recovery at 376 x 1241 on the rigid
ramp scenes of tools/bench_stages.py (four of them in turn, prev_scale carried from call to call as the tracker does).
    python tools/bench_iterative_scale.py [--pairs 40] [--warmup 5] [--host-loop] [--prev-scale S]
Prints one JSON line: wall time per call (mean, median), the rounds the loop took, and -- where the loop runs as one device call --
the device time of the enqueued rounds from HIP events (per call and per executed round).  --host-loop times the loop of
host calls instead (EssTracker.iterative_on_device = False); a tree without the device loop is timed as it is.
--prev-scale S sets prev_scale to S before every call: the loop then starts away from the answer and takes several rounds (the
first pair of a sequence, or a pair after a rejected one), where the carried scale of the default run mostly takes one.

--leg selects a whole-frame-loop measurement instead, images in -> pose out on bench.py's workload (the coded tunnel world at
376 x 1241, two frames in turn, --pairs timed pairs after --warmup untimed ones; one JSON line with frames/s):
    fused          the fused pipeline with scale_recovery "iterative" (dfvo_pipeline_set_iterative) through sequence.track_chunk
    fused-default  the same loop with the default configuration (scale_recovery "simple"), for orientation
    mirrors        the frame loop of DFVO.main over the drop-in classes (bench.py --surface mirrors, frame session on) with
                   scale_recovery.method iterative: the only way a tree without the fused method runs this configuration
--kp-src kp_best | kp_depth: scale_recovery.kp_src of the three legs (kp_best: ablation_scale_iterative.yml as shipped).
One leg per process: the pipeline and the frame session each take their own streams."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame_loop_leg(a):
    """--leg: frames/s of a whole frame loop on bench.py's workload"""
    import contextlib
    import io
    os.environ.setdefault("DFVO_CONV_PRECISION", "f16x3")  # bench.py's headline arithmetic, read when the layers are packed
    capi = importlib.import_module("df-vo_amd.capi")
    syn = importlib.import_module("df-vo_amd.synthetic")
    capi.require_gpu()
    H, W = 376, 1241
    code_mode = "mux" if syn._net_size(H, W) == (H, W) else "pot"
    seq = syn.coded_tunnel_sequence(H, W, 2, mode=code_mode, step=1.0, seed=7,
                                    poses=None if code_mode == "mux" else syn.tunnel_poses_lateral(2, 0.4))
    K = seq["K"]
    fsd, dsd = syn.crafted_liteflownet_state_dict(H, W, code_mode), syn.crafted_monodepth2_state_dict()
    res = dict(tool="bench_iterative_scale", leg=a.leg, height=H, width=W, pairs=a.pairs, warmup=a.warmup, kp_src=a.kp_src,
               conv_precision=os.environ["DFVO_CONV_PRECISION"])
    if a.leg == "mirrors":
        import bench
        cfg_mod = importlib.import_module("df-vo_amd.default_cfg")
        plain = cfg_mod.default_configuration

        def iterative_configuration(*args, **kw):  # default_configuration.yml with ablation_scale_iterative.yml's edits
            c = plain(*args, **kw)
            c.kp_selection.rigid_flow_kp.enable = True
            c.scale_recovery.method = "iterative"
            c.scale_recovery.kp_src = a.kp_src
            return c
        cfg_mod.default_configuration = iterative_configuration
        ns = argparse.Namespace(height=H, width=W, warmup=a.warmup, steps=a.pairs, conv_precision=os.environ["DFVO_CONV_PRECISION"])
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            bench.run_mirrors(ns, syn, capi, [seq["frames"][0], seq["frames"][1]], K, fsd, dsd, code_mode)
        line = json.loads(buf.getvalue().strip().splitlines()[-1])
        res.update(frames_per_s=line["value"], ms_per_pair=line["ms_per_step"], tracked_by_E=line["config"]["tracked_by_E"],
                   tracked_by_PnP=line["config"]["tracked_by_PnP"], scale_recovery_ms_per_pair=line["stage_ms_per_pair"]["scale_recovery"],
                   session=line["session"])
        print(json.dumps(res))
        return
    pmod = importlib.import_module("df-vo_amd.pipeline")
    smod = importlib.import_module("df-vo_amd.sequence")
    import torch
    keys = dict(scale_recovery="iterative", iter_kp_src=a.kp_src) if a.leg == "fused" else {}
    pipe = pmod.TrackingPipeline(H, W, 192, 640, K, fsd, dsd, seed=4869, **keys)
    d_frames = smod.frames_to_device([seq["frames"][0], seq["frames"][1]])

    class PingPong:  # the sequence A, B, A, B, ... as an indexable of device frames
        def __getitem__(self, i):
            return d_frames[i % 2]

    rounds = []

    def collect(j, out):
        rounds.append(pipe.get_iterative(j % smod.SLOTS)["n_iter"])
    smod.track_chunk(pipe, PingPong(), 0, a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rel, status = smod.track_chunk(pipe, PingPong(), 0, a.pairs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if a.leg == "fused":  # (outside the timed region: the same chunk again, for the rounds its loops took)
        smod.track_chunk(pipe, PingPong(), 0, a.pairs, collect=collect)
        res.update(rounds_mean=float(np.mean(rounds)), rounds=sorted(set(rounds)), prev_scale=pipe.get_prev_scale())
    res.update(frames_per_s=round(a.pairs / dt, 3), ms_per_pair=round(dt / a.pairs * 1e3, 3), tracked_by_E=int((status == 0).sum()),
               tracked_by_PnP=int((status == 3).sum()))
    pipe.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-loop", action="store_true")
    ap.add_argument("--prev-scale", type=float, default=None)
    ap.add_argument("--leg", default=None, choices=["fused", "fused-default", "mirrors"])
    ap.add_argument("--kp-src", default="kp_best", choices=["kp_best", "kp_depth"])
    a = ap.parse_args()
    if a.pairs is None:
        a.pairs = 20 if a.leg else 40
    if a.leg:
        return frame_loop_leg(a)
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
