"""GPU: what the dense drawer panels cost (df-vo_amd/csrc/vis.hip, libs/general/frame_drawer.py).  One JSON line.

At 376 x 1241 into the 600 x 1000 window (the reference's defaults), on the coded tunnel world bench.py uses:
  device_ms            HIP-event time of the panels of one frame: the one session launch (forward flow, backward flow,
                       consistency map: two reductions + the panel kernel) and each uploaded panel by itself
  panels_ms_per_frame  wall time of the four DensePanels calls of FrameDrawer.main, resident path and upload path
  host_ms_per_frame    the host arithmetic they replace on the same arrays: the numpy restatement of flow_to_image
                       (tests/drawer_np.py) twice, matplotlib's magma of the disparity with np.percentile, jet of the
                       consistency map, and the 8-bit resize of each into its cell
  loop_frames_per_s    the class-surface frame loop of bench.py --surface mirrors with panels off and on

    python tools/vis_bench.py [--steps 30 --warmup 5]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class NS(dict):
    __getattr__ = dict.__getitem__


def host_panels(D, fwd, bwd, diff, depth, vmax_jet):
    """the reference's four dense panels on the host: restated wheel, live matplotlib, the 8-bit resize"""
    import matplotlib as mpl
    import matplotlib.cm  # noqa: F401
    out = [D.cell_from_rgb(D.flow_to_image_np(fwd)[0], 150, 250), D.cell_from_rgb(D.flow_to_image_np(bwd)[0], 150, 250)]
    disp = 1 / (depth + 1e-3)
    disp[depth == 0] = 0
    m = mpl.cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=0, vmax=np.percentile(disp, 90)), cmap="magma")
    out.append(D.cell_from_rgb((m.to_rgba(disp)[:, :, :3] * 255).astype(np.uint8), 150, 250))
    m = mpl.cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=0, vmax=vmax_jet), cmap="jet")
    out.append(D.cell_from_rgb((m.to_rgba(diff)[:, :, :3] * 255).astype(np.uint8), 150, 250))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=376)
    ap.add_argument("--width", type=int, default=1241)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    torch.zeros(8, device="cuda").sum().item()
    import __graft_entry__ as g
    g.dfvo_amd()
    import drawer_np as D
    capi = importlib.import_module("df-vo_amd.capi")
    syn = importlib.import_module("df-vo_amd.synthetic")
    cfg_mod = importlib.import_module("df-vo_amd.default_cfg")
    dm_mod = importlib.import_module("df-vo_amd.libs.deep_models.deep_models")
    cam_mod = importlib.import_module("df-vo_amd.libs.geometry.camera_modules")
    ks_mod = importlib.import_module("df-vo_amd.libs.matching.keypoint_sampler")
    trk_mod = importlib.import_module("df-vo_amd.libs.tracker")
    fd = importlib.import_module("df-vo_amd.libs.general.frame_drawer")
    capi.require_gpu()
    H, W = args.height, args.width
    mode = "mux" if syn._net_size(H, W) == (H, W) else "pot"
    seq = syn.coded_tunnel_sequence(H, W, 2, mode=mode, step=1.0, seed=7, poses=None if mode == "mux" else syn.tunnel_poses_lateral(2, 0.4))
    K, frames = seq["K"], [seq["frames"][0], seq["frames"][1]]
    flow_path, depth_dir = syn.write_weight_files(tempfile.mkdtemp(prefix="dfvo_vis_bench_"), syn.crafted_liteflownet_state_dict(H, W, mode),
                                                  syn.crafted_monodepth2_state_dict())
    cfg = cfg_mod.default_configuration(H, W, flow_path, depth_dir)
    cfg["visualization"] = NS(depth=NS(use_tracking_depth=False, depth_disp="disp"),
                              flow=NS(vis_forward_flow=True, vis_backward_flow=True, vis_flow_diff=True, vis_rigid_diff=True))
    deep_models = dm_mod.DeepModel(cfg)
    deep_models.initialize_models()
    cam = cam_mod.Intrinsics([K[0, 2], K[1, 2], K[0, 0], K[1, 1]])
    sampler = ks_mod.KeypointSampler(cfg)
    e_tracker, pnp_tracker = trk_mod.EssTracker(cfg, cam, None), trk_mod.PnpTracker(cfg, cam)
    fh, fw = deep_models.depth.feed_height, deep_models.depth.feed_width
    ys = np.minimum(np.floor(np.arange(H) * (fh / float(H))).astype(np.int64), fh - 1)
    xs = np.minimum(np.floor(np.arange(W) * (fw / float(W))).astype(np.int64), fw - 1)
    y0, y1 = int(H * cfg.crop.depth_crop[0][0]), int(H * cfg.crop.depth_crop[0][1])
    x0, x1 = int(W * cfg.crop.depth_crop[1][0]), int(W * cfg.crop.depth_crop[1][1])
    crop_mask = np.zeros((H, W))
    crop_mask[y0:y1, x0:x1] = 1
    drawer = fd.DensePanels(NS(window_h=600, window_w=1000))
    upload_drawer = fd.DensePanels(NS(window_h=600, window_w=1000))

    def loop(panels, n_warm, n_steps, probe=None):
        """bench.py's run_mirrors loop (dfvo.py:347-425); panels: the drawer's dense calls where dfvo.py:389-393 has them"""
        np.random.seed(cfg.seed)
        ref_data, cur_data = {}, {}
        t_begin, t_panels = None, 0.0
        for img_id in range(n_warm + n_steps + 1):
            if img_id == n_warm + 1:
                t_begin, t_panels = time.perf_counter(), 0.0
            cur_data["id"], cur_data["timestamp"], cur_data["img"] = img_id, img_id, frames[img_id % 2]
            raw = deep_models.forward_depth(imgs=[cur_data["img"]])
            cur_data["raw_depth"] = raw[ys][:, xs]
            d = cur_data["raw_depth"]
            cur_data["depth"] = d * (crop_mask * ((d < cfg.depth.max_depth) * (d > cfg.depth.min_depth)))
            if img_id >= 1:
                flows = deep_models.forward_flow(cur_data, ref_data, forward_backward=True)
                ref_data["flow"] = flows[(ref_data["id"], cur_data["id"])].copy()
                cur_data["flow"] = flows[(cur_data["id"], ref_data["id"])].copy()
                ref_data["flow_diff"] = flows[(ref_data["id"], cur_data["id"], "diff")].copy()
                kp_sel = sampler.kp_selection(cur_data, ref_data)
                if kp_sel["good_kp_found"]:
                    sampler.update_kp_data(cur_data, ref_data, kp_sel)
                    E_pose = e_tracker.compute_pose_2d2d(ref_data["kp_best"], cur_data["kp_best"], True)["pose"]
                    scale = -1
                    if np.linalg.norm(E_pose.t) != 0:
                        scale = e_tracker.scale_recovery(cur_data, ref_data, E_pose, False)["scale"]
                    if np.linalg.norm(E_pose.t) == 0 or scale == -1:
                        pnp_tracker.compute_pose_3d2d(ref_data["kp_best"], cur_data["kp_best"], ref_data["depth"], True)
            if panels:
                tp = time.perf_counter()
                drawer.main(NS(cfg=cfg, cur_data=cur_data, ref_data=ref_data, tracking_stage=min(img_id, 1)))
                t_panels += time.perf_counter() - tp
            last = (dict(ref_data), dict(cur_data))
            ref_data = dict(cur_data)
            ref_data["flow"] = cur_data["flow"] = ref_data["flow_diff"] = None
        capi.check(capi.lib().dfvo_sync_device())
        dt = time.perf_counter() - t_begin
        if probe is not None:
            probe(*last)  # (the session still holds the last pair: its arrays take the resident path)
        return n_steps / dt, t_panels / n_steps * 1e3

    result = {"tool": "vis_bench", "map": [H, W], "window": [600, 1000], "steps": args.steps, "warmup": args.warmup,
              "conv_precision": deep_models.conv_precision}
    fps_off, _ = loop(False, args.warmup, args.steps)
    probe_out = {}

    def probe(ref_data, cur_data):
        """on the last frame's arrays: device times, upload-path wall time, host arithmetic"""
        vo = NS(cfg=cfg, cur_data=cur_data, ref_data=ref_data, tracking_stage=1)
        dev = {"session_launch": [], "upload_flow": [], "upload_disparity": [], "upload_jet": []}
        plain = {"fwd": np.array(np.asarray(ref_data["flow"])), "bwd": np.array(np.asarray(cur_data["flow"])),
                 "diff": np.array(np.asarray(cur_data["fb_flow_mask"])), "depth": np.array(cur_data["raw_depth"])}
        for _ in range(10):
            drawer.forget_resident()  # (the next call launches the session's panels again)
            drawer.draw_flow(ref_data["flow"], "flow1")
            dev["session_launch"].append(drawer.vis_device_ms())
            upload_drawer.draw_flow(plain["fwd"], "flow1")
            dev["upload_flow"].append(upload_drawer.vis_device_ms())
            upload_drawer.draw_depth(NS(cfg=cfg, cur_data={"raw_depth": plain["depth"]}))
            dev["upload_disparity"].append(upload_drawer.vis_device_ms())
            upload_drawer.draw_flow_consistency(NS(cfg=cfg, cur_data={"fb_flow_mask": plain["diff"]}))
            dev["upload_jet"].append(upload_drawer.vis_device_ms())
        probe_out["device_ms"] = {k: round(statistics.median(v), 4) for k, v in dev.items()}
        up_vo = NS(cfg=cfg, cur_data={"raw_depth": plain["depth"], "flow": plain["bwd"], "fb_flow_mask": plain["diff"]},
                   ref_data={"flow": plain["fwd"]}, tracking_stage=1)
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            upload_drawer.main(up_vo)
            ts.append((time.perf_counter() - t0) * 1e3)
        probe_out["upload_ms"] = round(statistics.median(ts), 3)
        ts = []
        for _ in range(10):
            drawer.forget_resident()
            t0 = time.perf_counter()
            drawer.main(vo)
            ts.append((time.perf_counter() - t0) * 1e3)
        probe_out["resident_ms"] = round(statistics.median(ts), 3)
        vmax_jet = 0.1 if cfg.kp_selection.local_bestN.score_method == "flow_ratio" else 1
        ts = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            cells = host_panels(D, plain["fwd"].copy(), plain["bwd"].copy(), plain["diff"], plain["depth"], vmax_jet)
            ts.append((time.perf_counter() - t0) * 1e3)
        probe_out["host_ms"] = round(min(ts), 3)
        upload_drawer.main(up_vo)
        names = ("flow1", "flow2", "depth", "opt_flow_diff")
        probe_out["differing_pixels_vs_host"] = {n: int((upload_drawer.data[n] != c).any(-1).sum()) for n, c in zip(names, cells)}
        drawer.forget_resident()
        drawer.main(vo)
        probe_out["differing_pixels_vs_host_resident"] = {n: int((drawer.data[n] != c).any(-1).sum()) for n, c in zip(names, cells)}

    fps_on, panels_ms = loop(True, args.warmup, args.steps, probe)
    result["loop_frames_per_s"] = {"panels_off": round(fps_off, 2), "panels_on": round(fps_on, 2)}
    result["loop_ms_per_frame"] = {"panels_off": round(1e3 / fps_off, 3), "panels_on": round(1e3 / fps_on, 3)}
    result["device_ms"] = probe_out["device_ms"]
    result["panels_ms_per_frame"] = {"in_loop": round(panels_ms, 3), "resident": probe_out["resident_ms"], "upload": probe_out["upload_ms"]}
    result["host_ms_per_frame"] = probe_out["host_ms"]
    result["differing_pixels_vs_host"] = {"upload": probe_out["differing_pixels_vs_host"], "resident": probe_out["differing_pixels_vs_host_resident"]}
    result["drawer_stats"] = drawer.stats
    result["session"] = dict(deep_models.session.stats) if getattr(deep_models, "session", None) is not None else None
    drawer.close()
    upload_drawer.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
