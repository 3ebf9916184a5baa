"""GPU: the frame loop of DFVO.main with the pose net in it.  `main_loop` below re-types the branch of
/root/reference/libs/dfvo.py (deep_model_inference :299-345 with the forward_pose call :338-345, tracking :121-262 with the
depth-consistency call :142-143 and the deep-tracker branch :253-255, update_global_pose :109-119) over the mirror classes, as
tests/test_dropin_gpu.py does for the default branch.  Six frames of the coded tunnel world at 128 x 416, three ways:
  * tracking_method deep_pose: every pair's motion is forward_pose's matrix, the global pose their composition;
  * hybrid with kp_selection.depth_consistency.enable: the keypoints are the masked restatement's on the device's own flow /
    depth-difference arrays, the session counts every selection as plain and none as resident;
  * DFVO_SESSION=0 and 1 give identical results, the numpy RandomState included."""
import importlib
import os

import numpy as np
import pytest
import torch

import depth_consistency_ref as DC
import test_dropin_gpu as D
from oracle import tracker_np as T
from synth import coded_tunnel_sequence, crafted_liteflownet_state_dict, crafted_monodepth2_state_dict, write_weight_files

pytestmark = pytest.mark.gpu
H, W, N_FRAMES = 128, 416, 6
DEPTH_THRE = 0.01  # kp_selection.depth_consistency.thre of the hybrid run: the coded depths agree to a few per cent


def _pose_weights(constant_motion):
    """synthetic.posenet_state_dict; constant_motion: the last layer's weights are zero and its bias is the tunnel's drive (one
    metre forward per frame: M = R^T T(-t), so the raw translation is -(0, 0, 1) / 5.4) -- a pose the depth maps agree with"""
    sd = importlib.import_module("df-vo_amd.synthetic").posenet_state_dict(4869)
    if constant_motion:
        sd["net.3.weight"] = torch.zeros_like(sd["net.3.weight"])
        sd["net.3.bias"] = torch.zeros(12)
        sd["net.3.bias"][5] = 100.0 * (-1.0 / 5.4)
    return sd


def _world(tmp_path, constant_motion, tracking_method, depth_consistency):
    seq = coded_tunnel_sequence(H, W, N_FRAMES, mode="mux", step=1.0, seed=41)
    flow_path, depth_dir = write_weight_files(str(tmp_path), crafted_liteflownet_state_dict(H, W, "mux"), crafted_monodepth2_state_dict())
    pose_dir = os.path.join(str(tmp_path), "pose")
    os.makedirs(pose_dir, exist_ok=True)
    sd = _pose_weights(constant_motion)
    torch.save({k: v.clone() for k, v in sd.items() if k.startswith("encoder.")}, os.path.join(pose_dir, "pose_encoder.pth"))
    torch.save({k: v.clone() for k, v in sd.items() if k.startswith("net.")}, os.path.join(pose_dir, "pose.pth"))
    cfg = D.full_cfg(H, W, flow_path, depth_dir)
    cfg["deep_pose"] = D.NS(enable=True, pretrained_model=pose_dir)
    cfg["tracking_method"] = tracking_method
    cfg["kp_selection"]["depth_consistency"] = D.NS(enable=depth_consistency, thre=DEPTH_THRE)
    return seq, cfg


def main_loop(cfg, seq, mirrors, record):
    from oracle import cv2_shim
    deep_models, sampler, e_tracker, pnp_tracker, SE3 = mirrors
    cam_mod = importlib.import_module("df-vo_amd.libs.geometry.camera_modules")
    K = seq["K"]
    dc = None
    if cfg.kp_selection.depth_consistency.enable:                      # dfvo.py:84-85
        dc_mod = importlib.import_module("df-vo_amd.libs.matching.depth_consistency")
        dc = dc_mod.DepthConsistency(cfg, cam_mod.Intrinsics([K[0, 2], K[1, 2], K[0, 0], K[1, 1]]))
    np.random.seed(cfg.seed)
    ref_data, cur_data = {}, {}
    global_pose = SE3()
    poses, modes = [], []
    for img_id in range(N_FRAMES):
        cur_data["id"], cur_data["timestamp"], cur_data["img"] = img_id, img_id, seq["frames"][img_id].copy()
        raw = deep_models.forward_depth(imgs=[cur_data["img"]])       # deep_model_inference, dfvo.py:299-345
        cur_data["raw_depth"] = cv2_shim.resize(raw, (W, H), interpolation=cv2_shim.INTER_NEAREST)
        cur_data["depth"] = T.preprocess_depth(cur_data["raw_depth"], cfg.crop.depth_crop, [cfg.depth.min_depth, cfg.depth.max_depth])
        mode = "Ess. Mat."
        if img_id >= 1:
            flows = deep_models.forward_flow(cur_data, ref_data, forward_backward=cfg.deep_flow.forward_backward)
            kf, kb, kd = (ref_data["id"], cur_data["id"]), (cur_data["id"], ref_data["id"]), (ref_data["id"], cur_data["id"], "diff")
            ref_data["flow"], cur_data["flow"], ref_data["flow_diff"] = flows[kf].copy(), flows[kb].copy(), flows[kd].copy()
            if cfg.deep_pose.enable:                                    # dfvo.py:338-345
                pose = deep_models.forward_pose([ref_data["img"], cur_data["img"]])
                assert pose.shape == (4, 4) and pose.dtype == np.float32
                ref_data["deep_pose"] = pose
            rec = {"fwd": np.array(ref_data["flow"]), "diff": np.array(ref_data["flow_diff"]), "raw": np.array(cur_data["raw_depth"]),
                   "deep_pose": np.array(ref_data["deep_pose"])}
            if cfg.tracking_method == "hybrid":                         # dfvo.py:139-250
                if dc is not None:
                    dc.compute(cur_data, ref_data)
                    rec["depth_diff"] = np.array(ref_data["depth_diff"])
                    rec["raw_ref"] = np.array(ref_data["raw_depth"])
                kp_sel = sampler.kp_selection(cur_data, ref_data)
                assert kp_sel["good_kp_found"]
                sampler.update_kp_data(cur_data, ref_data, kp_sel)
                hybrid = SE3()
                e_out = e_tracker.compute_pose_2d2d(ref_data["kp_best"], cur_data["kp_best"], True)
                E_pose = e_out["pose"]
                hybrid.R = E_pose.R
                scale = -1
                if np.linalg.norm(E_pose.t) != 0:
                    scale = e_tracker.scale_recovery(cur_data, ref_data, E_pose, False)["scale"]
                    if scale != -1:
                        hybrid.t = E_pose.t * scale
                if np.linalg.norm(E_pose.t) == 0 or scale == -1:
                    hybrid = pnp_tracker.compute_pose_3d2d(ref_data["kp_best"], cur_data["kp_best"], ref_data["depth"], True)["pose"]
                    mode = "PnP"
                rec.update(kp_ref=np.array(ref_data["kp_best"]), kp_cur=np.array(cur_data["kp_best"]), R=np.array(E_pose.R),
                           t=np.array(E_pose.t), scale=scale, inliers=np.array(e_out["inliers"]))
            elif cfg.tracking_method == "deep_pose":                    # dfvo.py:252-255
                hybrid = SE3(ref_data["deep_pose"])
                mode = "DeepPose"
            global_pose.t = global_pose.R @ hybrid.t + global_pose.t   # update_global_pose, dfvo.py:109-119
            global_pose.R = global_pose.R @ hybrid.R
            rec["rng"] = np.random.get_state()[1].copy()
            record.append(rec)
        poses.append(global_pose.pose.copy())
        modes.append(mode)
        ref_data = dict(cur_data)                                       # update_data, dfvo.py:264-287
        ref_data["flow"] = cur_data["flow"] = ref_data["flow_diff"] = None
    return np.stack(poses), modes


def _run(cfg, seq, monkeypatch, session):
    monkeypatch.setenv("DFVO_SESSION", session)
    mirrors = D._build_mirrors(cfg, seq["K"])
    assert (mirrors[0].session is not None) == (session == "1")
    rec = []
    poses, modes = main_loop(cfg, seq, mirrors, rec)
    return poses, modes, rec, mirrors


def _same(a, b):
    (p0, m0, r0, _), (p1, m1, r1, _) = a, b
    assert m0 == m1 and np.array_equal(p0, p1)
    for x, y in zip(r0, r1):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), "pair result '%s' differs between the plain entry points and the session" % k


def test_deep_pose_tracking(gpu, tmp_path, monkeypatch):
    seq, cfg = _world(tmp_path, False, "deep_pose", False)
    runs = {s: _run(cfg, seq, monkeypatch, s) for s in ("0", "1")}
    _same(runs["0"], runs["1"])
    poses, modes, rec, _ = runs["1"]
    assert modes[1:] == ["DeepPose"] * (N_FRAMES - 1)
    want = np.eye(4)
    for k, r in enumerate(rec):
        assert np.isfinite(r["deep_pose"]).all() and np.array_equal(r["deep_pose"][3], [0, 0, 0, 1])
        want = want @ r["deep_pose"].astype(np.float64)
        assert np.abs(poses[k + 1] - want).max() <= 1e-12
    assert len({r["deep_pose"].tobytes() for r in rec}) == len(rec)  # a prediction per pair, not one repeated


def test_hybrid_tracking_with_the_depth_mask(gpu, tmp_path, monkeypatch):
    seq, cfg = _world(tmp_path, True, "hybrid", True)
    runs = {s: _run(cfg, seq, monkeypatch, s) for s in ("0", "1")}
    _same(runs["0"], runs["1"])
    poses, modes, rec, mirrors = runs["1"]
    st = mirrors[0].session.stats
    print("   modes", modes, "| session", st)
    n = N_FRAMES - 1
    assert st["kp_plain"] == n and st["kp_resident"] == 0 and st["flow_resident"] == n and st["flow_plain"] == 0
    c = cfg.kp_selection.local_bestN
    masked_fewer = 0
    for r in rec:
        # the pose net's constant drive: M = R^T T(-t) x 5.4 on the translation
        assert np.abs(r["deep_pose"] - np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1], [0, 0, 0, 1]])).max() <= 1e-5
        K = seq["K"].astype(np.float32)
        d64, _ = DC.depth_consistency_torch(r["raw"], r["raw_ref"], K, np.linalg.inv(seq["K"]).astype(np.float32), r["deep_pose"],
                                            dtype=torch.float64)
        fin = np.isfinite(d64)
        assert np.abs(r["depth_diff"][fin] - d64[fin]).max() <= 1e-4 and r["depth_diff"].dtype == np.float32
        res = DC.local_bestN_masked(r["fwd"], r["diff"], r["depth_diff"], num_bestN=c.num_bestN, num_row=c.num_row, num_col=c.num_col,
                                    thre=c.thre, depth_thre=DEPTH_THRE, score_method=c.score_method)
        assert res["good_kp_found"]
        assert np.array_equal(r["kp_ref"], res["kp1_best"][0]) and np.array_equal(r["kp_cur"], res["kp2_best"][0])
        plain = T.local_bestN(r["fwd"], r["diff"], num_bestN=c.num_bestN, num_row=c.num_row, num_col=c.num_col, thre=c.thre)
        masked_fewer += not np.array_equal(plain["kp1_best"], res["kp1_best"])
        print("   keypoints %d (without the mask %d), depth_diff < %g on %.0f %% of the image, its deciles 1 / 5 / 9: %s"
              % (res["kp1_best"].shape[1], plain["kp1_best"].shape[1], DEPTH_THRE, 100 * float((r["depth_diff"] < DEPTH_THRE).mean()),
                 np.quantile(r["depth_diff"], [0.1, 0.5, 0.9])))
    assert masked_fewer > 0, "the depth mask changed no selection: the test would pass without it"
    assert any(np.linalg.norm(p[:3, 3]) > 0.3 for p in poses)  # the sequence really moved
