"""The oracle's tracking chain for one pair under a TrackingPipeline option set (tests/test_pipeline_configs_gpu.py):
keypoint source -> compute_pose_2d2d(validity) -> find_scale_from_depth(method) -> PnP fallback, or PnP alone, with the
branch rules of libs/dfvo.py:121-262.  Consumes the global np.random exactly as the reference does.  CPU only."""
import numpy as np

from oracle import tracker_np as T

H, W = 128, 416          # the smoke test's image size; depth feed 64 x 96
BESTN_N = 777            # counts that are no multiple of 64
SAMPLED_N = 1999
FLOW_CROP = ((0.1, 0.9), (0.05, 0.95))

SOURCES = {
    "local_bestN": {},
    "bestN": {"kp_source": "bestN", "kp_num_bestN": BESTN_N},
    "sampled": {"kp_source": "sampled", "kp_sampled_num": SAMPLED_N, "flow_crop": FLOW_CROP},
}


def keypoints(o, flow, diff):
    """(good_kp_found, kp_ref [n,2], kp_cur [n,2]) of the option set's keypoint source"""
    h, w = diff.shape
    src = o.get("kp_source", "local_bestN")
    if src == "bestN":
        k1, k2 = T.bestN_flow_kp(flow, diff[..., None], N=o["kp_num_bestN"])
        return True, k1[0], k2[0]
    if src == "sampled":
        crop = o.get("flow_crop", ((0.0, 1.0), (0.0, 1.0)))
        idx = T.generate_kp_samples(h, w, crop, o["kp_sampled_num"])
        k1, k2 = T.sampled_kp(flow, idx, crop)
        return True, k1[0], k2[0]
    kp = T.local_bestN(flow, diff[..., None], num_bestN=o.get("kp_num_bestN", 2000), thre=o.get("kp_thre", 0.1),
                       score_method=o.get("kp_score_method", "flow"))
    if not kp["good_kp_found"]:
        return False, None, None
    return True, kp["kp1_best"][0], kp["kp2_best"][0]


def solve_pair(o, flow, diff, depth_cur, depth_ref, K):
    """dict(status 0 E | 1 constant motion | 2 needs PnP | 3 PnP, kp_ref, kp_cur, inliers, E (compute_pose_2d2d's dict),
    scale, scale_diag, pnp (compute_pose_3d2d's dict))"""
    good, k1, k2 = keypoints(o, flow, diff)
    r = {"good_kp_found": good, "kp_ref": k1, "kp_cur": k2, "E": None, "scale": -1, "scale_diag": {}, "pnp": None}
    if not good:
        r["status"] = 1
        return r
    pnp_only = o.get("tracking_method", "hybrid") == "PnP"
    need_pnp = pnp_only
    r["inliers"] = np.ones(len(k1), bool)
    if not pnp_only:
        res = T.compute_pose_2d2d(k1, k2, K, validity=o.get("validity", "GRIC"), validity_thre=o.get("validity_thre"))
        r["E"] = res
        r["inliers"] = np.asarray(res["inliers"]).reshape(-1).astype(bool)
        if np.linalg.norm(res["t"]) != 0:  # dfvo.py:198
            pose = np.eye(4)
            pose[:3, :3], pose[:3, 3:] = res["R"], res["t"]
            r["scale"] = T.find_scale_from_depth(k1, k2, np.linalg.inv(pose), depth_cur, K, diag=r["scale_diag"],
                                                 method=o.get("scale_method", "depth_ratio"))
        need_pnp = np.linalg.norm(res["t"]) == 0 or r["scale"] == -1
    if not need_pnp:
        r["status"] = 0
    elif depth_ref is None:
        r["status"] = 2
    else:
        r["pnp"] = T.compute_pose_3d2d(k1, k2, depth_ref, K, 0.0, 50.0, 5, 100, 1.0)
        r["status"] = 3
    return r


def tunnel_inputs(h=192, w=640):
    """the input on which GRIC accepts E for every keypoint source: the coded tunnel world's true flow and depth with a
    little noise (the 128 x 416 ramp scenes are too close to a plane for the whole-image sources)"""
    from synth import coded_tunnel_sequence, tunnel_truth
    seq = coded_tunnel_sequence(h, w, 3, mode="pot")
    gt_f, _, z1 = tunnel_truth(seq, 0)
    rng = np.random.default_rng(5)
    flow = (gt_f + 0.03 * rng.standard_normal(gt_f.shape)).astype(np.float32)
    diff = np.abs(0.05 * rng.standard_normal((h, w))).astype(np.float32)
    diff[rng.random((h, w)) < 0.3] = 2.0
    depth = np.clip(z1, 0, 50).astype(np.float64)
    return {"K": seq["K"], "flow": flow, "diff": diff, "depth_cur": depth, "depth_ref": depth}
