"""The oracle's tracking chain for one pair with the trackers' iterative keypoint refinement on (tests/test_pipeline_refine_gpu.py):
libs/dfvo.py:164-250 restated over oracle.tracker_np -- pipeline_configs_oracle.keypoints -> compute_pose_2d2d with 3 repeats ->
find_scale_from_depth -> kp_selection_good_depth under inv(hybrid_pose) -> compute_pose_2d2d on kp_depth with `repeat` repeats ->
(scale_recovery.iterative_kp) find_scale_from_depth on kp_depth -> the PnP branch, itself in two passes under
pnp_tracker.iterative_kp.  Consumes the global np.random exactly as the reference does and records every intermediate;
tests/test_pipeline_refine_cpu.py holds it to the reference's own DFVO.tracking() (tests/golden/iterative_kp.npz).  CPU only."""
import numpy as np

from oracle import tracker_np as T
import pipeline_configs_oracle as PO

REFINE_DEFAULTS = dict(e_iterative_kp=False, scale_iterative_kp=False, pnp_iterative_kp=False, e_iterative_score="opt_flow",
                       pnp_iterative_score="rigid_flow", rigid_num_bestN=2000, rigid_num_row=10, rigid_num_col=10, rigid_flow_thre=5.0,
                       optical_flow_thre=0.1)


def _pose(R, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3:] = R, np.asarray(t).reshape(3, 1)
    return P


def select(ro, flow, diff, raw_ref, pose, K, score):
    """compute_rigid_flow_kp (E_tracker.py:422-440, pnp_tracker.py:127-145) for the SE3 `pose`: rigid_flow_pose = inv(pose).
    dict(ref_kp, cur_kp: the best set kp_depth, mask: rigid_flow_diff, rigid_flow_pose), or None where the reference asserts"""
    rfp = np.linalg.inv(pose)
    try:
        sel = T.kp_selection_good_depth(flow, diff[..., None], raw_ref, rfp, K, score, num_bestN=ro["rigid_num_bestN"],
                                        num_row=ro["rigid_num_row"], num_col=ro["rigid_num_col"], rigid_thre=ro["rigid_flow_thre"],
                                        opt_thre=ro["optical_flow_thre"])
    except AssertionError as e:
        assert str(e) == "sampling threshold is too small."
        return None
    return dict(ref_kp=sel["kp1_depth"][0], cur_kp=sel["kp2_depth"][0], mask=sel["rigid_flow_mask"], rigid_flow_pose=rfp)


def solve_pair(o, ro, flow, diff, depth_cur, depth_ref, raw_ref, K):
    """o: TrackingPipeline's option keys (kp_source .., validity, scale_method, tracking_method, e_repeat, pnp_repeat), ro: its
    refinement keys (REFINE_DEFAULTS filled in).  Returns dict(status 0 E | 1 constant motion | 2 needs PnP | 3 PnP | None: the
    pair raised, error None | "empty", kp_ref, kp_cur, inliers: the tracked set and pass one's mask; E1, scale1: pass one; sel_e:
    select()'s record or None; E2: the second pass; inliers2; scale2 (None: the stage did not run); R, t, scale: the E path's
    final pose; pnp1, sel_pnp, pnp: the PnP branch; kp_depth: (ref, cur) of the pair's last selection, mask: its distance map)"""
    full = dict(REFINE_DEFAULTS)
    full.update(ro)
    ro = full
    validity = dict(validity=o.get("validity", "GRIC"), validity_thre=o.get("validity_thre"))
    e_repeat, pnp_repeat = o.get("e_repeat", 5), o.get("pnp_repeat", 5)
    method = o.get("scale_method", "depth_ratio")
    good, k1, k2 = PO.keypoints(o, flow, diff)
    r = dict(good_kp_found=good, kp_ref=k1, kp_cur=k2, status=None, error=None, E1=None, scale1=None, sel_e=None, E2=None, inliers2=None,
             scale2=None, R=None, t=None, scale=-1, pnp1=None, sel_pnp=None, pnp=None, kp_depth=None, mask=None)
    if not good:
        r["status"] = 1
        return r
    pnp_only = o.get("tracking_method", "hybrid") == "PnP"
    need_pnp = pnp_only
    r["inliers"] = np.ones(len(k1), bool)
    if not pnp_only:
        e_ref = bool(ro["e_iterative_kp"])
        res = T.compute_pose_2d2d(k1, k2, K, repeat=3 if e_ref else e_repeat, **validity)  # is_iterative = not enable
        r["E1"] = res
        r["inliers"] = np.asarray(res["inliers"]).reshape(-1).astype(bool)
        R, t, scale = res["R"], res["t"], -1
        hybrid_t = np.zeros((3, 1))
        t_zero = np.linalg.norm(t) == 0
        if not t_zero:  # dfvo.py:182
            scale = T.find_scale_from_depth(k1, k2, np.linalg.inv(_pose(R, t)), depth_cur, K, method=method)
            r["scale1"] = scale
            if scale != -1:
                hybrid_t = t * scale
        if not t_zero and e_ref:  # dfvo.py:195
            sel = select(ro, flow, diff, raw_ref, _pose(R, hybrid_t), K, ro["e_iterative_score"])
            r["sel_e"] = sel
            if sel is None:
                r["error"] = "empty"
                r["R"], r["t"], r["scale"] = R, t, scale
                return r
            r["kp_depth"], r["mask"] = (sel["ref_kp"], sel["cur_kp"]), sel["mask"]
            res2 = T.compute_pose_2d2d(sel["ref_kp"], sel["cur_kp"], K, repeat=e_repeat, **validity)
            r["E2"] = res2
            r["inliers2"] = np.asarray(res2["inliers"]).reshape(-1).astype(bool)
            R, t = res2["R"], res2["t"]
            t_zero = np.linalg.norm(t) == 0
            if not t_zero and ro["scale_iterative_kp"]:
                scale = T.find_scale_from_depth(sel["ref_kp"], sel["cur_kp"], np.linalg.inv(_pose(R, t)), depth_cur, K, method=method)
                r["scale2"] = scale
        r["R"], r["t"], r["scale"] = R, t, scale
        need_pnp = t_zero or scale == -1
    if not need_pnp:
        r["status"] = 0
        return r
    if depth_ref is None:
        r["status"] = 2
        return r
    p_ref = bool(ro["pnp_iterative_kp"])
    pnp = T.compute_pose_3d2d(k1, k2, depth_ref, K, o.get("min_depth", 0.0), o.get("max_depth", 50.0), 3 if p_ref else pnp_repeat, 100, 1.0)
    if p_ref:
        r["pnp1"] = pnp
        sel = select(ro, flow, diff, raw_ref, pnp["pose"], K, ro["pnp_iterative_score"])
        r["sel_pnp"] = sel
        if sel is None:
            r["error"] = "empty"
            r["pnp"] = pnp
            return r
        r["kp_depth"], r["mask"] = (sel["ref_kp"], sel["cur_kp"]), sel["mask"]
        pnp = T.compute_pose_3d2d(sel["ref_kp"], sel["cur_kp"], depth_ref, K, o.get("min_depth", 0.0), o.get("max_depth", 50.0), pnp_repeat,
                                  100, 1.0)
    r["pnp"] = pnp
    r["status"] = 3
    return r


def hybrid_pose(r):
    """the pair's 4x4 (cur -> ref) as dfvo.py leaves it in ref_data['pose'], and tracking_mode"""
    if r["status"] == 3:
        return r["pnp"]["pose"], "PnP"
    return _pose(r["R"], r["t"] * r["scale"]), "Ess. Mat."


def rng_words():
    st = np.random.get_state()
    return np.ascontiguousarray(np.r_[st[1].astype(np.uint32), np.uint32(st[2])])
