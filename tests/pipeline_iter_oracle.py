"""The oracle's tracking chain for one pair under scale_recovery.method iterative (tests/test_pipeline_iterative_gpu.py):
pipeline_configs_oracle.keypoints -> compute_pose_2d2d(validity) -> scale_recovery_iterative from the carried prev_scale -> PnP
fallback, with the branch rules of libs/dfvo.py:121-262.  Consumes the global np.random exactly as the reference does.
The loop is oracle.tracker_np.scale_recovery_iterative's body with a record of every round (rounds completed, the scale each round
started from and found, its uniform keypoint count) and with the two places where the reference raises turned into a record;
tests/test_pipeline_iterative_cpu.py holds it to that function.  CPU only."""
import numpy as np

from oracle import tracker_np as T
import pipeline_configs_oracle as PO

ITER_DEFAULTS = dict(iter_kp_src="kp_best", rigid_num_bestN=2000, rigid_num_row=10, rigid_num_col=10, rigid_flow_thre=5.0,
                     optical_flow_thre=0.1)


def iterative_loop(flow, diff, raw_ref, depth_cur, E_pose, K, prev_scale, kp_src="kp_depth", kp_best=None, **kw):
    """E_tracker.py:509-569 -> dict(scale: the last completed round's (prev_scale when none completed), n_iter, scale_in,
    scale_out, n_kp: per round, ref_kp / cur_kp / mask: the uniform keypoints and distance map of the last round that selected any,
    error: None | "empty" (the assertion of kp_selection.py) | "no_consensus" (sklearn's ValueError))"""
    rec = dict(scale=prev_scale, n_iter=0, scale_in=[], scale_out=[], n_kp=[], ref_kp=None, cur_kp=None, mask=None, error=None)
    E_pose = np.asarray(E_pose, np.float64)
    T21 = np.linalg.inv(E_pose)
    scale = prev_scale
    for it in range(5):
        P = E_pose.copy()
        P[:3, 3] *= scale
        rec["scale_in"].append(scale)
        try:
            sel = T.kp_selection_good_depth(flow, diff[..., None], raw_ref, np.linalg.inv(P), K, "opt_flow", **kw)
        except AssertionError as e:
            assert str(e) == "sampling threshold is too small."
            rec["n_kp"].append(0)
            rec["error"] = "empty"
            return rec
        ref_kp_depth, cur_kp_depth = sel["kp1_depth_uniform"][0], sel["kp2_depth_uniform"][0]
        rec["n_kp"].append(len(ref_kp_depth))
        rec["ref_kp"], rec["cur_kp"], rec["mask"] = ref_kp_depth, cur_kp_depth, sel["rigid_flow_mask"]
        ref_kp, cur_kp = (ref_kp_depth, cur_kp_depth) if kp_src == "kp_depth" else kp_best
        try:
            new_scale = T.find_scale_from_depth(ref_kp, cur_kp, T21, depth_cur, K)
        except ValueError:
            rec["error"] = "no_consensus"
            return rec
        delta = np.abs(new_scale - scale)
        scale = new_scale
        rec["scale_out"].append(scale)
        rec["scale"] = scale  # self.prev_scale = new_scale
        rec["n_iter"] = it + 1
        if delta < 0.001:
            break
    return rec


def solve_pair(o, io, flow, diff, depth_cur, depth_ref, raw_ref, K, state):
    """pipeline_configs_oracle.solve_pair with the iterative loop as the scale stage.  o: TrackingPipeline's option keys, io: its
    iterative keys (ITER_DEFAULTS filled in); state["prev_scale"] is read and, after a completed round, written.  Adds
    r["iter"] (iterative_loop's record, None when the loop did not run) and r["error"]; a pair that raises has no status."""
    full = dict(ITER_DEFAULTS)
    full.update(io)
    good, k1, k2 = PO.keypoints(o, flow, diff)
    r = {"good_kp_found": good, "kp_ref": k1, "kp_cur": k2, "E": None, "scale": -1, "pnp": None, "iter": None, "error": None,
         "status": None}
    if not good:
        r["status"] = 1
        return r
    res = T.compute_pose_2d2d(k1, k2, K, validity=o.get("validity", "GRIC"), validity_thre=o.get("validity_thre"))
    r["E"] = res
    r["inliers"] = np.asarray(res["inliers"]).reshape(-1).astype(bool)
    t_zero = np.linalg.norm(res["t"]) == 0
    if not t_zero:  # dfvo.py:182
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3:] = res["R"], res["t"]
        rec = iterative_loop(flow, diff, raw_ref, depth_cur, pose, K, state["prev_scale"], full["iter_kp_src"], (k1, k2),
                             num_bestN=full["rigid_num_bestN"], num_row=full["rigid_num_row"], num_col=full["rigid_num_col"],
                             rigid_thre=full["rigid_flow_thre"], opt_thre=full["optical_flow_thre"])
        r["iter"] = rec
        if rec["n_iter"] > 0:
            state["prev_scale"] = rec["scale"]
        if rec["error"]:
            r["error"] = rec["error"]
            return r
        r["scale"] = rec["scale"]
    if not (t_zero or r["scale"] == -1):
        r["status"] = 0
    elif depth_ref is None:
        r["status"] = 2
    else:
        r["pnp"] = T.compute_pose_3d2d(k1, k2, depth_ref, K, 0.0, 50.0, 5, 100, 1.0)
        r["status"] = 3
    return r


def rng_words():
    st = np.random.get_state()
    return np.ascontiguousarray(np.r_[st[1].astype(np.uint32), np.uint32(st[2])])
