"""Seeded two-view inputs for the pose solver chain over camera motions, scenes, coordinate kinds, degenerate match sets
and point counts (CPU only; imported by test_pose_world_cpu.py, test_pose_world_gpu.py and test_host_lanes.py), and the
branch signature the ORACLE takes on each of them (homography / five-point RANSAC trajectory, GRIC validity, cheirality,
scale recovery, PnP), which tests/golden/pose_world_branches.json records.

`pose_case("forward", "box", "float", n, seed, out_frac, noise)` is synthetic.two_view / make_golden_cases.tracker_case
bit for bit (test_pose_world_cpu.py asserts it), so the older fixtures and this matrix are one family.

CASES is the one literal table: (id, motion, scene, coords, n, seed, out_frac, noise, degenerate, host_only).
host_only cases stay on the host build (tests/test_host_lanes.py) and are skipped, with the reason printed, by the GPU
tests: the single-lane homography sampler (k_h_subsets) retries a rejected subset up to 10000 times for each of up to
2000 subsets, so a case is run on the GPU only when the oracle's sampler needs fewer than MAX_GPU_ATTEMPTS draws on it.
"""
import contextlib

import numpy as np

MOTIONS = {  # rotation vector [rad], translation (view 1 -> view 2, as synthetic.two_view)
    "forward": ((0.002, 0.01, 0.001), (0.02, 0.01, 0.8)),
    "still": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
    "creep": ((0.0, 1e-5, 0.0), (0.0005, 0.0, 0.004)),  # flow far below the 0.2 px threshold
    "pure_yaw": ((0.0, 0.05, 0.0), (0.0, 0.0, 0.0)),
    "sideways": ((0.001, 0.002, 0.0005), (0.6, 0.0, 0.02)),
    "backward": ((0.002, -0.005, 0.001), (0.01, 0.0, -0.8)),
    "turn": ((0.0, 0.12, 0.0), (0.15, 0.0, 0.6)),
    "roll": ((0.0, 0.0, 0.3), (0.02, 0.01, 0.5)),
    "climb": ((0.02, 0.0, 0.0), (0.0, -0.4, 0.3)),
    # a baseline of centimetres: parallax of pixels on the near points (E explains what no homography does, GRIC validates), but
    # every depth is more than 50 baselines away, beyond recoverPose's distance threshold: the cheirality count collapses
    "nudge": ((0.0, 0.0, 0.0), (0.1, 0.0, 0.003)),
}
SCENES = ("box", "ground", "far", "two_planes")
COORDS = ("float", "grid")
DEGENERATE = ("one_row", "one_point", "dup_third", "all_outliers", "nonfinite", "scale_1e6", "scale_1em6", "cfg5")
GROUND_Y = 1.65
WALL_Z = 30.0
MAX_GPU_ATTEMPTS = 200000  # ~1.2 us per sampler draw on the device (solver_ransac.hip, k_h_subsets): a few tenths of a second


def rotation(wv):
    """Rodrigues formula as synthetic.two_view writes it; the zero vector (which two_view divides by) gives the identity"""
    wv = np.asarray(wv, np.float64)
    th = np.linalg.norm(wv)
    if th == 0:
        return np.eye(3)
    k = wv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def intrinsics(w, h):
    f = 718.856 * w / 1241.0
    return np.array([[f, 0, 607.19 * w / 1241.0], [0, f, 185.22 * h / 376.0], [0, 0, 1]])


def _scene_points(r, scene, n):
    """3-D points in the frame of view 1 and a flag per point: 1 = on the ground plane, 2 = on the wall, 0 = free"""
    if scene == "box":  # exactly two_view's three draws
        return np.stack([r.uniform(-20, 20, n), r.uniform(-3, 3, n), r.uniform(5, 60, n)], 1), np.zeros(n, np.int8)
    if scene == "ground":
        return np.stack([r.uniform(-20, 20, n), np.full(n, GROUND_Y), r.uniform(5, 60, n)], 1), np.ones(n, np.int8)
    if scene == "far":
        z = r.uniform(5e3, 6e4, n)
        return np.stack([z * r.uniform(-0.8, 0.8, n), z * r.uniform(-0.24, 0.24, n), z], 1), np.zeros(n, np.int8)
    if scene == "shelf":  # the box with depths uniform in 1 / Z: parallax spread evenly, so that no single homography fits
        return np.stack([r.uniform(-20, 20, n), r.uniform(-3, 3, n), 1.0 / r.uniform(1 / 60.0, 1 / 5.5, n)], 1), np.zeros(n, np.int8)
    assert scene == "two_planes"
    g = r.random(n) < 0.5
    X = np.stack([r.uniform(-20, 20, n), np.where(g, GROUND_Y, r.uniform(-3, GROUND_Y, n)),
                  np.where(g, r.uniform(5, WALL_Z, n), WALL_Z)], 1)
    return X, np.where(g, 1, 2).astype(np.int8)


def _project(K, X):
    x = (K @ X.T).T
    return x[:, :2] / x[:, 2:]


def pose_case(motion, scene, coords, n, seed, out_frac=0.3, noise=0.15, w=1241, h=376):
    """-> dict(kp_ref, kp_cur [n,2] f64, K, R, t (true motion, view 1 -> view 2), outliers, depth_cur [h,w] (CNN-like depth
    of the CURRENT view at int(kp_cur): true depth x 1.25, 2 % noise, a fifth of the pixels arbitrary), depth_ref [h,w]
    (depth of the REFERENCE view at int(kp_ref) for PnP: 2 % holes, the top tenth of the rows beyond the 50 m cap), w, h)"""
    r = np.random.Generator(np.random.PCG64(seed))
    X, plane = _scene_points(r, scene, n)
    K = intrinsics(w, h)
    wv, tv = MOTIONS[motion]
    R, t = rotation(wv), np.asarray(tv, np.float64)
    if coords == "float":  # two_view, draw for draw
        x1 = _project(K, X)
        X2 = (R @ X.T).T + t
        x2 = _project(K, X2)
        x1 = x1 + r.normal(0, noise, x1.shape)
        x2 = x2 + r.normal(0, noise, x2.shape)
        o = r.random(n) < out_frac
        x2[o] = np.stack([r.uniform(0, w, int(o.sum())), r.uniform(0, h, int(o.sum()))], 1)
    else:
        # what the pipeline hands the solvers: kp_ref on the integer pixel grid, kp_cur = kp_ref + float32 flow.  The 3-D
        # point is moved onto the ray of its pixel (staying on its plane), and the flow is the difference of two
        # projections evaluated the same way, so that no motion gives a flow of exactly zero.
        assert coords == "grid"
        pix = np.rint(_project(K, X))
        ray = (np.linalg.inv(K) @ np.c_[pix, np.ones(n)].T).T
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where((plane == 1) & (ray[:, 1] > 0), GROUND_Y / ray[:, 1], X[:, 2])
        X = ray * z[:, None]
        X2 = (R @ X.T).T + t
        flow = _project(K, X2) - _project(K, X)
        flow = flow + r.normal(0, noise, flow.shape) if noise > 0 else flow
        o = r.random(n) < out_frac
        wild = np.stack([r.uniform(0, w, int(o.sum())), r.uniform(0, h, int(o.sum()))], 1)
        flow[o] = wild - pix[o]
        x1 = pix
        x2 = pix + flow.astype(np.float32).astype(np.float64)
    x1, x2 = np.ascontiguousarray(x1), np.ascontiguousarray(x2)
    g = np.random.Generator(np.random.PCG64(seed + 1000))
    zs = X2[:, 2] * 1.25 * (1 + g.normal(0, 0.02, n))
    wild = g.random(n) < 0.2
    zs[wild] = g.uniform(5, 60, int(wild.sum()))
    depth_cur = _scatter(x2, zs, h, w)
    z1 = X[:, 2].copy()
    z1[g.random(n) < 0.02] = 0.0
    depth_ref = _scatter(x1, z1, h, w)
    depth_ref[:int(0.1 * h)][depth_ref[:int(0.1 * h)] > 0] = 70.0
    return dict(kp_ref=x1, kp_cur=x2, K=K, R=R, t=t, outliers=o, depth_cur=depth_cur, depth_ref=depth_ref, w=w, h=h)


def _scatter(kp, vals, h, w):
    d = np.zeros((h, w))
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(kp).all(1) & (kp[:, 0] >= 0) & (kp[:, 0] < w) & (kp[:, 1] >= 0) & (kp[:, 1] < h)
    ix, iy = kp[ok, 0].astype(int), kp[ok, 1].astype(int)
    d[iy, ix] = vals[ok]
    return d


def degenerate(c, kind, seed):
    """a degenerate match set built on top of a case (keypoints only; K and the depth maps stay)"""
    c = dict(c)
    a, b = c["kp_ref"].copy(), c["kp_cur"].copy()
    n = a.shape[0]
    g = np.random.Generator(np.random.PCG64(seed + 2000))
    if kind == "one_row":  # all keypoints on one image row, in both views: every subset is collinear
        a[:, 1] = 200.0
        b[:, 1] = 200.0
    elif kind == "one_point":
        a[:] = a[0]
        b[:] = b[0]
    elif kind == "dup_third":  # a third of the correspondences are copies of others
        src = g.integers(0, n, n // 3)
        dst = g.choice(n, n // 3, replace=False)
        a[dst], b[dst] = a[src], b[src]
    elif kind == "all_outliers":
        b = np.stack([g.uniform(0, c["w"], n), g.uniform(0, c["h"], n)], 1)
    elif kind == "nonfinite":  # NaN, +inf, -inf in the first five rows and elsewhere
        for row, col, v in ((1, 0, np.nan), (3, 1, np.inf), (4, 0, -np.inf), (n // 2, 1, np.nan), (n - 2, 0, np.inf),
                            (n // 3, 0, -np.inf)):
            b[row, col] = v
    elif kind == "scale_1e6":
        a, b = a * 1e6, b * 1e6
    elif kind == "scale_1em6":
        a, b = a * 1e-6, b * 1e-6
    else:
        raise KeyError(kind)
    c["kp_ref"], c["kp_cur"] = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return c


def _matrix():
    rows = []
    seed = 9000
    # every motion x scene x coordinate kind at one mid count
    for m in MOTIONS:
        for s in SCENES:
            for k in COORDS:
                seed += 1
                rows.append(("%s-%s-%s" % (m, s, k), m, s, k, 1500, seed, 0.3, 0.15 if k == "float" else 0.1, None, False))
    # every degenerate set on forward and on still
    for m in ("forward", "still"):
        for d in DEGENERATE:
            seed += 1
            rows.append(("%s-%s" % (m, d), m, "box", "grid" if m == "still" else "float", 1500, seed, 0.3, 0.15, d, False))
    # the count axis
    for m, s in (("forward", "box"), ("still", "box"), ("forward", "ground")):
        for n in (5, 6, 7, 9, 10, 11, 63, 64, 65, 255, 256, 257, 2000):
            seed += 1
            k = "grid" if m == "still" else "float"
            rows.append(("%s-%s-n%d" % (m, s, n), m, s, k, n, seed, 0.0 if n < 12 else 0.2, 0.0 if m == "still" else 0.1, None,
                         False))
    # 20000 points for each motion class that changes the branch taken
    for m, s in (("still", "box"), ("pure_yaw", "box"), ("forward", "ground")):
        seed += 1
        rows.append(("%s-%s-n20000" % (m, s), m, s, "grid", 20000, seed, 0.3, 0.1, None, False))
    return rows


# Cases found by seed sweeps on the oracle for branches the regular matrix does not reach; the seeds are frozen here.
EXTRA = [
    # (id, motion, scene, coords, n, seed, out_frac, noise, degenerate, host_only)
    ("still-box-grid-exact", "still", "box", "grid", 1500, 9201, 0.0, 0.0, None, False),      # the two views equal bit for bit
    ("still-box-grid-exact-outl", "still", "box", "grid", 1500, 9202, 0.3, 0.0, None, False),
    ("still-exact-n17-e-none-rep0", "still", "box", "grid", 17, 9306, 0.0, 0.0, None, False),  # findEssentialMat -> None at once
    ("still-exact-n17-e-none-rep4", "still", "box", "grid", 17, 9304, 0.0, 0.0, None, False),  # ... in the fifth repeat
    ("still-exact-n18-e-none-rep2", "still", "box", "grid", 18, 9308, 0.0, 0.0, None, False),  # ... in the third
    # GRIC validates, recoverPose's cheirality count is under / exactly at the 10 % gate: the pose is rejected
    ("nudge-shelf-float", "nudge", "shelf", "float", 1500, 9203, 0.1, 0.02, None, False),
    ("nudge-shelf-grid", "nudge", "shelf", "grid", 1500, 9203, 0.1, 0.02, None, False),
    ("nudge-shelf-n100-cheirality-at-gate", "nudge", "shelf", "float", 100, 9502, 0.15, 0.05, None, False),
    # under the tight residual threshold RANSACRegressor ends on a one-sample consensus set / without one (ValueError)
    ("forward-box-n14-scale-one-sample-consensus", "forward", "box", "float", 14, 9614, 0.0, 0.1, None, False),
    ("forward-box-n16-scale-no-consensus", "forward", "box", "float", 16, 9606, 0.0, 0.1, None, False),
]

CASES = _matrix() + EXTRA
CASE_IDS = [c[0] for c in CASES]
FIELDS = ("id", "motion", "scene", "coords", "n", "seed", "out_frac", "noise", "degenerate", "host_only")


def build(case):
    """case tuple -> inputs"""
    cid, motion, scene, coords, n, seed, of, noise, deg, _ = case
    wh = (1920, 1280) if deg == "cfg5" else (1241, 376)
    c = pose_case(motion, scene, coords, n, seed, of, noise, w=wh[0], h=wh[1])
    if deg and deg != "cfg5":
        c = degenerate(c, deg, seed)
    c["seed"] = seed
    c["id"] = cid
    return c


# ------------------------------------------------------------------------------------------------------------------
# the oracle's branch signature
# ------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _recording(rec):
    """record the RANSAC diagnostics of every findEssentialMat and the finiteness of every GRIC residual vector that
    oracle.tracker_np.compute_pose_2d2d goes through"""
    from oracle import cv2_shim, tracker_np as T
    fe, gr = cv2_shim.findEssentialMat, T.calc_GRIC

    def find_e(*a, **kw):
        out = fe(*a, **kw)
        st = cv2_shim.ransac_stats()
        rec["e"].append(dict(found=out[0] is not None, iters=st["iters"], best_iter=st["best_iter"], best_model=st["best_model"],
                             ties=st["ties"], inliers=None if out[1] is None else int(out[1].sum())))
        return out

    def gric(res, sigma, n, model):
        rec["gric_nonfinite"] = rec["gric_nonfinite"] or not bool(np.isfinite(np.asarray(res)[:n]).all())
        return gr(res, sigma, n, model)

    cv2_shim.findEssentialMat, T.calc_GRIC = find_e, gric
    try:
        yield
    finally:
        cv2_shim.findEssentialMat, T.calc_GRIC = fe, gr


def oracle_run(c, repeat=5, validity="GRIC", validity_thre=None):
    """the oracle chain on one case under RandomState 4869 + seed: dict(pose2d (or None), raised, rng_after, rec)"""
    import warnings
    from oracle import tracker_np as T
    np.random.seed(4869 + c["seed"])
    rec = {"e": [], "gric_nonfinite": False}
    out, raised = None, None
    with _recording(rec), warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        try:
            out = T.compute_pose_2d2d(c["kp_ref"], c["kp_cur"], c["K"], repeat=repeat, validity=validity,
                                      validity_thre=validity_thre)
        except Exception as e:  # the reference raises here too (None homography / None E)
            raised = type(e).__name__
    st = np.random.get_state()
    return dict(pose=out, raised=raised, rec=rec, rng_after=np.ascontiguousarray(np.r_[st[1].astype(np.uint32), np.uint32(st[2])]))


TIGHT_THRE = 1e-3


def oracle_scale(c, R, t, method="depth_ratio", thre=0.1):
    """find_scale_from_depth on pose (R, t) under the CURRENT RandomState -> (scale or None, diag, raised)"""
    import warnings
    from oracle import tracker_np as T
    pose = np.eye(4)
    pose[:3, :3] = R
    pose[:3, 3:] = np.asarray(t).reshape(3, 1)
    T21 = np.ascontiguousarray(np.linalg.inv(pose))
    diag, s, raised = {}, None, None
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        try:
            s = T.find_scale_from_depth(c["kp_ref"], c["kp_cur"], T21, c["depth_cur"], c["K"], diag=diag, method=method, thre=thre)
        except ValueError:  # sklearn: "RANSAC could not find a valid consensus set"
            raised = "ValueError"
    return s, diag, raised, T21


def pnp_inputs(c):
    """the correspondences PnP is given: the pipeline's reference keypoints are pixels of the image, and the reference indexes
    the depth map with them unchecked (IndexError outside), so rows whose reference keypoint is outside are dropped"""
    a = c["kp_ref"]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(a).all(1) & (a[:, 0] >= 0) & (a[:, 0] < c["w"]) & (a[:, 1] >= 0) & (a[:, 1] < c["h"])
    return np.ascontiguousarray(a[ok]), np.ascontiguousarray(c["kp_cur"][ok])


def oracle_pnp(c, repeat=5):
    """compute_pose_3d2d under the CURRENT RandomState -> (result or None, planar initialisation ran, raised)"""
    from oracle import cv2_shim, tracker_np as T
    before = cv2_shim.pnp_planar_count()
    res, raised = None, None
    kp1, kp2 = pnp_inputs(c)
    with np.errstate(all="ignore"):
        try:
            res = T.compute_pose_3d2d(kp1, kp2, c["depth_ref"], c["K"], 0.0, 50.0, repeat, 100, 1.0)
        except (NotImplementedError, IndexError, ValueError) as e:
            raised = type(e).__name__
    return res, cv2_shim.pnp_planar_count() > before, raised


def signature(case):
    """the branch signature of one case: plain ints / bools / strings (JSON)"""
    from oracle import cv2_shim
    c = build(case)
    n = c["kp_ref"].shape[0]
    sig = {"n": int(n)}
    # stage level: homography as the GRIC path calls it, E on the unshuffled points
    hs = {}
    with np.errstate(all="ignore"):
        H, hm = cv2_shim.findHomography(c["kp_cur"], c["kp_ref"], method=cv2_shim.RANSAC, confidence=0.99,
                                        ransacReprojThreshold=1, _stats=hs)
    sig["h"] = dict(found=H is not None, iters=hs.get("iters", -1), gave_up=bool(hs.get("subset_failed", 0)),
                    attempts=hs.get("attempts", 0), inliers=int(hm.sum()))
    es = {}
    with np.errstate(all="ignore"):
        E, em = cv2_shim.findEssentialMat(c["kp_cur"], c["kp_ref"], focal=c["K"][0, 0], pp=(c["K"][0, 2], c["K"][1, 2]),
                                          method=cv2_shim.RANSAC, prob=0.99, threshold=0.2, _stats=es)
    sig["e"] = dict(found=E is not None, iters=es["iters"], best_iter=es["best_iter"], best_model=es["best_model"],
                    ties=es.get("ties", 0), inliers=None if em is None else int(em.sum()))
    # the chain
    o = oracle_run(c)
    p = o["pose"]
    sig["raised"] = o["raised"]
    sig["gric_nonfinite"] = bool(o["rec"]["gric_nonfinite"])
    sig["rep"] = [[e["iters"], e["best_iter"], e["best_model"], e["ties"], e["inliers"]] for e in o["rec"]["e"]]
    accepted = False
    if p is not None:
        accepted = bool(p["major_valid"] and p["cheirality"] > n * 0.1)
        sig.update(rep_valid=[bool(v) for v in p["rep_valid"]], major_valid=bool(p["major_valid"]),
                   cheirality=int(p["cheirality"]), accepted=accepted, best_inlier_cnt=int(p["best_inlier_cnt"]))
    if accepted:
        s, diag, raised, _ = oracle_scale(c, p["R"], p["t"])
        sig["scale"] = dict(n_valid=diag.get("n_valid"), n_trials=diag.get("n_trials"), n_inliers=diag.get("n_inliers"),
                            outcome=raised or ("few" if s == -1 else "fit"))
        # and under the tight residual threshold of tests/test_tracker_gpu.py::test_scale_recovery_sklearn_versions, where
        # RANSACRegressor can end without a consensus set (ValueError)
        s, diag, raised, _ = oracle_scale(c, p["R"], p["t"], thre=TIGHT_THRE)
        sig["scale_tight"] = dict(n_valid=diag.get("n_valid"), n_trials=diag.get("n_trials"), n_inliers=diag.get("n_inliers"),
                                  outcome=raised or ("few" if s == -1 else "fit"))
    np.random.seed(4869 + c["seed"])
    res, planar, raised = oracle_pnp(c)
    sig["pnp"] = dict(raised=raised, planar=bool(planar), n_filtered=None if res is None else int(len(res["kp1"])),
                      best_inlier=None if res is None else int(res["best_inlier"]))
    return sig


def coverage(table, max_iters=1000):
    """branch-coverage conditions over a {case id: signature} table -> {condition: [case ids that meet it]}"""
    cov = {k: [] for k in (
        "h_sampler_gives_up", "h_not_found", "e_not_found", "gric_prefers_h_although_e_has_majority", "valid_but_cheirality_low",
        "winning_model_not_0", "e_iters_below_128", "e_iters_128_or_129", "e_iters_between", "e_iters_max", "tie_first_wins",
        "gric_residual_nonfinite", "scale_few_ratios", "scale_value_error", "scale_fit", "pnp_few_survivors", "pnp_planar",
        "pnp_normal", "nothing_found_anywhere")}
    for cid, s in table.items():
        n = s["n"]
        runs = [[s["e"]["iters"], s["e"]["best_iter"], s["e"]["best_model"], s["e"]["ties"], s["e"]["inliers"]]] + s["rep"]
        if s["h"]["gave_up"]:
            cov["h_sampler_gives_up"].append(cid)
        if not s["h"]["found"]:
            cov["h_not_found"].append(cid)
        if not s["e"]["found"] and n >= 5:
            cov["e_not_found"].append(cid)
        if "rep_valid" in s and not s["major_valid"] and len(s["rep"]) and min(r[4] for r in s["rep"]) > n / 2:
            cov["gric_prefers_h_although_e_has_majority"].append(cid)
        if s.get("major_valid") and not s["accepted"]:
            cov["valid_but_cheirality_low"].append(cid)
        for it, bi, bm, ties, inl in runs:
            if it < 0:
                continue
            if bm > 0:
                cov["winning_model_not_0"].append(cid)
            if ties > 0:
                cov["tie_first_wins"].append(cid)
            key = ("e_iters_below_128" if 1 <= it < 128 else "e_iters_128_or_129" if it in (128, 129) else
                   "e_iters_max" if it == max_iters else "e_iters_between" if 129 < it < max_iters else None)
            if key:
                cov[key].append(cid)
        if s["gric_nonfinite"]:
            cov["gric_residual_nonfinite"].append(cid)
        for sc in (s.get("scale"), s.get("scale_tight")):
            if not sc:
                continue
            cov[{"few": "scale_few_ratios", "ValueError": "scale_value_error", "fit": "scale_fit"}[sc["outcome"]]].append(cid)
        p = s["pnp"]
        if p["raised"] is None:
            cov["pnp_few_survivors" if p["n_filtered"] < 5 else "pnp_planar" if p["planar"] else "pnp_normal"].append(cid)
        if not s["h"]["found"] and not s["e"]["found"] and not s.get("accepted") and not (p["best_inlier"] or 0):
            cov["nothing_found_anywhere"].append(cid)
    return {k: sorted(set(v)) for k, v in cov.items()}
