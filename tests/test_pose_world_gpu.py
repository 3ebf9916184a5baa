"""GPU parity of the pose solver chain over the motion / scene / coordinate / degenerate / count matrix of
tests/pose_world.py (tests/test_pose_world_cpu.py states which branch the oracle takes on each case), through the C ABI,
stage by stage on identical inputs and then as a chain, one tracker over interleaved cases last.

Bars are the existing ones (tests/test_solvers_gpu.py, tests/test_tracker_gpu.py): bit-exact -- compared on .view(uint64)
where NaN can occur -- except GRIC scores to 1e-9 relative (libm log / acos) and the least-squares scale to 1e-12 relative
(LAPACK).

What each entry refuses, by its own guard (no case below is sent under these, see pose_world.CASES: n >= 5):
  dfvo_find_homography      n < 5: k_h_init_to_float sets `done`, the sampler is never entered (found = 0)
  dfvo_find_essential_mat   n < 5: enqueue_find_essential_batch skips the loop (found = 0)
  dfvo_compute_pose_3d2d    n_filtered <= 4: k_pnp_init sets `done` (found = 0, the shuffles are still drawn)
The homography sampler retries rejected subsets; pose_world.MAX_GPU_ATTEMPTS bounds what is sent here (host_only cases are
skipped with the reason printed).

Where the REFERENCE raises inside compute_pose_2d2d -- homography_residual(None) when findHomography finds nothing under
GRIC validity, `inv(K.T) @ None` / `None.sum()` / recoverPose(None) when findEssentialMat finds nothing in a repeat -- the
device's answer is a contract (include/dfvo_hip.h, docs/parity.md): identity / zero pose, no valid repeat, the all-ones
inlier mask, and the RandomState advanced by exactly the shuffles the reference drew before it raised.

Found by this file and fixed with it (docs/pose_world.md): np.mean's block-wise reduction above 8192 elements (validity
'flow' at 20000 keypoints, one ulp), findEssentialMat with exactly five points (OpenCV's single kernel run), a pose
returned although no homography was found under GRIC validity, and the RandomState drawn past the repeat in which the
reference raises on a None essential matrix.  Wall time on one MI355X: 42 s for the file (the whole -m gpu suite
before it: about 300 s)."""
import ctypes as C
import time

import numpy as np
import pytest

import pose_world as PW
from oracle import cv2_shim as cv2o
from oracle import tracker_np as T

pytestmark = pytest.mark.gpu

GPU_CASES = [c for c in PW.CASES if not c[9]]
GPU_IDS = [c[0] for c in GPU_CASES]
_BY_ID = {c[0]: c for c in PW.CASES}
_WORLD, _ORACLE = {}, {}


def test_host_only_cases_are_listed():
    for c in PW.CASES:
        if c[9]:
            print("host_only (not run on the GPU: homography sampler above %d draws): %s" % (PW.MAX_GPU_ATTEMPTS, c[0]))
    assert len(GPU_CASES) >= len(PW.CASES) - 5


def world(cid):
    if cid not in _WORLD:
        _WORLD[cid] = PW.build(_BY_ID[cid])
    return _WORLD[cid]


def oracle(key, fn):
    """oracle results are the slow side: computed once per (case, stage, parameters)"""
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


@pytest.fixture(scope="module")
def trk(gpu):
    import sklearn
    lib = gpu.lib()
    t = C.c_void_p()
    gpu.check(lib.dfvo_tracker_create(None, C.byref(t)))
    gpu.set_sklearn_compat(sklearn.__version__)  # the oracle runs the installed RANSACRegressor
    t0 = time.time()
    yield t
    print("test_pose_world_gpu: %.1f s of wall time with this tracker" % (time.time() - t0))
    lib.dfvo_tracker_destroy(t)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def np_state():
    st = np.random.get_state()
    return np.ascontiguousarray(np.r_[st[1].astype(np.uint32), np.uint32(st[2])])


def set_np_state(words):
    np.random.set_state(("MT19937", np.asarray(words[:624], np.uint32), int(words[624]), 0, 0.0))


def push_rng(gpu, trk, words):
    gpu.check(gpu.lib().dfvo_tracker_set_rng_state(trk, gpu.as_ptr(np.ascontiguousarray(words, np.uint32))))


def pull_rng(gpu, trk):
    s = np.zeros(625, np.uint32)
    gpu.check(gpu.lib().dfvo_tracker_get_rng_state(trk, gpu.as_ptr(s)))
    return s


# ------------------------------------------------------------------------------------------------------------------
# device calls
# ------------------------------------------------------------------------------------------------------------------
def hip_E(gpu, trk, a, b, K, prob=0.99, thr=0.2, iters=1000):
    n = a.shape[0]
    E, mask, info = np.zeros(9), np.zeros(max(n, 1), np.uint8), np.zeros(5, np.int32)
    gpu.check(gpu.lib().dfvo_find_essential_mat(trk, gpu.as_ptr(a), gpu.as_ptr(b), n, K[0, 0], K[0, 2], K[1, 2], prob, thr, iters,
                                                gpu.as_ptr(E), gpu.as_ptr(mask), gpu.as_ptr(info)))
    return E.reshape(3, 3), mask[:n], info


def hip_H(gpu, trk, a, b, thr=1.0, iters=2000, conf=0.99):
    n = a.shape[0]
    H, mask, info = np.zeros(9), np.zeros(max(n, 1), np.uint8), np.zeros(5, np.int32)
    gpu.check(gpu.lib().dfvo_find_homography(trk, gpu.as_ptr(a), gpu.as_ptr(b), n, thr, iters, conf, gpu.as_ptr(H), gpu.as_ptr(mask),
                                             gpu.as_ptr(info)))
    return H.reshape(3, 3), mask[:n], info


def hip_pose2d2d(gpu, trk, c, repeat, method, thre):
    K, n = c["K"], c["kp_ref"].shape[0]
    cfg = gpu.Pose2d2dCfg(fx=K[0, 0], cx=K[0, 2], cy=K[1, 2], reproj_thre=0.2, repeat=repeat, max_iters=1000,
                          validity_method=method, validity_thre=thre)
    KinvT, Kinv = np.linalg.inv(K.T), np.linalg.inv(K)
    for i in range(9):
        cfg.KinvT[i] = KinvT.flat[i]
        cfg.Kinv[i] = Kinv.flat[i]
    out = gpu.Pose2d2dOut()
    inl = np.zeros(max(n, 1), np.uint8)
    gpu.check(gpu.lib().dfvo_compute_pose_2d2d(trk, gpu.as_ptr(c["kp_ref"]), gpu.as_ptr(c["kp_cur"]), n, C.byref(cfg), C.byref(out),
                                               gpu.as_ptr(inl)))
    return out, inl[:n]


def hip_scale(gpu, trk, c, T21, method, thre):
    K, n = c["K"], c["kp_ref"].shape[0]
    scfg = gpu.ScaleCfg(cx=K[0, 2], cy=K[1, 2], fx=K[0, 0], fy=K[1, 1], min_samples=3, max_trials=100, stop_prob=0.99, thre=thre,
                        method=method)
    scale, info = C.c_double(), np.zeros(4, np.int32)
    h, w = c["depth_cur"].shape
    gpu.check(gpu.lib().dfvo_find_scale_from_depth(trk, gpu.as_ptr(c["kp_ref"]), gpu.as_ptr(c["kp_cur"]), n, gpu.as_ptr(T21),
                                                   gpu.as_ptr(np.ascontiguousarray(c["depth_cur"])), h, w, C.byref(scfg),
                                                   C.byref(scale), gpu.as_ptr(info)))
    return scale.value, info


def pnp_cfg(gpu, K, repeat):
    cfg = gpu.Pose3d2dCfg(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], min_depth=0.0, max_depth=50.0, repeat=repeat, iters=100,
                          reproj_thre=1.0)
    Kinv = np.linalg.inv(K)
    for i in range(9):
        cfg.Kinv[i] = Kinv.flat[i]
    return cfg


def hip_pnp(gpu, trk, c, kp1, kp2, repeat=5):
    cfg = pnp_cfg(gpu, c["K"], repeat)
    out = gpu.Pose3d2dOut()
    keep = np.zeros(max(len(kp1), 1), np.uint8)
    h, w = c["depth_ref"].shape
    gpu.check(gpu.lib().dfvo_compute_pose_3d2d(trk, gpu.as_ptr(kp1), gpu.as_ptr(kp2), len(kp1), gpu.as_ptr(c["depth_ref"]), h, w,
                                               C.byref(cfg), C.byref(out), gpu.as_ptr(keep)))
    return out, keep[:len(kp1)].astype(bool)


# ------------------------------------------------------------------------------------------------------------------
# oracle calls (cached)
# ------------------------------------------------------------------------------------------------------------------
def oracle_E(cid, rep):
    """findEssentialMat(kp_cur, kp_ref) on the rep-th reshuffle of the case (rep 0: the points as they are)"""
    def run():
        c = world(cid)
        n = c["kp_ref"].shape[0]
        rng = np.random.RandomState(4869 + c["seed"])
        perm = np.arange(n)
        for _ in range(rep):
            rng.shuffle(perm)
        a, b = np.ascontiguousarray(c["kp_cur"][perm]), np.ascontiguousarray(c["kp_ref"][perm])
        st = {}
        with np.errstate(all="ignore"):
            E, m = cv2o.findEssentialMat(a, b, focal=c["K"][0, 0], pp=(c["K"][0, 2], c["K"][1, 2]), method=cv2o.RANSAC, prob=0.99,
                                         threshold=0.2, _stats=st)
        return a, b, E, m, st
    return oracle(("E", cid, rep), run)


def oracle_H(cid):
    def run():
        c = world(cid)
        st = {}
        with np.errstate(all="ignore"):
            H, m = cv2o.findHomography(c["kp_cur"], c["kp_ref"], method=cv2o.RANSAC, confidence=0.99, ransacReprojThreshold=1, _stats=st)
        return H, m, st
    return oracle(("H", cid), run)


VALIDITY = {"GRIC": (0, None, 0.0), "flow": (1, 5.0, 5.0), "homo_ratio": (2, 0.4, 0.4)}


def oracle_chain(cid, validity, repeat):
    def run():
        o = PW.oracle_run(world(cid), repeat=repeat, validity=validity, validity_thre=VALIDITY[validity][1])
        o["key"] = (cid, validity, repeat)
        return o
    return oracle(("chain", cid, validity, repeat), run)


# ------------------------------------------------------------------------------------------------------------------
# 1. RANSAC stages
# ------------------------------------------------------------------------------------------------------------------
def check_E(gpu, trk, cid, rep):
    a, b, Eo, mo, st = oracle_E(cid, rep)
    K = world(cid)["K"]
    Eh, mh, info = hip_E(gpu, trk, a, b, K)
    print("E %-34s rep %d n=%d oracle found=%s iters=%d best=(%d,%d) inliers=%s ties=%s | hip info=%s" % (
        cid, rep, len(a), Eo is not None, st["iters"], st["best_iter"], st["best_model"], None if mo is None else int(mo.sum()),
        st.get("ties"), info.tolist()))
    if Eo is None:
        assert info[0] == 0 and not mh.any(), "oracle finds no E; device info %s, mask sum %d" % (info.tolist(), int(mh.sum()))
        if len(a) > 5:
            assert info[1] == st["iters"], "iterations replayed before giving up"
        return
    assert info[0] == 1
    assert np.array_equal(mh, mo[:, 0]), "inlier masks differ at %d points" % int((mh != mo[:, 0]).sum())
    assert np.array_equal(bits(Eh), bits(Eo)), "E differs: max %g" % np.nanmax(np.abs(Eh - Eo))
    if len(a) > 5:  # (count == 5 is OpenCV's single kernel run: no trajectory)
        assert (info[1], info[2], info[3]) == (st["iters"], st["best_iter"], st["best_model"])
    assert info[4] == int(mo.sum())


@pytest.mark.parametrize("cid", GPU_IDS)
def test_find_essential_mat(gpu, trk, cid):
    for rep in range(3):  # the reference re-shuffles the points between calls (E_tracker.py:225-228)
        check_E(gpu, trk, cid, rep)


def check_H(gpu, trk, cid):
    Ho, mo, st = oracle_H(cid)
    c = world(cid)
    Hh, mh, info = hip_H(gpu, trk, c["kp_cur"], c["kp_ref"])
    print("H %-34s n=%d oracle found=%s iters=%s gave_up=%s attempts=%s inliers=%d | hip info=%s" % (
        cid, len(mh), Ho is not None, st.get("iters"), st.get("subset_failed"), st.get("attempts"), int(mo.sum()), info.tolist()))
    if Ho is None:
        assert info[0] == 0 and not mh.any(), "oracle finds no H; device info %s, mask sum %d" % (info.tolist(), int(mh.sum()))
        assert info[1] == st["iters"], "iterations replayed before the sampler gave up"
        return
    assert info[0] == 1
    assert np.array_equal(mh, mo[:, 0]), "inlier masks differ at %d points" % int((mh != mo[:, 0]).sum())
    assert np.array_equal(bits(Hh), bits(Ho)), "H differs: max %g" % np.nanmax(np.abs(Hh - Ho))
    assert info[1] == st["iters"] and info[2] == st["best_iter"] and info[3] == st["best_model"] and info[4] == st["max_good"]


@pytest.mark.parametrize("cid", GPU_IDS)
def test_find_homography(gpu, trk, cid):
    check_H(gpu, trk, cid)


# ------------------------------------------------------------------------------------------------------------------
# 2. recoverPose and triangulation on the oracle's E
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", GPU_IDS)
def test_recover_pose_and_triangulation(gpu, trk, cid):
    a, b, Eo, mo, st = oracle_E(cid, 0)
    if Eo is None:
        print("recoverPose %s: the oracle finds no E on this case (tests/golden/pose_world_branches.json) -- nothing to decompose" % cid)
        return
    c = world(cid)
    K, n = c["K"], len(a)
    with np.errstate(all="ignore"):
        good_o, Ro, to, mko = cv2o.recoverPose(Eo, a, b, focal=K[0, 0], pp=(K[0, 2], K[1, 2]))
    Rh, th, mk, good = np.zeros(9), np.zeros(3), np.zeros(n, np.uint8), C.c_int()
    gpu.check(gpu.lib().dfvo_recover_pose(trk, gpu.as_ptr(np.ascontiguousarray(Eo.reshape(9))), gpu.as_ptr(a), gpu.as_ptr(b), n,
                                          K[0, 0], K[0, 2], K[1, 2], gpu.as_ptr(Rh), gpu.as_ptr(th), gpu.as_ptr(mk), C.byref(good)))
    Ki = np.linalg.inv(K)
    with np.errstate(all="ignore"):
        xa = np.ascontiguousarray((Ki @ np.c_[a, np.ones(n)].T)[:2])
        xb = np.ascontiguousarray((Ki @ np.c_[b, np.ones(n)].T)[:2])
        P1, P2 = np.ascontiguousarray(np.eye(4)[:3]), np.ascontiguousarray(np.c_[Ro, to])
        Xo = cv2o.triangulatePoints(P1, P2, xa, xb)
    Xh = np.zeros((4, n))
    gpu.check(gpu.lib().dfvo_triangulate_points(trk, gpu.as_ptr(P1), gpu.as_ptr(P2), gpu.as_ptr(xa), gpu.as_ptr(xb), n, gpu.as_ptr(Xh)))
    with np.errstate(all="ignore"):
        at_inf = int((np.abs(Xo[3]) < 1e-12 * np.abs(Xo[:3]).max(0)).sum())
    print("recoverPose %-30s n=%d good: oracle %d hip %d | triangulated: %d non-finite, %d at infinity" % (
        cid, n, good_o, good.value, int((~np.isfinite(Xo)).any(0).sum()), at_inf))
    assert good.value == good_o
    assert np.array_equal(bits(Rh.reshape(3, 3)), bits(Ro)) and np.array_equal(bits(th), bits(to[:, 0]))
    assert np.array_equal(mk, mko[:, 0])
    assert np.array_equal(bits(Xh), bits(Xo)), "triangulation differs in %d entries" % int((bits(Xh) != bits(Xo)).sum())


# ------------------------------------------------------------------------------------------------------------------
# 3. compute_pose_2d2d under the three validity methods, then scale recovery
# ------------------------------------------------------------------------------------------------------------------
def check_pose2d2d(gpu, trk, cid, validity, repeat):
    c = world(cid)
    n = c["kp_ref"].shape[0]
    o = oracle_chain(cid, validity, repeat)
    method, _, thre = VALIDITY[validity]
    np.random.seed(4869 + c["seed"])
    push_rng(gpu, trk, np_state())
    out, inl = hip_pose2d2d(gpu, trk, c, repeat, method, thre)
    rng = pull_rng(gpu, trk)
    R, t = np.array(out.R[:]).reshape(3, 3), np.array(out.t[:]).reshape(3, 1)
    p = o["pose"]
    print("pose2d2d %-32s %-10s repeat %d n=%d: oracle %s E iters %s | hip h_found %d reps %s valid %s cheir %d major %d" % (
        cid, validity, repeat, n,
        ("RAISES " + o["raised"]) if p is None else "reps %s valid %s cheir %d major %s" % (
            p["rep_inliers"], [int(v) for v in p["rep_valid"]], p["cheirality"], p["major_valid"]),
        [e["iters"] for e in o["rec"]["e"]], out.h_found, list(out.rep_inliers[:repeat]), list(out.rep_valid[:repeat]),
        out.cheirality, out.major_valid))
    if p is None:
        # the reference raised: the contract of include/dfvo_hip.h
        assert np.array_equal(R, np.eye(3)) and not t.any(), "pose must be identity / zero where the reference raises"
        assert out.h_found == 0 or not any(out.rep_valid[:repeat])
        assert out.major_valid == 0 and out.cheirality == 0
        assert inl.all(), "inlier mask must be the all-ones one"
        assert np.array_equal(rng, o["rng_after"]), "RandomState must have advanced by the shuffles drawn before the reference raised"
        return o, None
    gated = (validity == "GRIC" and n <= 10) or (validity == "flow" and not p["rep_inliers"])
    if not gated:
        assert list(out.rep_inliers[:repeat]) == p["rep_inliers"]
        assert [bool(v) for v in out.rep_valid[:repeat]] == [bool(v) for v in p["rep_valid"]]
        assert out.cheirality == p["cheirality"] and bool(out.major_valid) == bool(p["major_valid"])
        if validity == "GRIC":
            assert abs(out.h_gric - p["h_gric"]) <= 1e-9 * abs(p["h_gric"])
            for x, y in zip(out.rep_gric[:repeat], p["rep_gric"]):
                assert abs(x - y) <= 1e-9 * abs(y)
        elif validity == "flow":
            assert [int(v) for v in out.rep_gric[:repeat]] == p["rep_cheirality"]
        else:
            assert out.h_gric == p["h_inliers"]
            assert np.array_equal(bits(np.array(out.rep_gric[:repeat])), bits(np.array(p["rep_ratio"])))
    if validity == "flow":
        assert out.h_gric == p["avg_flow"] or (np.isnan(out.h_gric) and np.isnan(p["avg_flow"]))
    assert np.array_equal(inl == 1, p["inliers"]), "inlier masks differ at %d points" % int(((inl == 1) != p["inliers"]).sum())
    assert np.array_equal(bits(R), bits(p["R"])) and np.array_equal(bits(t), bits(p["t"]))
    assert np.array_equal(rng, o["rng_after"]), "RandomState diverged after compute_pose_2d2d"
    return o, p


def check_scale(gpu, trk, cid, o, p, method, thre):
    c = world(cid)
    name = ("depth_ratio", "abs_diff")[method]

    def run():
        set_np_state(o["rng_after"])
        s, diag, raised, T21 = PW.oracle_scale(c, p["R"], p["t"], method=name, thre=thre)
        return s, diag, raised, T21, np_state()
    s_ref, diag, raised, T21, rng_ref = oracle(("scale", o["key"], method, thre), run)
    push_rng(gpu, trk, o["rng_after"])
    scale, info = hip_scale(gpu, trk, c, T21, method, thre)
    print("   scale %-11s thre %g: oracle %s (valid %s trials %s inliers %s) | hip %.15g info %s" % (
        name, thre, raised or "%.15g" % s_ref, diag.get("n_valid"), diag.get("n_trials"), diag.get("n_inliers"), scale, info.tolist()))
    assert np.array_equal(pull_rng(gpu, trk), rng_ref), "RandomState diverged after scale recovery"
    if raised:
        assert info[3] == -1
        return
    assert info[0] == diag["n_valid"]
    if s_ref == -1:
        assert scale == -1
    else:
        assert info[1] == diag["n_trials"] and info[2] == diag["n_inliers"]
        assert abs(scale - s_ref) <= 1e-12 * abs(s_ref)


@pytest.mark.parametrize("cid", GPU_IDS)
def test_compute_pose_2d2d_gric_and_scale(gpu, trk, cid):
    for repeat in (5, 3):
        o, p = check_pose2d2d(gpu, trk, cid, "GRIC", repeat)
        if p is not None and np.linalg.norm(p["t"]) != 0 and repeat == 5:
            check_scale(gpu, trk, cid, o, p, 0, 0.1)
            check_scale(gpu, trk, cid, o, p, 1, 0.1)
            check_scale(gpu, trk, cid, o, p, 0, PW.TIGHT_THRE)


@pytest.mark.parametrize("validity", ["flow", "homo_ratio"])
@pytest.mark.parametrize("cid", GPU_IDS)
def test_compute_pose_2d2d_other_validity(gpu, trk, cid, validity):
    check_pose2d2d(gpu, trk, cid, validity, 5)


# ------------------------------------------------------------------------------------------------------------------
# 4. PnP
# ------------------------------------------------------------------------------------------------------------------
PNP_IDS = [c[0] for c in GPU_CASES if c[2] in ("box", "ground", "two_planes") and c[4] == 1500 and c[8] is None]


def oracle_pnp(cid, repeat=5):
    def run():
        c = world(cid)
        np.random.seed(4869 + c["seed"])
        res, planar, raised = PW.oracle_pnp(c, repeat)
        return res, planar, raised, np_state()
    return oracle(("pnp", cid, repeat), run)


def check_pnp(gpu, trk, cid, at_kp=False):
    c = world(cid)
    res, planar, raised, rng_ref = oracle_pnp(cid)
    assert raised is None
    kp1, kp2 = PW.pnp_inputs(c)
    np.random.seed(4869 + c["seed"])
    push_rng(gpu, trk, np_state())
    out, keep = hip_pnp(gpu, trk, c, kp1, kp2)
    rng = pull_rng(gpu, trk)
    print("pnp %-34s n=%d oracle filtered %d inliers %d planar %s | hip found %d filtered %d inliers %d status %d" % (
        cid, len(kp1), len(res["kp1"]), res["best_inlier"], planar, out.found, out.n_filtered, out.best_inliers, out.status))
    assert out.n_filtered == len(res["kp1"])
    assert np.array_equal(kp1[keep], res["kp1"]) and np.array_equal(kp2[keep], res["kp2"])
    assert bool(out.found) == (res["best_inlier"] > 0) and out.best_inliers == res["best_inlier"]
    assert np.array_equal(bits(np.array(out.R[:]).reshape(3, 3)), bits(res["R"]))
    assert np.array_equal(bits(np.array(out.tvec[:]).reshape(3, 1)), bits(res["t"]))
    assert np.array_equal(rng, rng_ref), "RandomState diverged after compute_pose_3d2d"
    if not at_kp:
        return
    h, w = c["depth_ref"].shape
    at = np.ascontiguousarray(c["depth_ref"][kp1[:, 1].astype(int), kp1[:, 0].astype(int)])
    o1, keep1 = gpu.Pose3d2dOut(), np.zeros(max(len(kp1), 1), np.uint8)
    np.random.seed(4869 + c["seed"])
    rng1 = np_state()
    cfg = pnp_cfg(gpu, c["K"], 5)
    gpu.check(gpu.lib().dfvo_compute_pose_3d2d_at_kp(trk, gpu.as_ptr(kp1), gpu.as_ptr(kp2), len(kp1), gpu.as_ptr(at), h, w, C.byref(cfg),
                                                     gpu.as_ptr(rng1), C.byref(o1), gpu.as_ptr(keep1)))
    assert (out.found, out.best_inliers, out.n_filtered, out.status) == (o1.found, o1.best_inliers, o1.n_filtered, o1.status)
    assert np.array_equal(keep, keep1[:len(kp1)].astype(bool))
    assert list(out.rvec) == list(o1.rvec) and list(out.tvec) == list(o1.tvec) and list(out.R) == list(o1.R)
    assert np.array_equal(rng1, rng_ref)


@pytest.mark.parametrize("cid", PNP_IDS)
def test_compute_pose_3d2d(gpu, trk, cid):
    check_pnp(gpu, trk, cid, at_kp=True)


# ------------------------------------------------------------------------------------------------------------------
# 5. one tracker, cases interleaved: nothing of an earlier case may reach a later one
# ------------------------------------------------------------------------------------------------------------------
INTERLEAVED = ["forward-box-n2000", "forward-box-n6", "still-box-n20000", "forward-one_row", "forward-box-n64", "forward-box-float",
               "still-exact-n17-e-none-rep0", "forward-ground-n20000", "still-box-n5", "turn-box-grid", "still-one_point",
               "forward-box-n11", "pure_yaw-box-n20000", "forward-box-n10", "still-box-grid-exact", "forward-box-n257",
               "forward-all_outliers", "forward-box-n65", "still-exact-n17-e-none-rep4", "nudge-shelf-float", "forward-nonfinite",
               "forward-box-n7", "roll-ground-float", "still-one_row", "forward-box-n2000"]


def test_one_tracker_over_interleaved_cases(gpu):
    """sizes going up and down, "found" followed by "nothing found": RansacWorkspace::ensure grows and never shrinks, so stale
    counts / nmodels / masks / permutations / best-inlier flags of a larger earlier case must not reach a later one"""
    import sklearn
    lib = gpu.lib()
    t = C.c_void_p()
    gpu.check(lib.dfvo_tracker_create(None, C.byref(t)))
    gpu.set_sklearn_compat(sklearn.__version__)
    try:
        for cid in INTERLEAVED:
            assert not _BY_ID[cid][9]
            check_E(gpu, t, cid, 1)
            check_H(gpu, t, cid)
            o, p = check_pose2d2d(gpu, t, cid, "GRIC", 5)
            if p is not None and np.linalg.norm(p["t"]) != 0:
                check_scale(gpu, t, cid, o, p, 0, 0.1)
            check_pose2d2d(gpu, t, cid, "homo_ratio", 5)
            if cid in PNP_IDS:
                check_pnp(gpu, t, cid)
    finally:
        lib.dfvo_tracker_destroy(t)
