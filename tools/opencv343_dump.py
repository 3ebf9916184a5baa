#!/usr/bin/env python
"""Dump OpenCV 3.4.3's outputs for the committed seeded cases, so that the restatement in oracle/cv3_*.c can be pinned to
the real library.  Run on ANY machine that has `opencv-python==3.4.3.18` (the reference's pin,
envs/requirement.yml:296) and numpy:

    pip install opencv-python==3.4.3.18 numpy
    python tools/opencv343_dump.py            # writes tests/golden/opencv343_cases.npz

then commit the file: tests/test_oracle_opencv_pin.py compares the oracle with it bit for bit (masks, inlier lists) /
to 1e-12 (matrices) and stops reporting "parity unpinned".  The calls are exactly the reference's call sites:
    cv2.findEssentialMat   libs/tracker/E_tracker.py:231-239      cv2.findHomography  :199-205
    cv2.recoverPose        libs/tracker/E_tracker.py:292-295      cv2.triangulatePoints  libs/geometry/ops_3d.py:63
    cv2.solvePnPRansac     libs/tracker/pnp_tracker.py:98-105     cv2.Rodrigues  :116
The inputs are regenerated from seeds by numpy.random.Generator(PCG64) only (no dependency on this repository beyond
this file), and stored alongside the outputs so that the comparison does not depend on regenerating them identically."""
import os
import sys

import numpy as np


def two_view(n, out_frac, noise, seed, w=1241, h=376):
    """identical to df-vo_amd/synthetic.py:two_view (kept self-contained on purpose)"""
    r = np.random.Generator(np.random.PCG64(seed))
    X = np.stack([r.uniform(-20, 20, n), r.uniform(-3, 3, n), r.uniform(5, 60, n)], 1)
    f = 718.856 * w / 1241.0
    K = np.array([[f, 0, 607.19 * w / 1241.0], [0, f, 185.22 * h / 376.0], [0, 0, 1]])
    wv = np.array([0.002, 0.01, 0.001])
    th = np.linalg.norm(wv)
    k = wv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = np.array([0.02, 0.01, 0.8])
    x1 = (K @ X.T).T
    x1 = x1[:, :2] / x1[:, 2:]
    X2 = (R @ X.T).T + t
    x2 = (K @ X2.T).T
    x2 = x2[:, :2] / x2[:, 2:]
    x1 = x1 + r.normal(0, noise, x1.shape)
    x2 = x2 + r.normal(0, noise, x2.shape)
    o = r.random(n) < out_frac
    x2[o] = np.stack([r.uniform(0, w, int(o.sum())), r.uniform(0, h, int(o.sum()))], 1)
    return np.ascontiguousarray(x1), np.ascontiguousarray(x2), X, K


CASES = [(2000, 0.3, 0.15, 31), (2000, 0.6, 0.3, 32), (600, 0.2, 0.1, 33), (2000, 0.97, 0.2, 34), (200, 0.0, 0.05, 35), (40, 0.1, 0.2, 36)]


def planar_view(n, seed, tilt, noise=0.2, w=1241, h=376):
    """object points on one plane (a road / wall seen obliquely): solvePnPRansac's refinement takes
    cvFindExtrinsicCameraParams2's planar initialisation (W[2] / W[1] < 1e-3)"""
    r = np.random.Generator(np.random.PCG64(seed))
    f = 718.856 * w / 1241.0
    K = np.array([[f, 0, 607.19 * w / 1241.0], [0, f, 185.22 * h / 376.0], [0, 0, 1]])
    X = np.stack([r.uniform(-15, 15, n), np.full(n, 1.65), r.uniform(6, 45, n)], 1)
    X[:, 1] += tilt * X[:, 0]
    wv = np.array([0.003, -0.015, 0.002])
    th = np.linalg.norm(wv)
    k = wv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = np.array([0.04, -0.02, 0.9])
    X2 = (R @ X.T).T + t
    x2 = (K @ X2.T).T
    x2 = x2[:, :2] / x2[:, 2:] + r.normal(0, noise, (n, 2))
    return np.ascontiguousarray(X), np.ascontiguousarray(x2), K


PLANAR_CASES = [(400, 41, 0.0), (400, 42, 0.25), (60, 43, 0.1)]


# (seed, h, w, oh, ow).  1-5: the frame's direction (down to the configured size).  6-7: the depth map's direction (feed size
# up to KITTI's frames, dfvo.py:314-317).  8-10: small sizes at which cv::resize's double inverse scale, floor(x * (1.0 /
# (W / w))), picks other source indices than float32 or exact integer arithmetic would.
RESIZE_CASES = [(1, 376, 1241, 192, 640), (2, 370, 1226, 192, 640), (3, 96, 128, 48, 64), (4, 60, 80, 130, 210),
                (5, 480, 640, 256, 320), (6, 192, 640, 376, 1241), (7, 192, 640, 370, 1226), (8, 14, 12, 18, 34),
                (9, 28, 30, 36, 85), (10, 21, 18, 27, 51)]


def distinct_depth(h, w):
    """a distinct float32 value in every pixel (identical to tests/resample_cases.py:depth_input): a wrong source index of the
    nearest resize changes the output, which one uint8 channel's 256 values do not show reliably"""
    return (1.0 + np.arange(h * w, dtype=np.float64) * 2.0 ** -12).astype(np.float32).reshape(h, w)


def main(out_path):
    import cv2
    if not cv2.__version__.startswith("3.4.3"):
        print("WARNING: this is OpenCV %s, the reference pins 3.4.3.18 -- the dump records the version" % cv2.__version__)
    out = {"cv_version": np.array(cv2.__version__), "n_cases": len(CASES)}
    for ci, (n, of, noise, seed) in enumerate(CASES):
        x1, x2, X, K = two_view(n, of, noise, seed)
        p = "c%d_" % ci
        out[p + "spec"] = np.array([n, of, noise, seed])
        out[p + "x1"], out[p + "x2"], out[p + "X"], out[p + "K"] = x1, x2, X, K
        fx, pp = K[0, 0], (K[0, 2], K[1, 2])
        # E_tracker.py:231-239 (kp_cur, kp_ref order as the reference passes them)
        E, mask = cv2.findEssentialMat(x2, x1, focal=fx, pp=pp, method=cv2.RANSAC, prob=0.99, threshold=0.2)
        out[p + "E"], out[p + "E_mask"] = (E if E is not None else np.zeros((0, 3))), (mask if mask is not None else np.zeros((0, 1), np.uint8))
        if E is not None and E.shape == (3, 3):
            cnt, R, t, m2 = cv2.recoverPose(E, x2, x1, focal=fx, pp=pp)  # E_tracker.py:292-295
            out[p + "rp_cnt"], out[p + "rp_R"], out[p + "rp_t"], out[p + "rp_mask"] = np.array(cnt), R, t, m2
            P1, P2 = np.c_[np.eye(3), np.zeros(3)], np.c_[R, t]
            Kinv = np.linalg.inv(K)
            n1 = (np.c_[x1, np.ones(n)] @ Kinv.T)[:, :2].T.copy()
            n2 = (np.c_[x2, np.ones(n)] @ Kinv.T)[:, :2].T.copy()
            out[p + "tri"] = cv2.triangulatePoints(P1, P2, n1, n2)  # ops_3d.py:63
        H, hm = cv2.findHomography(x2, x1, method=cv2.RANSAC, confidence=0.99, ransacReprojThreshold=1)  # E_tracker.py:199-205
        out[p + "H"], out[p + "H_mask"] = (H if H is not None else np.zeros((0, 3))), (hm if hm is not None else np.zeros((0, 1), np.uint8))
        # pnp_tracker.py:98-105: object points = view-1 structure, image points = view-2 keypoints
        ok, rvec, tvec, inl = cv2.solvePnPRansac(objectPoints=X, imagePoints=x2, cameraMatrix=K, distCoeffs=None,
                                                 iterationsCount=100, reprojectionError=1)
        out[p + "pnp_ok"], out[p + "pnp_rvec"], out[p + "pnp_tvec"] = np.array(bool(ok)), rvec, tvec
        out[p + "pnp_inliers"] = inl if inl is not None else np.zeros((0, 1), np.int32)
        out[p + "rod"] = cv2.Rodrigues(rvec)[0]
    # coplanar object points: the homography initialisation of cvFindExtrinsicCameraParams2 (calibration.cpp) behind
    # solvePnPRansac (pnp_tracker.py:98-105); and cv2.solvePnP(ITERATIVE) alone on the same points (no RANSAC in front)
    out["n_planar"] = len(PLANAR_CASES)
    for pi, (n, seed, tilt) in enumerate(PLANAR_CASES):
        X, x2, K = planar_view(n, seed, tilt)
        p = "p%d_" % pi
        out[p + "X"], out[p + "x2"], out[p + "K"] = X, x2, K
        ok, rvec, tvec, inl = cv2.solvePnPRansac(objectPoints=X, imagePoints=x2, cameraMatrix=K, distCoeffs=None,
                                                 iterationsCount=100, reprojectionError=1)
        out[p + "pnp_ok"], out[p + "pnp_rvec"], out[p + "pnp_tvec"] = np.array(bool(ok)), rvec, tvec
        out[p + "pnp_inliers"] = inl if inl is not None else np.zeros((0, 1), np.int32)
        Xf, xf = X.astype(np.float32).astype(np.float64), x2.astype(np.float32).astype(np.float64)
        ok2, rv2, tv2 = cv2.solvePnP(Xf, xf, K, None, flags=cv2.SOLVEPNP_ITERATIVE)
        out[p + "it_ok"], out[p + "it_rvec"], out[p + "it_tvec"] = np.array(bool(ok2)), rv2, tv2
    # five points exactly (count == modelPoints: the registrator returns the kernel's first model) and the five-tuples of
    # case 0 on which the restated five-point solver leaves the largest constraint residual (tests/test_oracle_opencv_
    # properties.py): findEssentialMat on those five correspondences alone answers whether OpenCV's solver does the same
    x1, x2, X, K = two_view(2000, 0.3, 0.15, 31)
    r5 = np.random.Generator(np.random.PCG64(77))
    tuples = [r5.choice(2000, 5, replace=False) for _ in range(40)]
    out["five_idx"] = np.array(tuples)
    for ti, idx in enumerate(tuples):
        E5, m5 = cv2.findEssentialMat(x2[idx], x1[idx], focal=K[0, 0], pp=(K[0, 2], K[1, 2]), method=cv2.RANSAC, prob=0.99, threshold=0.2)
        out["five_E_%d" % ti] = E5 if E5 is not None else np.zeros((0, 3))
    # cv::solvePoly directly (it IS exposed in Python): the Durand-Kerner sweep behind every five-point hypothesis.  Random
    # degree-10 polynomials, and polynomials built to hit `p - roots[j] == 0` exactly -- the 3.4 line is recalled to skip such
    # factors and count `num_same_root` (then take square / cube roots of the correction), where the restatement and the
    # device multiply by the zero factor: x^10, (x - 1)^10 expanded, products of exactly repeated integer roots, and
    # polynomials whose roots sit ON the start spiral (1 + i)^k, so that a root equals its start value from the first sweep
    rp = np.random.Generator(np.random.PCG64(91))
    polys = [rp.normal(0, 1, 11) * 10.0 ** rp.integers(-3, 4, 11) for _ in range(20)]
    polys.append(np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0]))
    polys.append(np.poly(np.ones(10))[::-1].copy())
    polys.append(np.poly([1, 1, 2, 2, 3, 3, -1, -1, 0.5, 0.5])[::-1].copy())
    polys.append(np.poly([2, 2, 2, -3, -3, 4, 5, 6, 7, 8])[::-1].copy())
    spiral = [(1 + 1j) ** k for k in range(10)]
    polys.append(np.real(np.poly(spiral[:2] + [np.conj(spiral[1])] + [3.0, -2.0, 0.25, 7.0, -0.5, 1.5, 9.0]))[::-1].copy())
    out["n_poly"] = len(polys)
    for qi, c in enumerate(polys):
        c = np.ascontiguousarray(c, np.float64)
        _, roots = cv2.solvePoly(c, maxIters=300)
        out["poly_c_%d" % qi], out["poly_r_%d" % qi] = c, np.asarray(roots, np.float64).reshape(-1, 2)
    # utils.py:51 (read_image): cv2.resize(img, (w, h)) of the uint8 frame, default INTER_LINEAR; dfvo.py:314-317 nearest
    out["n_resize"] = len(RESIZE_CASES)
    for ri, (seed, h, w, oh, ow) in enumerate(RESIZE_CASES):
        img = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (h, w, 3), dtype=np.uint8)
        out["r%d_spec" % ri] = np.array([seed, h, w, oh, ow])
        out["r%d_img" % ri] = img
        out["r%d_linear" % ri] = cv2.resize(img, (ow, oh))
        out["r%d_nearest" % ri] = cv2.resize(img[..., 0].astype(np.float32), (ow, oh), interpolation=cv2.INTER_NEAREST)
        out["r%d_nearest_distinct" % ri] = cv2.resize(distinct_depth(h, w), (ow, oh), interpolation=cv2.INTER_NEAREST)
    # cv::RNG: not exposed in Python; findEssentialMat's subset stream is exercised through the masks above
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, "with OpenCV", cv2.__version__)


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "tests", "golden", "opencv343_cases.npz"))
