"""GPU: dfvo_depth_consistency and dfvo_kp_local_bestn_depth.

Depth consistency: scenes of synthetic.py's tunnel world (depth in [2, 40] m, |t| <= 0.5 m: the reprojected depth stays
away from 0 and the ratio is well conditioned -- checked on the float64 restatement) against the float64 evaluation of
tests/depth_consistency_ref.py; every pixel within 1.5 times the LARGEST distance of the torch-CPU float32 restatement to
float64 on that scene.  One edge scene by category.  Masked local_bestN: bit for bit -- keypoints, count, order -- against
the restatement and the fixture the reference's kp_selection.local_bestN wrote."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import depth_consistency_ref as DC
import posenet_ref as PR
from oracle import tracker_np as T

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def run_host(capi, cur, ref, K, Kinv, pose):
    out = np.full(cur.shape, -7.0, np.float32)
    capi.check(capi.lib().dfvo_depth_consistency_host(*[capi.as_ptr(np.ascontiguousarray(a, dtype=np.float32)) for a in (cur, ref)],
                                                      cur.shape[0], cur.shape[1],
                                                      *[capi.as_ptr(np.ascontiguousarray(a, dtype=np.float32)) for a in (K, Kinv, pose)],
                                                      capi.as_ptr(out)))
    return out


def run_device(capi, cur, ref, K, Kinv, pose):
    h, w = cur.shape
    d_cur, d_ref = torch.from_numpy(np.ascontiguousarray(cur)).cuda(), torch.from_numpy(np.ascontiguousarray(ref)).cuda()
    band = 64  # sentinels in front of and behind the destination
    buf = torch.full((2 * band + h * w,), -7.0, device="cuda")
    mats = [np.ascontiguousarray(a, dtype=np.float32) for a in (K, Kinv, pose)]
    torch.cuda.synchronize()
    capi.check(capi.lib().dfvo_depth_consistency(C.c_void_p(d_cur.data_ptr()), C.c_void_p(d_ref.data_ptr()), h, w, capi.as_ptr(mats[0]),
                                                 capi.as_ptr(mats[1]), capi.as_ptr(mats[2]), C.c_void_p(buf.data_ptr() + 4 * band), None))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:band] == -7.0).all() and (host[band + h * w:] == -7.0).all(), "wrote outside the destination"
    return host[band:band + h * w].reshape(h, w)


@pytest.mark.parametrize("h,w,k", [(48, 80, 3), (48, 80, 9), (37, 53, 20)])
def test_depth_consistency_distance_to_the_exact_function(gpu, h, w, k):
    cur, ref, K, Kinv, pose = DC.tunnel_scene(h, w, k)
    assert cur.min() >= 2 and cur.max() <= 40 and ref.min() >= 2 and ref.max() <= 40
    d64, reproj64 = DC.depth_consistency_torch(cur, ref, K, Kinv, pose, dtype=torch.float64)
    assert reproj64.min() > 1  # the ratio's denominator stays away from 0
    d32, _ = DC.depth_consistency_torch(cur, ref, K, Kinv, pose)
    got = run_host(gpu, cur, ref, K, Kinv, pose)
    assert np.array_equal(got, run_device(gpu, cur, ref, K, Kinv, pose)), "host-array and device-pointer forms differ"
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    e_dev = np.abs(got.astype(np.float64) - d64)
    e_ora = float(np.abs(d32.astype(np.float64) - d64).max())
    print("DEPTH CONSISTENCY %dx%d k=%d: max |device - exact| %.3e  max |torch fp32 - exact| %.3e  max value %.3e"
          % (h, w, k, float(e_dev.max()), e_ora, float(d64.max())))
    PR.record_parity("depth_consistency", {"%dx%d k=%d" % (h, w, k): {"device_to_exact_max": float(e_dev.max()),
                                                                       "torch_fp32_to_exact_max": e_ora, "max_value": float(d64.max())}})
    assert d64.max() > 1e-3  # a map with content
    assert (e_dev <= 1.5 * e_ora).all(), "worst pixel %.3e vs 1.5 x %.3e" % (float(e_dev.max()), e_ora)
    if (h, w, k) in ((48, 80, 3), (37, 53, 20)):  # the reference-made fixtures (to the restatement's own tolerance + the bound)
        g = np.load(os.path.join(G, "depth_consistency_tunnel.npz"))
        tag = "a" if h == 48 else "b"
        assert np.abs(got - g[tag + "_depth_diff"]).max() <= 1e-6 + 2.5 * e_ora


def test_depth_consistency_edge_scene_by_category(gpu):
    h, w = 37, 53
    cur, ref, K, Kinv, _ = DC.tunnel_scene(h, w, 20)
    # (a) every projection out of view to the right: the sample is the border column's, interpolated along it
    ref_rows = np.repeat((5.0 + 0.1 * np.arange(h, dtype=np.float32))[:, None], w, axis=1)
    ref_rows[:, :-1] += 3.0  # only the last column holds the ramp: a sample taken anywhere else is off by 3 m
    pose = np.eye(4, dtype=np.float32)
    pose[0, 3] = 400.0
    want, _ = DC.depth_consistency_torch(cur, ref_rows, K, Kinv, pose, dtype=torch.float64)
    got = run_host(gpu, cur, ref_rows, K, Kinv, pose)
    assert np.array_equal(got, run_device(gpu, cur, ref_rows, K, Kinv, pose))
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    elsewhere, _ = DC.depth_consistency_torch(cur, ref_rows + 3.0 * (np.arange(w) == w - 1), K, Kinv, pose, dtype=torch.float64)
    assert np.abs(want - elsewhere).max() > 0.05  # (a sample taken off the border column would show)
    assert np.abs(got - want).max() <= 1e-5
    # (b) zero depth, no translation, zero reference depth at the pixel the origin projects to: 0 / 0, and the NaN survives
    cur0, ref0 = cur.copy(), ref.copy()
    cur0[10:14, 20:31] = 0.0
    ref0[0, 0] = 0.0
    rot = np.eye(4, dtype=np.float32)
    c, s = math.cos(0.01), math.sin(0.01)
    rot[0, 0], rot[0, 2], rot[2, 0], rot[2, 2] = c, s, -s, c
    want, _ = DC.depth_consistency_torch(cur0, ref0, K, Kinv, rot, dtype=torch.float64)
    got = run_host(gpu, cur0, ref0, K, Kinv, rot)
    assert np.array_equal(got, run_device(gpu, cur0, ref0, K, Kinv, rot), equal_nan=True)
    assert np.isnan(want[10:14, 20:31]).all() and np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(got)
    assert got[fin].min() >= 0 and got[fin].max() <= 1
    # (c) a camera turned round: the reprojected depth is negative and the clamp leaves 0 or 1
    back = np.eye(4, dtype=np.float32)
    back[0, 0] = back[2, 2] = -1.0
    got = run_host(gpu, cur, ref, K, Kinv, back)
    assert np.array_equal(got, run_device(gpu, cur, ref, K, Kinv, back))
    assert np.isin(got, (0.0, 1.0)).all()


# ---- local_bestN with the depth mask ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trk(gpu):
    lib = gpu.lib()
    t = C.c_void_p()
    gpu.check(lib.dfvo_tracker_create(None, C.byref(t)))
    yield t
    lib.dfvo_tracker_destroy(t)


def run_masked(gpu, trk, flow, diff, ddiff, nr, nc, num_bestN, thre, depth_thre, score):
    h, w = diff.shape
    kp1, kp2 = np.full((num_bestN, 2), -7.0), np.full((num_bestN, 2), -7.0)
    n, good = C.c_int(-7), C.c_int(-7)
    flow, diff, ddiff = (np.ascontiguousarray(a, dtype=np.float32) for a in (flow, diff, ddiff))
    gpu.check(gpu.lib().dfvo_kp_local_bestn_depth(trk, gpu.as_ptr(flow), gpu.as_ptr(diff), gpu.as_ptr(ddiff), h, w, nr, nc, num_bestN,
                                                  thre, depth_thre, score, gpu.as_ptr(kp1), gpu.as_ptr(kp2), C.byref(n), C.byref(good)))
    return n.value, good.value, kp1, kp2


def check_against(res, n, good, kp1, kp2):
    assert bool(good) == bool(res["good_kp_found"])
    if not good:
        assert n == 0
        return
    assert n == res["kp1_best"].shape[1]
    assert np.array_equal(kp1[:n], res["kp1_best"][0]) and np.array_equal(kp2[:n], res["kp2_best"][0])
    assert (kp1[n:] == -7.0).all() and (kp2[n:] == -7.0).all()


@pytest.mark.parametrize("tag,method", [("a", "flow"), ("b", "flow"), ("r", "flow_ratio")])
def test_masked_local_bestn_reproduces_the_reference_fixture(gpu, trk, tag, method):
    g = np.load(os.path.join(G, "kp_masked.npz"))
    h, w, seed, frac, thre, grid = g[tag + "_spec"]
    diff, flow, ddiff = DC.masked_kp_case(int(h), int(w), int(seed), float(frac))
    n, good, kp1, kp2 = run_masked(gpu, trk, flow, diff[..., 0], ddiff, int(grid), int(grid), 2000, float(thre), 0.05,
                                   {"flow": 0, "flow_ratio": 1}[method])
    check_against({"good_kp_found": True, "kp1_best": g[tag + "_kp1"], "kp2_best": g[tag + "_kp2"]}, n, good, kp1, kp2)


@pytest.mark.parametrize("case", ["empty_cells", "too_few_cells", "nan"])
@pytest.mark.parametrize("method", ["flow", "flow_ratio"])
def test_masked_local_bestn_crafted_maps(gpu, trk, case, method):
    h, w, nr, nc, N = 70, 100, 4, 5, 400
    thre = 0.1 if method == "flow" else 0.03
    diff, flow, ddiff = DC.masked_kp_case(h, w, 57, 0.5, nan_frac=0.05 if case == "nan" else 0.0)
    if case == "too_few_cells":  # the mask leaves one cell of twenty: fewer than a tenth
        keep = ddiff[40:50, 45:55].copy()
        ddiff[:] = 1.0
        ddiff[40:50, 45:55] = keep
    res = DC.local_bestN_masked(flow, diff, ddiff, num_bestN=N, num_row=nr, num_col=nc, thre=thre, depth_thre=0.05, score_method=method)
    n, good, kp1, kp2 = run_masked(gpu, trk, flow, diff[..., 0], ddiff, nr, nc, N, thre, 0.05, {"flow": 0, "flow_ratio": 1}[method])
    check_against(res, n, good, kp1, kp2)
    if case == "too_few_cells":
        assert good == 0
    else:
        assert good == 1 and 0 < n < T.local_bestN(flow, diff, num_bestN=N, num_row=nr, num_col=nc, thre=thre,
                                                   score_method=method)["kp1_best"].shape[1]
    if case == "empty_cells":  # the top-left cell is empty under the mask: no keypoint in it
        assert not ((kp1[:n, 0] < 20) & (kp1[:n, 1] < 17)).any()


def test_all_pass_mask_equals_the_plain_entry_point(gpu, trk):
    h, w, nr, nc, N = 70, 100, 4, 5, 400
    diff, flow, _ = DC.masked_kp_case(h, w, 58, 0.5)
    for score in (0, 1):
        n, good, kp1, kp2 = run_masked(gpu, trk, flow, diff[..., 0], np.zeros((h, w), np.float32), nr, nc, N, 0.1, 1.0, score)
        p1, p2 = np.full((N, 2), -7.0), np.full((N, 2), -7.0)
        pn, pg = C.c_int(), C.c_int()
        f, d = np.ascontiguousarray(flow), np.ascontiguousarray(diff[..., 0])
        gpu.check(gpu.lib().dfvo_kp_local_bestn_ex(trk, gpu.as_ptr(f), gpu.as_ptr(d), h, w, nr, nc, N, 0.1, score, gpu.as_ptr(p1),
                                                   gpu.as_ptr(p2), C.byref(pn), C.byref(pg)))
        assert (n, good) == (pn.value, pg.value) and good == 1 and n > 0
        assert np.array_equal(kp1, p1) and np.array_equal(kp2, p2)
