"""CPU: the motion / scene / coordinate matrix of tests/pose_world.py -- the generator itself, and which branch the ORACLE
takes on every case (tests/golden/pose_world_branches.json, regenerated here and compared), so that the GPU tests of the
same table (tests/test_pose_world_gpu.py) cannot pass by never entering a branch.

The coverage conditions below are conditions on the oracle alone.  All of them are met; none had to be dropped.  Two notes:
  * "E not found" inside compute_pose_2d2d needs five-point RANSAC to produce no model in 1000 iterations.  That happens
    when the two views are equal bit for bit (the car stands still, integer keypoint grid, zero flow): the reference then
    raises ValueError from `np.linalg.inv(K.T) @ None` in the repeat where it happens (cases still-*-e-none-*, and
    still-box-grid-exact with 1500 points, where it is the fifth repeat).
  * sklearn's ValueError ("RANSAC could not find a valid consensus set") is out of reach at the default residual threshold
    0.1: the least-squares coefficient of any three ratios is ~1 / (the largest of them), so the largest is an inlier of its
    own sample.  It is reached at the threshold 1e-3 that test_tracker_gpu.py::test_scale_recovery_sklearn_versions uses
    (signature key scale_tight)."""
import json
import os

import numpy as np
import pytest

import pose_world as PW
from synth import two_view

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "golden", "pose_world_branches.json")


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


@pytest.mark.parametrize("n,of,noise,seed", [(2000, 0.3, 0.15, 2002), (333, 0.6, 0.5, 9), (10, 0.0, 0.1, 12), (64, 0.2, 0.1, 11)])
def test_forward_box_float_is_two_view(n, of, noise, seed):
    x1, x2, R, t, K, o = two_view(n, of, noise, seed)
    c = PW.pose_case("forward", "box", "float", n, seed, of, noise)
    for a, b in ((x1, c["kp_ref"]), (x2, c["kp_cur"]), (R, c["R"]), (t, c["t"]), (K, c["K"]), (o, c["outliers"])):
        assert np.array_equal(a, b)
    x1, x2, R, t, K, o = two_view(500, 0.3, 0.15, 555, w=1920, h=1280)
    c = PW.pose_case("forward", "box", "float", 500, 555, 0.3, 0.15, w=1920, h=1280)
    assert np.array_equal(x1, c["kp_ref"]) and np.array_equal(x2, c["kp_cur"]) and np.array_equal(K, c["K"])


def test_case_table_is_well_formed():
    assert len(set(PW.CASE_IDS)) == len(PW.CASES)
    seen = {(c[1], c[2], c[3]) for c in PW.CASES if c[4] == 1500 and c[8] is None}
    for m in ("forward", "still", "creep", "pure_yaw", "sideways", "backward", "turn", "roll", "climb"):
        for s in PW.SCENES:
            for k in PW.COORDS:
                assert (m, s, k) in seen
    for m in ("forward", "still"):
        assert {c[8] for c in PW.CASES if c[1] == m and c[8]} == set(PW.DEGENERATE)
    for m, s in (("forward", "box"), ("still", "box"), ("forward", "ground")):
        counts = {c[4] for c in PW.CASES if c[1] == m and c[2] == s and c[8] is None}
        assert {5, 6, 7, 9, 10, 11, 63, 64, 65, 255, 256, 257, 1500, 2000} <= counts
    assert sum(c[4] == 20000 for c in PW.CASES) == 3


def test_generator_geometry():
    # zero rotation is the identity, exactly
    assert np.array_equal(PW.rotation((0, 0, 0)), np.eye(3))
    # grid coordinates: integer reference keypoints, float32 flow widened to double
    c = PW.pose_case("turn", "box", "grid", 500, 3, 0.3, 0.1)
    assert np.array_equal(c["kp_ref"], np.rint(c["kp_ref"]))
    flow = c["kp_cur"] - c["kp_ref"]
    assert np.abs(flow - flow.astype(np.float32)).max() <= 2 ** -18  # (the sum with a pixel index rounds once more in double)
    # standing still with no noise: the views are equal bit for bit
    c = PW.pose_case("still", "box", "grid", 500, 4, 0.0, 0.0)
    assert np.array_equal(c["kp_ref"].view(np.uint64), c["kp_cur"].view(np.uint64))
    # float coordinates, no noise, no outliers: the true motion has zero epipolar error, the ground plane one homography
    for motion in PW.MOTIONS:
        c = PW.pose_case(motion, "ground", "float", 300, 5, 0.0, 0.0)
        Kinv = np.linalg.inv(c["K"])
        a = Kinv @ np.c_[c["kp_ref"], np.ones(300)].T
        b = Kinv @ np.c_[c["kp_cur"], np.ones(300)].T
        tx = np.array([[0, -c["t"][2], c["t"][1]], [c["t"][2], 0, -c["t"][0]], [-c["t"][1], c["t"][0], 0]])
        assert np.abs(np.einsum("in,ij,jn->n", b, tx @ c["R"], a)).max() < 1e-12
        Hm = c["R"] + np.outer(c["t"], [0, 1.0 / PW.GROUND_Y, 0])  # X2 = (R + t n^T / d) X on the plane n.X = d
        q = Hm @ a
        assert np.abs(q[:2] / q[2] - b[:2]).max() < 1e-9
    # the depth maps agree with the geometry at the keypoints' pixels
    c = PW.pose_case("forward", "box", "grid", 3000, 6, 0.0, 0.0)
    assert (c["depth_cur"] > 0).sum() > 2000 and (c["depth_ref"] > 0).sum() > 2000 and (c["depth_ref"] == 70.0).any()


@pytest.mark.parametrize("case", PW.CASES, ids=PW.CASE_IDS)
def test_branch_signature_matches_committed_table(table, case):
    """the committed table regenerates identically from its generator (golden/make_golden_cases.py: pose_world_branches)"""
    got = json.loads(json.dumps(PW.signature(case)))
    assert got == table[case[0]], case[0]


def test_table_has_exactly_the_cases(table):
    assert sorted(table) == sorted(PW.CASE_IDS)


def test_branch_coverage(table):
    cov = PW.coverage(table)
    for k, v in cov.items():
        print("%-42s %3d  %s" % (k, len(v), ", ".join(v[:5])))
    for k, v in cov.items():
        if k != "nothing_found_anywhere":
            assert v, "no case of the matrix reaches: " + k
    # GRIC prefers the homography on the motions that produce no parallax and on the road-only scene
    hit = set(cov["gric_prefers_h_although_e_has_majority"])
    assert {"still-box-grid", "pure_yaw-box-grid", "forward-ground-grid", "still-box-n20000", "pure_yaw-box-n20000",
            "forward-ground-n20000"} <= hit
    # the all-collinear set is where the homography sampler gives up, at its first subset after 10000 attempts
    for cid in ("forward-one_row", "still-one_row"):
        assert table[cid]["h"] == dict(found=False, iters=0, gave_up=True, attempts=10000, inliers=0)
        assert table[cid]["raised"] == "AttributeError"  # homography_residual(None, ...)
    # a None essential matrix in the first, third and fifth repeat
    assert [len(table[c]["rep"]) for c in ("still-exact-n17-e-none-rep0", "still-exact-n18-e-none-rep2",
                                           "still-exact-n17-e-none-rep4")] == [1, 3, 5]
    # the cheirality count exactly at the 10 % gate: rejected (`good > n * 0.1`)
    s = table["nudge-shelf-n100-cheirality-at-gate"]
    assert s["major_valid"] and s["cheirality"] * 10 == s["n"] and not s["accepted"]
    # no more than a tenth of the matrix finds nothing at every stage
    assert len(cov["nothing_found_anywhere"]) <= len(table) // 10


def test_gpu_cases_stay_under_the_sampler_cap(table):
    """k_h_subsets is one lane; its run time is the number of sampler draws (10000 per rejected subset, up to 2000 subsets).
    Every case the GPU tests run needs fewer than MAX_GPU_ATTEMPTS draws on the oracle; a case above stays host_only."""
    for case in PW.CASES:
        att = table[case[0]]["h"]["attempts"]
        assert case[9] == (att >= PW.MAX_GPU_ATTEMPTS), (case[0], att)
