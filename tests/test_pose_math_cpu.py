"""CPU: the pose net's 6 -> 4x4 arithmetic (df-vo_amd/csrc/pose_math.h, run on the device by k_pose_head) compiled for the
host as a stand-alone program (tests/host_harness/pose_math_check.cpp, AddressSanitizer and UBSan) against the torch-CPU
float32 transformation_from_parameters(invert=True): the reference's own function, recorded in tests/golden/posenet_64x96.npz
by tests/golden/make_golden_posenet.py, and the tests' restatement of it (posenet_ref.transformation_inverted).

Bound: 16 * 2^-24 absolute on the rotation entries -- each is a sum of at most three products of sin / cos-class values, each
within about 2 ulp of 1 --, and the same bound relative to |t| on the translation column."""
import os
import subprocess

import numpy as np
import pytest
import torch

import posenet_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "pose_math_check.cpp")
DEPS = [SRC, os.path.join(HERE, "..", "df-vo_amd", "csrc", "pose_math.h")]
BOUND = 16 * 2.0 ** -24


@pytest.fixture(scope="module")
def checker():
    out_dir = os.path.join(HERE, "host_harness", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pose_math_check")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in DEPS):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-fast-math", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    return exe


def host_pose(checker, params, mult):
    """pose_from_parameters of every row of `params` ([n, 6] float32) -> [n, 4, 4] float32"""
    params = np.asarray(params, np.float32).reshape(-1, 6)
    text = "".join("%.9g %s\n" % (mult, " ".join("%.9g" % v for v in p)) for p in params)
    r = subprocess.run([checker], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [[int(t, 16) for t in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(params)
    return np.asarray(rows, np.uint32).view(np.float32).reshape(-1, 4, 4)


def check_pose(name, got, want, params):
    """the module's bound: absolute on the rotation, relative to |t| on the translation; the last row exact"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    e_rot = np.abs(got[:3, :3] - want[:3, :3]).max()
    tn = float(np.linalg.norm(np.asarray(params, np.float64)[3:]))
    e_t = np.abs(got[:3, 3] - want[:3, 3]).max()
    print("%s: max |dR| %.3e (bound %.3e), max |dt| %.3e (bound %.3e)" % (name, e_rot, BOUND, e_t, BOUND * tn))
    assert e_rot <= BOUND, (name, e_rot)
    assert e_t <= BOUND * tn, (name, e_t, tn)
    assert np.array_equal(got[3], [0, 0, 0, 1])


def test_host_build_matches_transformation_from_parameters(checker):
    g = np.load(os.path.join(HERE, "golden", "posenet_64x96.npz"))
    assert np.array_equal(g["math_params"], np.asarray(PR.MATH_CASES, np.float32))
    got = host_pose(checker, PR.MATH_CASES, 1.0)
    for i, p in enumerate(np.asarray(PR.MATH_CASES, np.float32)):
        check_pose("case %d vs the reference's function" % i, got[i], g["math_pose"][i], p)
        check_pose("case %d vs the restatement" % i, got[i], PR.transformation_inverted(torch.from_numpy(p)).numpy(), p)
    # the net's own prediction on the fixture's image pair
    p = np.concatenate([g["axisangle"][0, 0, 0], g["translation"][0, 0, 0]]).astype(np.float32)
    check_pose("the fixture's prediction", host_pose(checker, p, 1.0)[0], g["pose"][0], p)


def test_zero_angle_is_the_identity_rotation(checker):
    got = host_pose(checker, [[0, 0, 0, 0.01, -0.02, 0.03]], 1.0)[0]
    assert np.array_equal(got[:3, :3], np.eye(3, dtype=np.float32))
    assert np.array_equal(got[:3, 3], np.asarray([-0.01, 0.02, -0.03], np.float32))


def test_multiplier_scales_the_translation_only(checker):
    one = host_pose(checker, PR.MATH_CASES, 1.0)
    kitti = host_pose(checker, PR.MATH_CASES, 5.4)
    assert np.array_equal(one[:, :, :3], kitti[:, :, :3]) and np.array_equal(one[:, 3], kitti[:, 3])
    assert np.array_equal(kitti[:, :3, 3], one[:, :3, 3] * np.float32(5.4))
