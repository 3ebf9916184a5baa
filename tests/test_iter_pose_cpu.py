"""CPU: the rigid_flow_pose of the iterative scale loop.  The device builds inv([R | t * scale]) in closed form
(sm::rigid_pose_inv_f32, df-vo_amd/csrc/np_legacy.h, called by k_iter_begin) where the reference calls np.linalg.inv; only the
float32 cast of it reaches the RigidFlow layer.  The function is compiled for the host with the solver units' -ffp-contract=off
(stand-alone program tests/host_harness/iter_pose_check.cpp, AddressSanitizer and UBSan) and compared on the poses of the five
committed rigid scenes x 2001 scales in [0, 5]: no element may differ."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "iter_pose_check.cpp")
DEPS = [SRC, os.path.join(HERE, "..", "df-vo_amd", "csrc", "np_legacy.h"), os.path.join(HERE, "..", "df-vo_amd", "csrc", "solver_math.h")]


@pytest.fixture(scope="module")
def checker():
    out_dir = os.path.join(HERE, "host_harness", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "iter_pose_check")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in DEPS):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                        "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    return exe


def unit_poses():
    """E-tracker poses (cur -> ref, unit translation) of the committed rigid scenes"""
    from synth import rigid_scene
    out = []
    for h, w, seed in ((192, 640, 61), (192, 640, 62), (120, 200, 63), (60, 100, 64), (48, 64, 65)):
        sc = rigid_scene(h, w, seed=seed)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = sc["R"], sc["t"]
        E = np.linalg.inv(T)
        E[:3, 3] /= np.linalg.norm(E[:3, 3])
        out.append(E)
    return out


@pytest.mark.parametrize("scales", [np.linspace(0.0, 5.0, 2001), np.array([-1.0])], ids=["0_to_5", "minus_one"])
def test_closed_form_inverse_equals_numpy_after_the_float32_cast(checker, tmp_path, scales):
    """(-1: the scale the loop carries on with when a round finds too few valid depth ratios, E_tracker.py:557-568)"""
    recs, want = [], []
    for E in unit_poses():
        for s in scales:
            recs.append(np.r_[E.ravel(), s])
            P = E.copy()
            P[:3, 3:] *= s  # rigid_flow_pose.t *= scale (E_tracker.py:533)
            want.append(np.linalg.inv(P).astype(np.float32))
    recs, want = np.asarray(recs, np.float64), np.asarray(want).reshape(-1, 16)
    assert recs.shape == (5 * len(scales), 17)
    src, dst = str(tmp_path / "poses.bin"), str(tmp_path / "inv.bin")
    with open(src, "wb") as f:
        f.write(np.int32(len(recs)).tobytes())
        f.write(recs.tobytes())
    r = subprocess.run([checker, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    got = np.fromfile(dst, np.float32).reshape(-1, 16)
    bad = (got != want).any(axis=1)
    print("closed-form inverse: %d of %d matrices differ from np.linalg.inv(...).astype(float32)" % (bad.sum(), len(bad)))
    assert not bad.any(), (recs[bad][:3], got[bad][:3], want[bad][:3])
