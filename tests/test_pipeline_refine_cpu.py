"""CPU: the trackers' iterative keypoint refinement (the iterative_kp blocks of e_tracker / scale_recovery / pnp_tracker) in the fused
pipeline's host layer and its oracle:
  - tests/pipeline_refine_oracle.solve_pair, the GPU test's expected values, against the reference's own DFVO.tracking()
    (tests/golden/iterative_kp.npz, written by tests/golden/make_golden_iterative_kp.py) on every stored quantity, and what the
    cases exercise;
  - pipeline.options_from_cfg on the accepted combinations and on every refusal, check_refine_options' value checks;
  - the PnP hand-over's rigid_flow_pose: np.linalg.inv(np.linalg.inv(X)).astype(float32) against the device's formula
    (sm::rigid_pose_f32, compiled for the host);
  - the rules of dfvo_pipeline_set_refine as a stand-alone program under AddressSanitizer and UBSan
    (tests/host_harness/pipeline_refine_check.cpp)."""
import importlib
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from test_pipeline_options_cpu import default_cfg, uniform

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_iterative_kp as MG  # noqa: E402
import pipeline_refine_oracle as RO  # noqa: E402

SRC = os.path.join(HERE, "host_harness", "pipeline_refine_check.cpp")
CSRC = os.path.join(HERE, "..", "df-vo_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "np_legacy.h"), os.path.join(CSRC, "pipeline_setup.h"), os.path.join(HERE, "..", "include", "dfvo_hip.h")]


@pytest.fixture(scope="module")
def pmod():
    import __graft_entry__ as g
    g.dfvo_amd()
    return importlib.import_module("df-vo_amd.pipeline")


@pytest.fixture(scope="module")
def checker():
    out_dir = os.path.join(HERE, "host_harness", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pipeline_refine_check")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in DEPS):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                        "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    return exe


# ---- the oracle helper against the reference's DFVO.tracking() -------------------------------------------------------------
def case_options(name, score):
    e, s, p, method, _ = MG.CONFIGS[name]
    o = dict(validity=MG.VALIDITY[0], validity_thre=MG.VALIDITY[1], tracking_method=method)
    ro = dict(e_iterative_kp=e, scale_iterative_kp=s, pnp_iterative_kp=p, e_iterative_score=score, pnp_iterative_score=score,
              rigid_flow_thre=MG.RIGID_FLOW_THRE)
    return o, ro


_runs = {}


def fixture_run(case):
    """the helper's two consecutive pairs of a fixture case, once: [(record, RandomState words after)]"""
    tag, h, w, seed, name, score = case
    if tag not in _runs:
        import make_golden as G
        c = G.rigid_case(h, w, seed)
        o, ro = case_options(name, score)
        depth_cur = np.zeros_like(c["depth_cur"]) if MG.CONFIGS[name][4] else c["depth_cur"]
        ref_depth, ref_raw = c["raw_depth"].astype(np.float64), c["raw_depth"]
        np.random.seed(4869 + seed)
        out = []
        for _ in range(2):
            r = RO.solve_pair(o, ro, c["flow"], c["diff"], depth_cur, ref_depth, ref_raw, c["K"])
            out.append((r, RO.rng_words()))
            ref_depth, ref_raw = depth_cur, c["depth_cur"].astype(np.float32)
        _runs[tag] = out
    return _runs[tag]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "iterative_kp.npz"))


@pytest.mark.parametrize("case", MG.cases(), ids=[c[0] for c in MG.cases()])
def test_oracle_helper_equals_the_reference_tracking(golden, case):
    tag, name = case[0], case[4]
    for call, (r, rng) in enumerate(fixture_run(case)):
        k = "%s_c%d" % (tag, call)
        assert r["error"] is None
        pose, mode = RO.hybrid_pose(r)
        assert (mode == "PnP") == bool(golden[k + "_pnp"]), k
        assert np.array_equal(pose, golden[k + "_pose"]), (k, pose, golden[k + "_pose"])
        kr, kc = r["kp_depth"]
        assert np.array_equal(kr, golden[k + "_kp_ref"].astype(np.float64)), k
        assert zlib.crc32(np.ascontiguousarray(kc, np.float64).tobytes()) == int(golden[k + "_kp_cur_crc"]), k
        n_inl = int(golden[k + "_n_inliers"])
        if MG.CONFIGS[name][3] == "PnP":
            assert n_inl == -1 and r["E1"] is None
        else:
            inl = r["inliers2"] if r["inliers2"] is not None else r["inliers"]
            assert len(inl) == n_inl and np.array_equal(np.packbits(inl), golden[k + "_inliers"]), k
        assert zlib.crc32(np.ascontiguousarray(r["mask"], np.float32).tobytes()) == int(golden[k + "_mask_crc"]), k
        assert np.array_equal(rng, golden[k + "_rng_after"]), "RandomState after " + k


def test_the_fixture_cases_exercise_the_refinement():
    """asserted on the helper (which the test above holds to the reference): per configuration a pair whose final pose is not
    pass one's; pass one's scale -1 with the E refinement still running on [R | 0] and the PnP branch refining; a PnP refinement
    from the identity (no model: the rolled-over depth is all zero)"""
    runs = {c[0]: (c[4], fixture_run(c)) for c in MG.cases()}
    for name in ("e", "e_scale", "minus_one"):
        assert any(r["E2"] is not None and not (np.array_equal(r["E2"]["R"], r["E1"]["R"]) and np.array_equal(r["E2"]["t"], r["E1"]["t"]))
                   for n, run in runs.values() if n == name for r, _ in run), name
    for name in ("pnp", "minus_one"):
        assert any(r["pnp1"] is not None and not np.array_equal(r["pnp"]["pose"], r["pnp1"]["pose"])
                   for n, run in runs.values() if n == name for r, _ in run), name
    assert any(r["scale2"] is not None and r["scale2"] != r["scale1"] for n, run in runs.values() if n == "e_scale" for r, _ in run)
    minus = [r for n, run in runs.values() if n == "minus_one" for r, _ in run]
    assert all(r["scale1"] == -1 and r["sel_e"] is not None and r["E2"] is not None and r["status"] == 3 for r in minus)
    assert all(np.array_equal(r["sel_e"]["rigid_flow_pose"][:3, 3], np.zeros(3)) for r in minus)
    assert any(np.array_equal(r["pnp1"]["pose"], np.eye(4)) and r["sel_pnp"] is not None for r in minus)


def test_a_second_pass_on_ten_keypoints_is_rejected():
    """thresholds that leave 10 or fewer kp_depth keypoints (found with the helper): under GRIC compute_pose_2d2d needs more
    than 10 (E_tracker.py:196), so the second pass returns t = 0 and the pair takes the PnP branch"""
    import pipeline_refine_cases as PC
    for r, _ in PC.chain(PC.REJECTED_SECOND):
        assert np.linalg.norm(r["E1"]["t"]) != 0 and r["scale1"] != -1
        assert 0 < len(r["sel_e"]["ref_kp"]) <= 10 and np.linalg.norm(r["E2"]["t"]) == 0 and r["scale2"] is None and r["status"] == 3
        assert r["sel_pnp"] is not None and r["pnp"]["best_inlier"] > 0
    gric = [r for r, _ in PC.chain(PC.REJECTED_SECOND_GRIC)]  # hundreds of keypoints, rejected by the validity rule itself
    assert all(len(r["sel_e"]["ref_kp"]) > 100 and np.linalg.norm(r["E2"]["t"]) == 0 and r["status"] == 3 for r in gric)


# ---- options_from_cfg ---------------------------------------------------------------------------------------------------------
def refine_cfg(e=False, s=False, p=False):
    c = default_cfg()
    c.kp_selection.rigid_flow_kp.enable = True
    c.e_tracker.iterative_kp.enable, c.scale_recovery.iterative_kp.enable, c.pnp_tracker.iterative_kp.enable = e, s, p
    return c


def test_accepted_combinations_map_to_the_refinement_keys(pmod):
    assert pmod.options_from_cfg(default_cfg()) == {}
    assert pmod.options_from_cfg(refine_cfg(e=True)) == {"e_iterative_kp": True}
    assert pmod.options_from_cfg(refine_cfg(e=True, s=True)) == {"e_iterative_kp": True, "scale_iterative_kp": True}
    assert pmod.options_from_cfg(refine_cfg(p=True)) == {"pnp_iterative_kp": True}
    assert pmod.options_from_cfg(refine_cfg(e=True, s=True, p=True)) == {"e_iterative_kp": True, "scale_iterative_kp": True,
                                                                         "pnp_iterative_kp": True}
    c = refine_cfg(e=True, p=True)
    c.e_tracker.iterative_kp.score_method = "rigid_flow"
    c.pnp_tracker.iterative_kp.score_method = "opt_flow"
    c.kp_selection.rigid_flow_kp.num_bestN = 1500
    c.kp_selection.rigid_flow_kp.num_col = 5
    c.kp_selection.rigid_flow_kp.rigid_flow_thre = 3
    c.e_tracker.ransac.repeat = 4
    assert pmod.options_from_cfg(c) == {"e_iterative_kp": True, "pnp_iterative_kp": True, "e_iterative_score": "rigid_flow",
                                        "pnp_iterative_score": "opt_flow", "rigid_num_bestN": 1500, "rigid_num_col": 5,
                                        "rigid_flow_thre": 3, "e_repeat": 4}
    c = refine_cfg(p=True)  # PnP-only tracking; the E-tracker's blocks are not read there (dfvo.py:165)
    c.tracking_method = "PnP"
    assert pmod.options_from_cfg(c) == {"tracking_method": "PnP", "pnp_iterative_kp": True}
    c.e_tracker.iterative_kp.enable = True
    assert pmod.options_from_cfg(c) == {"tracking_method": "PnP", "pnp_iterative_kp": True}
    for source, edit in (("sampled", uniform),):  # any tracked keypoint source
        c = refine_cfg(e=True)
        edit(c)
        assert pmod.options_from_cfg(c) == {"kp_source": source, "e_iterative_kp": True}
    c = refine_cfg(e=True)
    c.kp_selection.local_bestN.enable, c.kp_selection.bestN.enable = False, True
    assert pmod.options_from_cfg(c) == {"kp_source": "bestN", "e_iterative_kp": True}
    c = refine_cfg(e=True)
    c.depth.depth_src = "gt"
    assert pmod.options_from_cfg(c) == {"depth_source": "external", "e_iterative_kp": True}
    assert not set(pmod.REFINE_DEFAULTS) & (set(pmod.ITER_DEFAULTS) | set(pmod.OPTION_DEFAULTS) | set(pmod.DEFAULTS))


def _edit(c, path, value):
    node = c
    keys = path.split(".")
    for k in keys[:-1]:
        node = node[k]
    node[keys[-1]] = value


REFUSALS = [
    # (what is enabled, further edits, the path the message names)
    (dict(e=True), [("scale_recovery.method", "iterative")], "e_tracker.iterative_kp.enable"),
    (dict(e=True, s=True), [("scale_recovery.method", "iterative"), ("e_tracker.iterative_kp.enable", False)],
     "scale_recovery.iterative_kp.enable"),
    (dict(p=True), [("scale_recovery.method", "iterative")], "pnp_tracker.iterative_kp.enable"),
    (dict(e=True), [("e_tracker.kp_src", "kp_depth")], "e_tracker.kp_src"),
    (dict(p=True), [("pnp_tracker.kp_src", "kp_depth")], "pnp_tracker.kp_src"),
    (dict(e=True), [("scale_recovery.kp_src", "kp_depth")], "scale_recovery.kp_src"),
    (dict(e=True), [("e_tracker.iterative_kp.kp_src", "kp_best")], "e_tracker.iterative_kp.kp_src"),
    (dict(e=True, s=True), [("scale_recovery.iterative_kp.kp_src", "kp_best")], "scale_recovery.iterative_kp.kp_src"),
    (dict(p=True), [("pnp_tracker.iterative_kp.kp_src", "kp_list")], "pnp_tracker.iterative_kp.kp_src"),
    (dict(s=True), [], "scale_recovery.iterative_kp.enable"),
    (dict(), [], "kp_selection.rigid_flow_kp.enable"),
    (dict(e=True), [("kp_selection.rigid_flow_kp.enable", False)], "e_tracker.iterative_kp.enable"),
    (dict(e=True, s=True), [("kp_selection.rigid_flow_kp.enable", False), ("e_tracker.iterative_kp.enable", False)],
     "scale_recovery.iterative_kp.enable"),
    (dict(p=True), [("kp_selection.rigid_flow_kp.enable", False)], "pnp_tracker.iterative_kp.enable"),
    (dict(e=True), [("tracking_method", "deep_pose"), ("deep_pose.enable", True)], "e_tracker.iterative_kp.enable"),
    (dict(p=True), [("tracking_method", "deep_pose"), ("deep_pose.enable", True)], "pnp_tracker.iterative_kp.enable"),
    (dict(e=True), [("tracking_method", "PnP")], "kp_selection.rigid_flow_kp.enable"),  # (nothing reads it: no E-tracker runs)
    (dict(e=True), [("online_finetune.enable", True)], "online_finetune.enable"),
]


@pytest.mark.parametrize("on,edits,path", REFUSALS, ids=["%d-%s" % (i, r[2]) for i, r in enumerate(REFUSALS)])
def test_what_stays_refused_names_its_path(pmod, on, edits, path):
    c = refine_cfg(**on)
    for p, v in edits:
        _edit(c, p, v)
    with pytest.raises(NotImplementedError) as e:
        pmod.options_from_cfg(c)
    assert path in str(e.value), str(e.value)


def test_check_refine_options(pmod):
    chk = pmod.check_refine_options
    base, io = dict(pmod.REFINE_DEFAULTS), dict(pmod.ITER_DEFAULTS)
    assert chk(base) is None and chk(base, io) is None
    f = chk(dict(base, e_iterative_kp=True, scale_iterative_kp=True, pnp_iterative_kp=True), dict(io, rigid_num_bestN=1500, rigid_flow_thre=3))
    assert f == dict(e_enable=1, scale_enable=1, pnp_enable=1, e_score_rigid=0, pnp_score_rigid=1, num_row=10, num_col=10, num_bestN=1500,
                     rigid_flow_thre=3.0, optical_flow_thre=0.1)
    assert chk(dict(base, pnp_iterative_kp=True, pnp_iterative_score="opt_flow"), io, "PnP")["pnp_score_rigid"] == 0
    bad = [
        (dict(e_iterative_kp=1), {}, "hybrid", "e_iterative_kp"), (dict(pnp_iterative_kp="yes"), {}, "hybrid", "pnp_iterative_kp"),
        (dict(scale_iterative_kp=None), {}, "hybrid", "scale_iterative_kp"),
        (dict(e_iterative_kp=True, e_iterative_score="flow"), {}, "hybrid", "e_iterative_score"),
        (dict(pnp_iterative_score="rigid"), {}, "hybrid", "pnp_iterative_score"),
        (dict(scale_iterative_kp=True), {}, "hybrid", "without e_iterative_kp"),
        (dict(e_iterative_kp=True), dict(scale_recovery="iterative"), "hybrid", "scale_recovery 'simple'"),
        (dict(pnp_iterative_kp=True), {}, "deep_pose", "deep_pose"), (dict(e_iterative_kp=True), {}, "PnP", "no E-tracker"),
        (dict(e_iterative_kp=True), dict(rigid_num_row=0), "hybrid", "rigid_num_row"),
        (dict(e_iterative_kp=True), dict(rigid_num_bestN=99), "hybrid", "rigid_num_bestN"),
        (dict(pnp_iterative_kp=True), dict(rigid_flow_thre=float("nan")), "hybrid", "rigid_flow_thre"),
        (dict(pnp_iterative_kp=True), dict(optical_flow_thre=None), "hybrid", "optical_flow_thre"),
    ]
    for ro, iov, tracking, word in bad:
        with pytest.raises(ValueError) as e:
            chk(dict(base, **ro), dict(io, **iov), tracking)
        assert word in str(e.value), (ro, iov, str(e.value))
    with pytest.raises(ValueError, match="scale_iterative_kp"):  # the constructor checks before it touches the device
        pmod.TrackingPipeline(128, 416, 64, 96, np.eye(3), {}, {}, scale_iterative_kp=True)


# ---- the host program -----------------------------------------------------------------------------------------------------------
def test_set_refine_rules_host_program(checker):
    r = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "pipeline_refine: ok" in r.stdout, r.stdout[-4000:]


def pnp_hand_over_poses():
    """X = [Rodrigues(r) | t] of every PnP first pass the GPU cases and the fixture cases refine from, and 4000 seeded rigid poses"""
    from oracle import cv2_shim as cv2
    out = []
    for c in MG.cases():
        out += [(r["pnp1"]["R"], r["pnp1"]["t"]) for r, _ in fixture_run(c) if r["pnp1"] is not None]
    import pipeline_refine_cases as PC
    out += PC.gpu_case_pnp_poses()
    n_cases = len(out)
    rng = np.random.Generator(np.random.PCG64(20))
    for i in range(4000):
        rv = rng.standard_normal(3) * (10.0 ** rng.uniform(-4, 0.4))
        out.append((cv2.Rodrigues(rv.reshape(3, 1))[0], rng.standard_normal(3) * (10.0 ** rng.uniform(-3, 2))))
    out.append((np.eye(3), np.zeros(3)))  # no model found
    return out, n_cases


def test_pnp_hand_over_pose_equals_the_double_inverse_after_the_float32_cast(checker, tmp_path):
    poses, n_cases = pnp_hand_over_poses()
    assert n_cases > 0
    recs, want = [], []
    for R, t in poses:
        X = np.eye(4)
        X[:3, :3], X[:3, 3] = R, np.asarray(t).reshape(3)
        recs.append(np.r_[np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel()])
        want.append(np.linalg.inv(np.linalg.inv(X)).astype(np.float32))  # pnp_tracker.py:118, then :136
    recs, want = np.asarray(recs, np.float64), np.asarray(want).reshape(-1, 16)
    src, dst = str(tmp_path / "poses.bin"), str(tmp_path / "T.bin")
    with open(src, "wb") as f:
        f.write(np.int32(len(recs)).tobytes())
        f.write(recs.tobytes())
    r = subprocess.run([checker, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    got = np.fromfile(dst, np.float32).reshape(-1, 16)
    bad = (got != want).any(axis=1)
    print("PnP hand-over: %d of %d matrices differ from inv(inv(X)).astype(float32) (%d of the %d the cases rest on)"
          % (bad.sum(), len(bad), bad[:n_cases].sum(), n_cases))
    assert not bad[:n_cases].any(), "a GPU case rests on a pose where the device's formula is not numpy's"
    assert not bad.any(), (recs[bad][:3], got[bad][:3], want[bad][:3])
