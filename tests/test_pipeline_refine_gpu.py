"""GPU: the trackers' iterative keypoint refinement in the fused pipeline (dfvo_pipeline_set_refine; TrackingPipeline's
e_iterative_kp / scale_iterative_kp / pnp_iterative_kp / *_iterative_score keys) against the oracle's chain
(tests/pipeline_refine_oracle.solve_pair, which tests/test_pipeline_refine_cpu.py holds to the reference's own DFVO.tracking()).

Model: test_pipeline_iterative_gpu.  Flow, consistency and depth maps are handed in as overrides (the raw reference depth is
depth_ref.astype(float32), the rolled-over one depth_cur.astype(float32)); three pairs run through one pipeline with the numpy
RandomState carried; pair 1 goes through prefetch_track.  After every pair: status, the tracked keypoints and pass one's inlier
mask, R, t bit for bit, the scale within 1e-9 relative, the PnP counts, the RandomState word for word -- and of the refinement
(get_refine): which passes ran, pass one's pose and scale, kp_depth of both frames and the second pass's inlier mask bit for bit,
the distance map bit for bit.  The cases and their expected values live in tests/pipeline_refine_cases.py (computed once)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from oracle import nets_torch as O
import pipeline_configs_oracle as PO
import pipeline_refine_cases as PC
import pipeline_refine_oracle as RO
from pipeline_configs_oracle import H, W
from test_pipeline_configs_gpu import run_case
from test_pipeline_iterative_gpu import Feed, _d, rel, same_rng

pytestmark = pytest.mark.gpu

E, PNP = 0, 3  # DFVO_TRACK_E, DFVO_TRACK_PNP


@pytest.fixture(scope="module")
def mods(gpu):
    return importlib.import_module("df-vo_amd.pipeline"), importlib.import_module("df-vo_amd.sequence")


@pytest.fixture(scope="module")
def weights():
    return O.liteflownet_state_dict(4869), O.monodepth2_state_dict(4869)


def make_pipe(pmod, weights, sc, o, ro):
    h, w = sc["diff"].shape
    feed_h, feed_w = (64, 96) if h == H else (192, 640)
    return pmod.TrackingPipeline(h, w, feed_h, feed_w, sc["K"], weights[0], weights[1], seed=4869, **o, **ro)


def check_refine(pipe, slot, r, frame):
    """dfvo_pipeline_get_refine's record against the helper's"""
    g = pipe.get_refine(slot, want_map=True)
    e_ran = r["sel_e"] is not None or (r["error"] == "empty" and r["pnp1"] is None and r["E1"] is not None)
    pnp_ran = r["pnp1"] is not None
    print("pair %d refine: e_ran %s scale_ran %s pnp_ran %s empty %s | kp_depth %d | scale1 %.12g scale2 %.12g" % (
        frame, g["e_ran"], g["scale_ran"], g["pnp_ran"], g["empty"], len(g["ref_kp"]), g["scale1"], g["scale2"]))
    assert g["e_ran"] == e_ran and g["pnp_ran"] == pnp_ran and g["empty"] == (r["error"] == "empty"), "pair %d" % frame
    assert g["scale_ran"] == (r["scale2"] is not None), "pair %d" % frame
    if r["E1"] is not None and pipe.refine_opts["e_iterative_kp"]:
        assert np.array_equal(g["R1"], r["E1"]["R"]) and np.array_equal(g["t1"].reshape(3, 1), r["E1"]["t"]), "pass one, pair %d" % frame
        if r["scale1"] is None:
            assert g["scale1"] == 0.0
        else:
            assert g["scale1"] == r["scale1"] or rel(g["scale1"], r["scale1"]), "pass one's scale, pair %d" % frame
    if r["scale2"] is not None:
        assert g["scale2"] == r["scale2"] or rel(g["scale2"], r["scale2"]), "second scale, pair %d" % frame
    if pnp_ran:
        found = r["pnp1"]["best_inlier"] > 0
        assert g["pnp_found1"] == found
        assert np.array_equal(g["pnp_R1"], r["pnp1"]["R"] if found else np.eye(3)), "PnP pass one, pair %d" % frame
        assert np.array_equal(g["pnp_t1"].reshape(3, 1), r["pnp1"]["t"] if found else np.zeros((3, 1)))
    if r["kp_depth"] is None:
        assert len(g["ref_kp"]) == 0
    else:
        assert np.array_equal(g["ref_kp"], r["kp_depth"][0]) and np.array_equal(g["cur_kp"], r["kp_depth"][1]), "kp_depth, pair %d" % frame
    if r["inliers2"] is None:
        assert len(g["inliers"]) == 0
    else:
        assert np.array_equal(g["inliers"], r["inliers2"]), "second pass's inlier mask, pair %d" % frame
    if r["mask"] is None:
        assert g["rigid_flow_diff"] is None or r["error"] == "empty"
    else:
        assert np.array_equal(g["rigid_flow_diff"], np.asarray(r["mask"], np.float32)), "distance map, pair %d" % frame
    return g


def check_pair(pipe, frame, out, want, slot=None):
    """one tracked pair against the oracle's (record, RandomState)"""
    r, rng = want
    slot = frame % 2 if slot is None else slot
    print("pair %d: status hip %d oracle %s | scale hip %.12g oracle %.12g | kp %d inliers %d pnp inliers %d" % (
        frame, out.status, r["status"], out.scale, r["scale"], out.n_kp, out.best_inlier_cnt, out.pnp_inliers))
    assert out.status == r["status"], "pair %d" % frame
    kp_ref, kp_cur, inl = pipe.get_keypoints(slot)
    assert out.good_kp_found == 1 and r["good_kp_found"] and out.n_kp == len(r["kp_ref"])
    assert np.array_equal(kp_ref, r["kp_ref"]) and np.array_equal(kp_cur, r["kp_cur"]), "keypoints, pair %d" % frame
    assert np.array_equal(inl, r["inliers"]), "pass one's inlier mask, pair %d" % frame
    R = np.array(out.R[:]).reshape(3, 3)
    t = np.array(out.t[:]).reshape(3, 1)
    if r["status"] == E:
        last = r["E2"] if r["E2"] is not None else r["E1"]
        assert np.array_equal(R, r["R"]) and np.array_equal(t, r["t"]), "pair %d" % frame
        assert out.best_inlier_cnt == last["best_inlier_cnt"]
        assert rel(out.scale, r["scale"])
    else:
        pnp = r["pnp"]
        assert r["status"] == PNP and out.pnp_n_filtered == len(pnp["kp1"]) and out.pnp_inliers == pnp["best_inlier"]
        assert np.array_equal(R, pnp["R"]) and np.array_equal(t, pnp["t"]), "pair %d" % frame
        rel_pose, mode = pipe.hybrid_pose(out, np.eye(4))
        assert mode == "PnP" and np.abs(rel_pose - pnp["pose"]).max() <= 1e-12
    g = check_refine(pipe, slot, r, frame)
    assert same_rng(pipe, rng), "RandomState diverged after pair %d" % frame
    return g


def run_chain(mods, weights, case):
    key, name, o, ro, zero = case
    sc = PC.scene_inputs(name)
    want = PC.chain(case)
    feed = Feed(sc, PC.depth_plan(sc, zero))
    pipe = make_pipe(mods[0], weights, sc, o, ro)
    recs = []
    try:
        feed.set_ref(pipe)
        for frame in range(3):
            recs.append(check_pair(pipe, frame, feed.track(pipe, frame), want[frame]))
    finally:
        pipe.close()
    return want, recs


@pytest.mark.parametrize("case", PC.PARITY, ids=[c[0] for c in PC.PARITY])
def test_refined_pipeline_matches_oracle_chain(gpu, mods, weights, case):
    want, _ = run_chain(mods, weights, case)
    assert all(r["error"] is None and (r["sel_e"] is not None or r["sel_pnp"] is not None) for r, _ in want), "a pair did not refine"


def test_the_parity_cases_exercise_the_refinement():
    """asserted on the oracle: every configuration has a pair whose final pose is not pass one's, the second scale differs from
    the first, the minus-one cases refine on [R | 0] and from a PnP without a model"""
    chains = {c[0]: [r for r, _ in PC.chain(c)] for c in PC.PARITY}
    for key in ("e-opt", "e-rigid", "e_scale-opt", "e_scale-rigid-tunnel", "e_scale-sampled"):
        assert all(r["status"] == E and not np.array_equal(r["E2"]["R"], r["E1"]["R"]) for r in chains[key]), key
    assert not np.array_equal(chains["e-opt"][0]["kp_depth"][0], chains["e-rigid"][0]["kp_depth"][0]), "the score changes nothing"
    assert all(r["scale2"] != r["scale1"] for r in chains["e_scale-opt"])
    for key in ("pnp-rigid", "pnp-opt"):
        assert all(r["status"] == PNP and not np.array_equal(r["pnp"]["pose"], r["pnp1"]["pose"]) for r in chains[key]), key
    m = chains["minus_one-rigid"]
    assert [r["status"] for r in m] == [PNP, PNP, E] and m[0]["scale1"] == -1 and m[0]["scale2"] == -1
    assert np.linalg.norm(m[1]["E2"]["t"]) == 0 and m[1]["pnp1"]["best_inlier"] == 0 and m[1]["sel_pnp"] is not None


def test_a_rejected_first_pass_refines_nothing(gpu, mods, weights):
    """validity 'flow' with a threshold nothing passes: E is rejected in pass one, so no selection, no second pass, no extra
    draw -- the PnP fallback with its 5 repeats on all three pairs, and get_refine says "not run" """
    want = PC.chain(PC.REJECTED_FIRST)
    assert all(r["status"] == PNP and r["sel_e"] is None and r["pnp1"] is None and np.linalg.norm(r["E1"]["t"]) == 0 for r, _ in want)
    _, recs = run_chain(mods, weights, PC.REJECTED_FIRST)
    assert all(not g["e_ran"] and not g["scale_ran"] and not g["pnp_ran"] and len(g["ref_kp"]) == 0 for g in recs)


def test_scale_minus_one_in_pass_one_still_refines(gpu, mods, weights):
    """a current depth of all zeros: pass one's scale is -1, the selection runs under inv([R | 0]); with scale_iterative_kp the
    second scale decides (-1 again: PnP), and pair 1, with the real depth, takes the E path on the second scale"""
    want = PC.chain(PC.MINUS_ONE_SCALE)
    r0, r1 = want[0][0], want[1][0]
    assert r0["scale1"] == -1 and r0["sel_e"] is not None and r0["scale2"] == -1 and r0["status"] == PNP
    assert np.array_equal(r0["sel_e"]["rigid_flow_pose"][:3, 3], np.zeros(3))
    assert r1["status"] == E and r1["scale"] == r1["scale2"] != r1["scale1"]
    _, recs = run_chain(mods, weights, PC.MINUS_ONE_SCALE)
    assert recs[0]["e_ran"] and recs[0]["scale_ran"] and recs[0]["scale1"] == -1.0 and recs[0]["scale2"] == -1.0


@pytest.mark.parametrize("case", [PC.REJECTED_SECOND, PC.REJECTED_SECOND_GRIC], ids=["ten_keypoints", "gric"])
def test_a_rejected_second_pass_takes_the_pnp_branch(gpu, mods, weights, case):
    want = PC.chain(case)
    assert all(np.linalg.norm(r["E1"]["t"]) != 0 and r["scale1"] != -1 and np.linalg.norm(r["E2"]["t"]) == 0 and r["status"] == PNP
               and r["scale2"] is None and r["sel_pnp"] is not None for r, _ in want)
    if case is PC.REJECTED_SECOND:
        assert all(len(r["sel_e"]["ref_kp"]) <= 10 for r, _ in want)
    run_chain(mods, weights, case)


@pytest.mark.parametrize("case", [PC.EMPTY, PC.EMPTY_PNP], ids=["e", "pnp"])
def test_empty_selection_is_an_error_code_and_the_pipeline_stays_usable(gpu, mods, weights, case):
    """rigid_flow_thre 1e-6 selects nothing: the oracle asserts.  track raises with DFVO_ERR_EMPTY_SELECTION, the RandomState is
    the oracle's at the raise (pass one's draws and no more), the depths are rolled; the same pipeline tracks the next pair, which
    ends the same way, from the carried RandomState"""
    key, name, o, ro, zero = case
    sc = PC.scene_inputs(name)
    want = PC.chain(case)
    assert all(r["error"] == "empty" for r, _ in want)
    feed = Feed(sc, PC.depth_plan(sc, zero))
    pipe = make_pipe(mods[0], weights, sc, o, ro)
    try:
        feed.set_ref(pipe)
        for frame in range(3):
            with pytest.raises(gpu.DfvoError, match="sampling threshold is too small") as e:
                feed.track(pipe, frame)
            assert e.value.code == gpu.ERR_EMPTY_SELECTION
            r, rng = want[frame]
            assert same_rng(pipe, rng), "RandomState at the raise, pair %d" % frame
            kp_ref, kp_cur, inl = pipe.get_keypoints(frame % 2)
            assert np.array_equal(kp_ref, r["kp_ref"]) and np.array_equal(inl, r["inliers"])
            g = check_refine(pipe, frame % 2, r, frame)
            assert g["empty"] and len(g["ref_kp"]) == 0
            ref_raw, ref_dep = pipe.get_ref_depth()
            assert np.array_equal(ref_dep, sc["depth_cur"]) and np.array_equal(ref_raw, sc["depth_cur"].astype(np.float32)), "roll-over"
    finally:
        pipe.close()


def test_set_refine_refusals(gpu, mods, weights):
    """DFVO_ERR_ARG with a message: bad flags, scale without E, a grid the launcher refuses, more kp_depth keypoints than the second
    scale stage takes, the iterative scale method or deep_pose beside it (either order of calls), a call after the first enqueue"""
    pmod = mods[0]
    sc = PC.scene_inputs("rigid")
    lib = gpu.lib()

    def ro(**kw):
        f = dict(e_enable=1, scale_enable=0, pnp_enable=0, e_score_rigid=0, pnp_score_rigid=1, num_row=10, num_col=10, num_bestN=2000,
                 rigid_flow_thre=5.0, optical_flow_thre=0.1)
        f.update(kw)
        return gpu.PipelineRefineOpts(**f)

    it = gpu.PipelineIterOpts(enable=1, kp_src=0, num_row=10, num_col=10, num_bestN=2000, rigid_flow_thre=5.0, optical_flow_thre=0.1)
    pipe = pmod.TrackingPipeline(H, W, 64, 96, sc["K"], weights[0], weights[1], seed=4869)
    try:
        for bad, msg in ((ro(e_enable=2), b"0 or 1"), (ro(e_enable=0, scale_enable=1), b"scale_enable without e_enable"),
                         (ro(e_enable=0), b"nothing enabled"), (ro(num_row=40, num_col=40), b"grid too large"),
                         (ro(num_bestN=99), b"n_best out of range"), (ro(num_row=1, num_col=1, num_bestN=200), b"does not fit in LDS"),
                         (ro(scale_enable=1, num_bestN=16400), b"16384"), (ro(num_col=0), b"positive"),
                         (ro(optical_flow_thre=float("nan")), b"NaN")):
            assert lib.dfvo_pipeline_set_refine(pipe.h, C.byref(bad)) == -2, msg  # DFVO_ERR_ARG
            assert msg in lib.dfvo_last_error(), lib.dfvo_last_error()
        assert lib.dfvo_pipeline_set_refine(pipe.h, None) == -2
        assert lib.dfvo_pipeline_set_refine(pipe.h, C.byref(ro(num_bestN=16400))) == 0  # (the bound is the second scale stage's)
        out = gpu.RefineOut()
        assert lib.dfvo_pipeline_get_refine(pipe.h, 0, C.byref(out), 0, None, None, None, None) == 0
        assert lib.dfvo_pipeline_set_iterative(pipe.h, C.byref(it)) == -2 and b"dfvo_pipeline_set_refine" in lib.dfvo_last_error()
        po = gpu.PipelineOpts(tracking_method=1)  # PnP-only tracking beside the E refinement
        po.flow_crop[1] = po.flow_crop[3] = 1.0
        assert lib.dfvo_pipeline_set_options(pipe.h, C.byref(po)) == -2 and b"no E-tracker runs" in lib.dfvo_last_error()
        assert lib.dfvo_pipeline_set_refine(pipe.h, C.byref(gpu.PipelineRefineOpts())) == 0  # all zero: off again
        assert lib.dfvo_pipeline_get_refine(pipe.h, 0, C.byref(out), 0, None, None, None, None) == -2
        assert lib.dfvo_pipeline_set_options(pipe.h, C.byref(po)) == 0
        assert lib.dfvo_pipeline_set_refine(pipe.h, C.byref(ro())) == -2 and b"no E-tracker runs" in lib.dfvo_last_error()
        assert lib.dfvo_pipeline_set_refine(pipe.h, C.byref(ro(e_enable=0, pnp_enable=1))) == 0
        assert lib.dfvo_pipeline_set_refine(pipe.h, C.byref(gpu.PipelineRefineOpts())) == 0
        assert lib.dfvo_pipeline_set_iterative(pipe.h, C.byref(it)) == 0
        assert lib.dfvo_pipeline_set_refine(pipe.h, C.byref(ro(e_enable=0, pnp_enable=1))) == -2
        assert b"dfvo_pipeline_set_iterative" in lib.dfvo_last_error()
        pipe.set_ref_depth(depth=_d(sc["depth_ref"]))
        with pytest.raises(gpu.DfvoError, match="before the first"):
            gpu.check(lib.dfvo_pipeline_set_refine(pipe.h, C.byref(ro())))
    finally:
        pipe.close()
    with pytest.raises(gpu.DfvoError, match="16384"):  # through the constructor: the pipeline is closed again
        pmod.TrackingPipeline(H, W, 64, 96, sc["K"], weights[0], weights[1], e_iterative_kp=True, scale_iterative_kp=True,
                              rigid_num_bestN=16400)
    with pytest.raises(ValueError, match="scale_recovery 'simple'"):
        pmod.TrackingPipeline(H, W, 64, 96, sc["K"], weights[0], weights[1], e_iterative_kp=True, scale_recovery="iterative")


def test_set_refine_is_refused_under_deep_pose(gpu, mods, weights):
    from test_deep_pose_gpu import _pose_weights
    pmod = mods[0]
    sc = PC.scene_inputs("rigid")
    lib = gpu.lib()
    pipe = pmod.TrackingPipeline(H, W, 64, 96, sc["K"], weights[0], weights[1], pose_sd=_pose_weights(False), seed=4869, pose_net=True,
                                 tracking_method="deep_pose")
    try:
        r = gpu.PipelineRefineOpts(pnp_enable=1, pnp_score_rigid=1, num_row=10, num_col=10, num_bestN=2000, rigid_flow_thre=5.0,
                                   optical_flow_thre=0.1)
        assert lib.dfvo_pipeline_set_refine(pipe.h, C.byref(r)) == -2 and b"runs no tracker to refine" in lib.dfvo_last_error()
    finally:
        pipe.close()
    with pytest.raises(ValueError, match="deep_pose"):
        pmod.TrackingPipeline(H, W, 64, 96, sc["K"], weights[0], weights[1], pose_sd=_pose_weights(False), pose_net=True,
                              tracking_method="deep_pose", pnp_iterative_kp=True)


def test_a_pipeline_without_the_setter_is_unchanged(gpu, mods, weights):
    """no refinement key: three pairs equal pipeline_configs_oracle.solve_pair (5 repeats, one pass), RandomState included --
    run_case asserts both; and a pipeline given the keys at their defaults equals it bit for bit"""
    pmod = mods[0]
    sc = PC.scene_inputs("tunnel")
    h, w = sc["diff"].shape
    a = run_case(pmod, weights, sc, {}, (E, E, E))
    b = run_case(pmod, weights, sc, {}, (E, E, E),
                 make_pipe=lambda: pmod.TrackingPipeline(h, w, 192, 640, sc["K"], weights[0], weights[1], seed=4869, **pmod.REFINE_DEFAULTS))
    for (sa, Ra, ta, ca, rnga), (sb, Rb, tb, cb, rngb) in zip(a, b):
        assert sa == sb and np.array_equal(Ra, Rb) and np.array_equal(ta, tb) and ca == cb
        assert np.array_equal(rnga[1], rngb[1]) and rnga[2] == rngb[2]
    rigid = PC.scene_inputs("rigid")
    run_case(pmod, weights, rigid, PC.opts("local_bestN", validity="flow", validity_thre=1e3), (PNP, PNP, PNP))


def test_from_images_without_overrides(gpu, mods, weights):
    """two pairs of seeded frames through sequence.track_chunk with the synthetic weights at 128 x 416, the thresholds opened so
    that the nets' maps select keypoints; the device's own flow, consistency and depth maps (get_outputs) then go through the
    helper with the PREVIOUS frame's depths on the reference side, and the device's pair equals it, refinement record and
    RandomState included.  (The flow of untrained weights on noise is no camera motion: what refines here is whichever branch the
    helper takes on those maps; the branches themselves are compared in the tests above.)"""
    pmod, smod = mods
    rng = np.random.Generator(np.random.PCG64(5))
    frames = smod.frames_to_device([rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(3)])
    K = PC.scene_inputs("rigid")["K"]
    o = dict(kp_thre=1e9, validity="flow", validity_thre=0.0)
    ro = PC.refine(e=True, s=True, p=True, score="rigid_flow", rigid_flow_thre=1e9, optical_flow_thre=1e9)
    pipe = pmod.TrackingPipeline(H, W, 64, 96, K, weights[0], weights[1], seed=4869, **o, **ro)
    pipe.enqueue_nets(3, frames[0], frames[0])  # depth of frame 0 exactly as the device computes it
    pipe.sync()
    raw0, dep0 = pipe.get_outputs(3)[3:5]
    ref = {"raw": raw0, "dep": dep0}
    np.random.seed(4869)
    seen = []

    def collect(j, out):
        slot = j % smod.SLOTS
        fwd, bwd, diff, raw, dep = pipe.get_outputs(slot)
        ref_raw, ref_dep = pipe.get_ref_depth()
        assert raw.any() and np.array_equal(ref_raw, raw) and np.array_equal(ref_dep, dep), "roll-over behind pair %d" % j
        r = RO.solve_pair(o, ro, fwd, diff, dep, ref["dep"], ref["raw"], K)
        assert r["error"] is None and r["good_kp_found"]
        g = check_pair(pipe, j, out, (r, np.random.get_state()), slot=slot)
        ref["raw"], ref["dep"] = raw, dep
        seen.append((out.status, g["e_ran"] or g["pnp_ran"]))

    try:
        rel_pose, status = smod.track_chunk(pipe, frames, 0, 2, collect=collect)
        assert len(seen) == 2 and list(status) == [s for s, _ in seen] and all(ran for _, ran in seen)
    finally:
        pipe.close()
