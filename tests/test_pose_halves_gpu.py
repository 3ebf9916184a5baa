"""GPU: the two halves of a pair's pose stage (enqueue_pose_h_part: findHomography + refinement + GRIC-H, run ahead behind the
nets; enqueue_pose_e_part: the RandomState-ordered chain) meet where the chain first reads the homography -- in front of the
validity bookkeeping -- and not at the chain's start.  In the lane layout the five-point batch shares the chain's stream, so
only that one wait orders the bookkeeping behind the homography half.

One process, two pipelines per case (DFVO_STREAM_LAYOUT=lanes and =wide, read by dfvo_pipeline_create).  Each runs three
pairs with the pre-part prefetched behind the nets and three with it left to track_begin; the late pre-part is one stream in
strict order and serves as the reference.  Flow / consistency / depth maps are synthetic.rigid_scene overrides (the nets'
size does not matter), on the smallest frame the pipeline tests build (128 x 416); GRIC accepts E on no 128 x 416 ramp
scene, so the default settings also run on pipeline_configs_oracle.tunnel_inputs (192 x 640).  Compared bit for bit: pose,
status, keypoints, inlier mask and counts, scale fields, PnP fields, the RandomState.  The last test drives the coded frames
of tests/stream_layout_child.py (the nets' own outputs, features carried, every slot reused) through both layouts."""
import importlib
import zlib

import numpy as np
import pytest
import torch

from oracle import nets_torch as O
from synth import coded_tunnel_sequence, crafted_liteflownet_state_dict, crafted_monodepth2_state_dict, rigid_scene
import pipeline_configs_oracle as PO
from pipeline_configs_oracle import H, W

pytestmark = pytest.mark.gpu

E, PNP = 0, 3  # DFVO_TRACK_E, DFVO_TRACK_PNP
SLOTS = 4
LAYOUTS = ("lanes", "wide")
OUT_FIELDS = ("scale", "status", "n_kp", "good_kp_found", "best_inlier_cnt", "num_valid", "cheirality", "scale_n_valid",
              "scale_n_trials", "scale_n_inliers", "pnp_found", "pnp_inliers", "pnp_n_filtered")


@pytest.fixture(scope="module")
def pmod(gpu):
    return importlib.import_module("df-vo_amd.pipeline")


@pytest.fixture(scope="module")
def weights():
    return O.liteflownet_state_dict(4869), O.monodepth2_state_dict(4869)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def few_keypoints(sc, cells, rows, cols):
    """`sc` with a consistency map that passes the threshold at one pixel in each of the first `cells` cells of a rows x cols
    grid: with one keypoint per cell asked for, local_bestN selects exactly `cells` keypoints"""
    h, w = sc["diff"].shape
    diff = np.full((h, w), 2.0, np.float32)
    for c in range(cells):
        r, q = divmod(c, cols)
        diff[int(h / rows * r) + 3, int(w / cols * q) + 5] = 0.01
    return dict(sc, diff=diff)


_scenes = {}


def scene(name):
    """the inputs of a case, computed once and never modified"""
    if name not in _scenes:
        if name == "rigid":
            _scenes[name] = rigid_scene(H, W, seed=3 + H)
        elif name == "tunnel":
            _scenes[name] = PO.tunnel_inputs()
        elif name == "ten":  # 10 cells of the default 10 x 10 grid
            _scenes[name] = few_keypoints(scene("rigid"), 10, 10, 10)
        elif name == "three":  # 3 cells of a 2 x 2 grid
            _scenes[name] = few_keypoints(scene("rigid"), 3, 2, 2)
    return _scenes[name]


def make_pipe(pmod, layout, h, w, feed, K, fsd, dsd, monkeypatch, **o):
    monkeypatch.setenv("DFVO_STREAM_LAYOUT", layout)
    for k in ("DFVO_STREAM_POOL", "DFVO_STREAM_POOL_FORCE_FAIL", "DFVO_FLOW_INSTANCES"):
        monkeypatch.delenv(k, raising=False)
    pipe = pmod.TrackingPipeline(h, w, feed[0], feed[1], K, fsd, dsd, seed=4869, **o)
    lay = pipe.stream_layout()
    if lay["layout"] != layout:
        pipe.close()
        pytest.fail("asked for the %s layout, got: %s" % (layout, lay["text"]))
    return pipe, lay


def differing(a, b):
    """the fields in which two runs' (rows, RandomState CRC) differ, for the assertion message"""
    d = ["pair %d %s: %s != %s" % (k, f, ra[f], rb[f]) for k, (ra, rb) in enumerate(zip(a[0], b[0])) for f in ra if ra[f] != rb.get(f)]
    return d + (["RandomState"] if a[1] != b[1] else []) + (["row count"] if len(a[0]) != len(b[0]) else [])


def pair_row(pipe, slot, out, batch_ran=True):
    """batch_ran = False: the pair had too few keypoints for the five-point batch.  compute_pose_2d2d returns before recoverPose
    there (E_tracker.py:196), so the pipeline's T21 is the previous pair's and scale_n_valid, the number of depth ratios the
    gated scale stage counted under it, is a number the reference does not have: it is left out of the row"""
    kp_ref, kp_cur, inl = pipe.get_keypoints(slot)
    row = {f: getattr(out, f) for f in OUT_FIELDS if batch_ran or f != "scale_n_valid"}
    row["scale"] = np.float64(out.scale).tobytes().hex()
    row["R"] = np.array(out.R[:]).tobytes().hex()
    row["t"] = np.array(out.t[:]).tobytes().hex()
    row["kp"] = (len(kp_ref), crc(kp_ref), crc(kp_cur), crc(inl))
    return row


def run_overrides(pipe, sc, prefetch, depth_of_pair=None, validity="GRIC"):
    """three pairs of `sc` as overrides through `pipe` from a fresh seed; the rows and the RandomState's CRC"""
    h, w = sc["diff"].shape
    rng = np.random.Generator(np.random.PCG64(11))
    dref, dcur = (_d(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(2))  # (the nets' outputs are overridden)
    dflow, ddiff, ddepth = _d(sc["flow"]), _d(sc["diff"]), _d(sc["depth_cur"])
    dzero = torch.zeros_like(ddepth)
    pipe.seed(4869)
    pipe.set_ref_depth(depth=_d(sc["depth_ref"]))
    rows = []
    for k in range(3):
        slot = k % SLOTS
        pipe.enqueue_nets(slot, dref, dcur)
        if prefetch:
            pipe.prefetch_track(slot, dflow, ddiff)
        pipe.track_begin(slot, dflow, ddiff, dzero if depth_of_pair == ("zero", k) else ddepth)
        out = pipe.track_end(slot)
        rows.append(pair_row(pipe, slot, out, out.n_kp > 10 if validity == "GRIC" else out.n_kp >= 5))
    pipe.sync()
    return rows, crc(pipe.get_rng_state()[1])


# (scene, options, depth override rule, what the pairs have to be: None = any)
CASES = {
    # GRIC on the ramp scene: the homography wins, E is rejected in the bookkeeping, every pair takes the PnP fallback
    "default": ("rigid", {}, None, dict(status=(PNP, PNP, PNP))),
    # GRIC accepting E (192 x 640)
    "default_tunnel": ("tunnel", {}, None, dict(status=(E, E, E))),
    # the five-point batch ends long before findHomography's 2000 hypotheses and its refinement
    "e_max_iters_8": ("rigid", dict(e_max_iters=8), None, dict(n_min=11)),
    # 10 keypoints: GRIC (and the batch) skipped, E_tracker.py:196
    "ten_keypoints": ("ten", dict(kp_num_bestN=100), None, dict(n_kp=10)),
    # 3 keypoints: below the five-point solver's minimum
    "three_keypoints": ("three", dict(kp_num_bestN=4, kp_num_row=2, kp_num_col=2), None, dict(n_kp=3)),
    "validity_flow": ("rigid", dict(validity="flow", validity_thre=1.0), None, dict(status=(E, E, E))),
    "validity_homo_ratio": ("rigid", dict(validity="homo_ratio", validity_thre=0.5), None, dict(status=(E, E, E))),
    # an E-tracked configuration whose middle pair finds no depth to recover the scale from: that pair alone falls back to PnP
    "pnp_fallback_pair": ("rigid", dict(validity="flow", validity_thre=1.0), ("zero", 1), dict(status=(E, PNP, E))),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_prefetched_half_matches_the_late_pre_part_in_both_layouts(gpu, pmod, weights, monkeypatch, case):
    name, o, depth_rule, want = CASES[case]
    sc = scene(name)
    h, w = sc["diff"].shape
    feed = (64, 96) if h == H else (192, 640)
    results = {}
    for layout in LAYOUTS:
        pipe, lay = make_pipe(pmod, layout, h, w, feed, sc["K"], weights[0], weights[1], monkeypatch, **o)
        try:
            late = run_overrides(pipe, sc, False, depth_rule, o.get("validity", "GRIC"))
            ahead = run_overrides(pipe, sc, True, depth_rule, o.get("validity", "GRIC"))
        finally:
            pipe.close()
        print(layout, lay["text"])
        for k, r in enumerate(late[0]):
            print("  pair %d: status %d kp %d inliers %d pnp inliers %d" % (k, r["status"], r["n_kp"], r["best_inlier_cnt"], r["pnp_inliers"]))
        assert ahead == late, "%s, prefetched against late pre-part: %s" % (layout, differing(ahead, late))
        results[layout] = late
    assert results["lanes"] == results["wide"], "lanes against wide: %s" % differing(results["lanes"], results["wide"])
    rows = results["lanes"][0]
    assert all(r["good_kp_found"] == 1 for r in rows)
    if "status" in want:
        assert tuple(r["status"] for r in rows) == want["status"], "the pairs left the branch this case is about"
    if "n_kp" in want:
        assert all(r["n_kp"] == want["n_kp"] for r in rows)
    if "n_min" in want:
        assert all(r["n_kp"] >= want["n_min"] for r in rows)


def test_coded_frames_drive_agrees_between_the_layouts(gpu, pmod, monkeypatch):
    """bench.py's software pipeline on coded frames A, B, A, B ...: nets three pairs ahead with the pre-part prefetched right
    behind them, features carried from the second pair on, SLOTS + 3 pairs so that every slot is reused"""
    h, w, ahead, n = 192, 640, 3, SLOTS + 3
    gpu.check(gpu.lib().dfvo_set_conv_precision(b"f16x3"))
    try:
        mode = "mux" if pmod.TrackingPipeline._net_size(h, w) == (h, w) else "pot"
        seq = coded_tunnel_sequence(h, w, 2, mode=mode, step=1.0, seed=7)
        fsd, dsd = crafted_liteflownet_state_dict(h, w, mode), crafted_monodepth2_state_dict()
        results = {}
        for layout in LAYOUTS:
            pipe, lay = make_pipe(pmod, layout, h, w, (192, 640), seq["K"], fsd, dsd, monkeypatch)
            try:
                d_frames = [_d(f) for f in seq["frames"][:2]]
                pipe.set_ref_image(d_frames[0])

                def feed(j):
                    pipe.enqueue_nets(j % SLOTS, None if j > 0 else d_frames[j % 2], d_frames[1 - j % 2], None)
                    pipe.prefetch_track(j % SLOTS)

                feed(0)
                fed, rows = 1, []
                for k in range(n):
                    pipe.track_begin(k % SLOTS)
                    while fed < n and fed <= k + ahead:
                        feed(fed)
                        fed += 1
                    out = pipe.track_end(k % SLOTS)
                    row = pair_row(pipe, k % SLOTS, out)
                    fwd, bwd, diff, _, dep = pipe.get_outputs(k % SLOTS)
                    row["maps"] = (crc(fwd), crc(bwd), crc(diff), crc(dep))
                    rows.append(row)
                pipe.sync()
                results[layout] = (rows, crc(pipe.get_rng_state()[1]))
            finally:
                pipe.close()
            print(layout, lay["text"], [(r["status"], r["n_kp"]) for r in rows])
        assert all(r["status"] in (E, PNP) and r["n_kp"] > 10 for r in results["lanes"][0])
        assert results["lanes"] == results["wide"], differing(results["lanes"], results["wide"])
    finally:
        gpu.check(gpu.lib().dfvo_set_conv_precision(b"fp32"))
