"""GPU: the dense drawer panels (df-vo_amd/csrc/vis.hip, libs/general/frame_drawer.py) against what the reference's own
drawer computed on the same seeded inputs (tests/golden/frame_drawer.npz, see tests/golden/make_golden_drawer.py).

Equality is required wherever the reference's arithmetic is robust against the last bits of arctan2 (checked when the
fixture was made: perturbing the angle by +-4 ulp changes 0 of 15 360 pixels on each of the four generic flows).  On the
lattice flows exact wheel nodes make one grey level depend on the last bit of atan2 (the same perturbation moves 1.21 %, 0.35 %
and 0.53 % of the pixels by one level): there no pixel may differ by more than one level and at most 2 % may differ -- a
wrong side of the rad <= 1 or signed-zero discontinuity would show as tens of levels."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import drawer_np as D

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


class NS(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "frame_drawer.npz"))


@pytest.fixture(scope="module")
def fd(gpu):
    return importlib.import_module("df-vo_amd.libs.general.frame_drawer")


@pytest.fixture(scope="module")
def panels(fd):
    """one DensePanels per window size, shared by the tests (each test draws the cells it looks at)"""
    made = {}

    def get(wh, ww):
        if (wh, ww) not in made:
            made[(wh, ww)] = fd.DensePanels(NS(window_h=wh, window_w=ww))
        return made[(wh, ww)]
    yield get
    for p in made.values():
        p.close()


def make_vo(cur_data, depth_disp="disp", tracking=False, ratio=False):
    cfg = NS(visualization=NS(depth=NS(use_tracking_depth=tracking, depth_disp=depth_disp)),
             depth=NS(max_depth=D.MAX_DEPTH),
             kp_selection=NS(local_bestN=NS(enable=True, score_method="flow_ratio" if ratio else "flow"),
                             rigid_flow_kp=NS(rigid_flow_thre=D.RIGID_FLOW_THRE)))
    return NS(cfg=cfg, cur_data=cur_data)


def draw_case(p, spec, x):
    """run panel case `spec` through the mirror's method; returns the item it drew"""
    kind = spec.split(":")[0]
    if kind == "flow":
        p.draw_flow(x, "flow1")
        return "flow1"
    if kind in ("disp", "depth"):
        f8 = spec.endswith("f8")
        p.draw_depth(make_vo({"depth" if f8 else "raw_depth": x}, depth_disp=kind, tracking=f8))
        return "depth"
    if spec.endswith("rigid"):
        p.draw_rigid_flow_consistency(make_vo({"rigid_flow_mask": x}))
        return "rigid_flow_diff"
    p.draw_flow_consistency(make_vo({"fb_flow_mask": x}, ratio=spec.endswith("ratio")))
    return "opt_flow_diff"


# ---- wheel at full resolution -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(37, 53), (96, 160)])
@pytest.mark.parametrize("name", D.FLOW_GENERIC + D.FLOW_LATTICE)
def test_flow_rgb_equals_flow_to_image(gpu, fx, panels, name, h, w):
    p = panels(600, 1000)
    flow = D.flow_case(name, h, w)
    rgb = np.zeros((h, w, 3), np.uint8)
    n = C.c_longlong(-1)
    gpu.check(gpu.lib().dfvo_vis_flow_rgb(p._vis(), gpu.as_ptr(flow), h, w, gpu.as_ptr(rgb), C.byref(n)))
    ref = fx["flow_rgb/%s@%dx%d" % (name, h, w)]
    diff = np.abs(rgb.astype(int) - ref.astype(int))
    n_diff = int((diff > 0).any(-1).sum())
    print("   %s %dx%d: %d of %d pixels differ, max %d levels, %d unknown" % (name, h, w, n_diff, h * w, diff.max(), n.value))
    assert n.value == (2 if name == "specials" else 0)
    if name in D.FLOW_GENERIC:
        assert n_diff == 0
    else:
        assert diff.max() <= 1 and n_diff <= 0.02 * h * w


def test_draw_flow_zeroes_unknown_entries_in_the_callers_array(gpu, fx, panels):
    """flow_to_image's u[idxUnknow] = 0 acts on a view of its caller's array: the mirror applies the same write"""
    p = panels(600, 1000)
    for h, w in ((37, 53), (96, 160)):
        flow = D.flow_case("specials", h, w)
        before = flow.copy()
        p.draw_flow(flow, "flow1")
        changed = np.argwhere(flow.view(np.uint32) != before.view(np.uint32))
        assert np.array_equal(changed, fx["flow_after_idx/specials@%dx%d" % (h, w)])
        assert np.array_equal(flow[tuple(changed.T)], fx["flow_after_val/specials@%dx%d" % (h, w)])
        assert np.isnan(flow[0, h // 3, w // 4])  # (a NaN is not "unknown": it stays)
        ch, cw = p.data["flow1"].shape[:2]
        assert np.array_equal(p.data["flow1"], D.cell_from_rgb(fx["flow_rgb/specials@%dx%d" % (h, w)], ch, cw))


# ---- percentile ----------------------------------------------------------------------------------------------------
def _pct_inputs():
    return D.percentile_cases() + [("map192x640_float32", None), ("map192x640_float64", None)]


@pytest.mark.parametrize("name", [c[0] for c in _pct_inputs()])
def test_disparity_percentile_is_numpys(gpu, fx, panels, name):
    p = panels(600, 1000)
    if name.startswith("map192x640"):
        d = D.depth_case("rand", 192, 640, np.float64 if name.endswith("64") else np.float32).ravel()
    else:
        d = dict(D.percentile_cases())[name]
    out = C.c_double()
    gpu.check(gpu.lib().dfvo_vis_disparity_percentile90(p._vis(), gpu.as_ptr(np.ascontiguousarray(d)), int(d.dtype == np.float64), d.size,
                                                        C.byref(out)))
    want = float(fx["pct/" + name])
    print("   %s: device %r numpy %r" % (name, out.value, want))
    assert out.value == want
    if d.size > 1:  # a NaN anywhere: np.percentile hands out NaN
        d = d.copy()
        d[d.size // 2] = np.nan
        gpu.check(gpu.lib().dfvo_vis_disparity_percentile90(p._vis(), gpu.as_ptr(d), int(d.dtype == np.float64), d.size, C.byref(out)))
        assert np.isnan(out.value)


# ---- cells ---------------------------------------------------------------------------------------------------------
def _cell_params():
    return [(m, win, spec) for m, win in D.MAP_WINDOWS for spec in D.PANELS_BY_MAP[m]]


@pytest.mark.parametrize("m,win,spec", _cell_params(), ids=["%dx%d-%dx%d-%s" % (m + win + (s,)) for m, win, s in _cell_params()])
def test_cell_equals_resized_reference_image(gpu, fx, panels, m, win, spec):
    p = panels(*win)
    (h, w) = m
    x = D.panel_input(spec, h, w)
    for it in ("depth", "flow1", "flow2", "opt_flow_diff"):
        p._blank(it)
    item = draw_case(p, spec, x)
    ch, cw = p.data[item].shape[:2]
    want = D.cell_from_rgb(fx[D.panel_key(spec, h, w)], ch, cw)
    got = p.data[item]
    diff = np.abs(got.astype(int) - want.astype(int))
    print("   %s %s -> cell %dx%d: %d pixels differ (max %d)" % (spec, m, ch, cw, int((diff > 0).any(-1).sum()), diff.max()))
    assert np.array_equal(got, want)
    # nothing outside the cell was touched, on the host window and on the device canvas
    y0, x0, y1, x1 = D.layout(*win)[D.CELLS[item]]
    expect = np.zeros((win[0], win[1], 3), np.uint8)
    expect[y0:y1, x0:x1] = want
    assert np.array_equal(p.img, expect)
    canvas = np.empty_like(expect)
    gpu.check(gpu.lib().dfvo_vis_fetch(p._vis(), -1, gpu.as_ptr(canvas)))
    assert np.array_equal(canvas, expect)


def test_guards_and_toggles(gpu, fx, panels):
    p = panels(192, 320)
    h, w = 96, 160
    for it in ("depth", "flow1", "flow2", "opt_flow_diff"):
        p._blank(it)
    # missing keys return early, nothing is drawn
    p.draw_depth(make_vo({}))
    p.draw_depth(make_vo({"raw_depth": D.depth_case("rand", h, w)}, tracking=True))  # tracking depth asked for, only raw there
    p.draw_flow_consistency(make_vo({}))
    p.draw_rigid_flow_consistency(make_vo({"fb_flow_mask": D.diff_case("rand", h, w)}))
    p.draw_depth(make_vo({"raw_depth": D.depth_case("rand", h, w)}, depth_disp=None))
    assert not p.img.any()
    # flow2 and rigid_flow_diff share one rectangle: the later draw wins
    p.draw_flow(D.flow_case("randn5", h, w), "flow2")
    flow2 = p.data["flow2"].copy()
    assert flow2.any() and np.array_equal(p.data["rigid_flow_diff"], flow2)
    p.draw_rigid_flow_consistency(make_vo({"rigid_flow_mask": D.diff_case("rand", h, w)}))
    ch, cw = flow2.shape[:2]
    assert np.array_equal(p.data["flow2"], D.cell_from_rgb(fx[D.panel_key("jet:rand:rigid", h, w)], ch, cw))
    # a toggled-off cell is zero, on the host and on the device
    p.draw_depth(make_vo({"raw_depth": D.depth_case("rand", h, w)}))
    assert p.data["depth"].any()
    p.display["depth"] = p.display["flow2"] = False
    try:
        p.draw_depth(make_vo({"raw_depth": D.depth_case("rand", h, w)}))
        p.draw_flow(D.flow_case("randn5", h, w), "flow2")
    finally:
        p.display["depth"] = p.display["flow2"] = True
    assert not p.data["depth"].any() and not p.data["flow2"].any()
    canvas = np.empty_like(p.img)
    gpu.check(gpu.lib().dfvo_vis_fetch(p._vis(), -1, gpu.as_ptr(canvas)))
    assert np.array_equal(canvas, p.img)
    # Normalize raises for vmin > vmax, before anything is drawn
    vo = make_vo({"raw_depth": D.depth_case("rand", h, w)}, depth_disp="depth")
    vo.cfg.depth["max_depth"] = -1.0
    with pytest.raises(ValueError):
        p.draw_depth(vo)
    with pytest.raises(ValueError):  # 90th percentile of negative disparities
        p.draw_depth(make_vo({"raw_depth": np.full((h, w), -3.0, np.float32)}))
    assert np.array_equal(canvas, p.img)


# ---- resident path against upload path -----------------------------------------------------------------------------
def _vis_cfg(cfg):
    cfg["visualization"] = NS(depth=NS(use_tracking_depth=False, depth_disp="disp"),
                              flow=NS(vis_forward_flow=True, vis_backward_flow=True, vis_flow_diff=True, vis_rigid_diff=True))
    return cfg


def _loop(cfg, seq, n, h, w, mirrors, drawer, draws):
    """the frame loop of DFVO.main as tests/test_dropin_gpu.py::_main_loop runs it over the mirrors, with the drawer where
    dfvo.py:389-393 has it and `draws` np.random.randint draws per frame standing in for draw_match_temporal's colours"""
    from oracle import cv2_shim, tracker_np as T
    deep_models, sampler, e_tracker, pnp_tracker, SE3 = mirrors
    np.random.seed(cfg.seed)
    ref_data, cur_data = {}, {}
    rec = []
    for img_id in range(n):
        cur_data["id"], cur_data["timestamp"], cur_data["img"] = img_id, img_id, seq["frames"][img_id].copy()
        raw = deep_models.forward_depth(imgs=[cur_data["img"]])
        cur_data["raw_depth"] = cv2_shim.resize(raw, (w, h), interpolation=cv2_shim.INTER_NEAREST)
        cur_data["depth"] = T.preprocess_depth(cur_data["raw_depth"], cfg.crop.depth_crop, [cfg.depth.min_depth, cfg.depth.max_depth])
        if img_id >= 1:
            flows = deep_models.forward_flow(cur_data, ref_data, forward_backward=True)
            kf, kb, kd = (ref_data["id"], cur_data["id"]), (cur_data["id"], ref_data["id"]), (ref_data["id"], cur_data["id"], "diff")
            ref_data["flow"], cur_data["flow"], ref_data["flow_diff"] = flows[kf].copy(), flows[kb].copy(), flows[kd].copy()
            kp_sel = sampler.kp_selection(cur_data, ref_data)
            assert kp_sel["good_kp_found"]
            sampler.update_kp_data(cur_data, ref_data, kp_sel)
            e_out = e_tracker.compute_pose_2d2d(ref_data["kp_best"], cur_data["kp_best"], True)
            rec.append({"R": np.array(e_out["pose"].R), "t": np.array(e_out["pose"].t), "inliers": np.array(e_out["inliers"])})
        if drawer is not None:
            drawer.main(NS(cfg=cfg, cur_data=cur_data, ref_data=ref_data, tracking_stage=min(img_id, 1)))
            rec_canvas = drawer.img.copy()
        else:
            rec_canvas = None
        if draws:
            np.random.randint(0, 255, draws)
        if img_id >= 1:
            rec[-1]["canvas"] = rec_canvas
            rec[-1]["rng"] = np.random.get_state()[1].copy()
        last = (dict(ref_data), dict(cur_data), raw)
        ref_data = dict(cur_data)
        ref_data["flow"] = cur_data["flow"] = ref_data["flow_diff"] = None
    return rec, last


@pytest.mark.parametrize("draws", [0, 300])
def test_resident_path_equals_upload_path_over_a_frame_loop(gpu, fd, tmp_path, monkeypatch, draws):
    """4 frames through the mirrors with the drawer where DFVO.main has it, once over the plain entry points (every panel
    uploaded) and once over the frame session (panels from its device buffers).  draws = 300: np.random.randint draws per
    frame, as the reference's match drawing makes them -- the session's ahead-of-time pose half must survive them."""
    from synth import coded_tunnel_sequence, crafted_liteflownet_state_dict, crafted_monodepth2_state_dict, write_weight_files
    from test_dropin_gpu import _build_mirrors, full_cfg
    h, w, n = 256, 640, 4
    seq = coded_tunnel_sequence(h, w, n, mode="mux", step=1.0, seed=33)
    flow_path, depth_dir = write_weight_files(str(tmp_path), crafted_liteflownet_state_dict(h, w, "mux"), crafted_monodepth2_state_dict())
    cfg = _vis_cfg(full_cfg(h, w, flow_path, depth_dir))
    runs = {}
    for key, sess in (("plain", "0"), ("session", "1")):
        monkeypatch.setenv("DFVO_SESSION", sess)
        mirrors = _build_mirrors(cfg, seq["K"])
        assert (mirrors[0].session is not None) == (sess == "1")
        drawer = fd.DensePanels(NS(window_h=600, window_w=1000))
        rec, last = _loop(cfg, seq, n, h, w, mirrors, drawer, draws)
        runs[key] = (rec, last, mirrors, drawer)
    pairs = n - 1
    assert len(runs["plain"][0]) == len(runs["session"][0]) == pairs
    for ra, rb in zip(runs["plain"][0], runs["session"][0]):
        for k in ("R", "t", "inliers", "rng", "canvas"):
            assert np.array_equal(ra[k], rb[k]), "'%s' differs between the plain entry points and the session" % k
    assert runs["plain"][0][-1]["canvas"][300:, 500:].any() and not runs["plain"][0][-1]["canvas"][:300].any()
    rec, (ref_data, cur_data, raw), mirrors, drawer = runs["session"]
    st = mirrors[0].session.stats
    print("   drawer", drawer.stats, drawer.vis_counters(), "| session", st)
    # one launch per pair serves flow1, flow2 and the consistency map from the session's buffers; the depth map of this
    # loop is the session's resized to the image size (dfvo.py:314-317), i.e. another array: uploaded, every frame
    assert drawer.stats["session_launches"] == pairs and drawer.stats["resident"] == 3 * pairs
    assert drawer.stats["uploaded"] == n and drawer.vis_counters()["panels_resident"] == 3 * pairs
    assert st["pose_ahead"] == pairs and st["kp_resident"] == pairs and st["pose_resident"] == pairs and st["pose_plain"] == 0
    plain = runs["plain"][3]
    assert plain.stats["resident"] == 0 and plain.stats["uploaded"] == n + 3 * pairs
    if draws == 0:
        # an edited copy of the flow takes the upload path and shows the edit
        before = dict(drawer.stats)
        edited = ref_data["flow"].copy()
        assert getattr(edited, "_dfvo_tok", None) is not None
        np.asarray(edited)[:, 40:120, 100:300] = 25.0  # (through a plain view: the token stays, the contents no longer match)
        drawer.draw_flow(edited, "flow1")
        assert drawer.stats["uploaded"] == before["uploaded"] + 1 and drawer.stats["resident"] == before["resident"]
        ch, cw = drawer.data["flow1"].shape[:2]
        assert np.array_equal(drawer.data["flow1"], D.cell_from_rgb(D.flow_to_image_np(np.asarray(edited))[0], ch, cw))
        assert not np.array_equal(drawer.data["flow1"], rec[-1]["canvas"][300:450, 750:1000])
        # ... the untouched copy is served from the session again, and equals what the upload path drew for the same values
        drawer.draw_flow(ref_data["flow"], "flow1")
        assert drawer.stats["resident"] == before["resident"] + 1
        assert np.array_equal(drawer.data["flow1"], rec[-1]["canvas"][300:450, 750:1000])
        # the session's raw depth (feed size) handed over as it is: resident, and equal to the restatement on its values
        before = dict(drawer.stats)
        drawer.draw_depth(NS(cfg=cfg, cur_data={"raw_depth": raw}))
        assert drawer.stats["resident"] == before["resident"] + 1 and drawer.stats["uploaded"] == before["uploaded"]
        assert np.array_equal(drawer.data["depth"], D.cell_from_rgb(D.depth_panel_np(np.array(raw), "disp")[0], 150, 250))
    for key in runs:
        runs[key][3].close()


def test_a_plain_pass_on_the_nets_sends_the_sessions_arrays_to_the_upload_path(gpu, fd, tmp_path, monkeypatch):
    """The resident path compares an array with the session's pinned HOST copy and draws from the nets' DEVICE output buffers.
    A plain pass on the same net (forward_flow on a pair the session does not hold, forward_depth on a frame it does not take)
    overwrites those buffers while generation, tokens and host copies stay: the session's arrays of that generation still
    pass token + contents, and must then be uploaded, not coloured from the other pass's output."""
    from synth import coded_tunnel_sequence, crafted_liteflownet_state_dict, crafted_monodepth2_state_dict, write_weight_files
    from test_dropin_gpu import _build_mirrors, full_cfg
    h, w = 256, 640
    seq = coded_tunnel_sequence(h, w, 3, mode="mux", step=1.0, seed=33)
    flow_path, depth_dir = write_weight_files(str(tmp_path), crafted_liteflownet_state_dict(h, w, "mux"), crafted_monodepth2_state_dict())
    cfg = _vis_cfg(full_cfg(h, w, flow_path, depth_dir))
    monkeypatch.setenv("DFVO_SESSION", "1")
    deep_models = _build_mirrors(cfg, seq["K"])[0]
    s = deep_models.session
    f0, f1, f2 = (seq["frames"][i].copy() for i in range(3))
    drawer = fd.DensePanels(NS(window_h=600, window_w=1000))
    deep_models.forward_depth(imgs=[f0])
    raw = deep_models.forward_depth(imgs=[f1])
    flows = deep_models.forward_flow({"id": 1, "img": f1}, {"id": 0, "img": f0}, True)
    A = flows[(0, 1)].copy()
    want_flow = D.cell_from_rgb(D.flow_to_image_np(np.asarray(A))[0], 150, 250)
    want_depth = D.cell_from_rgb(D.depth_panel_np(np.array(raw), "disp")[0], 150, 250)
    vo_depth = NS(cfg=cfg, cur_data={"raw_depth": raw})
    drawer.draw_flow(A, "flow1")
    drawer.draw_depth(vo_depth)
    assert drawer.stats["resident"] == 2 and drawer.stats["uploaded"] == 0
    assert np.array_equal(drawer.data["flow1"], want_flow) and np.array_equal(drawer.data["depth"], want_depth)
    # ---- a plain flow pass on another pair overwrites the flow net's output buffers
    before = dict(s.stats)
    other = deep_models.forward_flow({"id": 2, "img": f2}, {"id": 0, "img": f0}, True)
    assert s.stats["flow_plain"] == before["flow_plain"] + 1 and not np.array_equal(other[(0, 2)], np.asarray(A))
    assert s.vis_is_buffer(A, "fwd")                        # (token and contents still are the session's)
    for d in (drawer, fd.DensePanels(NS(window_h=600, window_w=1000))):   # the drawer that drew it before, and a fresh one
        up = d.stats["uploaded"] if hasattr(d, "stats") else 0
        d.draw_flow(A, "flow1")
        assert d.stats["uploaded"] == up + 1
        assert np.array_equal(d.data["flow1"], want_flow)
        d.draw_flow(flows[(1, 0)].copy(), "flow2")
        assert d.stats["uploaded"] == up + 2
        assert np.array_equal(d.data["flow2"], D.cell_from_rgb(D.flow_to_image_np(np.asarray(flows[(1, 0)]))[0], 150, 250))
        # the depth net was not touched: its panel is still served from the device
        res = d.stats["resident"]
        d.draw_depth(vo_depth)
        assert d.stats["resident"] == res + 1 and np.array_equal(d.data["depth"], want_depth)
    # ---- a plain depth pass on a frame the session does not take overwrites the depth net's output buffer
    small = np.ascontiguousarray(f2[:128, :320])
    assert not s.accepts(small)
    d_small = deep_models.forward_depth(imgs=[small])
    assert d_small.shape == raw.shape and not np.array_equal(d_small, np.asarray(raw)) and s.vis_is_depth(raw)
    for d in (drawer, fd.DensePanels(NS(window_h=600, window_w=1000))):
        up = d.stats["uploaded"] if hasattr(d, "stats") else 0
        d.draw_depth(vo_depth)
        assert d.stats["uploaded"] == up + 1 and np.array_equal(d.data["depth"], want_depth)
    # ---- the next pair through the session is resident again
    deep_models.forward_depth(imgs=[f1])
    deep_models.forward_depth(imgs=[f2])
    flows = deep_models.forward_flow({"id": 2, "img": f2}, {"id": 1, "img": f1}, True)
    res = drawer.stats["resident"]
    B = flows[(1, 2)].copy()
    drawer.draw_flow(B, "flow1")
    assert drawer.stats["resident"] == res + 1
    assert np.array_equal(drawer.data["flow1"], D.cell_from_rgb(D.flow_to_image_np(np.asarray(B))[0], 150, 250))
