"""CPU: depth.depth_src gt in the fused pipeline -- the option tables and options_from_cfg, the constructor's refusals, the
sequence driver's calls over a recording stub, the argument checks of dfvo_read_depth_u16 / dfvo_pipeline_set_depth_source
through the loaded library, and the restatement the device tests compare against (tests/depth_source_cases.py).  Neither the
GPU nor a device pointer is touched."""
import ctypes as C
import importlib

import numpy as np
import pytest

import depth_source_cases as DC
from test_pipeline_options_cpu import best_n, default_cfg, model_sel_flow, tracker_pnp, uniform

K = [[100.0, 0, 208], [0, 100.0, 64], [0, 0, 1]]


@pytest.fixture(scope="module")
def pmod():
    import __graft_entry__ as g
    g.dfvo_amd()
    return importlib.import_module("df-vo_amd.pipeline")


@pytest.fixture(scope="module")
def smod(pmod):
    return importlib.import_module("df-vo_amd.sequence")


# ---- option tables and options_from_cfg ---------------------------------------------------------------------------------
def test_the_three_tables_are_disjoint_and_the_default_maps_to_nothing(pmod):
    assert pmod.DEPTH_DEFAULTS == dict(depth_source="net", depth_scale=None, depth_size=None)
    tables = [set(pmod.DEFAULTS), set(pmod.OPTION_DEFAULTS), set(pmod.ITER_DEFAULTS), set(pmod.DEPTH_DEFAULTS)]
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not (a & b)
    c = default_cfg()
    assert c.depth.depth_src is None
    assert pmod.options_from_cfg(c) == {}
    assert pmod.check_depth_options(dict(pmod.DEPTH_DEFAULTS), 128, 416) == dict(source=0, scale=0.0, src_h=128, src_w=416)
    assert pmod.check_depth_options(dict(depth_source="external", depth_scale=500, depth_size=(480, 640)), 128, 416) == dict(
        source=1, scale=500.0, src_h=480, src_w=640)


def iterative(c):  # ablation_scale_iterative.yml
    c.scale_recovery.method = "iterative"
    c.kp_selection.rigid_flow_kp.enable = True


@pytest.mark.parametrize("edit,want", [
    (None, {}), (best_n, {"kp_source": "bestN"}), (uniform, {"kp_source": "sampled"}),
    (model_sel_flow, {"validity": "flow", "validity_thre": 5}), (tracker_pnp, {"tracking_method": "PnP"}),
    (iterative, {"scale_recovery": "iterative"}),
], ids=["default", "best_n", "uniform", "model_sel_flow", "tracker_pnp", "iterative"])
def test_depth_src_gt_maps_to_external_and_composes(pmod, edit, want):
    c = default_cfg()
    if edit:
        edit(c)
    assert pmod.options_from_cfg(c) == want  # (what the edit alone maps to)
    c.depth.depth_src = "gt"
    assert pmod.options_from_cfg(c) == dict(want, depth_source="external")


@pytest.mark.parametrize("value", ["pred", "lidar"])
def test_other_depth_sources_are_refused_by_name(pmod, value):
    c = default_cfg()
    c.depth.depth_src = value
    with pytest.raises(NotImplementedError) as e:
        pmod.options_from_cfg(c)
    assert "depth.depth_src" in str(e.value) and value in str(e.value)


# ---- the constructor's refusals (before the device or the library is touched) ---------------------------------------------
@pytest.mark.parametrize("key,o", [
    ("depth_source", dict(depth_source="sensor")),
    ("depth_scale", dict(depth_source="external")),  # depth_scale = None
    ("depth_scale", dict(depth_source="external", depth_scale=None)),
    ("depth_scale", dict(depth_source="external", depth_scale=0)),
    ("depth_scale", dict(depth_source="external", depth_scale=-1)),
    ("depth_scale", dict(depth_source="external", depth_scale=float("nan"))),
    ("depth_scale", dict(depth_source="external", depth_scale=float("inf"))),
    ("depth_scale", dict(depth_source="external", depth_scale=True)),
    ("depth_size", dict(depth_source="external", depth_scale=500, depth_size=(0, 5))),
    ("depth_size", dict(depth_source="external", depth_scale=500, depth_size=(3.5, 4))),
    ("depth_size", dict(depth_source="external", depth_scale=500, depth_size=7)),
    ("depth_size", dict(depth_size=(0, 5))),  # checked in net mode too
])
def test_bad_depth_option_values_raise_value_error(pmod, key, o):
    for depth_sd in ({}, None):
        with pytest.raises(ValueError, match=key):
            pmod.TrackingPipeline(128, 416, 64, 96, K, {}, depth_sd, **o)


def test_no_depth_weights_is_legal_in_external_mode_only(pmod):
    with pytest.raises(ValueError, match="depth_sd"):
        pmod.TrackingPipeline(128, 416, 64, 96, K, {}, None)
    with pytest.raises(ValueError, match="depth_sd"):
        pmod.TrackingPipeline(128, 416, 64, 96, K, {}, None, depth_source="net", depth_scale=500)


def test_from_cfg_without_depth_scale_names_it(pmod):
    c = default_cfg()
    c.depth.depth_src = "gt"
    with pytest.raises(ValueError, match="depth_scale"):
        pmod.TrackingPipeline.from_cfg(c, K, {}, None, 192, 640)


# ---- the sequence driver over a recording stub ---------------------------------------------------------------------------
class _Out:
    status, scale = 1, 0.0  # constant motion: the driver reads nothing else of it


class _Recorder:
    """records every call the driver makes.  enqueue_nets takes `depth`; the stubs of test_dist_cpu / test_bench_cpu do not"""

    def __init__(self):
        self.calls = []

    def set_ref_image(self, f):
        self.calls.append(("set_ref_image", f))

    def set_ref_depth_image(self, d):
        self.calls.append(("set_ref_depth_image", d))

    def seed(self, s):
        self.calls.append(("seed", s))

    def enqueue_nets(self, slot, ref, cur, d_feed=None, **kw):
        self.calls.append(("enqueue_nets", slot, ref, cur, d_feed, kw))

    def prefetch_track(self, slot):
        self.calls.append(("prefetch_track", slot))

    def track_begin(self, slot):
        self.calls.append(("track_begin", slot))

    def track_end(self, slot):
        self.calls.append(("track_end", slot))
        return _Out()

    def sync(self):
        self.calls.append(("sync",))


class _NoDepthStub(_Recorder):
    """the shape of the existing stubs: no `depth` keyword, no set_ref_depth_image"""
    set_ref_depth_image = None

    def enqueue_nets(self, slot, ref, cur, feed=None):
        self.calls.append(("enqueue_nets", slot, ref, cur, feed, {}))


FRAMES = ["f%d" % i for i in range(9)]
DEPTHS = ["d%d" % i for i in range(9)]


@pytest.mark.parametrize("lo,hi,carry", [(0, 4, True), (3, 8, True), (2, 6, False), (5, 6, True)])
def test_track_chunk_with_depths_feeds_the_depth_of_every_current_frame(smod, lo, hi, carry):
    p = _Recorder()
    smod.track_chunk(p, FRAMES, lo, hi, carry_features=carry, depths=DEPTHS)
    names = [c[0] for c in p.calls]
    assert names.count("set_ref_depth_image") == 1 and "set_ref_image" not in names
    assert p.calls[0] == ("set_ref_depth_image", DEPTHS[lo])  # the halo's depth, ahead of everything
    feeds = [c for c in p.calls if c[0] == "enqueue_nets"]
    assert len(feeds) == hi - lo
    for j, c in zip(range(lo, hi), feeds):
        ref = None if (carry and j > lo) else FRAMES[j]
        assert c == ("enqueue_nets", j % smod.SLOTS, ref, FRAMES[j + 1], None, {"depth": DEPTHS[j + 1]}), (j, c)


def test_track_chunk_without_depths_makes_the_calls_it_always_made(smod):
    want = [("set_ref_image", "f1"), ("seed", 4869),
            ("enqueue_nets", 1, "f1", "f2", None, {}), ("prefetch_track", 1),
            ("enqueue_nets", 2, None, "f3", None, {}), ("prefetch_track", 2),
            ("enqueue_nets", 3, None, "f4", None, {}), ("prefetch_track", 3),
            ("track_begin", 1), ("enqueue_nets", 0, None, "f5", None, {}), ("prefetch_track", 0), ("track_end", 1),
            ("track_begin", 2), ("track_end", 2),
            ("track_begin", 3), ("track_end", 3),
            ("track_begin", 0), ("track_end", 0),
            ("sync",)]
    for stub in (_NoDepthStub(), _Recorder()):
        smod.track_chunk(stub, FRAMES, 1, 5)
        assert stub.calls == want
        stub.calls.clear()
        smod.track_chunk(stub, FRAMES, 1, 5, depths=None)
        assert stub.calls == want


def test_run_sequence_and_run_sequences_hand_the_depths_on(smod):
    p = _Recorder()
    smod.run_sequence(p, FRAMES, 5, depths=DEPTHS)
    assert p.calls[0] == ("set_ref_depth_image", "d0")
    assert [c[5] for c in p.calls if c[0] == "enqueue_nets"] == [{"depth": "d%d" % j} for j in range(1, 5)]
    p = _Recorder()
    other = ["e%d" % i for i in range(9)]
    smod.run_sequences(p, [("a", FRAMES, 3, DEPTHS), ("b", FRAMES, 3), ("c", FRAMES, 2, other)])
    refs = [c for c in p.calls if c[0] in ("set_ref_image", "set_ref_depth_image")]
    assert refs == [("set_ref_depth_image", "d0"), ("set_ref_image", "f0"), ("set_ref_depth_image", "e0")]
    assert [c[5] for c in p.calls if c[0] == "enqueue_nets"] == [{"depth": "d1"}, {"depth": "d2"}, {}, {}, {"depth": "e1"}]
    p = _NoDepthStub()
    smod.run_sequences(p, [("a", FRAMES, 3), ("b", FRAMES, 3, None)])  # (a fourth element of None is no depths)
    assert [c[0] for c in p.calls].count("set_ref_image") == 2


# ---- the library's argument checks, no GPU (the pointers are never read) ---------------------------------------------------
def test_read_depth_u16_refuses_bad_arguments(capi):
    lib = capi.lib()
    src, raw, proc = np.ones(4, np.uint16), np.ones(4, np.float32), np.ones(4)
    s, r, p = (capi.as_ptr(a) for a in (src, raw, proc))

    def call(src=s, h=2, w=2, scale=500.0, H=2, W=2, box=(0, 2, 0, 2), raw=r, proc=p):
        return lib.dfvo_read_depth_u16(src, h, w, scale, H, W, box[0], box[1], box[2], box[3], 0.0, 50.0, raw, proc, None)

    bad = [dict(src=None), dict(raw=None), dict(proc=None),
           dict(h=0), dict(w=0), dict(H=0, box=(0, 0, 0, 2)), dict(W=0, box=(0, 2, 0, 0)), dict(h=-1), dict(W=-3, box=(0, 2, 0, 0)),
           dict(scale=0.0), dict(scale=-500.0), dict(scale=float("inf")), dict(scale=float("-inf")), dict(scale=float("nan")),
           dict(box=(-1, 2, 0, 2)), dict(box=(0, 3, 0, 2)), dict(box=(0, 2, 0, 3)), dict(box=(2, 1, 0, 2)), dict(box=(0, 2, 2, 1))]
    for kw in bad:
        rc = call(**kw)
        assert rc == -2 and b"dfvo_read_depth_u16" in lib.dfvo_last_error(), (kw, rc)  # DFVO_ERR_ARG
    assert (raw == 1).all() and (proc == 1).all()


def test_pipeline_depth_source_entry_points_refuse_a_null_pipeline(capi):
    lib = capi.lib()
    ds = capi.PipelineDepthSrc(source=capi.DEPTH_EXTERNAL, scale=500.0, src_h=2, src_w=2)
    assert lib.dfvo_pipeline_set_depth_source(None, C.byref(ds)) == -2
    assert b"dfvo_pipeline_set_depth_source" in lib.dfvo_last_error()
    src = np.ones(4, np.uint16)
    assert lib.dfvo_pipeline_enqueue_nets_depth(None, 0, None, None, capi.as_ptr(src)) == -2
    assert b"dfvo_pipeline_enqueue_nets_depth" in lib.dfvo_last_error()
    assert lib.dfvo_pipeline_set_ref_depth_u16(None, capi.as_ptr(src)) == -2
    assert b"dfvo_pipeline_set_ref_depth_u16" in lib.dfvo_last_error()


# ---- the restatement the device tests stand on ----------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(DC.SIZES))
def test_the_planted_boundary_values_survive_the_resampling(size):
    """per size and scale: every planted value is read by an output pixel inside the default crop, max_depth and min_depth
    themselves are dropped, their inner neighbours kept -- and the index formula is cv2_shim's INTER_NEAREST"""
    from oracle import cv2_shim
    (h, w), (H, W) = DC.SIZES[size]
    for i, scale in enumerate(DC.SCALES):
        src, planted = DC.source_image(40 + i, size, scale)
        assert src.shape == (h, w) and len({(Y, X) for Y, X, _ in planted}) == 9
        assert DC.planted_survive(src, planted, scale, H, W)
        y0, y1, x0, x1 = DC.crop_box(DC.crop_fractions("default", H, W), H, W)
        assert all(y0 <= Y < y1 and x0 <= X < x1 for Y, X, _ in planted)
        raw, proc = DC.read_depth_ref(src, scale, H, W, DC.crop_fractions("default", H, W), DC.DEPTH_RANGE)
        assert (proc[:y0] == 0).all() and (proc[y0:] != 0).any()
        full = src / scale
        want = cv2_shim.resize(full.astype(np.float32), (W, H), interpolation=cv2_shim.INTER_NEAREST)
        assert np.array_equal(want, full.astype(np.float32)[DC.nearest_index(H, h)[:, None], DC.nearest_index(W, w)[None, :]])
        # the one-pixel crop keeps its pixel (source_image puts a value just inside the range under it)
        _, one = DC.read_depth_ref(src, scale, H, W, DC.crop_fractions("one_pixel", H, W), DC.DEPTH_RANGE)
        assert np.count_nonzero(one) == 1 and one[H // 2, W // 2] == (int(DC.DEPTH_RANGE[1] * scale) - 1) / scale

