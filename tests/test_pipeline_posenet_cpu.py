"""CPU: the pose-lane options of the fused pipeline (pipeline.POSE_DEFAULTS / check_pose_options, tracking_method deep_pose,
status 4) -- what options_from_cfg accepts and what it still refuses by name, the ValueErrors of the option check, hybrid_pose
for the pose net's matrix, and the constructor refusing before it touches the device or the library."""
import importlib

import numpy as np
import pytest

from test_pipeline_options_cpu import _set, best_n, default_cfg, uniform

K = [[100.0, 0, 208], [0, 100.0, 64], [0, 0, 1]]


@pytest.fixture(scope="module")
def pmod():
    import __graft_entry__ as g
    g.dfvo_amd()
    return importlib.import_module("df-vo_amd.pipeline")


def cfg_with(*edits):
    c = default_cfg()
    for path, value in edits:
        _set(path, value)(c)
    return c


def test_pose_defaults_and_tables(pmod):
    assert pmod.POSE_DEFAULTS == dict(pose_net=False, depth_consistency=False, depth_consistency_thre=0.05)
    assert pmod._TRACKING["deep_pose"] == 2 and pmod.STATUS[4] == "DeepPose"
    assert pmod.check_pose_options(dict(pmod.POSE_DEFAULTS)) == dict(enable=0, depth_consistency=0, depth_thre=0.05)
    assert pmod.options_from_cfg(default_cfg()) == {}  # (the default configuration's own depth_consistency.thre travels nowhere)


def test_accepted_combinations(pmod):
    c = cfg_with(("deep_pose.enable", True), ("tracking_method", "deep_pose"))
    assert pmod.options_from_cfg(c) == {"tracking_method": "deep_pose", "pose_net": True}
    # the map is computed in the hybrid / PnP branch only (dfvo.py:139-143): under deep_pose tracking the key is not read
    c = cfg_with(("deep_pose.enable", True), ("tracking_method", "deep_pose"), ("kp_selection.depth_consistency.enable", True))
    assert pmod.options_from_cfg(c) == {"tracking_method": "deep_pose", "pose_net": True}
    c = cfg_with(("deep_pose.enable", True), ("kp_selection.depth_consistency.enable", True), ("kp_selection.depth_consistency.thre", 0.01))
    assert pmod.options_from_cfg(c) == {"pose_net": True, "depth_consistency": True, "depth_consistency_thre": 0.01}
    c = cfg_with(("deep_pose.enable", True), ("kp_selection.depth_consistency.enable", True), ("tracking_method", "PnP"))
    want = {"pose_net": True, "depth_consistency": True, "tracking_method": "PnP"}
    thre = c.kp_selection.depth_consistency.thre
    if thre != 0.05:
        want["depth_consistency_thre"] = thre
    assert pmod.options_from_cfg(c) == want


@pytest.mark.parametrize("edits,name", [
    ([("deep_pose.enable", True)], "deep_pose.enable"),                                        # no consumer
    ([("deep_pose.enable", True), ("tracking_method", "PnP")], "deep_pose.enable"),
    ([("kp_selection.depth_consistency.enable", True)], "kp_selection.depth_consistency.enable"),  # no pose to warp with
    ([("tracking_method", "deep_pose")], "deep_pose.enable"),                                  # no net to track with
], ids=["net-alone", "net-alone-pnp", "mask-alone", "tracking-alone"])
def test_refused_combinations_name_the_key(pmod, edits, name):
    with pytest.raises(NotImplementedError) as e:
        pmod.options_from_cfg(cfg_with(*edits))
    assert name in str(e.value), str(e.value)


@pytest.mark.parametrize("source", [best_n, uniform], ids=["bestN", "sampled"])
def test_mask_with_another_keypoint_source_is_refused(pmod, source):
    c = cfg_with(("deep_pose.enable", True), ("kp_selection.depth_consistency.enable", True))
    source(c)
    with pytest.raises(NotImplementedError, match="kp_selection.depth_consistency.enable"):
        pmod.options_from_cfg(c)


@pytest.mark.parametrize("o,key", [
    (dict(pose_net=1), "pose_net"), (dict(pose_net="yes"), "pose_net"), (dict(pose_net=True, depth_consistency=1), "depth_consistency"),
    (dict(pose_net=True, depth_consistency_thre=float("nan")), "depth_consistency_thre"),
    (dict(pose_net=True, depth_consistency_thre=float("inf")), "depth_consistency_thre"),
    (dict(pose_net=True, depth_consistency_thre=None), "depth_consistency_thre"),
    (dict(pose_net=True, depth_consistency_thre="0.05"), "depth_consistency_thre"),
    (dict(depth_consistency=True), "depth_consistency"),
], ids=["int", "str", "mask-int", "nan", "inf", "none", "thre-str", "mask-without-net"])
def test_check_pose_options_value_errors(pmod, o, key):
    full = dict(pmod.POSE_DEFAULTS)
    full.update(o)
    with pytest.raises(ValueError, match=key):
        pmod.check_pose_options(full)


@pytest.mark.parametrize("kp_source", ["bestN", "sampled"])
def test_check_pose_options_mask_needs_local_bestn(pmod, kp_source):
    full = dict(pmod.POSE_DEFAULTS, pose_net=True, depth_consistency=True)
    assert pmod.check_pose_options(full, "local_bestN")["depth_consistency"] == 1
    with pytest.raises(ValueError, match="kp_source"):
        pmod.check_pose_options(full, kp_source)


@pytest.mark.parametrize("o,key", [
    (dict(pose_net="on"), "pose_net"),
    (dict(depth_consistency=True), "depth_consistency"),
    (dict(pose_net=True, depth_consistency=True, kp_source="bestN"), "kp_source"),
    (dict(pose_net=True, depth_consistency_thre=float("nan")), "depth_consistency_thre"),
    (dict(tracking_method="deep_pose"), "pose_net"),
    (dict(tracking_method="deep_pose", pose_net=True, depth_consistency=True), "depth_consistency"),
    (dict(pose_net=True), "pose_sd"),  # no weights
], ids=["bad-bool", "mask-without-net", "mask-bestN", "nan", "deep-without-net", "deep-with-mask", "no-weights"])
def test_constructor_raises_before_the_library(pmod, o, key, monkeypatch):
    """ValueError before capi.require_gpu / capi.lib: neither is reached (both are made to fail the test if they are)"""
    capi = importlib.import_module("df-vo_amd.capi")

    def reached(*a, **k):
        raise AssertionError("the constructor touched the library before it checked its options")
    monkeypatch.setattr(capi, "require_gpu", reached)
    monkeypatch.setattr(capi, "lib", reached)
    with pytest.raises(ValueError, match=key):
        pmod.TrackingPipeline(128, 416, 64, 96, K, {}, {}, **o)


def test_hybrid_pose_for_the_pose_net_status(pmod):
    capi = importlib.import_module("df-vo_amd.capi")
    out = capi.TrackOut()
    rng = np.random.default_rng(3)
    R32, t32 = rng.standard_normal((3, 3)).astype(np.float32), rng.standard_normal(3).astype(np.float32)
    for i, v in enumerate(R32.reshape(-1)):
        out.R[i] = float(v)
    for i, v in enumerate(t32):
        out.t[i] = float(v)
    out.status, out.scale = 4, 1.0
    prev = np.eye(4)
    prev[0, 3] = 7.0
    T, mode = pmod.TrackingPipeline.hybrid_pose(out, prev)
    assert mode == "DeepPose" and T.dtype == np.float64
    assert np.array_equal(T[:3, :3], R32.astype(np.float64)) and np.array_equal(T[:3, 3], t32.astype(np.float64))  # [R|t] as it is
    assert np.array_equal(T[3], [0, 0, 0, 1])
    g = pmod.TrackingPipeline.accumulate(np.eye(4), T)
    assert np.array_equal(g, T)
