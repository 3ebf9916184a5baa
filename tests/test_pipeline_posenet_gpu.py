"""GPU: the pose lane of the fused pipeline -- dfvo_depth_consistency_dev (the depth-consistency kernel with its pose in device
memory), the pose net and the kp_selection.depth_consistency mask on the depth stream (dfvo_pipeline_set_pose_net), and
tracking_method deep_pose.

The world is the six-frame coded tunnel of tests/test_deep_pose_gpu.py (_world, _pose_weights) at 128 x 416.  The nets are fed
at 192 x 640, the size at which the crafted depth net decodes the coded frames and at which the class-surface test of the same
world (test_hybrid_tracking_with_the_depth_mask) asserts the two conditions repeated here: every pair finds good keypoints, and
the mask changes at least one pair's selection.  At a 64 x 96 feed the crafted depth net decodes nothing, and neither condition is
known to hold.  Every comparison between two runs of the device is bit for bit; the oracle chain is held to the tolerances of
tests/test_pipeline_configs_gpu.py (keypoints, inlier mask, R, t, counts and RandomState exactly, the scale to 1e-9 relative, the
PnP pose to 1e-12)."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

import depth_consistency_ref as DC
import depth_source_cases as DS
import pipeline_configs_oracle as PO
from oracle import tracker_np as T
from synth import crafted_liteflownet_state_dict, crafted_monodepth2_state_dict
from test_deep_pose_gpu import DEPTH_THRE, H, N_FRAMES, W, _pose_weights, _world

pytestmark = pytest.mark.gpu
FEED = (192, 640)
E, PNP, DEEP = 0, 3, 4
N_PAIRS = N_FRAMES - 1


@pytest.fixture(scope="module")
def mods(gpu):
    return (importlib.import_module("df-vo_amd.pipeline"), importlib.import_module("df-vo_amd.sequence"),
            importlib.import_module("df-vo_amd.dist"))


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _K32(K):
    K = np.asarray(K, np.float64)
    return np.ascontiguousarray(K, dtype=np.float32), np.ascontiguousarray(np.linalg.inv(K), dtype=np.float32)


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
BAND = 64  # guard floats in front of and behind the destination


def _run_plain(capi, cur, ref, K, Kinv, pose):
    h, w = cur.shape
    d_cur, d_ref = _d(cur), _d(ref)
    buf = torch.full((2 * BAND + h * w,), -7.0, device="cuda")
    torch.cuda.synchronize()
    capi.check(capi.lib().dfvo_depth_consistency(C.c_void_p(d_cur.data_ptr()), C.c_void_p(d_ref.data_ptr()), h, w, capi.as_ptr(K),
                                                 capi.as_ptr(Kinv), capi.as_ptr(np.ascontiguousarray(pose, dtype=np.float32)),
                                                 C.c_void_p(buf.data_ptr() + 4 * BAND), None))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _run_dev(capi, cur, ref, K, Kinv, pose):
    """the pose reaches its tensor through a device copy on the launch's own stream, behind a large fill that keeps the stream
    busy; the tensor holds another pose until then, and nothing waits between the copy and the launch: a read of the pose that is
    not ordered behind the copy -- by the host, or ahead of the stream -- computes a different map"""
    h, w = cur.shape
    d_cur, d_ref = _d(cur), _d(ref)
    buf = torch.full((2 * BAND + h * w,), -7.0, device="cuda")
    stale = np.eye(4, dtype=np.float32)
    stale[:3, 3] = (3.0, -2.0, 5.0)
    d_pose, d_src = _d(stale), _d(np.ascontiguousarray(pose, dtype=np.float32))
    big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big.fill_(1.0)
        d_pose.copy_(d_src, non_blocking=True)
        capi.check(capi.lib().dfvo_depth_consistency_dev(C.c_void_p(d_cur.data_ptr()), C.c_void_p(d_ref.data_ptr()), h, w, capi.as_ptr(K),
                                                         capi.as_ptr(Kinv), C.c_void_p(d_pose.data_ptr()),
                                                         C.c_void_p(buf.data_ptr() + 4 * BAND), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _yaw_pose(deg, t):
    pose = np.eye(4, dtype=np.float32)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    pose[0, 0], pose[0, 2], pose[2, 0], pose[2, 2] = c, s, -s, c
    pose[:3, 3] = t
    return pose


def _kernel_scenes(h, w):
    """(name, cur, ref, K, Kinv, pose): tunnel scenes, one pose with a rotation, one pair of maps with NaN and zero depths"""
    if (h, w) == (2, 2):  # the smallest map the launcher admits
        K = np.array([[1.5, 0, 0.5], [0, 1.5, 0.5], [0, 0, 1]], np.float64)
        cur = np.array([[5.0, 6.0], [7.0, 8.0]], np.float32)
        ref = np.array([[5.5, 6.5], [7.5, 8.5]], np.float32)
        K32, Kinv32 = _K32(K)
        yield "2x2", cur, ref, K32, Kinv32, _yaw_pose(0.0, (0.1, 0.0, 0.3))
        yield "2x2 rotated", cur, ref, K32, Kinv32, _yaw_pose(2.0, (0.2, -0.1, 0.0))
        return
    for k in (3, 20):
        cur, ref, K, Kinv, pose = DC.tunnel_scene(h, w, k)
        yield "tunnel k=%d" % k, cur, ref, K, Kinv, pose
    cur, ref, K, Kinv, pose = DC.tunnel_scene(h, w, 9)
    yield "rotated", cur, ref, K, Kinv, _yaw_pose(2.0, (0.3, 0.0, -0.2))
    cur, ref = cur.copy(), ref.copy()
    cur[h // 3:h // 3 + 4, w // 4:w // 2] = 0.0
    cur[h // 2, ::5] = np.float32("nan")
    ref[0, 0] = 0.0
    ref[h // 2:, w // 2] = np.float32("nan")
    yield "NaN and zero depths", cur, ref, K, Kinv, _yaw_pose(0.6, (0.0, 0.0, 0.0))


@pytest.mark.parametrize("h,w", [(37, 53), (48, 80), (2, 2)])
def test_device_pose_kernel_equals_the_host_pose_kernel(gpu, h, w):
    """np.array_equal on the float bits, NaNs included, guard bands untouched.  (A kernel that assigns the pose to the camera
    element by element compiles to other fused multiply-adds than the host-pose kernel and misses this on one pixel in five, by
    up to 8.3e-07; the kernel copies the camera whole)"""
    seen_nan = False
    for name, cur, ref, K, Kinv, pose in _kernel_scenes(h, w):
        want, got = _run_plain(gpu, cur, ref, K, Kinv, pose), _run_dev(gpu, cur, ref, K, Kinv, pose)
        body = want[BAND:BAND + h * w]
        seen_nan |= bool(np.isnan(body).any())
        assert (got[:BAND] == -7.0).all() and (got[BAND + h * w:] == -7.0).all(), "%s: wrote outside the destination" % name
        assert not (body == -7.0).any(), "%s: the map has unwritten pixels" % name
        differ = got.view(np.uint32) != want.view(np.uint32)
        both = differ & np.isfinite(got) & np.isfinite(want)
        print("DEPTH CONSISTENCY DEV %dx%d %s: %d of %d pixels differ from the host-pose kernel, largest |difference| %.3e"
              % (h, w, name, int(differ.sum()), h * w, float(np.abs(got[both] - want[both]).max()) if both.any() else 0.0))
        assert not differ.any(), "%s: the float bits differ" % name
        stale = _run_plain(gpu, cur, ref, K, Kinv, np.array([[1, 0, 0, 3], [0, 1, 0, -2], [0, 0, 1, 5], [0, 0, 0, 1]], np.float32))
        assert not np.array_equal(stale.view(np.uint32), want.view(np.uint32)), "%s: the stale pose would give the same map" % name
    assert seen_nan or (h, w) == (2, 2), "no scene carried a NaN through"


def test_device_pose_kernel_refuses_bad_arguments(gpu):
    lib = gpu.lib()
    K, Kinv = _K32(np.array([[1.5, 0, 0.5], [0, 1.5, 0.5], [0, 0, 1]]))
    a = torch.zeros(64, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    for args in ((p(a), p(a), 1, 2, gpu.as_ptr(K), gpu.as_ptr(Kinv), p(a), p(a), None),      # below 2 x 2
                 (p(a), p(a), 2, 2, gpu.as_ptr(K), gpu.as_ptr(Kinv), None, p(a), None),      # no pose
                 (p(a), p(a), 2, 2, gpu.as_ptr(K), gpu.as_ptr(Kinv), p(a, 2), p(a), None),   # pose off a float boundary
                 (p(a), p(a), 2, 2, gpu.as_ptr(K), gpu.as_ptr(Kinv), p(a), p(a, 4), None)):  # destination off a 16-byte boundary
        assert lib.dfvo_depth_consistency_dev(*args) == -2 and b"depth_consistency_dev" in lib.dfvo_last_error()


# ---- the world and its runs -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    seq, cfg = _world(tmp_path_factory.mktemp("mask"), True, "hybrid", True)
    assert cfg.kp_selection.depth_consistency.thre == DEPTH_THRE == 0.01
    return {"seq": seq, "cfg": cfg, "K": seq["K"], "frames": [_d(f) for f in seq["frames"]],
            "flow_sd": crafted_liteflownet_state_dict(H, W, "mux"), "depth_sd": crafted_monodepth2_state_dict(),
            "pose_sd": _pose_weights(True)}


def _mask_pipe(pmod, world, **kw):
    """TrackingPipeline.from_cfg on the world's own configuration object: hybrid, local_bestN, the mask at 0.01"""
    o = pmod.options_from_cfg(world["cfg"])
    assert o == {"pose_net": True, "depth_consistency": True, "depth_consistency_thre": DEPTH_THRE}
    depth_sd = None if kw.get("depth_source") == "external" else world["depth_sd"]
    return pmod.TrackingPipeline.from_cfg(world["cfg"], world["K"], world["flow_sd"], depth_sd, FEED[0], FEED[1],
                                          pose_sd=world["pose_sd"], seed=4869, **kw)


def _record(pipe, slot, out):
    fwd, bwd, diff, raw, dep = pipe.get_outputs(slot)
    kp_ref, kp_cur, inl = pipe.get_keypoints(slot)
    pose, dmap = pipe.get_pose_net(slot)
    return {"out": out, "status": out.status, "R": np.array(out.R[:]).reshape(3, 3), "t": np.array(out.t[:]).reshape(3, 1),
            "scale": out.scale, "fwd": fwd, "diff": diff, "raw": raw, "dep": dep, "kp_ref": kp_ref, "kp_cur": kp_cur, "inl": inl,
            "pose": pose, "map": dmap, "rng": pipe.get_rng_state()}


def _chunk_run(smod, pipe, frames, depths=None, graph=1):
    """the sequence through track_chunk(ahead=3) with prefetch_track; (reference depths of pair 0, per-pair records)"""
    pipe.set_graph(graph)
    if depths is None:
        pipe.set_ref_image(frames[0])
    else:
        pipe.set_ref_depth_image(depths[0])
    pipe.sync()
    ref0 = pipe.get_ref_depth()
    recs = []
    rel, status = smod.track_chunk(pipe, frames, 0, N_PAIRS, seed=4869, ahead=3, depths=depths,
                                   collect=lambda j, out: recs.append(_record(pipe, j % smod.SLOTS, out)))
    assert len(recs) == N_PAIRS and list(status) == [r["status"] for r in recs]
    return ref0, recs


def _lockstep_run(pipe, frames, depths=None):
    """enqueue_nets -> track, one pair at a time, no prefetch: nothing runs ahead of the previous pair's track_end"""
    if depths is None:
        pipe.set_ref_image(frames[0])
    else:
        pipe.set_ref_depth_image(depths[0])
    pipe.seed(4869)
    recs = []
    for j in range(N_PAIRS):
        slot = j % 2
        pipe.enqueue_nets(slot, frames[0] if j == 0 else None, frames[j + 1], depth=None if depths is None else depths[j + 1])
        recs.append(_record(pipe, slot, pipe.track(slot)))
    return recs


def _same_runs(a, b, what):
    assert len(a) == len(b) == N_PAIRS
    for j, (x, y) in enumerate(zip(a, b)):
        assert x["status"] == y["status"], "%s: status of pair %d" % (what, j)
        for k in ("R", "t", "scale", "kp_ref", "kp_cur", "inl", "pose"):
            assert np.array_equal(x[k], y[k]), "%s: %s of pair %d differs" % (what, k, j)
        assert not np.isnan(y["map"]).all(), "%s: the map of pair %d was never written" % (what, j)
        assert np.array_equal(x["map"].view(np.uint32), y["map"].view(np.uint32)), "%s: depth-difference map of pair %d differs" % (what, j)
        assert np.array_equal(x["rng"][1], y["rng"][1]) and x["rng"][2] == y["rng"][2], "%s: RandomState after pair %d" % (what, j)


@pytest.fixture(scope="module")
def mask_run(mods, world):
    """graphs on, run-ahead 3: shared by the tests below, never modified"""
    pmod, smod, _ = mods
    pipe = _mask_pipe(pmod, world)
    try:
        layout = pipe.stream_layout()
        ref0, recs = _chunk_run(smod, pipe, world["frames"])
    finally:
        pipe.close()
    return {"ref0": ref0, "recs": recs, "layout": layout}


# ---- 2. the mask in the pipeline, every stage on the device's own arrays ---------------------------------------------------------
def test_mask_stages_match_kernel_selection_and_oracle_chain(gpu, mods, world, mask_run, monkeypatch):
    K = world["K"]
    K32, Kinv32 = _K32(K)
    c = world["cfg"].kp_selection.local_bestN
    raw_ref, depth_ref = mask_run["ref0"]
    np.random.seed(4869)
    changed = 0
    for j, r in enumerate(mask_run["recs"]):
        # the map: the stand-alone kernel on the raw depths the pipeline reports and the pose it reports
        want = _run_plain(gpu, r["raw"], raw_ref, K32, Kinv32, r["pose"])[BAND:BAND + H * W].reshape(H, W)
        assert np.array_equal(r["map"].view(np.uint32), want.view(np.uint32)), "pair %d: the map is not the kernel's on these depths" % j
        assert np.abs(r["pose"] - np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1], [0, 0, 0, 1]])).max() <= 1e-5  # the constant drive
        # the selection: the masked restatement on the device's flow, consistency map and depth-difference map
        res = DC.local_bestN_masked(r["fwd"], r["diff"][..., None], r["map"], num_bestN=c.num_bestN, num_row=c.num_row, num_col=c.num_col,
                                    thre=c.thre, depth_thre=DEPTH_THRE, score_method=c.score_method)
        assert res["good_kp_found"] and r["out"].good_kp_found == 1, "pair %d has no good keypoints" % j
        assert np.array_equal(r["kp_ref"], res["kp1_best"][0]) and np.array_equal(r["kp_cur"], res["kp2_best"][0]), "keypoints, pair %d" % j
        plain = T.local_bestN(r["fwd"], r["diff"][..., None], num_bestN=c.num_bestN, num_row=c.num_row, num_col=c.num_col, thre=c.thre)
        changed += not np.array_equal(plain["kp1_best"], res["kp1_best"])
        # the chain: solve_pair's own branch rules on those keypoints
        monkeypatch.setattr(PO, "keypoints", lambda o, flow, diff, _res=res: (True, _res["kp1_best"][0], _res["kp2_best"][0]))
        o = PO.solve_pair({}, r["fwd"], r["diff"], r["dep"], depth_ref, K)
        out = r["out"]
        print("pair %d: status hip %d oracle %d | kp %d (unmasked %d) | scale hip %.12g oracle %.12g" % (
            j, out.status, o["status"], out.n_kp, plain["kp1_best"].shape[1], out.scale, o["scale"]))
        assert out.status == o["status"] and out.n_kp == len(res["kp1_best"][0])
        assert np.array_equal(r["inl"], o["inliers"]), "inlier mask, pair %d" % j
        if o["status"] == E:
            assert np.array_equal(r["R"], o["E"]["R"]) and np.array_equal(r["t"], o["E"]["t"]), "pair %d" % j
            assert out.best_inlier_cnt == o["E"]["best_inlier_cnt"] and out.scale_n_valid == o["scale_diag"]["n_valid"]
            assert abs(out.scale - o["scale"]) <= 1e-9 * abs(o["scale"])
        else:
            assert o["status"] == PNP
            pnp = o["pnp"]
            assert out.pnp_n_filtered == len(pnp["kp1"]) and out.pnp_inliers == pnp["best_inlier"]
            assert np.array_equal(r["R"], pnp["R"]) and np.array_equal(r["t"], pnp["t"]), "pair %d" % j
            rel, mode = mods[0].TrackingPipeline.hybrid_pose(out, np.eye(4))
            assert mode == "PnP" and np.abs(rel - pnp["pose"]).max() <= 1e-12
        want_rng = np.random.get_state()
        assert np.array_equal(r["rng"][1], want_rng[1]) and r["rng"][2] == want_rng[2], "RandomState diverged after pair %d" % j
        raw_ref, depth_ref = r["raw"], r["dep"]
    assert changed > 0, "the depth mask changed no selection: the test would pass without it"


# ---- 3. run-ahead equals lock-step ----------------------------------------------------------------------------------------------
def test_run_ahead_equals_lock_step(gpu, mods, world, mask_run):
    """with the nets three pairs ahead, pair k's mask is enqueued before track_end(k - 1): it must read the raw depth the
    previous enqueue_nets call left, as the lock-step run does"""
    pipe = _mask_pipe(mods[0], world)
    try:
        lock = _lockstep_run(pipe, world["frames"])
    finally:
        pipe.close()
    _same_runs(mask_run["recs"], lock, "run-ahead against lock-step")
    maps = [r["map"] for r in lock]
    assert all(not np.array_equal(a, b) for a, b in zip(maps, maps[1:]))  # a map per pair, not one repeated


def test_run_ahead_equals_lock_step_on_depth_images(gpu, mods, world, mask_run):
    """depth_source external: no depth net runs, so the pose net's feed image is made for it alone -- its poses are the
    depth-net run's, bit for bit -- and the mask reads the depth images' raw depths"""
    pmod, smod, _ = mods
    raws = [mask_run["ref0"][0]] + [r["raw"] for r in mask_run["recs"]]
    depths = [_d(DS.quantise(raw)) for raw in raws]
    kw = dict(depth_source="external", depth_scale=DS.QUANT_SCALE)
    pipe = _mask_pipe(pmod, world, **kw)
    try:
        ref0, ahead = _chunk_run(smod, pipe, world["frames"], depths=depths)
    finally:
        pipe.close()
    pipe = _mask_pipe(pmod, world, **kw)
    try:
        lock = _lockstep_run(pipe, world["frames"], depths=depths)
    finally:
        pipe.close()
    _same_runs(ahead, lock, "depth images: run-ahead against lock-step")
    K32, Kinv32 = _K32(world["K"])
    raw_ref = ref0[0]
    for j, (r, n) in enumerate(zip(ahead, mask_run["recs"])):
        assert np.array_equal(r["pose"], n["pose"]), "pair %d: the pose net saw another feed than under the depth net" % j
        assert np.array_equal(r["raw"], (DS.quantise(raws[j + 1]) / DS.QUANT_SCALE).astype(np.float32))
        want = _run_plain(gpu, r["raw"], raw_ref, K32, Kinv32, r["pose"])[BAND:BAND + H * W].reshape(H, W)
        assert np.array_equal(r["map"].view(np.uint32), want.view(np.uint32)), "pair %d" % j
        raw_ref = r["raw"]


# ---- 4. pose override -----------------------------------------------------------------------------------------------------------
def test_pose_override_and_its_withdrawal(gpu, mods, world, mask_run):
    pipe = _mask_pipe(mods[0], world)
    fr = world["frames"]
    K32, Kinv32 = _K32(world["K"])
    ov = _yaw_pose(2.0, (0.4, 0.0, 1.0))  # a 2 degree yaw and a lateral translation beside the drive
    d_ov = _d(ov)
    torch.cuda.synchronize()
    try:
        pipe.set_ref_image(fr[0])
        pipe.seed(4869)
        pipe.set_pose_override(0, d_ov)
        pipe.enqueue_nets(0, fr[0], fr[1])
        pipe.sync()
        pose, dmap = pipe.get_pose_net(0)
        raw = pipe.get_outputs(0)[3]
        assert np.array_equal(pose, ov)
        want = _run_plain(gpu, raw, mask_run["ref0"][0], K32, Kinv32, ov)[BAND:BAND + H * W].reshape(H, W)
        differ = dmap.view(np.uint32) != want.view(np.uint32)
        print("POSE OVERRIDE: %d of %d pixels of the map differ from the stand-alone kernel's, largest |difference| %.3e"
              % (int(differ.sum()), H * W, float(np.nanmax(np.abs(dmap - want)))))
        assert np.abs(dmap - want).max() <= 1e-5  # (this pose's map, whatever its last bits; they are asserted at the end)
        assert not np.array_equal(dmap, mask_run["recs"][0]["map"])  # (the net's pose gives another map)
        pipe.track(0)  # track_end withdraws the override
        pipe.enqueue_nets(0, None, fr[2])
        pipe.sync()
        pose, dmap = pipe.get_pose_net(0)
        assert np.array_equal(pose, mask_run["recs"][1]["pose"]) and np.array_equal(dmap, mask_run["recs"][1]["map"])
        pipe.track(0)
        pipe.set_pose_override(1, d_ov)
        pipe.set_pose_override(1, None)  # withdrawn by hand
        pipe.enqueue_nets(1, None, fr[3])
        pipe.sync()
        assert np.array_equal(pipe.get_pose_net(1)[0], mask_run["recs"][2]["pose"])
        pipe.track(1)
        assert not differ.any(), "the overridden pose's map is not the stand-alone kernel's bit for bit"
    finally:
        pipe.close()


# ---- 5. deep_pose tracking ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deep_world(gpu, tmp_path_factory):
    seq, cfg = _world(tmp_path_factory.mktemp("deep"), False, "deep_pose", False)
    return {"seq": seq, "cfg": cfg, "K": seq["K"], "frames": [_d(f) for f in seq["frames"]], "pose_sd": _pose_weights(False)}


@pytest.fixture(scope="module")
def deep_pipe(mods, world, deep_world):
    pmod = mods[0]
    assert pmod.options_from_cfg(deep_world["cfg"]) == {"tracking_method": "deep_pose", "pose_net": True}
    pipe = pmod.TrackingPipeline.from_cfg(deep_world["cfg"], deep_world["K"], world["flow_sd"], world["depth_sd"], FEED[0], FEED[1],
                                          pose_sd=deep_world["pose_sd"], seed=4869)
    yield pipe
    pipe.close()


def _posenet_host(gpu, sd, frames_u8):
    """dfvo_posenet_forward_images_host on consecutive frames: the class surface's forward_pose"""
    lib = gpu.lib()
    net = C.c_void_p()
    gpu.check(lib.dfvo_posenet_create(FEED[0], FEED[1], 5.4, None, C.byref(net)))
    try:
        gpu.set_params(lib.dfvo_posenet_set_param, net, {k: v.detach().cpu().float().numpy() for k, v in sd.items()
                                                         if v.dim() > 0 and "num_batches_tracked" not in k and not k.startswith("encoder.fc")})
        gpu.check(lib.dfvo_posenet_finalize(net))
        poses = []
        for a, b in zip(frames_u8, frames_u8[1:]):
            pose = np.full((4, 4), np.nan, np.float32)
            gpu.check(lib.dfvo_posenet_forward_images_host(net, gpu.as_ptr(np.ascontiguousarray(a)), gpu.as_ptr(np.ascontiguousarray(b)),
                                                           H, W, gpu.as_ptr(pose)))
            poses.append(pose)
        return poses
    finally:
        lib.dfvo_posenet_destroy(net)


def test_deep_pose_tracking(gpu, mods, deep_world, deep_pipe):
    pmod, smod, dmod = mods
    pipe, fr = deep_pipe, deep_world["frames"]
    pipe.seed(4869)
    rng0 = pipe.get_rng_state()
    outs = []
    traj, gathered = smod.run_sequence(pipe, fr, N_FRAMES, seed=4869, collect=lambda j, out: outs.append(out))
    rng1 = pipe.get_rng_state()
    assert np.array_equal(rng0[1], rng1[1]) and rng0[2] == rng1[2], "deep_pose tracking drew from the RandomState"
    assert [o.status for o in outs] == [DEEP] * N_PAIRS and list(gathered[:, 16]) == [DEEP] * N_PAIRS
    assert all(o.scale == 1.0 and o.n_kp == 0 for o in outs)
    want = _posenet_host(gpu, deep_world["pose_sd"], deep_world["seq"]["frames"])
    g = np.eye(4)
    for j, (o, p32) in enumerate(zip(outs, want)):
        assert np.isfinite(p32).all() and np.array_equal(p32[3], [0, 0, 0, 1])
        Rt = np.concatenate([np.array(o.R[:]).reshape(3, 3), np.array(o.t[:]).reshape(3, 1)], 1)
        assert np.array_equal(Rt, p32[:3].astype(np.float64)), "pair %d: not the pose net's matrix" % j
        assert np.array_equal(gathered[j, :16].reshape(4, 4), p32.astype(np.float64))
        if j >= N_PAIRS - smod.SLOTS:  # (the slots still hold the last four pairs)
            assert np.array_equal(pipe.get_pose_net(j % smod.SLOTS)[0], p32)
        g = g @ p32.astype(np.float64)
        assert np.abs(traj[j + 1] - g).max() <= 1e-12
    assert len({p.tobytes() for p in want}) == N_PAIRS  # a prediction per pair, not one repeated
    # two ranks' chunks, tracked in this process and joined, are the single-chunk run exactly
    rows = []
    for rank in range(2):
        lo, hi = dmod.chunk_bounds(N_PAIRS, 2, rank)
        rel, status = smod.track_chunk(pipe, fr, lo, hi, seed=4869, rng_mode="per_pair")
        rows.append(dmod.pack_rows(rel, status))
    joined = np.concatenate(rows, 0)
    assert np.array_equal(joined, gathered)
    assert np.array_equal(dmod.compose_trajectory(joined), traj)


# ---- 6. graphs ------------------------------------------------------------------------------------------------------------------
def test_mask_pipeline_graphs_off_equals_graphs_on(gpu, mods, world, mask_run):
    pmod, smod, _ = mods
    pipe = _mask_pipe(pmod, world)
    try:
        ref0, off = _chunk_run(smod, pipe, world["frames"], graph=0)
    finally:
        pipe.close()
    assert np.array_equal(ref0[0], mask_run["ref0"][0]) and np.array_equal(ref0[1], mask_run["ref0"][1])
    _same_runs(mask_run["recs"], off, "graphs on against graphs off")
    for a, b in zip(mask_run["recs"], off):
        for k in ("fwd", "diff", "raw", "dep"):
            assert np.array_equal(a[k], b[k])
    for a, b in zip(off, off[1:]):  # the frames change every pair: a stale replay cannot equal the eager run
        assert not np.array_equal(a["raw"], b["raw"]) and not np.array_equal(a["map"], b["map"])


# ---- 7. off means off -----------------------------------------------------------------------------------------------------------
ROLES = {"text", "layout", "groups", "queues", "streams", "trk", "rep0", "rep1", "depth", "pre0", "pre1", "flow", "flow_x"}


def test_off_means_off(gpu, mods, world, mask_run):
    """a pipeline without pose options has no pose lane to ask for, and neither it nor the mask pipeline has a new stream role
    (what it computes is pinned by the existing pipeline tests)"""
    pipe = mods[0].TrackingPipeline(H, W, FEED[0], FEED[1], world["K"], world["flow_sd"], world["depth_sd"], seed=4869)
    try:
        lay = pipe.stream_layout()
        assert set(lay) == ROLES and set(mask_run["layout"]) == ROLES
        lib = gpu.lib()
        pose = np.zeros(16, np.float32)
        assert lib.dfvo_pipeline_get_pose_net(pipe.h, 0, gpu.as_ptr(pose), None) == -2 and b"not on" in lib.dfvo_last_error()
        assert lib.dfvo_pipeline_set_pose_override(pipe.h, 0, None) == -2 and b"not on" in lib.dfvo_last_error()
        fr = world["frames"]
        pipe.set_ref_image(fr[0])
        pipe.seed(4869)
        pipe.enqueue_nets(0, fr[0], fr[1])
        out = pipe.track(0)
        r = mask_run["recs"][0]
        fwd, _, diff, raw, dep = pipe.get_outputs(0)
        for k, a in (("fwd", fwd), ("diff", diff), ("raw", raw), ("dep", dep)):  # the nets' maps do not know about the lane
            assert np.array_equal(a, r[k]), k
        c = world["cfg"].kp_selection.local_bestN
        plain = T.local_bestN(fwd, diff[..., None], num_bestN=c.num_bestN, num_row=c.num_row, num_col=c.num_col, thre=c.thre)
        kp_ref, kp_cur, _ = pipe.get_keypoints(0)
        assert out.good_kp_found == 1 and np.array_equal(kp_ref, plain["kp1_best"][0]) and np.array_equal(kp_cur, plain["kp2_best"][0])
    finally:
        pipe.close()


# ---- 8. refusals by name --------------------------------------------------------------------------------------------------------
def test_refusals_by_name(gpu, mods, world, deep_world, deep_pipe):
    pmod = mods[0]
    lib = gpu.lib()
    fr = world["frames"]
    with pytest.raises(ValueError, match="pose_sd"):
        pmod.TrackingPipeline(H, W, FEED[0], FEED[1], world["K"], world["flow_sd"], world["depth_sd"], pose_net=True)
    with pytest.raises(ValueError, match="kp_source"):
        pmod.TrackingPipeline(H, W, FEED[0], FEED[1], world["K"], world["flow_sd"], world["depth_sd"], pose_sd=world["pose_sd"],
                              pose_net=True, depth_consistency=True, kp_source="bestN")
    on = gpu.PipelinePoseOpts(enable=1, depth_consistency=1, depth_thre=0.01)
    pipe = pmod.TrackingPipeline(H, W, FEED[0], FEED[1], world["K"], world["flow_sd"], world["depth_sd"], seed=4869, kp_source="bestN")
    try:
        # the library's own refusal of the mask over another keypoint source, in either order of the two setters
        assert lib.dfvo_pipeline_set_pose_net(pipe.h, C.byref(on)) == -2 and b"LOCAL_BESTN" in lib.dfvo_last_error()
        assert lib.dfvo_pipeline_set_pose_net(pipe.h, C.byref(gpu.PipelinePoseOpts(enable=0, depth_consistency=1))) == -2
        assert b"depth_consistency needs enable" in lib.dfvo_last_error()
        assert lib.dfvo_pipeline_set_pose_net(pipe.h, None) == -2
        po = gpu.PipelineOpts(tracking_method=2)  # deep_pose tracking without the net
        po.flow_crop[1] = po.flow_crop[3] = 1.0
        assert lib.dfvo_pipeline_set_options(pipe.h, C.byref(po)) == -2 and b"tracking_method" in lib.dfvo_last_error()
        pipe.set_ref_image(fr[0])  # the pipeline has started
        with pytest.raises(gpu.DfvoError, match="dfvo_pipeline_set_pose_net: comes before the first"):
            gpu.check(lib.dfvo_pipeline_set_pose_net(pipe.h, C.byref(gpu.PipelinePoseOpts(enable=1))))
    finally:
        pipe.close()
    with pytest.raises(gpu.DfvoError, match="dfvo_pipeline_get_keypoints: tracking_method DFVO_TRACKING_DEEP_POSE"):
        deep_pipe.get_keypoints(0)
    with pytest.raises(gpu.DfvoError, match="dfvo_pipeline_get_flow: tracking_method DFVO_TRACKING_DEEP_POSE"):
        deep_pipe.get_outputs(0)
    deep_pipe.prefetch_track(0)  # accepted, does nothing
    deep_pipe.prefetch_track(0)
    # the mask without a reference raw depth: refused before anything of the pair is enqueued
    pipe = _mask_pipe(pmod, world)
    try:
        with pytest.raises(gpu.DfvoError, match="reference frame's raw depth"):
            pipe.enqueue_nets(0, fr[0], fr[1])
        pipe.set_ref_image(fr[0])
        pipe.enqueue_nets(0, fr[0], fr[1])
        assert pipe.track(0).good_kp_found == 1
    finally:
        pipe.close()
