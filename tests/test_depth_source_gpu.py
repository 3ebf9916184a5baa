"""GPU: depth.depth_src gt -- 16-bit sensor depth images in the place of the depth net.

  1. dfvo_read_depth_u16 against the reference's arithmetic restated in numpy float64 (tests/depth_source_cases.py), bit for bit
  2. a pipeline of depth_source "external", fed the images, against a pipeline of the depth net fed the restated maps as
     overrides (which the existing tests pin to the oracle's chain): everything equal after every pair
  3. the calls of the other mode are refused by name, and the pipeline tracks on
  4. the sequence driver with depths: track_chunk against the hand-written loop, run_sequence over two ranks against one

The statuses the cases of (2) name were computed with the CPU oracle (pipeline_configs_oracle / pipeline_iter_oracle.solve_pair
on the restated depths, quantised at scale 500) when the cases were written: a case that lands in another branch fails."""
import importlib

import numpy as np
import pytest
import torch

import depth_source_cases as DC
from oracle import nets_torch as O
from pipeline_configs_oracle import H, W, SOURCES
from test_pipeline_configs_gpu import scene

pytestmark = pytest.mark.gpu

E, PNP = 0, 3  # DFVO_TRACK_E, DFVO_TRACK_PNP
FLOW_OPEN = dict(validity="flow", validity_thre=1.0)
CROP = [[0.3, 1], [0, 1]]   # DEFAULTS["depth_crop"]
RANGE = (0.0, 50.0)         # DEFAULTS["min_depth"], ["max_depth"]


@pytest.fixture(scope="module")
def mods(gpu):
    return importlib.import_module("df-vo_amd.pipeline"), importlib.import_module("df-vo_amd.sequence")


@pytest.fixture(scope="module")
def weights():
    return O.liteflownet_state_dict(4869), O.monodepth2_state_dict(4869)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the operator ----------------------------------------------------------------------------------------------------
GUARD = 64  # elements behind each output that must stay untouched


def _read_depth(gpu, src, scale, H_, W_, crop, depth_range, offset=0):
    """(raw, proc) of dfvo_read_depth_u16; offset 1 puts both outputs one element off their 16-byte alignment (the kernel's
    element-by-element path).  The elements around the maps are checked to be untouched."""
    h, w = src.shape
    n = H_ * W_
    d = _d(src)
    raw = torch.full((offset + n + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    proc = torch.full((offset + n + GUARD,), -7.0, dtype=torch.float64, device="cuda")
    y0, y1, x0, x1 = DC.crop_box(crop, H_, W_)
    torch.cuda.synchronize()
    gpu.check(gpu.lib().dfvo_read_depth_u16(d.data_ptr(), h, w, float(scale), H_, W_, y0, y1, x0, x1, float(depth_range[0]),
                                            float(depth_range[1]), raw.data_ptr() + 4 * offset, proc.data_ptr() + 8 * offset, None))
    torch.cuda.synchronize()
    raw, proc = raw.cpu().numpy(), proc.cpu().numpy()
    for a in (raw, proc):
        assert (a[:offset] == -7).all() and (a[offset + n:] == -7).all(), "a write outside the map"
    return raw[offset:offset + n].reshape(H_, W_), proc[offset:offset + n].reshape(H_, W_)


@pytest.mark.parametrize("size", list(DC.SIZES))
def test_read_depth_u16_bit_exact(gpu, size):
    (h, w), (H_, W_) = DC.SIZES[size]
    for i, scale in enumerate(DC.SCALES):
        src, planted = DC.source_image(40 + i, size, scale)
        assert DC.planted_survive(src, planted, scale, H_, W_), "a planted boundary value vanished in the resampling"
        for name in DC.CROPS:
            crop = DC.crop_fractions(name, H_, W_)
            want_raw, want_proc = DC.read_depth_ref(src, scale, H_, W_, crop, DC.DEPTH_RANGE)
            raw, proc = _read_depth(gpu, src, scale, H_, W_, crop, DC.DEPTH_RANGE)
            tag = "%s scale %d crop %s" % (size, scale, name)
            assert raw.dtype == want_raw.dtype and np.array_equal(raw, want_raw), tag
            assert proc.dtype == want_proc.dtype and np.array_equal(proc, want_proc), tag
            if name != "one_pixel":
                for Y, X, u in planted:  # (stated once more on the device's own output)
                    v = u / scale
                    assert raw[Y, X] == np.float32(v) and proc[Y, X] == (v if DC.DEPTH_RANGE[0] < v < DC.DEPTH_RANGE[1] else 0.0), (tag, u)


@pytest.mark.parametrize("size", ["odd up", "tiny"])
def test_read_depth_u16_unaligned_outputs(gpu, size):
    """output maps that do not start on a 16-byte boundary take the kernel's narrow stores: same values, nothing outside"""
    (h, w), (H_, W_) = DC.SIZES[size]
    src, _ = DC.source_image(77, size, 500)
    crop = DC.crop_fractions("default", H_, W_)
    want_raw, want_proc = DC.read_depth_ref(src, 500, H_, W_, crop, DC.DEPTH_RANGE)
    raw, proc = _read_depth(gpu, src, 500, H_, W_, crop, DC.DEPTH_RANGE, offset=1)
    assert np.array_equal(raw, want_raw) and np.array_equal(proc, want_proc)


def test_read_depth_u16_default_range_and_sensor_holes(gpu):
    """the pipeline's own range (0, 50) at KITTI's scale: 25000 / 500 IS max_depth and is dropped, 24999 kept; 0, a sensor
    hole, fails `> min_depth` and gives 0 in both maps"""
    src = np.array([[0, 1, 24999], [25000, 25001, 65535]], np.uint16)
    raw, proc = _read_depth(gpu, src, 500, 2, 3, [[0, 1], [0, 1]], RANGE)
    want_raw, want_proc = DC.read_depth_ref(src, 500, 2, 3, [[0, 1], [0, 1]], RANGE)
    assert np.array_equal(raw, want_raw) and np.array_equal(proc, want_proc)
    assert proc.tolist() == [[0.0, 1 / 500, 24999 / 500], [0.0, 0.0, 0.0]] and raw[1, 0] == 50.0 and raw[0, 0] == 0.0


# ---- 2. external mode against override mode -------------------------------------------------------------------------------
_plans = {}


class Plan:
    """the 16-bit images of a scene's frames -- [0] the first reference frame, [f + 1] the current frame of pair f -- and their
    restated (raw, proc) maps, computed once per (scene, half, zero pairs) and left unchanged"""

    def __init__(self, name, half, zero):
        sc = scene(name)
        q = lambda d: DC.quantise(d[::2, ::2] if half else d)
        u_ref, u_cur = q(sc["depth_ref"]), q(sc["depth_cur"])
        self.sc = sc
        self.size = u_cur.shape
        self.u = [u_ref] + [np.zeros_like(u_cur) if f in zero else u_cur for f in range(3)]
        self.maps = [DC.read_depth_ref(u, DC.QUANT_SCALE, H, W, CROP, RANGE) for u in self.u]


def plan(name, half=False, zero=()):
    key = (name, half, tuple(zero))
    if key not in _plans:
        _plans[key] = Plan(*key)
    return _plans[key]


class Dev:
    def __init__(self, pl):
        rng = np.random.Generator(np.random.PCG64(11))
        ref, cur = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))  # (the flow net's outputs are overridden)
        self.ref, self.cur, self.flow, self.diff = _d(ref), _d(cur), _d(pl.sc["flow"]), _d(pl.sc["diff"])
        self.u = [_d(u) for u in pl.u]
        self.raw = [_d(r) for r, _ in pl.maps]
        self.proc = [_d(p) for _, p in pl.maps]
        torch.cuda.synchronize()


def make_pair(pmod, weights, pl, o):
    """(A: external depth, no depth weights; B: the depth net, to be fed overrides), same options, same seed"""
    K = pl.sc["K"]
    a = pmod.TrackingPipeline(H, W, 64, 96, K, weights[0], None, seed=4869, depth_source="external", depth_scale=DC.QUANT_SCALE,
                              depth_size=pl.size, **o)
    try:
        b = pmod.TrackingPipeline(H, W, 64, 96, K, weights[0], weights[1], seed=4869, **o)
    except Exception:
        a.close()
        raise
    return a, b


def set_refs(a, b, dev):
    a.set_ref_depth_image(dev.u[0])
    b.set_ref_depth(depth=dev.proc[0], raw_depth=dev.raw[0])


def track_pair(pipe, external, dev, frame, split):
    """pair `frame` through slot frame % 2; split: prefetch_track and track_begin / track_end"""
    slot = frame % 2
    if external:
        pipe.enqueue_nets(slot, dev.ref, dev.cur, depth=dev.u[frame + 1])
        kw = {}
    else:
        pipe.enqueue_nets(slot, dev.ref, dev.cur)
        kw = dict(depth=dev.proc[frame + 1], raw_depth=dev.raw[frame + 1])
    if not split:
        return pipe.track(slot, dev.flow, dev.diff, **kw)
    pipe.prefetch_track(slot, dev.flow, dev.diff)
    pipe.track_begin(slot, dev.flow, dev.diff, **kw)
    return pipe.track_end(slot)


def out_fields(gpu, out):
    return {n: (list(getattr(out, n)) if hasattr(getattr(out, n), "__len__") else getattr(out, n)) for n, _ in gpu.TrackOut._fields_}


def same_state(gpu, a, b, oa, ob, slot, tag, iterative=False):
    """everything a pair leaves behind, equal in both pipelines"""
    fa, fb = out_fields(gpu, oa), out_fields(gpu, ob)
    assert fa == fb, "%s: TrackOut %s" % (tag, {k: (fa[k], fb[k]) for k in fa if fa[k] != fb[k]})
    for x, y in zip(a.get_keypoints(slot), b.get_keypoints(slot)):
        assert np.array_equal(x, y), tag + ": keypoints / inlier mask"
    sa, sb = a.get_rng_state(), b.get_rng_state()
    assert np.array_equal(sa[1], sb[1]) and sa[2] == sb[2], tag + ": RandomState"
    for x, y in zip(a.get_ref_depth(), b.get_ref_depth()):
        assert np.array_equal(x, y), tag + ": reference depth"
    if iterative:
        ia, ib = a.get_iterative(slot), b.get_iterative(slot)
        for k in ia:
            if isinstance(ia[k], (list, np.ndarray)):  # (rounds that did not run may hold NaN)
                same = np.array_equal(np.asarray(ia[k], np.float64), np.asarray(ib[k], np.float64), equal_nan=True)
            else:
                same = ia[k] == ib[k]
            assert same, "%s: iterative record %s" % (tag, k)
        assert a.get_prev_scale() == b.get_prev_scale(), tag + ": prev_scale"


def run_case(gpu, pmod, weights, pl, o, want_status):
    iterative = o.get("scale_recovery") == "iterative"
    dev = Dev(pl)
    a, b = make_pair(pmod, weights, pl, o)
    try:
        set_refs(a, b, dev)
        for x, y, m in zip(a.get_ref_depth(), b.get_ref_depth(), pl.maps[0]):
            assert np.array_equal(x, m) and np.array_equal(y, m), "first reference depth"
        for frame in range(3):
            tag = "pair %d" % frame
            oa = track_pair(a, True, dev, frame, split=frame == 1)
            ob = track_pair(b, False, dev, frame, split=frame == 1)
            a.sync()
            b.sync()
            print("%s: status %d / %d | kp %d | scale %.12g | scale inliers %d | pnp inliers %d" % (
                tag, oa.status, ob.status, oa.n_kp, oa.scale, oa.scale_n_inliers, oa.pnp_inliers))
            raw, proc = a.get_outputs(frame % 2)[3:5]
            want_raw, want_proc = pl.maps[frame + 1]
            assert np.array_equal(raw, want_raw) and np.array_equal(proc, want_proc), tag + ": the slot's depths against the restatement"
            same_state(gpu, a, b, oa, ob, frame % 2, tag, iterative)
            assert np.array_equal(a.get_ref_depth()[1], want_proc), tag + ": the roll-over"
            if iterative:
                assert np.array_equal(a.get_ref_depth()[0], want_raw), tag + ": the raw roll-over"
            assert oa.status == want_status[frame], "%s left the branch this case is about (status %d)" % (tag, oa.status)
            assert oa.good_kp_found == 1 and oa.n_kp > 0
            if oa.status == E:
                assert oa.scale_n_inliers > 0 and oa.scale > 0
            else:
                assert oa.pnp_n_filtered > 0
        flops_a, flops_b = a.net_flops(), b.net_flops()
        assert 0 < flops_a < flops_b, "external depth counts the flow net only"
    finally:
        a.close()
        b.close()


# (scene, half-size source, all-zero depth images, options, the status of every pair)
CASES = [
    ("rigid", False, (), {}, (PNP, PNP, PNP)),  # default_configuration.yml: GRIC rejects E on this scene, PnP on the image's depth
    ("sideways", False, (), {}, (PNP, PNP, PNP)),
    ("rigid", False, (), dict(FLOW_OPEN), (E, E, E)),  # the default keys on the E + scale path
    ("sideways", False, (), dict(FLOW_OPEN), (E, E, E)),
    ("rigid", True, (), dict(FLOW_OPEN), (E, E, E)),  # a 64 x 208 source, quantised from the 2x-decimated map
    ("rigid", False, (), dict(SOURCES["sampled"]), (PNP, PNP, PNP)),
    ("sideways", False, (), dict(SOURCES["sampled"], **FLOW_OPEN), (E, E, E)),
    ("rigid", False, (), dict(scale_method="abs_diff", **FLOW_OPEN), (E, E, E)),
    ("rigid", False, (), dict(tracking_method="PnP"), (PNP, PNP, PNP)),
    ("rigid", False, (), dict(scale_recovery="iterative", iter_kp_src="kp_best", **FLOW_OPEN), (E, E, E)),
    ("sideways", False, (), dict(scale_recovery="iterative", iter_kp_src="kp_depth", **FLOW_OPEN), (E, E, E)),
    # the middle pair's image is all holes: no scale, and the PnP fallback reads the reference depth that pair 0's image left
    ("rigid", False, (1,), dict(FLOW_OPEN), (E, PNP, E)),
]


def _case_id(c):
    name, half, zero, o, _ = c
    return "-".join([name] + (["half"] if half else []) + (["zero%d" % z for z in zero]) + [
        "%s" % v for k, v in sorted(o.items()) if k not in ("kp_num_bestN", "kp_sampled_num", "flow_crop")])


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_external_depth_equals_override_mode(gpu, mods, weights, case):
    name, half, zero, o, want = case
    run_case(gpu, mods[0], weights, plan(name, half, zero), o, want)


# ---- 3. mode errors -----------------------------------------------------------------------------------------------------
def test_calls_of_the_other_mode_are_refused_by_name(gpu, mods, weights):
    pmod = mods[0]
    pl = plan("rigid")
    dev = Dev(pl)
    feed = _d(np.zeros((64, 96, 3), np.uint8))
    o = dict(FLOW_OPEN)
    a, b = make_pair(pmod, weights, pl, o)
    try:
        set_refs(a, b, dev)
        refusals_a = [("enqueue_nets", lambda: a.enqueue_nets(0, dev.ref, dev.cur)),
                      ("enqueue_nets", lambda: a.enqueue_nets(0, dev.ref, dev.cur, d_feed=feed)),
                      ("enqueue_nets", lambda: a.enqueue_nets(0, dev.ref, dev.cur, d_feed=feed, depth=dev.u[1])),
                      ("enqueue_nets", lambda: a.enqueue_nets(0, dev.ref, dev.cur, depth=dev.u[1][:-1])),  # a wrong shape
                      ("enqueue_nets", lambda: a.enqueue_nets(0, dev.ref, dev.cur, depth=dev.raw[1])),     # a wrong dtype
                      ("set_ref_image", lambda: a.set_ref_image(dev.ref)),
                      ("set_ref_depth", lambda: a.set_ref_depth(d_feed=feed))]
        refusals_b = [("enqueue_nets", lambda: b.enqueue_nets(0, dev.ref, dev.cur, depth=dev.u[1])),
                      ("set_ref_depth_u16", lambda: b.set_ref_depth_image(dev.u[0]))]
        for call_name, call in refusals_a + refusals_b:
            with pytest.raises(gpu.DfvoError, match=call_name):
                call()
        # the library's refusals name the mode as well
        for call in (refusals_a[0][1], refusals_a[5][1], refusals_a[6][1]):
            assert "DFVO_DEPTH_EXTERNAL" in str(_raises(gpu, call))
        for _, call in refusals_b:
            assert "DFVO_DEPTH_NET" in str(_raises(gpu, call))
        # ... and both still track: three pairs, equal as in (2)
        for frame in range(3):
            if frame == 1:  # a refusal between two pairs changes nothing either
                for _, call in refusals_a + refusals_b:
                    with pytest.raises(gpu.DfvoError):
                        call()
            oa = track_pair(a, True, dev, frame, split=frame == 1)
            ob = track_pair(b, False, dev, frame, split=frame == 1)
            same_state(gpu, a, b, oa, ob, frame % 2, "pair %d" % frame)
            assert oa.status == E and oa.n_kp > 0 and oa.scale_n_inliers > 0
            assert np.array_equal(a.get_outputs(frame % 2)[4], pl.maps[frame + 1][1])
        # the depth source is final once the pipeline is built
        ds = gpu.PipelineDepthSrc(source=gpu.DEPTH_NET)
        import ctypes as C
        assert gpu.lib().dfvo_pipeline_set_depth_source(a.h, C.byref(ds)) == -2
        assert b"dfvo_pipeline_set_depth_source" in gpu.lib().dfvo_last_error()
    finally:
        a.close()
        b.close()


def _raises(gpu, call):
    with pytest.raises(gpu.DfvoError) as e:
        call()
    return e.value


# ---- 4. the sequence driver ---------------------------------------------------------------------------------------------
N_FRAMES = 5


@pytest.fixture(scope="module")
def sequence(mods):
    """five random frames and five different depth images (the rigid scene's, shifted per frame)"""
    smod = mods[1]
    rng = np.random.Generator(np.random.PCG64(5))
    frames = smod.frames_to_device([rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N_FRAMES)])
    u = DC.quantise(scene("rigid")["depth_cur"])
    depths = [smod.depth_to_device(np.roll(u, 9 * i, axis=1)) for i in range(N_FRAMES)]
    assert depths[0].dtype == torch.uint16 and depths[0].is_cuda and tuple(depths[0].shape) == (H, W)
    return frames, depths


def external_pipe(pmod, weights, **o):
    return pmod.TrackingPipeline(H, W, 64, 96, scene("rigid")["K"], weights[0], None, seed=4869, depth_source="external",
                                 depth_scale=DC.QUANT_SCALE, **o)


def test_track_chunk_with_depths_equals_the_hand_written_loop(gpu, mods, weights, sequence):
    """no overrides (untrained weights on noise: kp_thre is opened so that keypoints are selected, and a flow gate that stays
    closed sends every pair to the PnP fallback, on the previous frame's image)"""
    pmod, smod = mods
    frames, depths = sequence
    pipe = external_pipe(pmod, weights, kp_thre=1e9, validity="flow", validity_thre=1e3)
    try:
        seen = []
        rel, status = smod.track_chunk(pipe, frames, 0, 4, depths=depths, collect=lambda j, out: seen.append(out_fields(gpu, out)))
        rng_chunk = pipe.get_rng_state()
        ref_chunk = pipe.get_ref_depth()[1]
        pipe.set_ref_depth_image(depths[0])
        pipe.seed(4869)
        for j in range(4):
            pipe.enqueue_nets(j % smod.SLOTS, frames[j] if j == 0 else None, frames[j + 1], depth=depths[j + 1])
            out = pipe.track(j % smod.SLOTS)
            assert out_fields(gpu, out) == seen[j], "pair %d" % j
            assert out.n_kp > 0 and out.status == status[j]
            if out.status != 1:
                assert np.array_equal(pmod.TrackingPipeline.hybrid_pose(out, np.eye(4))[0], rel[j])
            want = DC.read_depth_ref(depths[j + 1].cpu().numpy(), DC.QUANT_SCALE, H, W, CROP, RANGE)[1]
            assert np.array_equal(pipe.get_outputs(j % smod.SLOTS)[4], want), "pair %d tracks on depths[%d]" % (j, j + 1)
        rng_loop = pipe.get_rng_state()
        assert np.array_equal(rng_chunk[1], rng_loop[1]) and rng_chunk[2] == rng_loop[2]
        assert np.array_equal(ref_chunk, pipe.get_ref_depth()[1])
        assert list(status) == [PNP] * 4, "a pair did not read the reference depth"
    finally:
        pipe.close()


def test_run_sequence_over_two_ranks_equals_one(gpu, mods, weights, sequence):
    """world 2, rng_mode per_pair, two pipelines on the one device, tracking_method PnP so that every pair
    reads its reference depth: rank 1's first pair reads its halo, depths[lo], and the rows equal the single rank's"""
    pmod, smod = mods
    frames, depths = sequence
    o = dict(kp_thre=1e9, tracking_method="PnP")
    one = external_pipe(pmod, weights, **o)
    try:
        outs = {}
        _, whole = smod.run_sequence(one, frames, N_FRAMES, rng_mode="per_pair", depths=depths,
                                     collect=lambda j, out: outs.setdefault(j, out_fields(gpu, out)))
    finally:
        one.close()
    assert whole.shape == (N_FRAMES - 1, 17) and (whole[:, 16] == PNP).all()
    assert all(outs[j]["pnp_n_filtered"] > 0 and outs[j]["n_kp"] > 0 for j in range(N_FRAMES - 1))
    ranks = [external_pipe(pmod, weights, **o) for _ in range(2)]
    try:
        parts = [smod.run_sequence(p, frames, N_FRAMES, world=2, rank=r, rng_mode="per_pair", depths=depths)[1] for r, p in enumerate(ranks)]
    finally:
        for p in ranks:
            p.close()
    assert [len(p) for p in parts] == [2, 2]
    assert np.array_equal(np.concatenate(parts, 0), whole)
    # the halo is what decides rank 1's first row: on another frame's depth it comes out differently
    wrong = external_pipe(pmod, weights, **o)
    try:
        shifted = {2: depths[0], 3: depths[3], 4: depths[4]}
        other = smod.run_sequence(wrong, frames, N_FRAMES, world=2, rank=1, rng_mode="per_pair", depths=shifted)[1]
    finally:
        wrong.close()
    assert not np.array_equal(other[0], whole[2]) and np.array_equal(other[1], whole[3])
