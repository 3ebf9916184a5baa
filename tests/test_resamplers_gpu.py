"""GPU: the resamplers between the decoded frame and the nets and between the nets and the solvers, at sizes where they
really resample (tests/resample_cases.py; tests/test_resamplers_cpu.py proves the cases sharp).
  dfvo_depth_postprocess       bit for bit against cv2_shim.resize(INTER_NEAREST) + the oracle's preprocess_depth
  dfvo_read_image_tail_u8      bit for bit against cv2_shim.resize of the contiguous cropped RGB frame
  dfvo_img_u8_to_flow_input,   per element against float64 inside the bounds of tests/flow_bounds.py, both down-sampling
  dfvo_flow_post
Every output buffer is 256 elements longer than the output and filled with a sentinel no correct output holds: every
output element must have been written and the tail must be untouched."""
import importlib

import numpy as np
import pytest
import torch

import resample_cases as RC
from oracle import nets_torch as O
from oracle.pil_resample import resize_lanczos_u8
from synth import image_pair, rigid_scene
from util import ptr

pytestmark = pytest.mark.gpu

TAIL = 256
F32_SENTINEL = 0x7FC0DEAD           # a NaN with a payload no arithmetic produces (the canonical NaN is 0x7FC00000)
F64_SENTINEL = 0x7FF8DEAD0000BEEF
U8_SENTINEL = 165                   # the frame tail's correct outputs are below 64 (tail_frame)


def _f32_buf(n):
    return torch.full((n + TAIL,), F32_SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _f64_buf(n):
    return torch.full((n + TAIL,), F64_SENTINEL, dtype=torch.int64, device="cuda").view(torch.float64)


def _split_f32(buf, n, what):
    """the first n floats of buf as numpy, after checking that all were written and the tail was not"""
    bits = buf.view(torch.int32).cpu().numpy().view(np.uint32)
    assert (bits[n:] == F32_SENTINEL).all(), "%s: wrote behind the output" % what
    assert (bits[:n] != F32_SENTINEL).all(), "%s: %d output elements not written" % (what, int((bits[:n] == F32_SENTINEL).sum()))
    return bits[:n].view(np.float32)


def _split_f64(buf, n, what):
    bits = buf.view(torch.int64).cpu().numpy().view(np.uint64)
    assert (bits[n:] == F64_SENTINEL).all(), "%s: wrote behind the output" % what
    assert (bits[:n] != F64_SENTINEL).all(), "%s: %d output elements not written" % (what, int((bits[:n] == F64_SENTINEL).sum()))
    return bits[:n].view(np.float64)


# ---- depth post -------------------------------------------------------------------------------------------------------
def _depth_post(gpu, depth, H, W, crop, depth_range):
    h, w = depth.shape
    y0, y1, x0, x1 = RC.crop_box(crop, H, W)
    src = torch.from_numpy(np.ascontiguousarray(depth)).cuda()
    raw, proc = _f32_buf(H * W), _f64_buf(H * W)
    gpu.check(gpu.lib().dfvo_depth_postprocess(ptr(src), h, w, H, W, y0, y1, x0, x1, depth_range[0], depth_range[1], ptr(raw),
                                               ptr(proc), None))
    torch.cuda.synchronize()
    return _split_f32(raw, H * W, "raw").reshape(H, W), _split_f64(proc, H * W, "proc").reshape(H, W)


def _check_depth(tag, got, want):
    (raw, proc), (want_raw, want_proc) = got, want
    assert raw.dtype == want_raw.dtype == np.float32 and proc.dtype == want_proc.dtype == np.float64, tag
    bad = raw.view(np.uint32) != want_raw.view(np.uint32)
    assert not bad.any(), "%s: raw differs in %d elements, first at %s" % (tag, int(bad.sum()), np.argwhere(bad)[0])
    bad = proc != want_proc
    assert not bad.any(), "%s: proc differs in %d elements, first at %s" % (tag, int(bad.sum()), np.argwhere(bad)[0])
    assert ((proc == 0) | (proc == raw.astype(np.float64))).all(), tag
    assert not np.signbit(proc).any(), tag


@pytest.mark.parametrize("size", RC.DEPTH_SIZES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_depth_post_bit_exact(gpu, size):
    (h, w), (H, W) = size
    d = RC.depth_input(h, w)
    for name in RC.CROPS:
        crop = RC.crop_fractions(name, H, W)
        _check_depth("%s %s" % (size, name), _depth_post(gpu, d, H, W, crop, RC.DEPTH_RANGE),
                     RC.depth_post_ref(d, H, W, crop, RC.DEPTH_RANGE))


@pytest.mark.parametrize("depth_range", RC.RANGES, ids=lambda r: "%g-%g" % r)
def test_depth_post_range_mask_is_strict_and_float32(gpu, depth_range):
    tag, d, H, W, crop, rng = next(c for c in RC.range_cases() if c[5] == depth_range)
    got, want = _depth_post(gpu, d, H, W, crop, rng), RC.depth_post_ref(d, H, W, crop, rng)
    _check_depth(tag, got, want)
    raw, proc = got
    lo, hi = np.float32(rng[0]), np.float32(rng[1])
    assert (proc[(raw == lo) | (raw == hi) | (raw <= 0)] == 0).all()
    for edge, inside in ((lo, np.float32(np.inf)), (hi, -np.float32(np.inf))):
        v = np.nextafter(edge, inside)
        assert (raw == v).any() and (proc[raw == v] == float(v)).all(), (tag, v)


def test_depth_post_answers_zero_for_non_finite_depth(gpu):
    """the one deliberate difference from the reference (include/dfvo_hip.h): raw passes NaN / inf through bit for bit, proc
    is 0.0 there, where utils.py's depth * mask is NaN.  Everywhere else the two agree."""
    d = RC.nonfinite_input()
    (_, _), (H, W) = RC.RANGE_SIZE
    crop = RC.crop_fractions("full", H, W)
    raw, proc = _depth_post(gpu, d, H, W, crop, RC.DEPTH_RANGE)
    want_raw, want_proc = RC.depth_post_ref(d, H, W, crop, RC.DEPTH_RANGE)
    assert np.array_equal(raw.view(np.uint32), want_raw.view(np.uint32))
    bad = ~np.isfinite(want_raw)
    for bits in RC.NONFINITE_BITS.values():
        assert (raw.view(np.uint32) == bits).any()
    assert bad.sum() >= 2 and np.isnan(want_proc[bad]).all()
    assert (proc[bad] == 0).all() and not np.signbit(proc[bad]).any()
    assert np.array_equal(proc[~bad], want_proc[~bad])


def test_pipeline_depth_post_resamples_to_the_frame(gpu, conv_precision):
    """enqueue_depth (feed 192x640 -> frame 200x664, a crop with all four sides inside the frame): the pipeline's raw /
    processed depth are the resize and preprocess_depth of the depth net's own output on the same feed image"""
    h, w = 192 + 8, 640 + 24
    crop = RC.crop_fractions("inner", h, w)
    dsd = O.monodepth2_state_dict(4869)
    pmod = importlib.import_module("df-vo_amd.pipeline")
    K = rigid_scene(64, 64, seed=1)["K"]
    pipe = pmod.TrackingPipeline(h, w, 192, 640, K, O.liteflownet_state_dict(4869), dsd,
                                 depth_crop=tuple(tuple(float(v) for v in r) for r in crop))
    ref, cur = image_pair(h, w, seed=31)
    feed = resize_lanczos_u8(cur, 640, 192)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pipe.enqueue_nets(0, d(ref), d(cur), d(feed))
    pipe.sync()
    raw, proc = pipe.get_outputs(0)[3:]
    pipe.close()
    md = importlib.import_module("df-vo_amd.libs.deep_models.depth.monodepth2.monodepth2").Monodepth2DepthNet(h, w)
    enc = {k: v for k, v in dsd.items() if k.startswith("encoder.")}
    enc.update(height=192, width=640)
    md.initialize_network_model({"encoder": enc, "decoder": {k: v for k, v in dsd.items() if k.startswith("decoder.")}},
                                "kitti_odom", False)
    small = md.inference_depth_u8(feed)
    assert small.shape == (192, 640) and small.dtype == np.float32 and np.isfinite(small).all()
    print("   depth net output: %d distinct values in %.3g .. %.3g" % (len(np.unique(small)), small.min(), small.max()))
    assert len(np.unique(small)) > 1000  # varied enough for a wrong source index to show
    want = RC.depth_post_ref(small, h, w, crop, (0.0, 50.0))
    assert 0 < (want[1] != 0).sum() < (h * w)
    _check_depth("pipeline", (raw, proc), want)


# ---- frame tail -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(RC.tail_cases()), ids=[c[0].replace(" ", "_") for c in RC.TAIL_CASES])
def test_frame_tail_bit_exact(gpu, case):
    tag, img, (y0, y1, x0, x1), oh, ow, bgr = case
    want = RC.tail_ref(img, (y0, y1, x0, x1), oh, ow, bgr)
    assert want.max() < 64
    n = oh * ow * 3
    src = torch.from_numpy(img).cuda()
    dst = torch.full((n + TAIL,), U8_SENTINEL, dtype=torch.uint8, device="cuda")
    gpu.check(gpu.lib().dfvo_read_image_tail_u8(ptr(src), img.shape[0], img.shape[1], bgr, y0, y1, x0, x1, ptr(dst), oh, ow, None))
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[n:] == U8_SENTINEL).all(), "%s: wrote behind the output" % tag
    assert (out[:n] != U8_SENTINEL).all(), "%s: output elements not written" % tag
    got = out[:n].reshape(oh, ow, 3)
    bad = got != want
    assert not bad.any(), "%s: %d elements differ, first at %s (got %d, want %d)" % (
        tag, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], want[bad][0])


def test_image_to_device_reads_inside_its_crop(gpu):
    (ih, iw), crop, (oh, ow), bgr = RC.TAIL_FRACTION_CASE
    box = RC.crop_box(crop, ih, iw)
    img = RC.tail_frame(77, ih, iw, box)
    smod = importlib.import_module("df-vo_amd.sequence")
    got = smod.image_to_device(img, oh, ow, crop, bgr=bool(bgr))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (oh, ow, 3)
    assert np.array_equal(got.cpu().numpy(), RC.tail_ref(img, box, oh, ow, bgr))


# ---- flow input and flow post -----------------------------------------------------------------------------------------
def _within(tag, out, ref, bound):
    assert out.shape == ref.shape == bound.shape, (tag, out.shape, ref.shape, bound.shape)
    assert bool(torch.isfinite(out).all()), tag
    err = (out.double() - ref).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    print("   %-44s max|ref| %.2e  max err %.2e  worst err / bound %.3f" % (tag, float(ref.abs().max()), float(err.max()), ratio))
    assert bool((err <= bound).all()), "%s: worst err / bound %.3f" % (tag, ratio)


@pytest.mark.parametrize("case", list(RC.flow_input_cases()), ids=lambda c: c[0])
def test_flow_input_down_sampling_vs_float64(gpu, case):
    tag, u8, th, tw = case
    n = th * tw * 4
    src = torch.from_numpy(u8).cuda()
    dst = _f32_buf(n)
    gpu.check(gpu.lib().dfvo_img_u8_to_flow_input(ptr(src), u8.shape[0], u8.shape[1], ptr(dst), th, tw, None))
    torch.cuda.synchronize()
    out = torch.from_numpy(_split_f32(dst, n, tag).reshape(1, th, tw, 4).copy()).permute(0, 3, 1, 2)
    ref, bound = RC.flow_input_ref(u8, th, tw)
    _within("flow input " + tag, out[:, :3], ref, bound)
    assert bool((out[:, 3] == 0).all()) and not bool(torch.signbit(out[:, 3]).any()), "%s: channel 3 is not zero" % tag


@pytest.mark.parametrize("case", list(RC.flow_post_cases()), ids=lambda c: c[0].replace(" ", "_"))
def test_flow_post_up_from_a_net_map_vs_float64(gpu, case):
    tag, flow, H, W = case
    _, _, h, w = flow.shape
    src = torch.zeros(2, h, w, 4)
    src[..., :2] = flow.permute(0, 2, 3, 1)
    src = src.cuda().contiguous()
    fwd, bwd, diff = _f32_buf(2 * H * W), _f32_buf(2 * H * W), _f32_buf(H * W)
    gpu.check(gpu.lib().dfvo_flow_post(ptr(src), 4, 0, h, w, RC.FLOW_POST_SCALE, H, W, ptr(fwd), ptr(bwd), ptr(diff), None))
    torch.cuda.synchronize()
    f = torch.from_numpy(_split_f32(fwd, 2 * H * W, tag + " fwd").reshape(1, 2, H, W).copy())
    b = torch.from_numpy(_split_f32(bwd, 2 * H * W, tag + " bwd").reshape(1, 2, H, W).copy())
    c = torch.from_numpy(_split_f32(diff, H * W, tag + " diff").reshape(1, 1, H, W).copy())
    (rf, rb), (bf, bb) = RC.flow_post_resize_ref(flow, H, W)
    _within("flow post resize fwd " + tag, f, rf, bf)
    _within("flow post resize bwd " + tag, b, rb, bb)
    rc, bc = RC.flow_consistency_ref(f, b)  # the consistency kernel against float64 on the fp32 maps it read
    _within("flow post consistency " + tag, c, rc, bc)
