"""Cases, input builders, references and deliberately wrong reference variants ("mutants") for the resamplers between the
decoded frame and the nets and between the nets and the solvers.  Pure numpy / torch, no device.
  depth post   dfvo_depth_postprocess: cv2.resize INTER_NEAREST of the depth map, crop mask, range mask
  frame tail   dfvo_read_image_tail_u8: crop + BGR swap + cv2.resize's 8-bit INTER_LINEAR of a window of a wider frame
  flow input   dfvo_img_u8_to_flow_input, flow post  dfvo_flow_post: bilinear, corners aligned, both down-sampling
tests/test_resamplers_cpu.py proves that every mutant changes the result on these cases (so a kernel that computes the
mutant fails tests/test_resamplers_gpu.py); the device tests compare the kernels with the references below."""
import numpy as np
import torch
import torch.nn.functional as F

import flow_bounds as B
import flow_world as FW
from oracle import cv2_shim
from oracle import nets_torch as O
from oracle import tracker_np as T

# ---- depth post -------------------------------------------------------------------------------------------------------
# (h, w) -> (H, W): KITTI's two frame sizes, the identity, the small sizes at which float32 and exact integer arithmetic
# pick other source indices than OpenCV's double inverse scale, two down-samples, and the one-pixel maps
DEPTH_SIZES = [((192, 640), (376, 1241)), ((192, 640), (370, 1226)), ((192, 640), (192, 640)), ((14, 12), (18, 34)),
               ((28, 30), (36, 85)), ((21, 18), (27, 51)), ((24, 40), (12, 20)), ((24, 40), (17, 23)), ((1, 1), (5, 7)),
               ((5, 7), (1, 1))]
DEPTH_RANGE = (0.0, 50.0)
CROPS = ("default", "full", "inner", "empty", "one_pixel")


def depth_input(h, w):
    """a distinct float32 value inside the depth range in every source pixel: a wrong source index changes the output"""
    d = (1.0 + np.arange(h * w, dtype=np.float64) * 2.0 ** -12).astype(np.float32).reshape(h, w)
    assert len(np.unique(d)) == h * w
    return d


def crop_fractions(name, H, W):
    """[[y0, y1], [x0, x1]] as fractions of the frame (cfg.crop.depth_crop); the box is int(H * c), as the pipeline and
    preprocess_depth both compute it.  (y + 0.5) / H keeps int(H * c) == y clear of the quotient's rounding."""
    if name == "default":
        return [[0.3, 1], [0, 1]]
    if name == "full":
        return [[0, 1], [0, 1]]
    if name == "inner":
        return [[0.2, 0.8], [0.05, 0.95]]
    y, x = H // 2, W // 2
    if name == "empty":
        return [[(y + 0.5) / H, (y + 0.5) / H], [0, 1]]
    assert name == "one_pixel"
    return [[(y + 0.5) / H, (y + 1.5) / H], [(x + 0.5) / W, (x + 1.5) / W]]


def crop_box(crop, H, W):
    return int(H * crop[0][0]), int(H * crop[0][1]), int(W * crop[1][0]), int(W * crop[1][1])


def depth_post_ref(depth, H, W, crop, depth_range):
    """(raw float32 [H,W], proc float64 [H,W]): dfvo.py:314-319 + utils.py:89-114 as the oracle states them"""
    raw = cv2_shim.resize(depth, (W, H), interpolation=cv2_shim.INTER_NEAREST)
    with np.errstate(invalid="ignore"):
        return raw, T.preprocess_depth(raw, crop, list(depth_range))


# source index of output index x, n source samples, N output samples
def _idx_double(x, n, N):
    return np.floor(x * (1.0 / (float(N) / n)))


def _idx_float32(x, n, N):
    f = np.float32(1) / (np.float32(N) / np.float32(n))
    return np.floor(x.astype(np.float32) * f)


def _idx_ratio(x, n, N):
    return np.floor(x * (float(n) / N))


def _idx_integer(x, n, N):
    return (x.astype(np.int64) * n) // N


def _idx_half_pixel(x, n, N):
    return np.floor((x + 0.5) * (float(n) / N))


def _idx_round(x, n, N):
    return np.rint(x * (float(n) / N))


def _idx_align_corners(x, n, N):
    return np.floor(x * ((n - 1) / (N - 1))) if N > 1 else np.zeros_like(x)


DEPTH_INDEX_MUTANTS = {"float32 index": _idx_float32, "x * (w / W)": _idx_ratio, "integer (x * w) // W": _idx_integer,
                       "half-pixel centres": _idx_half_pixel, "round to nearest": _idx_round,
                       "align-corners scale": _idx_align_corners}
DEPTH_OTHER_MUTANTS = ("h / w transposed", "<= in the range mask", "crop in source coordinates", "range compared in double")
DEPTH_MUTANTS = tuple(DEPTH_INDEX_MUTANTS) + DEPTH_OTHER_MUTANTS


def depth_post_variant(depth, H, W, crop, depth_range, mutant=None):
    """k_depth_post restated in numpy; mutant=None is the kernel as it should be (equal to depth_post_ref on finite input)"""
    h, w = depth.shape
    idx = DEPTH_INDEX_MUTANTS.get(mutant, _idx_double)
    sh, sw = (w, h) if mutant == "h / w transposed" else (h, w)  # the map read as [w, h]
    ys = np.clip(idx(np.arange(H, dtype=np.float64), sh, H).astype(np.int64), 0, sh - 1)
    xs = np.clip(idx(np.arange(W, dtype=np.float64), sw, W).astype(np.int64), 0, sw - 1)
    raw = depth.reshape(-1)[ys[:, None] * sw + xs[None, :]]
    mn, mx = depth_range
    if mutant == "range compared in double":
        d = raw.astype(np.float64)
    else:
        d, mn, mx = raw, np.float32(mn), np.float32(mx)
    in_range = ((d <= mx) & (d >= mn)) if mutant == "<= in the range mask" else ((d < mx) & (d > mn))
    y0, y1, x0, x1 = crop_box(crop, H, W)
    yy, xx = (ys, xs) if mutant == "crop in source coordinates" else (np.arange(H), np.arange(W))
    in_crop = ((yy >= y0) & (yy < y1))[:, None] & ((xx >= x0) & (xx < x1))[None, :]
    return raw, np.where(in_crop & in_range, raw.astype(np.float64), 0.0)


def depth_cases():
    """(tag, depth, H, W, crop, depth_range) of every size x crop"""
    for (h, w), (H, W) in DEPTH_SIZES:
        d = depth_input(h, w)
        assert DEPTH_RANGE[0] < d.min() and d.max() < DEPTH_RANGE[1]  # the range mask passes every pixel
        for name in CROPS:
            yield "%dx%d->%dx%d %s" % (h, w, H, W, name), d, H, W, crop_fractions(name, H, W), DEPTH_RANGE


RANGE_SIZE = ((4, 6), (7, 9))
RANGES = [(0.0, 50.0), (0.1, 50.0), (1.0, 2.5)]


def range_input(depth_range):
    """values on and next to both ends of the range (both comparisons are strict, and in float32: min_depth = 0.1 stands
    for float32(0.1), which is larger than the double 0.1), zeros of both signs, a negative value, values well inside"""
    (h, w), _ = RANGE_SIZE
    mn, mx = np.float32(depth_range[0]), np.float32(depth_range[1])
    inf = np.float32(np.inf)
    v = [mn, np.nextafter(mn, -inf), np.nextafter(mn, inf), mx, np.nextafter(mx, -inf), np.nextafter(mx, inf),
         np.float32(0.0), np.float32(-0.0), np.float32(-1.5), np.float32(0.5 * (float(mn) + float(mx)))]
    v += [np.float32(float(mn) + (float(mx) - float(mn)) * k / 16.0) for k in range(1, h * w - len(v) + 1)]
    return np.array(v, np.float32).reshape(h, w)


def range_cases():
    (h, w), (H, W) = RANGE_SIZE
    for r in RANGES:
        yield "range %g..%g" % r, range_input(r), H, W, crop_fractions("full", H, W), r


NONFINITE_BITS = {"nan": 0x7FC00000, "inf": 0x7F800000}


def nonfinite_input():
    """the range input with a NaN and +inf in it"""
    d = range_input(DEPTH_RANGE).copy()
    d.reshape(-1).view(np.uint32)[[3, 11]] = [NONFINITE_BITS["nan"], NONFINITE_BITS["inf"]]
    return d


# ---- frame tail -------------------------------------------------------------------------------------------------------
# (tag, frame (ih, iw), crop (y0, y1, x0, x1), output (oh, ow), bgr)
TAIL_CASES = [
    ("bottom-right corner", (37, 53), (10, 37, 20, 53), (16, 24), 0),
    ("top-left corner", (37, 53), (0, 20, 0, 30), (31, 47), 0),
    ("one column", (37, 53), (5, 30, 17, 18), (12, 5), 0),
    ("one row, the frame's last", (37, 53), (36, 37, 3, 50), (4, 30), 0),
    ("one pixel", (37, 53), (18, 19, 26, 27), (3, 4), 1),
    ("up-scale", (37, 53), (8, 20, 11, 29), (29, 41), 0),
    ("down-scale", (74, 106), (7, 70, 9, 100), (20, 33), 0),
    ("2x2 area, pitch > crop width", (74, 106), (10, 58, 21, 85), (24, 32), 0),
    ("2x2 area, pitch > crop width, bgr", (74, 106), (10, 58, 21, 85), (24, 32), 1),
    ("2x2 area at the bottom-right corner, bgr", (74, 106), (26, 74, 42, 106), (24, 32), 1),
    ("odd crop, bgr", (37, 53), (3, 32, 5, 48), (13, 17), 1),
]
TAIL_MUTANTS = ("clamps at the frame's bounds", "pitch = crop width", "bgr ignored")
# sequence.image_to_device takes the crop as fractions: int(37 * 0.3) = 11, int(53 * 0.4) = 21, up to the bottom-right corner
TAIL_FRACTION_CASE = ((37, 53), [[0.3, 1.0], [0.4, 1.0]], (16, 24), 1)


def tail_frame(seed, ih, iw, box):
    """the decoded frame: random in [0, 64) inside the crop window, 255 everywhere else, so that any read outside the window
    changes the output (every correct output is below 64)"""
    y0, y1, x0, x1 = box
    img = np.full((ih, iw, 3), 255, np.uint8)
    g = np.random.Generator(np.random.PCG64(seed))
    img[y0:y1, x0:x1] = g.integers(0, 64, (y1 - y0, x1 - x0, 3), dtype=np.uint8)
    return img


def tail_ref(img, box, oh, ow, bgr, mutant=None):
    """read_image behind the decoder (utils.py:44-51): cvtColor, crop, cv2.resize of the contiguous crop"""
    y0, y1, x0, x1 = box
    if bgr and mutant != "bgr ignored":
        img = img[..., ::-1]
    if mutant == "pitch = crop width":  # the window's rows read back to back from its first pixel
        n = (y1 - y0) * (x1 - x0)
        flat = img.reshape(-1, 3)[y0 * img.shape[1] + x0:][:n]
        return cv2_shim.resize(np.ascontiguousarray(flat.reshape(y1 - y0, x1 - x0, 3)), (ow, oh))
    if mutant == "clamps at the frame's bounds":
        return _tail_linear_frame_clamps(img, box, oh, ow)
    return cv2_shim.resize(np.ascontiguousarray(img[y0:y1, x0:x1]), (ow, oh))


def _tail_linear_frame_clamps(img, box, oh, ow):
    """cv2_shim.resize_linear_u8 of the window, but with `sx + 1` and the rows clamped at the frame's last column / row
    and not the window's: the window's right and lower neighbours take part in its last cell"""
    y0, y1, x0, x1 = box
    ch, cw = y1 - y0, x1 - x0
    scale_x, scale_y = 1.0 / (float(ow) / cw), 1.0 / (float(oh) / ch)
    eps = np.finfo(np.float64).eps
    if abs(scale_x - 2) < eps and abs(scale_y - 2) < eps:  # the area path reads inside the window only
        return cv2_shim.resize(np.ascontiguousarray(img[y0:y1, x0:x1]), (ow, oh))
    src = img[y0:, x0:].astype(np.int64)
    fh, fw = src.shape[:2]
    one, k = np.float32(1), np.float32(2048)
    sx, fx = cv2_shim._linear_axis_u8(cw, ow, scale_x)
    lo, hi = sx < 0, sx >= fw - 1
    fx = np.where(lo | hi, np.float32(0), fx)
    sx = np.where(lo, 0, np.where(hi, fw - 1, sx))
    a0, a1 = np.rint((one - fx) * k).astype(np.int64), np.rint(fx * k).astype(np.int64)
    sy, fy = cv2_shim._linear_axis_u8(ch, oh, scale_y)
    b0, b1 = np.rint((one - fy) * k).astype(np.int64), np.rint(fy * k).astype(np.int64)
    r0, r1 = np.clip(sy, 0, fh - 1), np.clip(sy + 1, 0, fh - 1)
    rows = src[:, sx] * a0[None, :, None] + src[:, np.minimum(sx + 1, fw - 1)] * a1[None, :, None]
    out = (((b0[:, None, None] * (rows[r0] >> 4)) >> 16) + ((b1[:, None, None] * (rows[r1] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def tail_cases():
    for i, (tag, (ih, iw), box, (oh, ow), bgr) in enumerate(TAIL_CASES):
        yield tag, tail_frame(100 + i, ih, iw, box), box, oh, ow, bgr


# ---- flow input and flow post -----------------------------------------------------------------------------------------
# frame size -> DeepFlow.get_target_size of it: every one down-samples on both axes
FLOW_INPUT_CASES = [((70, 100), (64, 96)), ((47, 155), (32, 128)), ((94, 310), (64, 288)), ((100, 70), (96, 64)),
                    ((37, 53), (32, 32))]
# net flow (h, w) -> frame (H, W), standard deviation of the net's flow
FLOW_POST_CASES = [((16, 24), (70, 100), 3.0), ((8, 32), (47, 155), 3.0), ((16, 72), (94, 310), 3.0),
                   ((24, 16), (100, 70), 3.0),
                   ((16, 24), (70, 100), 0.25)]  # and one whose samples mostly stay inside the frame
FLOW_POST_SCALE = next(L for L in FW.FLOW_LAYERS if L["op"] == "post")["scale"]
FLOW_MUTANTS = ("align_corners=False", "rw and rh swapped", "scale dropped", "bwd not negated")


def flow_input_frame(seed, h, w):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (h, w, 3), dtype=np.uint8)


def flow_input_cases():
    for i, ((h, w), (th, tw)) in enumerate(FLOW_INPUT_CASES):
        yield "%dx%d->%dx%d" % (h, w, th, tw), flow_input_frame(200 + i, h, w), th, tw


def flow_input_ref(u8, th, tw, mutant=None):
    """(float64 reference [1,3,th,tw], bound): the net's input of tests/flow_world.py"""
    img = torch.from_numpy(np.transpose(u8 / 255, (2, 0, 1))).unsqueeze(0).float().double()
    ref = F.interpolate(img, (th, tw), mode="bilinear", align_corners=mutant != "align_corners=False")
    return ref, B.input_bound(img)(th, tw)


def flow_post_input(seed, h, w, sd):
    """the net's level-2 flow [2,2,h,w] float32: sample 0 forward, sample 1 backward"""
    return (torch.randn(2, 2, h, w, generator=torch.Generator().manual_seed(seed)) * sd).float()


def flow_post_cases():
    for i, ((h, w), (H, W), sd) in enumerate(FLOW_POST_CASES):
        yield "%dx%d->%dx%d sd %g" % (h, w, H, W, sd), flow_post_input(300 + i, h, w, sd), H, W


def flow_post_resize_ref(flow, H, W, mutant=None):
    """((fwd, bwd) float64 [1,2,H,W], (fwd bound, bwd bound)) of k_flow_resize on flow [2,2,h,w] (fp32 values)"""
    f64 = flow.double()
    bounds = B.post_resize_bound(f64, FLOW_POST_SCALE, H, W)
    if mutant is None:
        return FW.post_resize_ref(f64, FLOW_POST_SCALE, H, W), bounds
    scale = 1.0 if mutant == "scale dropped" else FLOW_POST_SCALE
    rh, rw = float(H / f64.size(2)), float(W / f64.size(3))
    if mutant == "rw and rh swapped":
        rh, rw = rw, rh
    f = F.interpolate(f64 * scale, (H, W), mode="bilinear", align_corners=mutant != "align_corners=False")
    f = torch.stack([f[:, 0] * rw, f[:, 1] * rh], dim=1)
    return (f[0:1], f[1:2]), bounds


def flow_consistency_ref(fwd, bwd, mutant=None):
    """(float64 reference [1,1,H,W], bound) of k_flow_consistency on the fp32 maps fwd / bwd [1,2,H,W] it read"""
    fd, bd = fwd.double(), bwd.double()
    rc = FW.consistency_ref(fd, bd)
    bound = B.consistency_bound(fd, bd, rc)
    if mutant == "bwd not negated":
        rc = O.forward_backward_consistency(fd, -bd, O.flow_to_pix(fd))
    return rc.permute(0, 3, 1, 2), bound
