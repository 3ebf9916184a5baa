"""Cases, input builders and the numpy restatement for depth.depth_src gt: 16-bit sensor depth images in the place of the depth
net (dfvo_read_depth_u16, TrackingPipeline's depth_source "external").  Pure numpy, no device.

The restatement is the reference's own arithmetic in float64: read_depth (libs/general/utils.py:55-73) is
cv2.imread(path, -1) / scale_factor -- a uint16 array over a Python number, i.e. numpy's float64 division -- then cv2.resize
INTER_NEAREST to the image size; preprocess_depth (oracle.tracker_np) masks crop and range; the iterative scale loop reads the
resized map as float32 (E_tracker.py:677).  Every comparison against it is bit for bit."""
import numpy as np

from oracle import tracker_np as T

# source (h, w) -> output (H, W)
SIZES = {"identity": ((128, 416), (128, 416)), "exact 2x up": ((64, 208), (128, 416)), "odd up": ((37, 53), (128, 416)),
         "down": ((480, 640), (128, 416)), "tiny": ((5, 3), (11, 13))}
SCALES = (500, 1000, 5000, 256)
CROPS = ("default", "full", "one_pixel")
# a range whose two ends are quotients of a uint16 and every scale above, exactly: 0.5 = 250 / 500 = 128 / 256, 10 = 50000 / 5000
DEPTH_RANGE = (0.5, 10.0)


def crop_fractions(name, H, W):
    """[[y0, y1], [x0, x1]] as fractions (cfg.crop.depth_crop); the box is int(H * c) on both sides of the comparison"""
    if name == "default":
        return [[0.3, 1], [0, 1]]
    if name == "full":
        return [[0, 1], [0, 1]]
    assert name == "one_pixel"
    y, x = H // 2, W // 2
    return [[(y + 0.5) / H, (y + 1.5) / H], [(x + 0.5) / W, (x + 1.5) / W]]


def crop_box(crop, H, W):
    return int(H * crop[0][0]), int(H * crop[0][1]), int(W * crop[1][0]), int(W * crop[1][1])


def nearest_index(N, n):
    """cv::resize INTER_NEAREST, n source samples -> N: min(floor(x * (1.0 / ((double)N / n))), n - 1)"""
    return np.minimum(np.floor(np.arange(N, dtype=np.float64) * (1.0 / (float(N) / n))).astype(np.int64), n - 1)


def read_depth_ref(src_u16, scale, H, W, crop, depth_range):
    """(raw float32 [H,W], proc float64 [H,W]) of a uint16 depth image"""
    assert src_u16.dtype == np.uint16
    v = src_u16 / scale  # read_depth: float64
    assert v.dtype == np.float64
    r = v[nearest_index(H, v.shape[0])[:, None], nearest_index(W, v.shape[1])[None, :]]
    return r.astype(np.float32), T.preprocess_depth(r, crop, list(depth_range))


def boundary_values(scale, depth_range=DEPTH_RANGE):
    """0 (a sensor hole), 1, 65535, and the uint16 whose quotient IS max_depth / min_depth, each with its two neighbours"""
    lo, hi = int(round(depth_range[0] * scale)), int(round(depth_range[1] * scale))
    assert 1 < lo and hi < 65535 and lo / scale == depth_range[0] and hi / scale == depth_range[1]
    return [0, 1, 65535, hi - 1, hi, hi + 1, lo - 1, lo, lo + 1]


def source_image(seed, size, scale, depth_range=DEPTH_RANGE):
    """(src uint16 [h,w], planted [(Y, X, u)]): seeded random values with boundary_values(scale) planted at source pixels that
    the nearest resize reads for output pixels (Y, X) inside the default crop -- so they do not vanish in the resampling --
    and, at the output pixel of the one-pixel crop, a value just inside the range"""
    (h, w), (H, W) = SIZES[size]
    g = np.random.Generator(np.random.PCG64(seed))
    src = g.integers(0, 65536, (h, w), dtype=np.uint16)
    ys, xs = nearest_index(H, h), nearest_index(W, w)
    y0, y1, x0, x1 = crop_box(crop_fractions("default", H, W), H, W)
    centre = (ys[H // 2], xs[W // 2])
    src[centre] = int(round(depth_range[1] * scale)) - 1
    taken, planted = {centre}, []
    values = boundary_values(scale, depth_range)
    for k in g.permutation((y1 - y0) * (x1 - x0)):
        Y, X = y0 + int(k) // (x1 - x0), x0 + int(k) % (x1 - x0)
        s = (ys[Y], xs[X])
        if s in taken:
            continue
        taken.add(s)
        src[s] = values[len(planted)]
        planted.append((Y, X, values[len(planted)]))
        if len(planted) == len(values):
            break
    assert len(planted) == len(values), "the source is too small for the planted values"
    return src, planted


def planted_survive(src, planted, scale, H, W, depth_range=DEPTH_RANGE):
    """the planted values as the restatement's output has them, under the full crop: present in raw, and kept or dropped in
    proc by the strict comparisons"""
    raw, proc = read_depth_ref(src, scale, H, W, crop_fractions("full", H, W), depth_range)
    for Y, X, u in planted:
        v = u / scale
        if raw[Y, X] != np.float32(v):
            return False
        keep = depth_range[0] < v < depth_range[1]
        if proc[Y, X] != (v if keep else 0.0):
            return False
    lo, hi = depth_range
    kept = {u: lo < u / scale < hi for _, _, u in planted}
    b = boundary_values(scale, depth_range)
    return [kept[u] for u in b] == [False, False, False, True, False, False, False, False, True]


# ---- pipeline cases: the scenes' processed depths as 16-bit images --------------------------------------------------------
QUANT_SCALE = 500  # kitti.py:159; depths up to 50 m fit (25000)


def quantise(depth, scale=QUANT_SCALE):
    return np.clip(np.rint(depth * scale), 0, 65535).astype(np.uint16)
