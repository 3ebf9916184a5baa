"""Host restatement of the input stage's operator (include/dfvo_hip.h, dfvo_undistort_*), written from its contract: bilinear
Bayer demosaic as convolutions of masked planes, and the order-1 remap with one rounding per float64 operation.  numpy only;
tests/test_undistort_cpu.py holds it against live scipy.ndimage bit for bit, the GPU tests hold the kernels against it."""
import numpy as np

PATTERNS = ("rggb", "bggr", "grbg", "gbrg")
BORDERS = ("reflect", "mirror")
SIZES = ((2, 2), (3, 5), (33, 47), (96, 130))
K_RB = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.float64) / 4
K_G = np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]], np.float64) / 4


def masks(h, w, pattern):
    """{colour: bool [h, w]}: the sites of each colour; the pattern names sites (0,0), (0,1), (1,0), (1,1)"""
    m = {c: np.zeros((h, w), bool) for c in "rgb"}
    for c, (y, x) in zip(pattern.lower(), ((0, 0), (0, 1), (1, 0), (1, 1))):
        m[c][y::2, x::2] = True
    return m


def extend(p, border):
    """the plane with one pixel more on every side: reflect -1 -> 0, n -> n - 1; mirror -1 -> 1, n -> n - 2"""
    h, w = p.shape

    def idx(n):
        i = np.arange(-1, n + 1)
        if border == "reflect":
            i = np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
        else:
            assert n >= 2, "the mirror border needs two samples"
            i = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))
        return i
    return p[idx(h)][:, idx(w)]


def conv3(p, k, border):
    e = extend(p, border)
    h, w = p.shape
    out = np.zeros((h, w), np.float64)
    for dy in range(3):
        for dx in range(3):
            if k[dy, dx]:
                out += k[dy, dx] * e[dy:dy + h, dx:dx + w]  # multiples of 1/4 far below 2^53: exact in any order
    return out


def demosaic(mosaic, pattern, border="reflect"):
    """float64 [h, w, 3] RGB"""
    mosaic = np.asarray(mosaic, np.float64)
    m = masks(mosaic.shape[0], mosaic.shape[1], pattern)
    return np.stack([conv3(mosaic * m["r"], K_RB, border), conv3(mosaic * m["g"], K_G, border),
                     conv3(mosaic * m["b"], K_RB, border)], -1)


def remap(v, map_xy):
    """v float64 [h, w, C]; map_xy float64 [2][h * w] (x then y).  float64 [h, w, C], before the truncation"""
    h, w = v.shape[:2]
    cx, cy = map_xy[0].reshape(h, w), map_xy[1].reshape(h, w)
    inside = (cy >= 0) & (cy <= h - 1) & (cx >= 0) & (cx <= w - 1)
    cys, cxs = np.where(inside, cy, 0.0), np.where(inside, cx, 0.0)
    fy, fx = np.floor(cys), np.floor(cxs)
    ty, tx = cys - fy, cxs - fx
    wy, wx = (1.0 - ty, ty), (1.0 - tx, tx)
    fy, fx = fy.astype(np.int64), fx.astype(np.int64)
    t = np.zeros(v.shape, np.float64)
    for a in (0, 1):
        for b in (0, 1):
            c = v[np.minimum(fy + a, h - 1), np.minimum(fx + b, w - 1)]
            c = c * wy[a][..., None]
            c = c * wx[b][..., None]
            t = t + c
    return np.where(inside[..., None], t, 0.0)


def to_u8(t):
    """the value truncated; beyond 255 (the one-pixel frame under `reflect`) its low 8 bits"""
    return (t.astype(np.int64) & 255).astype(np.uint8)


def undistort_mosaic(mosaic, pattern, border, map_xy=None):
    v = demosaic(mosaic, pattern, border)
    return to_u8(v if map_xy is None else remap(v, map_xy))


def undistort_rgb(rgb, map_xy):
    return to_u8(remap(np.asarray(rgb, np.float64), map_xy))


def identity_map(h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([xx.reshape(-1), yy.reshape(-1)])


def random_map(h, w, seed, outside=0.12):
    """[2][h * w]: uniform samples of the frame; `outside` of them up to 2 px beyond it; planted integer coordinates, coordinates
    exactly n - 1, and coordinates one ulp and 1e-9 outside either end"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = h * w
    x, y = rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)
    out = rng.random(n) < outside
    x = np.where(out & (rng.random(n) < 0.5), rng.choice([-1.0, 1.0], n) * rng.uniform(0, 2, n) + np.where(rng.random(n) < 0.5, 0, w - 1), x)
    y = np.where(out & ~((x < 0) | (x > w - 1)), rng.choice([-2.0, h + 1.0], n) + rng.uniform(-1, 1, n), y)
    plant = [(0.0, 0.0), (w - 1.0, h - 1.0), (w - 1.0, 0.25), (0.5, h - 1.0), (float(w // 2), float(h // 2)), (float(w // 2), 0.75),
             (np.nextafter(0.0, -1), 0.0), (0.0, -1e-9), (np.nextafter(w - 1.0, w), 0.0), (0.0, h - 1 + 1e-9), (-0.0, -0.0),
             (np.nextafter(w - 1.0, 0), np.nextafter(h - 1.0, 0))]
    for i, (px, py) in enumerate(plant):
        k = (i * 7919) % n if n > len(plant) else i % n
        x[k], y[k] = px, py
    return np.stack([x, y])


def in_range(map_xy, h, w):
    x, y = map_xy
    return (y >= 0) & (y <= h - 1) & (x >= 0) & (x <= w - 1)


def mosaic_of(rgb, pattern):
    """the Bayer mosaic uint8 [h, w] of an RGB frame"""
    h, w = rgb.shape[:2]
    m = masks(h, w, pattern)
    return (rgb[..., 0] * m["r"] + rgb[..., 1] * m["g"] + rgb[..., 2] * m["b"]).astype(np.uint8)
