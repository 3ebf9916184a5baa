"""numpy restatement of the device arithmetic of the dense drawer panels (df-vo_amd/csrc/vis.hip), operation for operation:
what tests/test_frame_drawer_cpu.py pins against the reference's flow_to_image, live matplotlib and np.percentile, and what
tools/vis_bench.py times as "the host arithmetic the panels replace".  Also the seeded inputs the drawer fixture
(tests/golden/make_golden_drawer.py) and the tests share."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = {"depth": 0, "flow1": 1, "flow2": 2, "rigid_flow_diff": 2, "warp_diff": 2, "opt_flow_diff": 3}


def load_tables():
    """the colour tables the kernels use, parsed from the committed header: {'magma', 'jet' [256,3], 'wheel' [55,3]} uint8"""
    src = open(os.path.join(ROOT, "df-vo_amd", "csrc", "vis_tables.h")).read()
    out = {}
    for name, n in (("MAGMA", 256), ("JET", 256), ("WHEEL", 55)):
        body = re.search(r"VIS_TAB_%s\[%d\]\[3\] = \{(.*?)\};" % (name, n), src, re.S).group(1)
        a = np.array([int(x) for x in re.findall(r"\d+", body)], np.uint8).reshape(n, 3)
        out[name.lower()] = a
    return out


_TABLES = None


def tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = load_tables()
    return _TABLES


# ---- Middlebury wheel -----------------------------------------------------------------------------------------------
def flow_max_radius(flow):
    """k_vis_flow_max: (maxrad as the kernels use it: float32 maximum, -1 when a radius is NaN; unknown mask [H,W])"""
    u, v = np.array(flow[0], np.float32), np.array(flow[1], np.float32)
    unknown = (np.abs(u) > np.float32(1e7)) | (np.abs(v) > np.float32(1e7))
    u[unknown] = 0
    v[unknown] = 0
    with np.errstate(all="ignore"):
        rad = np.sqrt(u * u + v * v)
    m = rad.max() if rad.size else np.float32(0)
    return (-1.0 if np.isnan(m) else float(m)), unknown


def flow_to_image_np(flow):
    """wheel_px over a whole flow [2,H,W] float32 -> (RGB uint8 [H,W,3], number of unknown pixels); float64 behind the division"""
    wheel = tables()["wheel"].astype(np.float64)
    maxrad, unknown = flow_max_radius(flow)
    den = np.float64(maxrad) + np.float64(2.220446049250313e-16)
    with np.errstate(all="ignore"):
        u = np.where(unknown, np.float32(0), np.asarray(flow[0], np.float32)).astype(np.float64) / den
        v = np.where(unknown, np.float32(0), np.asarray(flow[1], np.float32)).astype(np.float64) / den
    bad = np.isnan(u) | np.isnan(v)
    u = np.where(bad, 0.0, u)
    v = np.where(bad, 0.0, v)
    rad = np.sqrt(u * u + v * v)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1.0) / 2.0 * 54.0 + 1.0
    k0 = np.clip(np.floor(fk).astype(np.int64), 1, 55)
    k1 = np.where(k0 + 1 == 56, 1, k0 + 1)
    f = fk - k0
    img = np.zeros(u.shape + (3,), np.uint8)
    for i in range(3):
        col0, col1 = wheel[k0 - 1, i] / 255.0, wheel[k1 - 1, i] / 255.0
        col = (1.0 - f) * col0 + f * col1
        col = np.where(rad <= 1.0, 1.0 - rad * (1.0 - col), col * 0.75)
        img[..., i] = np.clip(np.floor(255.0 * col), 0, 255).astype(np.uint8)
    img[bad | unknown] = 0
    return img, int(unknown.sum())


# ---- matplotlib Normalize(0, vmax) + Colormap.__call__ -------------------------------------------------------------
def cmap_np(x, vmax, name):
    """cmap_px over a map (float32 / float64) -> RGB uint8"""
    x = np.asarray(x)
    T = x.dtype.type
    tab = tables()[name]
    with np.errstate(all="ignore"):
        xn = np.zeros_like(x) if vmax == 0 else (x.astype(np.float64) / np.float64(vmax)).astype(x.dtype)
        xa = xn * T(256)
        xa = np.where(xa == T(256), T(255), xa)
        bad = np.isnan(xa)
        idx = np.where(xa < 0, 0, np.where(xa >= 256, 255, np.where(bad, 0, xa))).astype(np.int64)
    out = tab[idx]
    out[bad] = 0
    return out


def disparity_np(d):
    d = np.asarray(d)
    T = d.dtype.type
    with np.errstate(all="ignore"):
        x = T(1) / (d + T(1e-3))
    x[d == 0] = 0
    return x


def percentile90_np(x):
    """enqueue_percentile + k_sel_finish: np.percentile(x, 90) from the two neighbouring order statistics, in x's dtype"""
    x = np.asarray(x).ravel()
    T = x.dtype.type
    n = x.size
    if np.isnan(x).any():
        return T(np.nan)
    vi = T(n - 1) * (T(90) / T(100))
    if vi >= n - 1:
        prev, nxt, gamma = n - 1, n - 1, vi + T(1)
    else:
        prev = int(np.floor(vi))
        nxt, gamma = prev + 1, vi - T(prev)
    s = np.sort(x)
    a, b = s[prev], s[nxt]
    with np.errstate(all="ignore"):
        diff = b - a
        r = a + diff * gamma
        if gamma >= T(0.5):
            r = b - diff * (T(1) - gamma)
    return T(r)


def depth_panel_np(depth, mode, max_depth=None):
    """the RGB image draw_depth hands to update_data (frame_drawer.py:425-441) and the vmax it used"""
    if mode == "depth":
        return cmap_np(depth, float(max_depth), "magma"), float(max_depth)
    disp = disparity_np(depth)
    vmax = percentile90_np(disp)
    return cmap_np(disp, float(vmax), "magma"), float(vmax)


def cell_from_rgb(rgb, cell_h, cell_w):
    """update_data (frame_drawer.py:174-183): cvtColor(RGB2BGR), then cv2.resize into the cell"""
    from oracle import cv2_shim
    return cv2_shim.resize_linear_u8(np.ascontiguousarray(rgb[..., ::-1]), (cell_w, cell_h))


def layout(h, w):
    """initialize_drawer's rectangles of the dense cells: cell id -> (y0, x0, y1, x1)"""
    q = lambda e, k: int(e / 4 * k)
    return {0: (q(h, 2), q(w, 2), q(h, 3), q(w, 3)), 1: (q(h, 2), q(w, 3), q(h, 3), q(w, 4)),
            2: (q(h, 3), q(w, 2), q(h, 4), q(w, 3)), 3: (q(h, 3), q(w, 3), q(h, 4), q(w, 4))}


# ---- seeded inputs shared by the fixture script and the tests ------------------------------------------------------
def flow_case(name, h, w):
    """[2,h,w] float32"""
    rng = np.random.RandomState(1000 + h * 7 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "randn5":
        f = rng.randn(2, h, w) * 5
    elif name == "ramp":
        f = np.stack([np.linspace(-20, 20, w)[None, :].repeat(h, 0), np.linspace(-6, 6, h)[:, None].repeat(w, 1)])
    elif name == "xramp":  # every row the same (the large maps of the fixture: their images compress to almost nothing)
        f = np.stack([np.linspace(-20, 20, w)[None, :].repeat(h, 0), (3 * np.sin(np.arange(w) / 40.0))[None, :].repeat(h, 0)])
    elif name == "zero":
        f = np.zeros((2, h, w))
    elif name == "specials":
        f = rng.randn(2, h, w)
        f[0, h // 3, w // 4] = np.nan
        f[1, h // 2, w // 2] = 3e7
        f[0, 2 * h // 3, 3 * w // 4] = -np.inf
    elif name == "lattice_int":
        f = np.stack([(xx % 9) - 4, (yy % 9) - 4]).astype(np.float64)
    elif name == "lattice_half":
        f = np.stack([((xx % 17) - 8) * 0.5, ((yy % 17) - 8) * 0.5])
    elif name == "lattice_axes":  # axes with both signed zeros: u on the axis with v = +-0, v on the axis with u = +-0
        f = np.zeros((2, h, w))
        f[0] = np.where(yy % 2 == 0, (xx % 9) - 4, 0.0)
        f[1] = np.where(yy % 2 == 0, np.where(xx % 2 == 0, 0.0, -0.0), (xx % 9) - 4)
        f[0] = np.where(yy % 2 == 1, np.where(xx % 2 == 0, 0.0, -0.0), f[0])
    else:
        raise KeyError(name)
    return np.ascontiguousarray(f, dtype=np.float32)


FLOW_GENERIC = ("randn5", "ramp", "zero", "specials")
FLOW_LATTICE = ("lattice_int", "lattice_half", "lattice_axes")


def depth_case(name, h, w, dtype=np.float32):
    rng = np.random.RandomState(2000 + h * 7 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = 2.0 + 60.0 * ((h - yy) / h) ** 2 + 5.0 * np.sin(xx / 17.0)
    if name == "smooth":
        d = smooth
    elif name == "rand":
        d = smooth + rng.rand(h, w) * 3
    elif name == "holes":
        d = smooth + rng.rand(h, w) * 3
        d[rng.rand(h, w) < 0.3] = 0
    elif name == "zero":
        d = np.zeros((h, w))
    elif name == "nan":
        d = smooth + rng.rand(h, w) * 3
        d[h // 2, w // 3] = np.nan
    else:
        raise KeyError(name)
    return np.ascontiguousarray(d, dtype=dtype)


def diff_case(name, h, w):
    """a consistency map [h,w] float32 (values on both sides of every vmax the drawer uses, a negative one, an inf)"""
    rng = np.random.RandomState(3000 + h * 7 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "smooth":
        d = 0.002 + 3.5 * (xx / w) ** 2 * (0.2 + yy / h)
    else:
        d = np.abs(rng.randn(h, w)) * np.where(rng.rand(h, w) < 0.5, 0.05, 1.5)
        d[0, 0], d[1, 1], d[2, 2] = -0.25, np.inf, 1.0
    return np.ascontiguousarray(d, dtype=np.float32)


def percentile_cases():
    """(name, depth array) of the select's cases: n = 1, 2, 11, 1001, 37 * 53; 30 % zeros; all equal; (n - 1) * 0.9 integral;
    both dtypes"""
    out = []
    for dt in (np.float32, np.float64):
        rng = np.random.RandomState(77)
        for n in (1, 2, 11, 1001, 37 * 53):
            out.append(("n%d_%s" % (n, dt.__name__), (rng.rand(n) * 40 + 0.5).astype(dt)))
        d = (rng.rand(1001) * 40 + 0.5).astype(dt)
        d[rng.rand(1001) < 0.3] = 0
        out.append(("zeros30_%s" % dt.__name__, d))
        out.append(("equal_%s" % dt.__name__, np.full(501, 7.25, dt)))
        out.append(("integral_%s" % dt.__name__, (rng.rand(21) * 40 + 0.5).astype(dt)))  # (21 - 1) * 0.9 = 18
        out.append(("ties_%s" % dt.__name__, np.round(rng.rand(1001) * 8 + 1).astype(dt)))
        d = (rng.randn(1001) * 3).astype(dt)  # negative depths: negative and positive disparities
        out.append(("signed_%s" % dt.__name__, d))
    return out


# ---- the panel cases of the fixture: "<kind>:<input>[:<dtype or vmax rule>]" per map size, and the map / window pairs ----
MAX_DEPTH = 50.0
RIGID_FLOW_THRE = 3.0
MAP_WINDOWS = [((96, 160), (600, 1000)),   # down in one axis, up in the other
               ((37, 53), (600, 1000)),    # up in both
               ((192, 640), (600, 1000)),
               ((96, 160), (192, 320)),    # the exact-half 2 x 2 area path
               ((150, 250), (600, 1000))]  # identity
PANELS_BY_MAP = {
    (96, 160): ["flow:randn5", "disp:rand:f4", "disp:rand:f8", "depth:rand:f8", "jet:rand:one", "jet:rand:ratio", "jet:rand:rigid"],
    (37, 53): ["flow:randn5", "flow:specials", "disp:holes:f4", "disp:zero:f4", "disp:nan:f4", "depth:nan:f4", "depth:holes:f4",
               "jet:rand:one"],
    (192, 640): ["flow:xramp", "disp:smooth:f4", "jet:smooth:one"],
    (150, 250): ["flow:xramp", "disp:smooth:f4", "jet:smooth:ratio"],
}
JET_VMAX = {"one": 1.0, "ratio": 0.1, "rigid": RIGID_FLOW_THRE}


def panel_input(spec, h, w):
    """the input array of a panel case"""
    kind, name = spec.split(":")[:2]
    if kind == "flow":
        return flow_case(name, h, w)
    if kind in ("disp", "depth"):
        return depth_case(name, h, w, {"f4": np.float32, "f8": np.float64}[spec.split(":")[2]])
    return diff_case(name, h, w)


def panel_key(spec, h, w):
    """fixture entry of the full-resolution RGB image of a panel case (a flow panel's image is flow_to_image's)"""
    if spec.startswith("flow:"):
        return "flow_rgb/%s@%dx%d" % (spec.split(":")[1], h, w)
    return "img/%s@%dx%d" % (spec, h, w)
