"""The case matrix of the JPEG decode tests (test_jpeg_cpu.py, test_jpeg_gpu.py) and its fixture.

Sizes: 1x1; 8x8; 16x16 (exactly one 4:2:0 MCU); 17x23 and 33x15 (partial MCUs both ways, odd chroma sizes); 37x53; 64x200;
24x520 (upsampling neighbours across block, wave and workgroup boundaries: 65 luma blocks per row, 8 lanes per block).
Subsampling 4:4:4, 4:2:2, 4:2:0, grey.  Quality 5, 50, 92, 100: every quality for every subsampling at the six small sizes; at
the two large ones each subsampling takes one quality, rotated so that every quality occurs at both sizes (the fixture stays a
few hundred kB).  For a subset: optimised Huffman tables, restart intervals of 1 MCU, 3 MCUs and one MCU row.

Content: seeded noise over a ramp -- the left part of every frame smooth, the right part noise strong enough to saturate.

tests/golden/jpeg_cases.npz holds each case's file bytes as Pillow wrote them and the pixels Pillow (libjpeg-turbo) decoded from
them, so the expectation does not move with the installed Pillow; tests/golden/make_golden_jpeg.py regenerates it."""
import collections
import functools
import io
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "jpeg_cases.npz")

SMALL = [(1, 1), (8, 8), (16, 16), (17, 23), (33, 15), (37, 53)]  # (h, w)
LARGE = [(64, 200), (24, 520)]
SUBS = ["444", "422", "420", "grey"]
QUALITIES = [5, 50, 92, 100]
_PIL_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}

Case = collections.namedtuple("Case", "name h w sub quality optimize rst_blocks rst_rows")


def _case(h, w, sub, q, optimize=False, rst_blocks=0, rst_rows=0):
    name = "%dx%d-%s-q%d" % (h, w, sub, q)
    name += "-opt" if optimize else ""
    name += "-rst%d" % rst_blocks if rst_blocks else ""
    name += "-rstrow" if rst_rows else ""
    return Case(name, h, w, sub, q, optimize, rst_blocks, rst_rows)


def _cases():
    out = [_case(h, w, s, q) for (h, w) in SMALL for s in SUBS for q in QUALITIES]
    for i, (h, w) in enumerate(LARGE):
        out += [_case(h, w, s, QUALITIES[(i + j) % 4]) for j, s in enumerate(SUBS)]
    for (h, w), s, q in [((17, 23), "420", 50), ((37, 53), "422", 92), ((33, 15), "grey", 5), ((37, 53), "444", 100)]:
        out.append(_case(h, w, s, q, optimize=True))
    for (h, w), s, q in [((37, 53), "420", 50), ((33, 15), "422", 92), ((17, 23), "grey", 50), ((37, 53), "444", 5)]:
        out += [_case(h, w, s, q, rst_blocks=1), _case(h, w, s, q, rst_blocks=3), _case(h, w, s, q, rst_rows=1)]
    out.append(_case(24, 520, "420", 92, optimize=True, rst_rows=1))
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()
RESTART_CASES = [c for c in CASES if c.rst_blocks or c.rst_rows]


def make_image(case):
    """uint8 [h, w, 3] (or [h, w] for grey): a ramp, smooth on the left, under saturating noise on the right"""
    seed = int.from_bytes(case.name.encode(), "little") % (2 ** 32)
    rng = np.random.RandomState(seed)
    ch = 1 if case.sub == "grey" else 3
    y, x = np.mgrid[0:case.h, 0:case.w].astype(np.float64)
    img = np.empty((case.h, case.w, ch))
    for c in range(ch):
        ramp = 255.0 * (x * (c + 1) + y * (3 - c)) / max(1.0, (case.w - 1) * (c + 1) + (case.h - 1) * (3 - c))
        noise = rng.normal(0.0, 90.0, (case.h, case.w)) * (x >= case.w // 2)
        img[..., c] = ramp + noise
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return img[..., 0] if ch == 1 else img


def encode(case):
    """the case's file bytes as the installed Pillow writes them"""
    from PIL import Image
    im = Image.fromarray(make_image(case))
    kw = dict(quality=case.quality, optimize=case.optimize)
    if case.sub != "grey":
        kw["subsampling"] = _PIL_SUBSAMPLING[case.sub]
    if case.rst_blocks:
        kw["restart_marker_blocks"] = case.rst_blocks
    if case.rst_rows:
        kw["restart_marker_rows"] = case.rst_rows
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_decode(data):
    """uint8 [h, w, 3] or [h, w]: what the installed Pillow decodes"""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode in ("RGB", "L"), im.mode
        return np.asarray(im).copy()


@functools.lru_cache(maxsize=1)
def fixture():
    """{case name: (file bytes, Pillow's pixels)} from tests/golden/jpeg_cases.npz; read once, shared, never written to"""
    z = np.load(FIXTURE)
    meta = json.loads(bytes(z["meta"]).decode())
    jpg, px = z["jpg"], z["px"]
    out = {}
    for m in meta:
        shape = tuple(m["shape"])
        p = px[m["px0"]:m["px0"] + int(np.prod(shape))].reshape(shape)
        p.setflags(write=False)
        out[m["name"]] = (bytes(jpg[m["jpg0"]:m["jpg0"] + m["jpg_n"]]), p)
    return out
