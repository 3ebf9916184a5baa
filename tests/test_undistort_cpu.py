"""CPU: the input stage's host side.
  1. the restatement (tests/undistort_ref.py) against live scipy.ndimage, bit for bit: convolve under both border modes for the
     demosaic, map_coordinates of order 1 for the remap, four patterns, sizes 2x2, 3x5, 33x47, 96x130
  2. the layout of a distortion table file against the SDK's slicing
  3. RobotCar's K and path listing on a temporary tree
  4. FrameStream's mosaic arguments over a fake ring
  5. DFVO_ERR_ARG from every new entry point, with no device"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import undistort_ref as ur
from test_frame_stream_cpu import FakeRing, time_limit, workers_alive


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.dfvo_amd()
    return {n: importlib.import_module("df-vo_amd." + n) for n in ("frame_stream", "undistort", "robotcar", "default_cfg")}


def random_mosaic(h, w, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (h, w), dtype=np.uint8)


# ---- 1. the restatement against scipy -----------------------------------------------------------------------------------------
def scipy_demosaic(mosaic, pattern, border):
    """demosaicing_CFA_Bayer_bilinear's three convolutions, with scipy doing them"""
    from scipy.ndimage import convolve
    cfa = np.asarray(mosaic, np.float64)
    m = ur.masks(cfa.shape[0], cfa.shape[1], pattern)
    return np.stack([convolve(cfa * m["r"], ur.K_RB, mode=border), convolve(cfa * m["g"], ur.K_G, mode=border),
                     convolve(cfa * m["b"], ur.K_RB, mode=border)], -1)


def scipy_remap(v, map_xy):
    """camera_model.undistort: map_coordinates of order 1 per channel, the table as [cy, cx]"""
    from scipy.ndimage import map_coordinates
    h, w = v.shape[:2]
    lut = np.stack([map_xy[1].reshape(h, w), map_xy[0].reshape(h, w)])
    return np.stack([map_coordinates(v[..., c], lut, order=1) for c in range(v.shape[2])], -1)


@pytest.mark.parametrize("size", ur.SIZES)
def test_demosaic_restatement_equals_scipy_convolve(size):
    h, w = size
    for pattern in ur.PATTERNS:
        for border in ur.BORDERS:
            for mosaic in (random_mosaic(h, w, 3), np.full((h, w), 255, np.uint8)):
                got, want = ur.demosaic(mosaic, pattern, border), scipy_demosaic(mosaic, pattern, border)
                assert got.dtype == want.dtype == np.float64 and np.array_equal(got, want), (pattern, border)
                assert np.array_equal(got * 4, np.rint(got * 4)), "a value that is no multiple of 1/4"
                inner = got[1:-1, 1:-1]
                assert inner.size == 0 or inner.max() <= 255
                if border == "mirror":  # the mirror keeps a site's colour: nothing is counted twice
                    assert got.max() <= 255
                ok = got <= 255  # (beyond 255 float -> uint8 is not defined in C; only the frame under `reflect` gets there)
                assert np.array_equal(ur.to_u8(got)[ok], want.astype(np.int64).astype(np.uint8)[ok])


def test_reflect_counts_a_frame_site_twice_and_the_byte_wraps():
    got = ur.demosaic(np.full((4, 4), 255, np.uint8), "rggb", "reflect")
    assert got[0, 0, 0] == 255 * 9 / 4 and ur.to_u8(got)[0, 0, 0] == int(255 * 9 / 4) & 255


@pytest.mark.parametrize("size", ur.SIZES)
def test_remap_restatement_equals_scipy_map_coordinates(size):
    h, w = size
    rng = np.random.Generator(np.random.PCG64(11))
    maps = [ur.identity_map(h, w), ur.random_map(h, w, 5), ur.random_map(h, w, 6, outside=0.0)]
    frames = [ur.demosaic(random_mosaic(h, w, 9), "gbrg", "reflect"), ur.demosaic(np.full((h, w), 255, np.uint8), "rggb", "mirror"),
              rng.integers(0, 256, (h, w, 3)).astype(np.float64)]
    for m in maps:
        for v in frames:
            got, want = ur.remap(v, m), scipy_remap(v, m)
            assert np.array_equal(got, want), "%d of %d samples differ" % ((got != want).sum(), got.size)
            assert np.array_equal(ur.to_u8(got), want.astype(np.uint8))  # (every value is within 0 .. 255 * 9 / 4; see above)
    assert np.array_equal(ur.to_u8(ur.remap(frames[2], maps[0])), frames[2].astype(np.uint8))


def test_the_random_map_plants_what_it_says_and_the_constant_frame_shows_the_product_order():
    h, w = 33, 47
    m = ur.random_map(h, w, 5)
    inside = ur.in_range(m, h, w)
    assert inside.mean() >= 0.5 and (~inside).mean() >= 0.05
    x, y = m
    assert ((x == np.floor(x)) & (y == np.floor(y)) & inside).sum() >= 3 and ((x == w - 1) & inside).any() and ((y == h - 1) & inside).any()
    assert ((x < 0) & (x > -1e-6)).any() and ((y > h - 1) & (y < h - 1 + 1e-6)).any()
    # a constant 255 frame under a random in-range map: the weights' products do not sum to 1 exactly, the truncation shows it
    v = np.full((96, 130, 3), 255.0)
    mm = ur.random_map(96, 130, 6, outside=0.0)
    got = ur.to_u8(ur.remap(v, mm))[..., 0].reshape(-1)[ur.in_range(mm, 96, 130)]
    assert set(np.unique(got)) == {254, 255} and 0.03 < (got == 254).mean() < 0.25, (got == 254).mean()


# ---- 2. the table file --------------------------------------------------------------------------------------------------------
def test_lut_file_layout_follows_the_sdk_slicing(mods, tmp_path, monkeypatch):
    h, w = 5, 7
    m = ur.random_map(h, w, 2)
    path = tmp_path / "stereo_narrow_left_distortion_lut.bin"
    m.astype(np.float64).tofile(str(path))
    # CameraModel.__load_lut and undistort's slicing
    lut = np.fromfile(str(path), np.double)
    bilinear_lut = lut.reshape([2, lut.size // 2]).transpose()
    coords = bilinear_lut[:, 1::-1].T.reshape((2, h, w))
    got = mods["undistort"].read_lut_file(str(path), h, w)
    assert got.shape == (2, h * w) and got.dtype == np.float64
    assert np.array_equal(got[1].reshape(h, w), coords[0]) and np.array_equal(got[0].reshape(h, w), coords[1])  # (cy, cx)
    with pytest.raises(ValueError, match="lut.bin"):
        mods["undistort"].read_lut_file(str(path), h, w + 1)


def test_pattern_and_border_codes(mods):
    u = mods["undistort"]
    assert [u.pattern_code(p) for p in ur.PATTERNS] == [0, 1, 2, 3] and u.pattern_code("GBRG") == 3
    assert u.border_code("reflect") == 0 and u.border_code("mirror") == 1
    for bad in ("rgbg", "rgb", None, 3):
        with pytest.raises(ValueError, match="pattern"):
            u.pattern_code(bad)
    with pytest.raises(ValueError, match="border"):
        u.border_code("wrap")


# ---- 3. RobotCar's K and files ------------------------------------------------------------------------------------------------
def robotcar_tree(root, seq, stamps, h=4, w=6, mode="L", skip=()):
    from PIL import Image
    d = os.path.join(root, seq, "stereo", "centre")
    os.makedirs(d)
    for i, t in enumerate(stamps):
        if i not in skip:
            a = random_mosaic(h, w, i)
            Image.fromarray(a if mode == "L" else np.repeat(a[..., None], 3, 2)).save(os.path.join(d, "%d.png" % t))
    with open(os.path.join(root, seq, "stereo.timestamps"), "w") as f:
        for i, t in enumerate(stamps):
            f.write("%d %d\n" % (t, 1 + i // 3))
    models = os.path.join(root, "robotcar-dataset-sdk", "models")
    os.makedirs(models)
    with open(os.path.join(models, "stereo_narrow_left.txt"), "w") as f:
        f.write("983.044006 983.044006 643.646973 493.378998\n0 0 0 1\n")
    ur.random_map(h, w, 1).tofile(os.path.join(models, "stereo_narrow_left_distortion_lut.bin"))
    return root


def test_robotcar_intrinsics_and_paths(mods, tmp_path):
    rc = mods["robotcar"]
    stamps = [1418381798086398, 1418381798148890, 1418381798211382, 1418381798273874]
    root = robotcar_tree(str(tmp_path), "2014-12-12-10-45-15", stamps)
    files = rc.robotcar_paths(root, "2014-12-12-10-45-15")
    assert files["images"] == [os.path.join(root, "2014-12-12-10-45-15", "stereo", "centre", "%d.png" % t) for t in stamps]
    assert files["lut"].endswith("models/stereo_narrow_left_distortion_lut.bin") and files["intrinsics"].endswith("stereo_narrow_left.txt")
    und = rc.robotcar_paths(root, "2014-12-12-10-45-15", source="undistorted", ext="jpg")
    assert und["images"][1] == os.path.join(root, "2014-12-12-10-45-15", "undistorted_stereo", "centre", "%016d.jpg" % stamps[1])
    # oxford_robotcar.py get_intrinsics_param, restated with its own operations
    K = np.eye(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 983.044006, 983.044006, 643.646973, 493.378998
    K[0, 2] -= int(1280 * 0.0)
    K[1, 2] -= int(960 * 0.0)
    K[0] *= (640 / int(1280 * (1.0 - 0.0)))
    K[1] *= (192 / int(960 * (0.8 - 0.0)))
    got = rc.robotcar_intrinsics(files["intrinsics"], 192, 640)
    assert np.array_equal(got, K) and got[1, 1] == 983.044006 * (192 / 768)
    assert rc.CROP == [[0.0, 0.8], [0.0, 1.0]] and rc.PATTERN == "gbrg" and (rc.RAW_H, rc.RAW_W) == (960, 1280)
    with pytest.raises(ValueError, match="source"):
        rc.robotcar_paths(root, "2014-12-12-10-45-15", source="jpeg")


# ---- 4. FrameStream's mosaic arguments ----------------------------------------------------------------------------------------
class MosaicRing(FakeRing):
    """the fake ring with the mosaic submit: the host restatement, cropped (it does not resize)"""

    def submit_mosaic(self, slot, umap, pattern, border, h, w, box, out):
        assert slot not in self.todo and h * w <= self.stage[slot].size
        y0, y1, x0, x1 = box
        assert (y1 - y0, x1 - x0) == out.shape[:2]
        self.calls = getattr(self, "calls", []) + [(umap, pattern, border)]
        self.todo[slot] = (out, lambda s=slot: ur.undistort_mosaic(self.stage[s][:h * w].reshape(h, w), pattern, border, umap)[y0:y1, x0:x1])
        self.submits += 1


@time_limit
def test_frame_stream_mosaic_arguments(mods, tmp_path):
    fs = mods["frame_stream"]
    h, w = 4, 6
    root = robotcar_tree(str(tmp_path / "a"), "s", list(range(100, 109)), h, w)
    paths = mods["robotcar"].robotcar_paths(root, "s")["images"]
    m = ur.random_map(h, w, 1)
    ring = MosaicRing(3, h * w)
    with fs.FrameStream(paths, h, w, slots=3, workers=2, ring=ring, capacity=h * w, mosaic="gbrg", undistort=m, border="mirror") as s:
        for k in range(len(paths)):  # more frames than slots
            assert np.array_equal(s[k], ur.undistort_mosaic(random_mosaic(h, w, k), "gbrg", "mirror", m)), k
            s.release(k)
    assert all(c[1] == "gbrg" and c[2] == "mirror" and c[0] is m for c in ring.calls) and len(ring.calls) == len(paths)
    assert not workers_alive()
    ring = MosaicRing(3, h * w)
    with fs.FrameStream(paths, h, w, slots=3, workers=1, ring=ring, capacity=h * w, mosaic="RGGB") as s:  # no map: demosaic only
        assert np.array_equal(s[0], ur.undistort_mosaic(random_mosaic(h, w, 0), "rggb", "reflect"))
    assert ring.calls[0] == (None, "rggb", "reflect")
    # without `mosaic` an L file is a grey frame, as before
    ring = MosaicRing(3, h * w * 3)
    with fs.FrameStream(paths, h, w, slots=3, workers=1, ring=ring, capacity=h * w * 3) as s:
        assert np.array_equal(s[2], np.repeat(random_mosaic(h, w, 2)[..., None], 3, 2)) and not hasattr(ring, "calls")
    for kw, word in ((dict(mosaic="rgbg"), "pattern"), (dict(mosaic="gbrg", border="wrap"), "border"), (dict(undistort=m), "mosaic"),
                     (dict(border="mirror"), "mosaic"), (dict(mosaic="gbrg", kind="depth_u16"), "mosaic")):
        with pytest.raises(ValueError, match=word):
            fs.FrameStream(paths, h, w, ring=MosaicRing(12, h * w), capacity=h * w, **kw)
    assert not workers_alive()


@time_limit
def test_a_colour_file_in_a_mosaic_stream_raises_at_its_frame_only(mods, tmp_path):
    from PIL import Image
    fs = mods["frame_stream"]
    h, w = 4, 6
    root = robotcar_tree(str(tmp_path / "b"), "s", list(range(5)), h, w)
    paths = mods["robotcar"].robotcar_paths(root, "s")["images"]
    Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(paths[2])
    with fs.FrameStream(paths, h, w, slots=3, workers=2, ring=MosaicRing(3, h * w * 3), capacity=h * w * 3, mosaic="gbrg") as s:
        for k in (0, 1):
            assert np.array_equal(s[k], ur.undistort_mosaic(random_mosaic(h, w, k), "gbrg", "reflect"))
        with pytest.raises(fs.FrameStreamError) as e:
            s[2]
        assert paths[2] in str(e.value) and "mosaic" in str(e.value)
        s.release(2)
        assert np.array_equal(s[3], ur.undistort_mosaic(random_mosaic(h, w, 3), "gbrg", "reflect"))
    assert not workers_alive()


# ---- 5. argument errors, no device --------------------------------------------------------------------------------------------
def test_new_entry_points_refuse_bad_arguments_without_a_device(capi):
    lib = capi.lib()
    ERR_ARG = -2
    h = C.c_void_p()
    m = ur.identity_map(2, 3)

    def refused(rc, name, word):
        assert rc == ERR_ARG, (name, word, rc)
        msg = lib.dfvo_last_error()
        assert name in msg and word in msg, msg

    refused(lib.dfvo_undistort_create(2, 3, capi.as_ptr(m), None), b"dfvo_undistort_create", b"null out")
    refused(lib.dfvo_undistort_create(2, 3, None, C.byref(h)), b"dfvo_undistort_create", b"null map")
    for hh, ww in ((0, 3), (2, 0), (-1, 3), (1 << 15, 1 << 15)):
        refused(lib.dfvo_undistort_create(hh, ww, capi.as_ptr(m), C.byref(h)), b"dfvo_undistort_create", b"frame size")
    for bad in (np.nan, np.inf, -np.inf):
        mm = m.copy()
        mm[1, 4] = bad
        refused(lib.dfvo_undistort_create(2, 3, capi.as_ptr(mm), C.byref(h)), b"dfvo_undistort_create", b"non-finite")
        assert h.value is None
    lib.dfvo_undistort_destroy(None)

    def mosaic(map_=None, src=8, h_=4, w_=6, pattern=3, border=0, box=(0, 4, 0, 6), dst=16):
        return lib.dfvo_undistort_mosaic_u8(map_, src, h_, w_, pattern, border, box[0], box[1], box[2], box[3], dst, None)

    name = b"dfvo_undistort_mosaic_u8"
    refused(mosaic(src=None), name, b"null frame")
    refused(mosaic(dst=None), name, b"null frame")
    refused(mosaic(dst=18), name, b"aligned")
    refused(mosaic(pattern=4), name, b"pattern")
    refused(mosaic(pattern=-1), name, b"pattern")
    refused(mosaic(border=2), name, b"border")
    refused(mosaic(h_=0, box=(0, 0, 0, 6)), name, b"frame size")
    for box in ((0, 5, 0, 6), (-1, 4, 0, 6), (2, 2, 0, 6), (0, 4, 3, 7), (0, 4, 6, 6)):
        refused(mosaic(box=box), name, b"box")
    refused(mosaic(h_=1, box=(0, 1, 0, 6), border=1), name, b"mirror")
    refused(lib.dfvo_undistort_rgb_u8(None, 8, 0, 4, 0, 6, 16, None), b"dfvo_undistort_rgb_u8", b"null map")
    refused(lib.dfvo_frame_ring_submit_mosaic(None, 0, None, 3, 0, 4, 6, 0, 4, 0, 6, 16, 4, 6), b"dfvo_frame_ring_submit_mosaic", b"null ring")
