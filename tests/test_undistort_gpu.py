"""GPU: raw camera frames on the device (csrc/undistort.hip, df-vo_amd/undistort.py, the ring's mosaic submit).
  1. dfvo_undistort_mosaic_u8 / _rgb_u8 against the host restatement (tests/undistort_ref.py, which test_undistort_cpu.py holds
     against scipy.ndimage), byte for byte: every pattern, both borders, no map, the identity map, a random map with samples
     outside the frame and planted integer / n - 1 / just-outside coordinates, a constant-255 frame (a contracted or reordered
     product shows there), a box with a sentinel around it; sizes 2x2, 3x5, 33x47, 96x130
  2. FrameStream(mosaic=...) over PNG mosaics against mosaic_to_device, frame for frame, more frames than slots; a colour file
  3. a raw sequence through run_sequence against the same frames made by the restatement and image_to_device, bit for bit;
     robotcar.run_robotcar on a temporary RobotCar tree against the resident run"""
import importlib
import threading

import numpy as np
import pytest
import torch

import undistort_ref as ur
from synth import coded_tunnel_sequence, crafted_liteflownet_state_dict, crafted_monodepth2_state_dict

pytestmark = pytest.mark.gpu

SENTINEL = 171


@pytest.fixture(scope="module")
def mods(gpu):
    return {n: importlib.import_module("df-vo_amd." + n) for n in ("pipeline", "sequence", "frame_stream", "undistort", "synthetic")}


def workers_alive():
    return [t.name for t in threading.enumerate() if t.name.startswith("dfvo-frame-stream")]


def random_u8(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, shape, dtype=np.uint8)


def boxes(h, w):
    """the whole frame, and a box with odd offsets that ends inside it (one pixel at 2 x 2)"""
    y0, x0 = h // 3, w // 3 + (1 if w > 2 else 0)
    return [(0, h, 0, w), (y0, max(y0 + 1, h - max(1, h // 4)), x0, max(x0 + 1, w - max(1, w // 5)))]


def on_device(u, call, h, w, box):
    out = torch.full((h, w, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    call(out, box)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def framed(want, box):
    """the restatement inside the box, the sentinel outside"""
    y0, y1, x0, x1 = box
    out = np.full(want.shape, SENTINEL, np.uint8)
    out[y0:y1, x0:x1] = want[y0:y1, x0:x1]
    return out


# ---- 1. the operators ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ur.SIZES)
def test_operators_equal_the_restatement_byte_for_byte(gpu, mods, size):
    u = mods["undistort"]
    h, w = size
    rnd = ur.random_map(h, w, 5)
    inside = ur.in_range(rnd, h, w)
    assert inside.mean() >= 0.5 and (~inside).mean() >= 0.05, "the random map: %.3f inside" % inside.mean()
    inner = ur.random_map(h, w, 6, outside=0.0)
    maps = {"none": None, "identity": ur.identity_map(h, w), "random": rnd, "inner": inner}
    dev = {k: (None if m is None else u.UndistortMap(h, w, m)) for k, m in maps.items()}
    try:
        mosaic, white = random_u8((h, w), 3), np.full((h, w), 255, np.uint8)
        d_mosaic, d_white = torch.from_numpy(mosaic).cuda(), torch.from_numpy(white).cuda()
        n = 0
        for pattern in ur.PATTERNS:
            for border in ur.BORDERS:
                for name in ("none", "identity", "random"):
                    for box in boxes(h, w):
                        got = on_device(u, lambda out, b: u.undistort_mosaic(d_mosaic, dev[name], pattern, border, b, out), h, w, box)
                        want = framed(ur.undistort_mosaic(mosaic, pattern, border, maps[name]), box)
                        assert np.array_equal(got, want), (pattern, border, name, box, int((got != want).sum()))
                        n += 1
                # the constant frame: 1 - t and t do not always multiply and add up to 1; scipy's order truncates those to 254
                got = on_device(u, lambda out, b: u.undistort_mosaic(d_white, dev["inner"], pattern, border, b, out), h, w, (0, h, 0, w))
                want = ur.undistort_mosaic(white, pattern, border, inner)
                assert np.array_equal(got, want), (pattern, border, "constant 255", int((got != want).sum()))
                if border == "mirror" and h * w > 1000:
                    assert 0.03 < (want == 254).mean() < 0.25
        assert n == 4 * 2 * 3 * 2
        assert np.array_equal(ur.undistort_mosaic(mosaic, "gbrg", "reflect", maps["identity"]), ur.undistort_mosaic(mosaic, "gbrg", "reflect"))
        # the remap alone, on a distorted RGB frame
        for rgb in (random_u8((h, w, 3), 4), np.full((h, w, 3), 255, np.uint8)):
            d_rgb = torch.from_numpy(rgb).cuda()
            for name in ("identity", "random", "inner"):
                for box in boxes(h, w):
                    got = on_device(u, lambda out, b: u.undistort_rgb(d_rgb, dev[name], b, out), h, w, box)
                    want = framed(ur.undistort_rgb(rgb, maps[name]), box)
                    assert np.array_equal(got, want), ("rgb", name, box, int((got != want).sum()))
            assert np.array_equal(ur.undistort_rgb(rgb, maps["identity"]), rgb)
    finally:
        for m in dev.values():
            if m is not None:
                m.close()


def test_device_argument_errors_enqueue_nothing(gpu, mods):
    u = mods["undistort"]
    lib = gpu.lib()
    with pytest.raises(gpu.DfvoError, match="non-finite"):
        bad = ur.identity_map(3, 5)
        bad[0, 7] = np.nan
        u.UndistortMap(3, 5, bad)
    with u.UndistortMap(3, 5, ur.identity_map(3, 5)) as m:
        src = torch.zeros((4, 5), dtype=torch.uint8, device="cuda")
        out = torch.full((4, 5, 3), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert lib.dfvo_undistort_mosaic_u8(m.handle, src.data_ptr(), 4, 5, 3, 0, 0, 4, 0, 5, out.data_ptr(), None) == -2
        assert b"another frame size" in lib.dfvo_last_error()
        assert lib.dfvo_undistort_rgb_u8(m.handle, out.data_ptr(), 0, 3, 0, 5, out.data_ptr(), None) == -2
        assert lib.dfvo_undistort_rgb_u8(m.handle, src.data_ptr(), 0, 4, 0, 5, out.data_ptr(), None) == -2 and b"box" in lib.dfvo_last_error()
        torch.cuda.synchronize()
        assert (out == SENTINEL).all()
    ring = mods["frame_stream"].FrameRing(2, 4 * 5)
    try:
        def submit(slot=0, h=4, w=5, pattern=3, border=0, box=(0, 4, 0, 5), dst=out.data_ptr()):
            return lib.dfvo_frame_ring_submit_mosaic(ring.h, slot, None, pattern, border, h, w, box[0], box[1], box[2], box[3], dst, 4, 5)
        for kw, word in ((dict(slot=2), b"slot"), (dict(h=5, box=(0, 5, 0, 5)), b"staging capacity"), (dict(pattern=7), b"pattern"),
                         (dict(border=5), b"border"), (dict(box=(0, 5, 0, 5)), b"box"), (dict(dst=None), b"output")):
            assert submit(**kw) == -2 and word in lib.dfvo_last_error(), kw
        assert ring.pending() == 0
        ring.staging(0)[:] = 9
        gpu.check(submit())
        assert submit() == -2 and b"not been waited for" in lib.dfvo_last_error()
        ring.wait(0)
        assert np.array_equal(out.cpu().numpy(), ur.undistort_mosaic(np.full((4, 5), 9, np.uint8), "gbrg", "reflect"))
    finally:
        ring.close()


# ---- 2. the stream ------------------------------------------------------------------------------------------------------------
OUT_H, OUT_W = 24, 40
CROP = [[0.0, 0.8], [0.1, 1.0]]


@pytest.fixture(scope="module")
def mosaic_pngs(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("mosaics")
    paths = []
    for k in range(9):
        p = str(d / ("%d.png" % (1000 + k)))
        Image.fromarray(random_u8((33, 47), 100 + k)).save(p)
        paths.append(p)
    return paths


@pytest.mark.parametrize("mapped,border", [(True, "reflect"), (False, "mirror")])
def test_mosaic_stream_equals_mosaic_to_device_frame_for_frame(gpu, mods, mosaic_pngs, mapped, border):
    from PIL import Image
    fs, u = mods["frame_stream"], mods["undistort"]
    h, w = 33, 47
    m = ur.random_map(h, w, 8)
    umap = u.UndistortMap(h, w, m) if mapped else None
    try:
        mosaics = [np.array(Image.open(p)) for p in mosaic_pngs]
        want = [u.mosaic_to_device(a, OUT_H, OUT_W, umap, "gbrg", CROP, border).cpu().numpy() for a in mosaics]
        # mosaic_to_device itself: read_image's tail on the restatement's frame
        ref = mods["sequence"].image_to_device(ur.undistort_mosaic(mosaics[4], "gbrg", border, m if mapped else None), OUT_H, OUT_W, CROP)
        assert np.array_equal(want[4], ref.cpu().numpy())
        with fs.FrameStream(mosaic_pngs, OUT_H, OUT_W, crop=CROP, slots=4, workers=3, mosaic="gbrg", undistort=umap, border=border) as s:
            held = {}
            for k in range(len(mosaic_pngs)):  # nine frames through four slots and the ring's one RGB plane
                held[k] = s[k]
                assert np.array_equal(held[k].cpu().numpy(), want[k]), "frame %d" % k
                if k >= 2:
                    assert np.array_equal(held[k - 2].cpu().numpy(), want[k - 2]), "frame %d changed while it was held" % (k - 2)
                    s.release(k - 2)
                    del held[k - 2]
            assert s.max_live <= 4 and s._ring.pending() == 0
    finally:
        if umap is not None:
            umap.close()
    assert not workers_alive()


def test_a_colour_file_raises_at_its_frame_only(gpu, mods, mosaic_pngs, tmp_path):
    from PIL import Image
    fs, u = mods["frame_stream"], mods["undistort"]
    colour = str(tmp_path / "1002.png")
    Image.fromarray(random_u8((33, 47, 3), 1)).save(colour)
    paths = mosaic_pngs[:2] + [colour] + mosaic_pngs[3:5]
    with fs.FrameStream(paths, OUT_H, OUT_W, slots=3, workers=2, mosaic="gbrg") as s:
        for k in (0, 1):
            want = u.mosaic_to_device(np.array(Image.open(paths[k])), OUT_H, OUT_W, None, "gbrg")
            assert np.array_equal(s[k].cpu().numpy(), want.cpu().numpy())
        with pytest.raises(fs.FrameStreamError) as e:
            s[2]
        assert colour in str(e.value)
        s.release(2)
        want = u.mosaic_to_device(np.array(Image.open(paths[3])), OUT_H, OUT_W, None, "gbrg")
        assert np.array_equal(s[3].cpu().numpy(), want.cpu().numpy())
    assert not workers_alive()


# ---- 3. a raw sequence --------------------------------------------------------------------------------------------------------
H, W, FEED, N = 128, 416, (64, 96), 7  # tests/test_frame_stream_gpu.py's world and sizes


def barrel_map(h, w, k=-0.05):
    """a mild barrel distortion: every sample inside the frame"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cy, cx = (h - 1) / 2, (w - 1) / 2
    r2 = ((yy - cy) ** 2 + (xx - cx) ** 2) / (cy * cy + cx * cx)
    return np.stack([(cx + (xx - cx) * (1 + k * r2)).reshape(-1), (cy + (yy - cy) * (1 + k * r2)).reshape(-1)])


def test_run_robotcar_on_a_temporary_tree_equals_the_resident_run(gpu, mods, tmp_path):
    """the runner end to end: timestamps' order, the table file, K, the crop, the mosaic stream, the trajectory file"""
    from PIL import Image
    rc, dc, ev = (importlib.import_module("df-vo_amd." + n) for n in ("robotcar", "default_cfg", "evaluation"))
    pmod, smod, u, syn = (mods[k] for k in ("pipeline", "sequence", "undistort", "synthetic"))
    seq = coded_tunnel_sequence(H, W, N, mode="pot", seed=31, poses=syn.tunnel_poses_lateral(N, 0.4))
    m = barrel_map(H, W)
    mosaics = [ur.mosaic_of(f, "gbrg") for f in seq["frames"]]
    root, name = str(tmp_path / "robotcar"), "2014-05-06-12-54-54"
    stamps = [1399381446000000 + 62500 * k for k in range(N)]
    d = tmp_path / "robotcar" / name / "stereo" / "centre"
    d.mkdir(parents=True)
    for t, a in zip(stamps, mosaics):
        Image.fromarray(a).save(str(d / ("%d.png" % t)))
    (tmp_path / "robotcar" / name / "stereo.timestamps").write_text("".join("%d 1\n" % t for t in stamps))
    models = tmp_path / "robotcar" / "robotcar-dataset-sdk" / "models"
    models.mkdir(parents=True)
    (models / "stereo_narrow_left.txt").write_text("983.044006 983.044006 643.646973 493.378998\n0 0 0 1\n")
    m.tofile(str(models / "stereo_narrow_left_distortion_lut.bin"))
    cfg = dc.default_configuration(H, W, None, None)
    cfg.seq = name
    cfg.directory = dc.Cfg(img_seq_dir=root, depth_dir=None, gt_pose_dir=None)
    fsd, dsd = crafted_liteflownet_state_dict(H, W, "pot"), crafted_monodepth2_state_dict()
    out = rc.run_robotcar(cfg, fsd, dsd, out_dir=str(tmp_path / "result"), gt_poses=seq["poses"], feed_h=FEED[0], feed_w=FEED[1], slots=5,
                          workers=2, raw_size=(H, W))
    assert out["poses"].shape == (N, 4, 4) and out["metrics"] is not None and not workers_alive()
    K = rc.robotcar_intrinsics(str(models / "stereo_narrow_left.txt"), H, W)
    p = pmod.TrackingPipeline.from_cfg(cfg, K, fsd, dsd, FEED[0], FEED[1])
    try:
        with u.UndistortMap(H, W, m) as umap:
            frames = [u.mosaic_to_device(a, H, W, umap, rc.PATTERN, rc.CROP) for a in mosaics]
        host = smod.image_to_device(ur.undistort_mosaic(mosaics[3], "gbrg", "reflect", m), H, W, rc.CROP)
        assert np.array_equal(frames[3].cpu().numpy(), host.cpu().numpy())
        poses, rows = smod.run_sequence(p, frames, N, seed=cfg.seed)
    finally:
        p.close()
    print("run_robotcar: status", rows[:, 16].tolist())
    assert np.array_equal(out["gathered"], rows) and np.array_equal(out["poses"], poses)
    assert np.array_equal(ev.load_traj(str(tmp_path / "result" / (name + ".txt"))), poses)


def test_a_raw_sequence_tracks_like_the_host_made_frames(gpu, mods, tmp_path):
    """the "pot" encoding (smooth potentials, decoded as differences) survives the demosaic's interpolation; the per-site
    codes of "mux" would not"""
    from PIL import Image
    pmod, smod, fs, u, syn = (mods[k] for k in ("pipeline", "sequence", "frame_stream", "undistort", "synthetic"))
    seq = coded_tunnel_sequence(H, W, N, mode="pot", seed=31, poses=syn.tunnel_poses_lateral(N, 0.4))
    m = barrel_map(H, W)
    assert ur.in_range(m, H, W).all()
    mosaics = [ur.mosaic_of(f, "gbrg") for f in seq["frames"]]
    paths = []
    for k, a in enumerate(mosaics):
        paths.append(str(tmp_path / ("%d.png" % (5000 + k))))
        Image.fromarray(a).save(paths[-1])
    p = pmod.TrackingPipeline(H, W, FEED[0], FEED[1], seq["K"], crafted_liteflownet_state_dict(H, W, "pot"), crafted_monodepth2_state_dict(),
                              seed=4869)
    umap = u.UndistortMap(H, W, m)
    try:
        frames = [smod.image_to_device(ur.undistort_mosaic(a, "gbrg", "reflect", m), H, W) for a in mosaics]
        want_traj, want_rows = smod.run_sequence(p, frames, N)
        want_state = p.get_rng_state()
        print("host-made frames: status", want_rows[:, 16].tolist())
        assert (want_rows[:, 16] != 1).any(), "no pair was tracked: the comparison would be between identities"
        with fs.FrameStream(paths, H, W, slots=5, workers=3, mosaic="gbrg", undistort=umap) as s:
            traj, rows = smod.run_sequence(p, s, N)
            state = p.get_rng_state()
        assert np.array_equal(rows, want_rows) and np.array_equal(traj, want_traj)
        assert np.array_equal(state[1], want_state[1]) and state[2] == want_state[2]
        plain = [smod.image_to_device(ur.undistort_mosaic(a, "gbrg", "reflect"), H, W) for a in mosaics]  # the table matters
        assert not np.array_equal(smod.run_sequence(p, plain, N)[1], want_rows)
    finally:
        p.sync()
        umap.close()
        p.close()
    assert not workers_alive()
