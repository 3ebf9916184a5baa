"""GPU: baseline JPEG frames decoded on the device (df-vo_amd/jpeg.py, csrc/jpeg.hip, FrameStream(jpeg="device")).
  5. dfvo_jpeg_decode_u8 equals Pillow's pixels (tests/golden/jpeg_cases.npz) byte for byte on the whole case matrix;
  6. FrameStream(jpeg="device") frames equal FrameStream() frames byte for byte -- no crop and no resize, a crop plus a resize, a
     grey file, a sequence that mixes PNG and JPEG; a corrupt file in the middle raises at its own frame only;
  7. jpeg_to_device equals image_to_device of Pillow's decode;
  8. run_kitti_odom over a tiny JPEG sequence: the pose rows of jpeg="host" and jpeg="device" are bit-identical."""
import importlib
import os
import threading

import numpy as np
import pytest
import torch

import jpeg_cases
from synth import coded_tunnel_sequence, crafted_liteflownet_state_dict, crafted_monodepth2_state_dict

pytestmark = pytest.mark.gpu

H, W, FEED = 128, 416, (64, 96)
N = 6
SRC = (141, 451)  # the files' size where the stream resizes: partial MCUs both ways
CROP = [[11 / 141 + 1e-9, 130 / 141 + 1e-9], [21 / 451 + 1e-9, 440 / 451 + 1e-9]]


@pytest.fixture(scope="module")
def mods(gpu):
    return {n: importlib.import_module("df-vo_amd." + n) for n in ("pipeline", "sequence", "frame_stream", "kitti", "default_cfg", "jpeg")}


def workers_alive():
    return [t.name for t in threading.enumerate() if t.name.startswith("dfvo-frame-stream")]


# ---- 5. the operator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", jpeg_cases.CASES, ids=[c.name for c in jpeg_cases.CASES])
def test_device_decode_equals_pillows_pixels(mods, case):
    data, want = jpeg_cases.fixture()[case.name]
    got = mods["jpeg"].decode_to_device(data).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = np.argwhere(got != want)
    assert diff.size == 0, "%d bytes differ, the first at %s: %d, Pillow %d" % (len(diff), diff[0].tolist(), got[tuple(diff[0])],
                                                                               want[tuple(diff[0])])


def test_decode_refuses_a_header_that_is_not_its_own_layout(gpu, mods):
    data, _ = jpeg_cases.fixture()["17x23-420-q50"]
    info, buf, _ = mods["jpeg"].entropy_decode(data)
    d_buf = torch.from_numpy(buf).cuda()
    dst = torch.zeros((17, 23, 3), dtype=torch.uint8, device="cuda")
    lib = gpu.lib()
    import ctypes as C
    for field, value in (("width", 4000), ("components", 2), ("h_samp", 4)):
        bad = type(info).from_buffer_copy(info)
        setattr(bad, field, value)
        assert lib.dfvo_jpeg_decode_u8(d_buf.data_ptr(), C.byref(bad), dst.data_ptr(), None) == -2, field
        assert b"dfvo_jpeg_decode_u8" in lib.dfvo_last_error()
    bad = type(info).from_buffer_copy(info)
    bad.plane_offset[1] += 128
    assert lib.dfvo_jpeg_decode_u8(d_buf.data_ptr(), C.byref(bad), dst.data_ptr(), None) == -2
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0  # nothing was launched


# ---- 6. the stream ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """tunnel-world frames as files: "same" (128 x 416, 4:2:0 JPEG), "pot" (that size in the potential encoding, 4:2:0 at quality 95: the runner's), "ragged" (141 x 451, 4:2:2 JPEG), "grey" (141 x 451 mode-L
    JPEG), "mixed" (141 x 451: PNG and 4:4:4 JPEG by turns), and the sequence the frames came from"""
    from PIL import Image
    d = tmp_path_factory.mktemp("jpeg_frames")
    same = coded_tunnel_sequence(H, W, N, mode="mux", step=1.0, seed=31)
    ragged = coded_tunnel_sequence(SRC[0], SRC[1], N, mode="pot", step=1.0, seed=31)
    pot = coded_tunnel_sequence(H, W, N, mode="pot", step=1.0, seed=31)
    out = {"same": [], "pot": [], "ragged": [], "grey": [], "mixed": [], "seq": same}
    for k in range(N):
        for name, frame, kw in (("same", same["frames"][k], dict(quality=92, subsampling=2)),
                                ("pot", pot["frames"][k], dict(quality=95, subsampling=2)),
                                ("ragged", ragged["frames"][k], dict(quality=75, subsampling=1)),
                                ("grey", ragged["frames"][k][..., 2], dict(quality=85))):
            p = str(d / ("%s_%06d.jpg" % (name, k)))
            Image.fromarray(frame).save(p, **kw)
            out[name].append(p)
        p = str(d / ("mixed_%06d.%s" % (k, "png" if k % 2 else "jpg")))
        Image.fromarray(ragged["frames"][k]).save(p, **({} if k % 2 else dict(quality=95, subsampling=0)))
        out["mixed"].append(p)
    return out


def frames_of(fs, paths, h, w, **kw):
    with fs.FrameStream(paths, h, w, slots=4, workers=2, **kw) as s:
        s.begin(0, len(paths) - 1)
        got = []
        for k in range(len(paths)):
            got.append(s[k].cpu().numpy().copy())
            s.release(k)
    assert s.pending() == 0 and not workers_alive()
    return got


@pytest.mark.parametrize("which,size,crop", [("same", (H, W), None), ("ragged", (H, W), CROP), ("grey", (H, W), CROP),
                                             ("grey", SRC, None), ("mixed", (H, W), None), ("mixed", SRC, None)])
def test_stream_frames_equal_the_host_decoded_streams(mods, files, which, size, crop):
    fs = mods["frame_stream"]
    want = frames_of(fs, files[which], size[0], size[1], crop=crop)
    got = frames_of(fs, files[which], size[0], size[1], crop=crop, jpeg="device")
    assert len(got) == N
    for k in range(N):
        assert np.array_equal(got[k], want[k]), "frame %d of %s differs in %d bytes" % (k, which, int((got[k] != want[k]).sum()))
    assert any(not np.array_equal(want[0], f) for f in want[1:])  # (the frames are not all one frame)


def test_a_corrupt_jpeg_raises_at_its_own_frame_only(mods, files, tmp_path):
    fs = mods["frame_stream"]
    data = open(files["same"][3], "rb").read()
    cut, prog = str(tmp_path / "cut.jpg"), str(tmp_path / "progressive.jpg")
    with open(cut, "wb") as f:
        f.write(data[:len(data) // 2])
    from PIL import Image
    Image.open(files["same"][4]).save(prog, progressive=True)
    paths = files["same"][:3] + [cut, prog] + files["same"][5:]
    want = frames_of(fs, files["same"], H, W)
    s = fs.FrameStream(paths, H, W, slots=4, workers=2, jpeg="device")
    try:
        s.begin(0, N - 1)
        for k in range(N):
            if k == 3:
                with pytest.raises(fs.FrameStreamError) as e:
                    s[k]
                assert cut in str(e.value) and "data ends early" in str(e.value)
            elif k == 4:
                with pytest.raises(fs.FrameStreamError) as e:
                    s[k]
                assert prog in str(e.value) and "progressive" in str(e.value)
            else:
                assert np.array_equal(s[k].cpu().numpy(), want[k]), k
            s.release(k)
    finally:
        s.close()
    assert s.pending() == 0 and not workers_alive()


def test_stream_argument_errors(mods, files):
    fs = mods["frame_stream"]
    with pytest.raises(ValueError, match="jpeg"):
        fs.FrameStream(files["same"], H, W, jpeg="gpu")
    with pytest.raises(ValueError, match="jpeg"):
        fs.FrameStream(files["grey"], H, W, jpeg="device", mosaic="gbrg")
    with pytest.raises(ValueError, match="jpeg"):
        fs.FrameStream(files["grey"], H, W, jpeg="device", kind="depth_u16")
    assert not workers_alive()


# ---- 7. the resident twin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,crop", [("ragged", CROP), ("grey", None), ("same", None)])
def test_jpeg_to_device_equals_image_to_device_of_pillows_decode(mods, files, which, crop):
    from PIL import Image
    path = files[which][2]
    dec = np.array(Image.open(path))
    if dec.ndim == 2:
        dec = np.repeat(dec[..., None], 3, axis=2)  # (cv2.imread replicates a grey file)
    want = mods["sequence"].image_to_device(dec, H, W, crop=crop).cpu().numpy()
    got = mods["jpeg"].jpeg_to_device(path, H, W, crop=crop).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(mods["jpeg"].jpeg_to_device(open(path, "rb").read(), H, W, crop=crop).cpu().numpy(), want)


# ---- 8. the runner ------------------------------------------------------------------------------------------------------------
CALIB = "".join("P%d: 718.856 0.0 607.1928 0.0 0.0 718.856 185.2157 0.0 0.0 0.0 1.0 0.0\n" % i for i in range(4))


def test_run_kitti_odom_rows_are_bit_identical_between_host_and_device_decode(mods, files, tmp_path):
    import shutil
    kitti, dc = mods["kitti"], mods["default_cfg"]
    d = tmp_path / "odom_data" / "04" / "image_2"
    os.makedirs(str(d))
    for k, p in enumerate(files["pot"]):
        shutil.copy(p, str(d / ("%06d.jpg" % k)))
    with open(str(tmp_path / "odom_data" / "04" / "calib.txt"), "w") as f:
        f.write(CALIB)
    cfg = dc.default_configuration(H, W, None, None)
    cfg.seq = "04"
    cfg.image.ext = "jpg"
    cfg.directory = dc.Cfg(img_seq_dir=str(tmp_path / "odom_data"), depth_dir=None, gt_pose_dir=None)
    weights = crafted_liteflownet_state_dict(H, W, "pot"), crafted_monodepth2_state_dict()
    runs = {}
    for mode in ("host", "device"):
        runs[mode] = kitti.run_kitti_odom(cfg, weights[0], weights[1], feed_h=FEED[0], feed_w=FEED[1], slots=5, workers=2, jpeg=mode)
        assert not workers_alive()
    rows = runs["host"]["gathered"]
    print("status per pair:", rows[:, 16].tolist())
    assert (rows[:, 16] != 1).any(), "no pair was tracked: the comparison would be between constant-motion rows"
    assert np.array_equal(runs["device"]["gathered"], rows) and np.array_equal(runs["device"]["poses"], runs["host"]["poses"])
