"""CPU: FrameStream's window logic over a fake ring (a Python object with the ring's methods over host arrays), the decoder's
modes, and track_chunk's begin / release hooks.  No device: the fake ring's `upload` is a numpy copy that lands at wait(), so
a frame handed out before its wait, or a slot decoded into while its frame is still named by a pair in flight, shows as wrong
bytes.  Every case that could deadlock runs under a time limit (SIGALRM), so a deadlock fails instead of hanging."""
import functools
import importlib
import signal
import struct
import threading
import zlib

import numpy as np
import pytest

H, W = 6, 8
LIMIT_S = 10


def time_limit(fn):
    @functools.wraps(fn)
    def run(*a, **kw):
        def fire(signum, frame):
            raise AssertionError("%s did not finish in %d s (deadlock?)" % (fn.__name__, LIMIT_S))
        old = signal.signal(signal.SIGALRM, fire)
        signal.alarm(LIMIT_S)
        try:
            return fn(*a, **kw)
        finally:
            signal.alarm(0)
            signal.signal(signal.SIGALRM, old)
    return run


@pytest.fixture(scope="module")
def fmod():
    import __graft_entry__ as g
    g.dfvo_amd()
    return importlib.import_module("df-vo_amd.frame_stream")


@pytest.fixture(scope="module")
def smod(fmod):
    return importlib.import_module("df-vo_amd.sequence")


def workers_alive():
    return [t.name for t in threading.enumerate() if t.name.startswith("dfvo-frame-stream")]


class FakeRing:
    """the ring's methods over host arrays.  submit_* only notes the work; wait() performs it (the copy is asynchronous)"""

    def __init__(self, slots, capacity):
        self.stage = [np.zeros(capacity, np.uint8) for _ in range(slots)]
        self.todo = {}
        self.closed = False
        self.submits = 0

    def staging(self, slot):
        return self.stage[slot]

    def new_output(self, shape, dtype):
        return np.full(shape, 255, dtype)

    def submit_image(self, slot, h, w, ch, box, out):
        assert slot not in self.todo, "submit on a slot whose last submit has not been waited for"
        assert h * w * ch <= self.stage[slot].size
        y0, y1, x0, x1 = box
        assert (y1 - y0, x1 - x0) == out.shape[:2], "the fake ring does not resize"
        self.todo[slot] = (out, lambda s=slot: np.broadcast_to(self.stage[s][:h * w * ch].reshape(h, w, ch)[y0:y1, x0:x1], out.shape))
        self.submits += 1

    def submit_raw(self, slot, nbytes, out):
        assert slot not in self.todo and nbytes == out.nbytes
        self.todo[slot] = (out, lambda s=slot: self.stage[s][:nbytes].view(out.dtype).reshape(out.shape))
        self.submits += 1

    def wait(self, slot):
        if slot in self.todo:
            out, src = self.todo.pop(slot)
            out[...] = src()

    def pending(self):
        return len(self.todo)

    def close(self):
        self.closed = True


def frame(k):
    """frame k: every byte tells the frame, the channel and the row"""
    a = np.zeros((H, W, 3), np.uint8)
    a[...] = (np.arange(H)[:, None, None] + 10 * np.arange(3)[None, None, :] + 40 * k) % 251
    return a


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("frames")
    paths = []
    for k in range(12):
        p = d / ("%06d.png" % k)
        Image.fromarray(frame(k)).save(str(p))
        paths.append(str(p))
    return paths


def make(fmod, paths, slots=5, workers=2, **kw):
    ring = FakeRing(slots, kw.pop("capacity", H * W * 3))
    return fmod.FrameStream(paths, H, W, slots=slots, workers=workers, ring=ring, capacity=ring.stage[0].size, **kw), ring


class _Out:
    status, scale = 1, 0.0


class CheckingPipe:
    """a pipeline stub that keeps the arrays it is handed and checks, when a pair's track_end returns, that they still hold the
    pair's frames -- the pipeline's lifetime rule seen from the device's side"""

    def __init__(self, smod, expect=frame):
        self.smod, self.expect, self.held, self.checked, self.halo = smod, expect, {}, 0, None

    def set_ref_image(self, f):
        self.halo = f

    set_ref_depth_image = set_ref_image

    def seed(self, s):
        pass

    def enqueue_nets(self, slot, ref, cur, d_feed=None, depth=None):
        self.held[slot] = (ref, cur, depth)

    def prefetch_track(self, slot):
        pass

    def track_begin(self, slot):
        pass

    def track_end(self, slot):
        ref, cur, depth = self.held.pop(slot)
        j = self.j
        assert j % self.smod.SLOTS == slot
        if j == self.lo:
            assert np.array_equal(self.halo, self.expect(j) if depth is None else depth_plane(j)), "halo of the chunk"
        if ref is not None:
            assert np.array_equal(ref, self.expect(j)), "reference frame of pair %d changed before its track_end" % j
        assert np.array_equal(cur, self.expect(j + 1)), "current frame of pair %d changed before its track_end" % j
        if depth is not None:
            assert np.array_equal(depth, depth_plane(j + 1)), "depth image of pair %d" % j
        self.j = j + 1
        self.checked += 1
        return _Out()

    def sync(self):
        pass

    def chunk(self, frames, lo, hi, **kw):
        self.lo = self.j = lo
        return self.smod.track_chunk(self, frames, lo, hi, **kw)


@pytest.mark.parametrize("slots,workers,carry", [(5, 1, True), (5, 4, True), (5, 4, False), (8, 1, False), (8, 4, True), (12, 6, True)])
@time_limit
def test_a_chunk_over_the_stream_keeps_every_frame_until_its_pair_has_ended(fmod, smod, files, slots, workers, carry):
    """slots = ahead + 2 = 5 is the smallest ring track_chunk takes: the stream completes (decode on demand) and never holds more
    frames than it has slots"""
    s, ring = make(fmod, files, slots=slots, workers=workers)
    with s:
        pipe = CheckingPipe(smod)
        pipe.chunk(s, 0, len(files) - 1, carry_features=carry)
        assert pipe.checked == len(files) - 1
        assert 1 <= s.max_live <= slots
        assert ring.pending() == 0
    assert ring.closed and not workers_alive()


@time_limit
def test_two_chunks_of_one_rank_restart_the_prefetch(fmod, smod, files):
    s, ring = make(fmod, files, slots=5, workers=3)
    with s:
        pipe = CheckingPipe(smod)
        pipe.chunk(s, 0, 4)
        pipe.chunk(s, 6, 11)
        pipe.chunk(s, 2, 7, carry_features=False)  # back again: begin() restarts below what was released
        assert pipe.checked == 4 + 5 + 5 and s.max_live <= 5
    assert not workers_alive()


def test_fewer_slots_than_ahead_plus_two_is_a_value_error(fmod, smod, files):
    s, _ = make(fmod, files, slots=4, workers=1)
    with s:
        with pytest.raises(ValueError, match="slots"):
            CheckingPipe(smod).chunk(s, 0, 5)  # ahead = 3
        assert CheckingPipe(smod).chunk(s, 0, 5, ahead=2)[1].shape == (5,)
    assert not workers_alive()


@time_limit
def test_index_error_below_the_window_and_outside_the_sequence(fmod, files):
    s, _ = make(fmod, files, slots=3, workers=2)
    with s:
        assert np.array_equal(s[0], frame(0)) and np.array_equal(s[1], frame(1)) and np.array_equal(s[0], frame(0))
        s.release(1)
        with pytest.raises(IndexError, match="released"):
            s[1]
        with pytest.raises(IndexError):
            s[0]
        assert np.array_equal(s[2], frame(2)) and np.array_equal(s[4], frame(4))  # (3 is skipped: decoded, never asked for)
        for k in (len(files), -1):
            with pytest.raises(IndexError):
                s[k]
        s.begin(2, 5)
        with pytest.raises(IndexError, match="beyond"):
            s[6]
    assert not workers_alive()


@time_limit
def test_a_full_window_raises_instead_of_waiting_forever(fmod, files):
    s, _ = make(fmod, files, slots=2, workers=2)
    with s:
        s[0], s[1]
        with pytest.raises(RuntimeError, match="release"):
            s[2]
        s.release(0)
        assert np.array_equal(s[2], frame(2)) and np.array_equal(s[1], frame(1))
    assert not workers_alive()


@pytest.mark.parametrize("how", ["truncated", "missing", "too_large", "sixteen_bit"])
@time_limit
def test_a_bad_file_raises_at_its_own_index_naming_the_path(fmod, files, tmp_path, how):
    from PIL import Image
    bad = tmp_path / "000003.png"
    if how == "truncated":
        noise = np.random.Generator(np.random.PCG64(5)).integers(0, 256, (H, W, 3), dtype=np.uint8)  # (does not compress)
        Image.fromarray(noise).save(str(bad))
        whole = bad.read_bytes()
        bad.write_bytes(whole[:len(whole) // 2])  # cut inside the image data
    elif how == "too_large":
        Image.fromarray(np.zeros((H + 1, W, 3), np.uint8)).save(str(bad))
    elif how == "sixteen_bit":
        bad.write_bytes(png_rgb16(H, W))
    paths = files[:3] + [str(bad)] + files[4:7]
    s, ring = make(fmod, paths, slots=4, workers=3)
    with s:
        got = [s[k] for k in range(3)]
        with pytest.raises(fmod.FrameStreamError) as e:
            s[3]
        assert str(bad) in str(e.value)
        if how == "sixteen_bit":
            assert "16-bit" in str(e.value)
        if how == "too_large":
            assert "staging capacity" in str(e.value)
        for k in range(3):
            assert np.array_equal(got[k], frame(k)), "frame %d before the bad one" % k
        with pytest.raises(fmod.FrameStreamError):  # asked again: the same answer
            s[3]
        s.release(2)
        assert np.array_equal(s[4], frame(4))  # the bad frame holds no slot
    assert not workers_alive() and ring.pending() == 0 and s.pending() == 0  # (uploads of frames 5, 6 may have been in flight)


@time_limit
def test_no_worker_outlives_close_or_an_exception(fmod, smod, files, tmp_path):
    s, ring = make(fmod, files, slots=5, workers=4)
    assert len(workers_alive()) == 4
    s[0]
    s.close()
    s.close()
    assert ring.closed and not workers_alive()
    with pytest.raises(RuntimeError, match="closed"):
        s[0]
    paths = files[:4] + [str(tmp_path / "nothing_here.png")] + files[5:]
    s, ring = make(fmod, paths, slots=5, workers=4)
    with pytest.raises(fmod.FrameStreamError, match="nothing_here.png"):
        with s:
            CheckingPipe(smod).chunk(s, 0, 8)
    assert ring.closed and not workers_alive() and ring.pending() == 0


def test_workers_is_a_plain_argument_capped_at_sixteen(fmod, files):
    for w in (17, 64, 0, -1, 2.0, None):
        with pytest.raises(ValueError, match="workers"):
            fmod.FrameStream(files, H, W, workers=w, ring=FakeRing(8, H * W * 3), capacity=H * W * 3)
    with pytest.raises(ValueError, match="slots"):
        fmod.FrameStream(files, H, W, slots=0, ring=FakeRing(1, H * W * 3), capacity=H * W * 3)
    with pytest.raises(ValueError, match="kind"):
        fmod.FrameStream(files, H, W, kind="depth", ring=FakeRing(8, H * W * 3), capacity=H * W * 3)
    assert not workers_alive()
    assert fmod.MAX_WORKERS == 16
    import inspect
    assert "cpu_count" not in inspect.getsource(fmod)


# ---- the decoder's modes ---------------------------------------------------------------------------------------------------
def png_rgb16(h, w):
    """a 16-bit RGB PNG (Pillow writes none)"""
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    rows = b"".join(b"\x00" + bytes(6 * w) for _ in range(h))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows))
            + chunk(b"IEND", b""))


def depth_plane(k):
    return (np.arange(H * W, dtype=np.uint32).reshape(H, W) * 257 + 1000 * k).astype(np.uint16)


def test_decode_follows_imread_plus_bgr2rgb(fmod, tmp_path):
    from PIL import Image
    rgb = frame(3)
    stage = np.zeros(H * W * 3, np.uint8)

    def dec(im, name, kind="image"):
        p = tmp_path / name
        im.save(str(p))
        stage[:] = 7
        h, w, ch = fmod.decode(str(p), kind, stage)
        assert (h, w) == (H, W)
        return ch, stage[:h * w * ch].reshape(h, w, ch).copy()

    assert dec(Image.fromarray(rgb), "rgb.png")[0] == 3 and np.array_equal(dec(Image.fromarray(rgb), "rgb.png")[1], rgb)
    ch, a = dec(Image.fromarray(rgb[..., 0]), "grey.png")  # L: one channel staged, the grey tail replicates it
    assert ch == 1 and np.array_equal(a[..., 0], rgb[..., 0])
    alpha = np.full((H, W, 1), 9, np.uint8)
    ch, a = dec(Image.fromarray(np.concatenate([rgb, alpha], 2), "RGBA"), "rgba.png")  # alpha dropped, not blended
    assert ch == 3 and np.array_equal(a, rgb)
    ch, a = dec(Image.fromarray(np.concatenate([rgb[..., :1], alpha], 2), "LA"), "la.png")
    assert ch == 3 and np.array_equal(a, np.repeat(rgb[..., :1], 3, 2))
    pal = Image.fromarray(rgb).quantize(16)
    ch, a = dec(pal, "pal.png")
    assert pal.mode == "P" and ch == 3 and np.array_equal(a, np.asarray(pal.convert("RGB")))
    d16 = depth_plane(2)
    p16 = tmp_path / "d16.png"
    Image.fromarray(d16).save(str(p16))
    with pytest.raises(fmod.FrameStreamError, match="16-bit"):  # a 16-bit file as an image
        fmod.decode(str(p16), "image", stage)
    wide = np.zeros(H * W * 2, np.uint8)
    assert fmod.decode(str(p16), "depth_u16", wide) == (H, W, 1) and np.array_equal(wide.view(np.uint16).reshape(H, W), d16)
    with pytest.raises(fmod.FrameStreamError, match="rgb.png"):  # an 8-bit colour file as a depth image
        fmod.decode(str(tmp_path / "rgb.png"), "depth_u16", wide)
    (tmp_path / "rgb16.png").write_bytes(png_rgb16(H, W))
    with pytest.raises(fmod.FrameStreamError, match="16-bit"):
        fmod.decode(str(tmp_path / "rgb16.png"), "image", stage)


@time_limit
def test_frames_and_depths_stream_side_by_side(fmod, smod, files, tmp_path):
    from PIL import Image
    dpaths = []
    for k in range(len(files)):
        p = tmp_path / ("%010d.png" % k)
        Image.fromarray(depth_plane(k)).save(str(p))
        dpaths.append(str(p))
    s, ring = make(fmod, files, slots=5, workers=2)
    dring = FakeRing(5, H * W * 2)
    d = fmod.FrameStream(dpaths, H, W, slots=5, workers=2, kind="depth_u16", ring=dring)
    with s, d:
        pipe = CheckingPipe(smod)
        pipe.chunk(s, 1, 9, depths=d)
        assert pipe.checked == 8 and d.max_live <= 5 and s.max_live <= 5
        with pytest.raises(IndexError):  # the chunk's last frame went with its last pair
            d[9]
        d.begin(10, 11)
        assert d[10].dtype == np.uint16 and np.array_equal(d[10], depth_plane(10))
    assert not workers_alive()
    odd = tmp_path / "odd.png"
    Image.fromarray(np.zeros((H, W + 1), np.uint16)).save(str(odd))
    d = fmod.FrameStream([dpaths[0], str(odd)], H, W, slots=2, workers=1, kind="depth_u16", ring=FakeRing(2, H * (W + 1) * 2),
                         capacity=H * (W + 1) * 2)
    with d:
        d[0]
        with pytest.raises(fmod.FrameStreamError, match="odd.png"):
            d[1]


def test_ring_entry_points_refuse_null_and_out_of_range_arguments_without_a_device(capi):
    import ctypes as C
    lib = capi.lib()
    h = C.c_void_p()
    for slots, cap in ((0, 64), (-1, 64), (2000, 64), (2, 0)):
        assert lib.dfvo_frame_ring_create(slots, cap, C.byref(h)) == -2 and h.value is None, (slots, cap)
        assert b"dfvo_frame_ring_create" in lib.dfvo_last_error()
    assert lib.dfvo_frame_ring_create(2, 64, None) == -2
    n = C.c_int(5)
    for call, name in ((lambda: lib.dfvo_frame_ring_wait(None, 0), b"dfvo_frame_ring_wait"),
                     (lambda: lib.dfvo_frame_ring_staging(None, 0, C.byref(h), None), b"dfvo_frame_ring_staging"),
                     (lambda: lib.dfvo_frame_ring_submit_raw(None, 0, 8, None), b"dfvo_frame_ring_submit_raw"),
                     (lambda: lib.dfvo_frame_ring_submit_image(None, 0, 2, 2, 3, 0, 0, 2, 0, 2, None, 2, 2), b"dfvo_frame_ring_submit_image"),
                     (lambda: lib.dfvo_frame_ring_pending(None, C.byref(n)), b"dfvo_frame_ring_pending")):
        assert call() == -2
        assert name in lib.dfvo_last_error()
    lib.dfvo_frame_ring_destroy(None)
    assert lib.dfvo_read_image_tail_gray_u8(None, 2, 2, 0, 2, 0, 2, None, 2, 2, None) == -2
    assert b"dfvo_read_image_tail_gray_u8" in lib.dfvo_last_error()


def test_lists_see_no_hook_call(smod):
    """track_chunk over a plain list makes the calls it always made (tests/test_pipeline_depth_source_cpu.py pins the exact
    sequence); an object with only one of the two methods is no stream either"""
    class Half(list):
        def release(self, k):
            raise AssertionError("release without begin")

    pipe = CheckingPipe(smod, expect=lambda k: np.full(2, k))
    frames = Half(np.full(2, k) for k in range(6))
    pipe.chunk(frames, 0, 5)
    assert pipe.checked == 5
