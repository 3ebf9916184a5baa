"""Frames of a sequence from files on disk, as the `frames` / `depths` object of sequence.track_chunk: decoded by worker
threads into the pinned staging slots of a device frame ring (csrc/frame_ring.hip), uploaded and run through the read-image
tail on the ring's own stream, handed out as device tensors under the pipeline's frame contract.  Device memory is bounded by
`slots` whatever the length of the sequence; decoding runs beside tracking.

    with FrameStream(paths, H, W) as frames:
        traj, rows = sequence.run_sequence(pipe, frames, len(frames))   # (run_sequence ends with pipe.sync())

Threads: the worker threads touch nothing but the file and the staging memory of the slot they were given; every ring call
(submit, wait, destroy) is made by the thread that indexes the stream -- the one that drives the pipeline.

Window: track_chunk announces a chunk with begin(lo, hi) (prefetch restarts at frame lo) and calls release(k) once the
track_end of the last pair that names frame k has returned -- the pipeline's own lifetime rule for device frames; only then is
the frame's slot decoded into again.  Frames lo .. hi are requested in non-decreasing order, at most ahead + 2 of them live
at once, so `slots` >= ahead + 2 (sequence.track_chunk checks); with exactly that many the stream decodes on demand.
slots defaults to 12, not 8: with four hardware queues the ring's stream shares a queue with one of the pipeline's, an upload
runs behind the net passes that stream was given before it, and only an upload enqueued four pairs before its frame is fed
is complete by then without the host waiting -- 5 live frames + 3 ahead is the edge (measured, profiles/stream_rates.json:
8 slots 0.80 x the resident rate with 2.3 ms of event wait per frame, 12 slots 0.97 x with 0.06 ms).

Decoding follows what cv2.imread(path) + cvtColor(BGR2RGB) hand read_image (libs/general/utils.py:44-51): mode RGB as it is,
L through the grey tail (dfvo_read_image_tail_gray_u8: a third of the upload), P / RGBA / LA through convert("RGB") (alpha
dropped); 16-bit images are refused by name.  PNG is lossless, so the frames are exactly read_image's.  JPEG: Pillow and OpenCV
both decode with libjpeg, but of versions and IDCT / upsampling settings this project does not pin -- parity of JPEG frames
with the reference's (OpenCV's decoder) is NOT established.

jpeg="device" (default "host": everything above, untouched): a worker reads the file's bytes; bytes that start with FF D8 go
through the host entropy pass (dfvo_jpeg_entropy_decode, without the GIL) straight into the staging slot -- a header and the
quantised coefficients, up to 6 bytes per pixel -- and the ring dequantises, inverts the DCT, upsamples and converts the colours
on the device (dfvo_frame_ring_submit_jpeg, csrc/jpeg.hip) ahead of the same read-image tail.  That arithmetic is pinned: it is
Pillow's (libjpeg-turbo: 13-bit slow-integer IDCT, triangle upsampling, 16-bit colour tables) byte for byte for files a
conforming encoder wrote, so the frames are those of jpeg="host" (docs/parity.md); it is pinned to that decoder and to nothing
else.  Baseline sequential 8-bit files of one or three components (4:4:4, 4:2:2, 4:2:0) are decoded; a progressive, CMYK,
otherwise refused or corrupt JPEG raises FrameStreamError naming the file and the reason.  Any other file goes through Pillow as
above, and a sequence may mix both.

Raw frames (mosaic="gbrg", undistort=UndistortMap or None, border): a mode-L file is then an 8-bit Bayer mosaic, staged and
uploaded as it is; the ring demosaics and undistorts the crop's pixels on the device (dfvo_frame_ring_submit_mosaic, undistort.py)
ahead of the same read-image tail.  Any other mode is refused by name: a mosaic has one channel."""
import ctypes as C
import operator
import threading
import time

import numpy as np

from . import capi

MAX_WORKERS = 16  # `workers` is a plain argument capped here, never derived from the machine's core count (4 carry the pair rate)
KINDS = ("image", "depth_u16")
JPEG_MODES = ("host", "device")


class FrameStreamError(RuntimeError):
    """a frame that could not be read; names the file"""


class FrameRing:
    """dfvo_frame_ring_* (include/dfvo_hip.h).  Every method but staging()'s returned view is for the consumer thread."""

    def __init__(self, slots, capacity):
        import torch
        capi.require_gpu()
        self._torch = torch
        self.lib = capi.lib()
        self.slots, self.capacity = int(slots), int(capacity)
        h = C.c_void_p()
        capi.check(self.lib.dfvo_frame_ring_create(self.slots, self.capacity, C.byref(h)))
        self.h = h
        self._views = []
        for s in range(self.slots):
            p, cap = C.c_void_p(), C.c_size_t()
            capi.check(self.lib.dfvo_frame_ring_staging(self.h, s, C.byref(p), C.byref(cap)))
            self._views.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(int(cap.value),)))

    def staging(self, slot):
        """the slot's pinned staging memory as a flat uint8 array"""
        return self._views[slot]

    def new_output(self, shape, dtype):
        return self._torch.empty(tuple(shape), dtype=getattr(self._torch, dtype), device="cuda")

    def submit_image(self, slot, h, w, channels, box, out):
        capi.check(self.lib.dfvo_frame_ring_submit_image(self.h, slot, h, w, channels, 0, box[0], box[1], box[2], box[3],
                                                         C.c_void_p(out.data_ptr()), out.shape[0], out.shape[1]))

    def submit_mosaic(self, slot, umap, pattern, border, h, w, box, out):
        from . import undistort as ud
        capi.check(self.lib.dfvo_frame_ring_submit_mosaic(self.h, slot, None if umap is None else umap.handle, ud.pattern_code(pattern),
                                                          ud.border_code(border), h, w, box[0], box[1], box[2], box[3],
                                                          C.c_void_p(out.data_ptr()), out.shape[0], out.shape[1]))

    def submit_jpeg(self, slot, box, out):
        capi.check(self.lib.dfvo_frame_ring_submit_jpeg(self.h, slot, box[0], box[1], box[2], box[3], C.c_void_p(out.data_ptr()),
                                                        out.shape[0], out.shape[1]))

    def submit_raw(self, slot, nbytes, out):
        capi.check(self.lib.dfvo_frame_ring_submit_raw(self.h, slot, nbytes, C.c_void_p(out.data_ptr())))

    def wait(self, slot):
        capi.check(self.lib.dfvo_frame_ring_wait(self.h, slot))

    def pending(self):
        n = C.c_int(0)
        capi.check(self.lib.dfvo_frame_ring_pending(self.h, C.byref(n)))
        return int(n.value)

    def close(self):
        if self.h is not None:
            self._views = []
            self.lib.dfvo_frame_ring_destroy(self.h)  # (synchronises the ring's stream first)
            self.h = None


def _png_rawmode(im):
    tile = getattr(im, "tile", None) or []
    args = tile[0][3] if tile and len(tile[0]) > 3 else None
    if isinstance(args, (tuple, list)):
        args = args[0] if args else None
    return args if isinstance(args, str) else ""


def probe(path):
    """(h, w, bytes per pixel as decode() stages it) from the file's header"""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
        per = 1 if im.mode == "L" else (2 if im.mode.startswith("I") else 3)
    return h, w, per


def decode(path, kind, staging, mosaic=False):
    """decode `path` into the flat uint8 array `staging`; (h, w, channels).  Raises FrameStreamError naming the path.
    mosaic: the file is a raw 8-bit Bayer frame -- mode L, or refused."""
    from PIL import Image
    try:
        with Image.open(path) as im:
            w, h = im.size
            if kind == "depth_u16":
                if im.mode not in ("I;16", "I;16L", "I;16B", "I;16N", "I"):
                    raise ValueError("mode %s: a depth image is a 1-channel 16-bit file" % im.mode)
                a = np.asarray(im)
                if a.dtype != np.uint16:
                    if a.min() < 0 or a.max() > 65535:
                        raise ValueError("values outside uint16")
                    a = a.astype(np.uint16)
                ch = 1
            else:
                if im.mode.startswith("I") or im.mode == "F" or ";16" in _png_rawmode(im):
                    raise ValueError("mode %s (%s): 16-bit images are not read (cv2.imread would scale them to 8 bits)"
                                     % (im.mode, _png_rawmode(im) or "16-bit"))
                if mosaic and im.mode != "L":
                    raise ValueError("mode %s: a Bayer mosaic is a 1-channel 8-bit file (mode L)" % im.mode)
                if im.mode in ("P", "RGBA", "LA"):
                    im = im.convert("RGB")
                elif im.mode not in ("RGB", "L"):
                    raise ValueError("mode %s: not read (RGB, L, P, RGBA, LA are)" % im.mode)
                a = np.asarray(im)
                ch = 1 if a.ndim == 2 else 3
            if a.shape[:2] != (h, w) or a.dtype not in (np.uint8, np.uint16):
                raise ValueError("decoded to %s %s" % (a.dtype, a.shape))
            if a.nbytes > staging.size:
                raise ValueError("%d x %d x %d bytes: larger than the staging capacity of %d bytes" % (h, w, a.nbytes // (h * w), staging.size))
            np.copyto(staging[:a.nbytes].view(a.dtype).reshape(a.shape), a)
            return h, w, ch
    except Exception as e:  # (Pillow raises OSError, SyntaxError, ValueError ... for broken files)
        raise FrameStreamError("%s: %s: %s" % (path, type(e).__name__, e)) from e


def jpeg_capacity(h, w):
    """staging bytes that hold any decodable JPEG of h x w: the header and 2 bytes per sample of three full-size planes padded
    to whole MCUs"""
    return capi.JPEG_HEADER_BYTES + 6 * (-(-h // 16) * 16) * (-(-w // 16) * 16)


def decode_any(path, staging):
    """jpeg="device": a file that starts with FF D8 through the host entropy pass into `staging`, (h, w, channels, True); any
    other file through decode(), (h, w, channels, False).  Raises FrameStreamError naming the path (and the reason)."""
    from . import jpeg
    try:
        with open(path, "rb") as f:
            head = f.read(2)
            data = np.frombuffer(head + f.read(), np.uint8) if jpeg.is_jpeg(head) else None
        if data is not None:
            info = jpeg.entropy_decode_into(data, staging)
            return info.height, info.width, (1 if info.components == 1 else 3), True
    except Exception as e:
        raise FrameStreamError("%s: %s: %s" % (path, type(e).__name__, e)) from e
    return decode(path, "image", staging) + (False,)


class _Entry:
    __slots__ = ("slot", "state", "meta", "error", "dropped")

    def __init__(self, slot):
        self.slot, self.state, self.meta, self.error, self.dropped = slot, "decoding", None, None, False


class FrameStream:
    """FrameStream(paths, out_h, out_w, crop=None, slots=12, workers=6, kind="image", jpeg="host"): indexable by frame number.
    kind "image": frames[k] is the device uint8 tensor [out_h, out_w, 3] of read_image(paths[k], out_h, out_w, crop)
    (crop: [[y0, y1], [x0, x1]] fractions); kind "depth_u16": the device uint16 tensor [out_h, out_w] of the 16-bit depth image as
    it is in the file (out_h, out_w: the files' own size, TrackingPipeline's depth_size; the division and the resize are the
    pipeline's).  A tensor handed out is valid until release() of its frame, begin() or close().
    A file that is missing, corrupt, of a refused mode or larger than the staging capacity raises FrameStreamError at the
    __getitem__ of its frame; frames before it are not affected.
    mosaic ("rggb", "bggr", "grbg" or "gbrg"; kind "image"): the files are 8-bit Bayer mosaics of that pattern -- mode L, any
    other mode raises FrameStreamError at its frame; frames[k] is then read_image's crop and resize of the demosaiced frame,
    undistorted through `undistort` (an undistort.UndistortMap of the files' size, which the caller closes after the stream; None:
    demosaic only), the mosaic extended over the border by `border` ("reflect" or "mirror"; include/dfvo_hip.h).  Without
    `mosaic` an L file is a grey frame and nothing changes.
    jpeg "device" (kind "image", no mosaic): JPEG files are entropy-decoded by the workers and decoded on the device, to the
    frames jpeg="host" gives (module docstring); a refused or corrupt JPEG raises FrameStreamError with the reason at its frame.
    capacity: bytes per staging slot (default: the first readable file's decoded size; under jpeg="device" what any decodable
    JPEG of that size needs, jpeg_capacity).  ring: the ring object (tests).
    close() stops and joins the workers and destroys the ring; call it after pipe.sync() (the pipeline may still read the
    frames it was handed), or use the stream as a context manager around run_sequence, which ends with pipe.sync()."""

    def __init__(self, paths, out_h, out_w, crop=None, slots=12, workers=6, kind="image", capacity=None, ring=None,
                 mosaic=None, undistort=None, border="reflect", jpeg="host"):
        if kind not in KINDS:
            raise ValueError("kind: %r: one of %s" % (kind, ", ".join(KINDS)))
        if jpeg not in JPEG_MODES:
            raise ValueError("jpeg: %r: one of %s" % (jpeg, ", ".join(JPEG_MODES)))
        if jpeg == "device" and (mosaic is not None or kind != "image"):
            raise ValueError("jpeg=\"device\": for an image stream without mosaic= (a raw Bayer frame or a 16-bit depth image is no JPEG)")
        self.jpeg = jpeg
        if not (isinstance(workers, int) and 1 <= workers <= MAX_WORKERS):
            raise ValueError("workers: %r: 1 .. %d" % (workers, MAX_WORKERS))
        if not (isinstance(slots, int) and slots >= 1):
            raise ValueError("slots: %r: at least 1" % (slots,))
        if crop is not None and kind != "image":
            raise ValueError("crop: read_image's, not for kind %s" % kind)
        if mosaic is None:
            if undistort is not None or border != "reflect":
                raise ValueError("undistort / border: arguments of a mosaic stream (mosaic=<pattern>)")
        else:
            from . import undistort as ud
            if kind != "image":
                raise ValueError("mosaic: an image stream's, not for kind %s" % kind)
            mosaic = ud.PATTERNS[ud.pattern_code(mosaic)]
            ud.border_code(border)
        self.mosaic, self.undistort, self.border = mosaic, undistort, border
        self.paths = [str(p) for p in paths]
        self.out_h, self.out_w, self.crop, self.kind, self.slots = int(out_h), int(out_w), crop, kind, slots
        if capacity is None:
            capacity = self._probe_capacity()
        self._ring = FrameRing(slots, capacity) if ring is None else ring
        shape, dtype = ((self.out_h, self.out_w, 3), "uint8") if kind == "image" else ((self.out_h, self.out_w), "uint16")
        self._out = [self._ring.new_output(shape, dtype) for _ in range(slots)]
        self._cv = threading.Condition()
        self._entries = {}
        self._free = list(range(slots))
        self._low, self._next, self._end = 0, 0, -1  # window: frames _low .. _end, _next the first not yet given to a worker
        self._started = self._stop = self._closed = False
        self._decoding = self._pending_at_close = 0
        self.max_live = 0  # most slots ever held at once
        self.wait_decode_s = self.wait_device_s = 0.0  # consumer time spent waiting for a decode / for a slot's event
        self._threads = [threading.Thread(target=self._work, name="dfvo-frame-stream-%d" % i, daemon=True) for i in range(workers)]
        for t in self._threads:
            t.start()

    def _probe_capacity(self):
        if self.kind == "depth_u16":
            return self.out_h * self.out_w * 2
        for p in self.paths[:8]:
            try:
                if self.jpeg == "device":  # (dfvo_jpeg_probe for a JPEG; a sequence may mix samplings and PNG files of that size)
                    from . import jpeg
                    with open(p, "rb") as f:
                        data = f.read()
                    if jpeg.is_jpeg(data):
                        info = jpeg.probe(data)
                        h, w = info.height, info.width
                    else:
                        h, w, _ = probe(p)
                    return max(jpeg_capacity(h, w), h * w * 3)
                h, w, per = probe(p)
                return h * w * (1 if self.mosaic else max(per, 3))
            except Exception:
                continue
        return self.out_h * self.out_w * (1 if self.mosaic else 3)

    def __len__(self):
        return len(self.paths)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # ---- workers ---------------------------------------------------------------------------------------------------
    def _work(self):
        while True:
            with self._cv:
                while not self._stop and not (self._free and self._next <= self._end):
                    self._cv.wait()
                if self._stop:
                    return
                k = self._next
                self._next += 1
                e = self._entries[k] = _Entry(self._free.pop())
                self._decoding += 1
                self.max_live = max(self.max_live, self.slots - len(self._free))
            meta = error = None
            try:
                if self.jpeg == "device":
                    meta = decode_any(self.paths[k], self._ring.staging(e.slot))
                else:
                    meta = decode(self.paths[k], self.kind, self._ring.staging(e.slot), mosaic=self.mosaic is not None)
                if self.kind == "depth_u16" and meta[:2] != (self.out_h, self.out_w):
                    raise FrameStreamError("%s: %d x %d: the stream's depth images are %d x %d" % ((self.paths[k],) + meta[:2] + (self.out_h, self.out_w)))
            except BaseException as ex:
                error = ex
            with self._cv:
                self._decoding -= 1
                e.meta, e.error = meta, error
                e.state = "decoded" if error is None else "error"
                if error is not None or e.dropped:  # nothing of it will be read: its slot decodes the next frame
                    self._free.append(e.slot)
                    e.slot = None
                    if e.dropped:
                        self._entries.pop(k, None)
                self._cv.notify_all()

    # ---- the consumer ----------------------------------------------------------------------------------------------
    def begin(self, lo, hi):
        """frames lo .. hi are about to be read in non-decreasing order: drop what is held and restart prefetch at lo"""
        self._check_open()
        lo, hi = int(lo), min(int(hi), len(self.paths) - 1)
        with self._cv:
            self._end = -1  # no new decode starts
            while self._decoding:
                self._cv.wait()
            entries, self._entries = self._entries, {}
        for e in entries.values():
            if e.state == "submitted":
                self._ring.wait(e.slot)
        with self._cv:
            self._free = list(range(self.slots))
            self._low = self._next = lo
            self._end = hi
            self._started = True
            self._cv.notify_all()

    def release(self, k):
        """frames up to and including k are not read again (by the caller or the device): their slots are decoded into again"""
        if self._closed:
            return
        k = int(k)
        self._pump()
        with self._cv:
            done = [f for f in self._entries if f <= k]
            waits = []
            for f in done:
                e = self._entries[f]
                if e.state == "decoding":
                    e.dropped = True  # the worker frees the slot when it leaves it
                    continue
                del self._entries[f]
                if e.slot is not None:
                    if e.state == "submitted":
                        waits.append(e.slot)
                    else:
                        self._free.append(e.slot)
        for s in waits:  # (a frame that was uploaded but never asked for)
            self._ring.wait(s)
        with self._cv:
            self._free.extend(waits)
            self._low = max(self._low, k + 1)
            self._next = max(self._next, self._low)
            self._cv.notify_all()

    def pending(self):
        """slots submitted to the ring and not waited for (after close(): what close() left, 0)"""
        return self._pending_at_close if self._closed else self._ring.pending()

    def _check_open(self):
        if self._closed:
            raise RuntimeError("FrameStream is closed")

    def _submit(self, e):
        out = self._out[e.slot]
        h, w, ch = e.meta[:3]
        if self.kind == "image":
            box = (0, h, 0, w)
            if self.crop is not None:  # utils.py:46-50
                box = (int(h * self.crop[0][0]), int(h * self.crop[0][1]), int(w * self.crop[1][0]), int(w * self.crop[1][1]))
            if len(e.meta) > 3 and e.meta[3]:
                self._ring.submit_jpeg(e.slot, box, out)
            elif self.mosaic is not None:
                self._ring.submit_mosaic(e.slot, self.undistort, self.mosaic, self.border, h, w, box, out)
            else:
                self._ring.submit_image(e.slot, h, w, ch, box, out)
        else:
            self._ring.submit_raw(e.slot, h * w * 2, out)
        e.state = "submitted"

    def _pump(self):
        """submit every frame that is decoded: an upload shares a hardware queue with one of the pipeline's streams and runs
        behind what that stream was given before it, so it is enqueued as early as the consumer thread can"""
        with self._cv:
            ready = sorted(((f, x) for f, x in self._entries.items() if x.state == "decoded"), key=lambda t: t[0])
        for _, x in ready:
            self._submit(x)

    def __getitem__(self, k):
        self._check_open()
        k = operator.index(k)
        if not 0 <= k < len(self.paths):
            raise IndexError("frame %d of %d" % (k, len(self.paths)))
        if not self._started:
            self.begin(k, len(self.paths) - 1)
        self._pump()
        t0 = time.perf_counter()
        with self._cv:
            if k < self._low:
                raise IndexError("frame %d was released (the window starts at frame %d)" % (k, self._low))
            if k > self._end:
                raise IndexError("frame %d is beyond the chunk announced by begin (frames %d .. %d)" % (k, self._low, self._end))
            while True:
                e = self._entries.get(k)
                if e is not None and e.state != "decoding":
                    break
                if e is None and not self._free and not self._decoding:  # only release() could free a slot: no deadlock
                    raise RuntimeError("frame %d needs a slot, but frames %d .. %d hold all %d: release() them or use more slots"
                                       % (k, self._low, self._next - 1, self.slots))
                self._cv.wait()
        t1 = time.perf_counter()
        self.wait_decode_s += t1 - t0
        if e.state == "error":
            raise e.error
        self._pump()
        if e.state == "submitted":
            self._ring.wait(e.slot)
            e.state = "ready"
            self.wait_device_s += time.perf_counter() - t1
        return self._out[e.slot]

    def close(self):
        """stop and join the workers, destroy the ring (after pipe.sync(): the pipeline may still read frames it was handed)"""
        if self._closed:
            return
        self._closed = True
        with self._cv:
            self._stop = True
            self._cv.notify_all()
        for t in self._threads:
            t.join()
        self._threads = []
        entries, self._entries = self._entries, {}
        try:
            for e in entries.values():  # no slot stays pending
                if e.state == "submitted":
                    self._ring.wait(e.slot)
            self._pending_at_close = self._ring.pending()
        finally:
            self._ring.close()
        self._out = []
