"""Raw camera frames on the device (csrc/undistort.hip, dfvo_undistort_*): bilinear Bayer demosaic and undistortion through a
per-pixel table, what the RobotCar SDK does on the host (sdk_python/image.py load_image, camera_model.py undistort) before the
reference reads the result back as a JPEG.  Here the mosaic is uploaded as it is in the file -- a third of an RGB frame's bytes
-- and everything behind the decoder is exact arithmetic (include/dfvo_hip.h states it).

    umap = UndistortMap.from_lut_file(".../stereo_narrow_left_distortion_lut.bin", 960, 1280)
    frame = mosaic_to_device(np.asarray(Image.open(png)), 192, 640, umap, "gbrg", crop=[[0, 0.8], [0, 1]])

A sequence from disk goes through frame_stream.FrameStream(paths, h, w, mosaic="gbrg", undistort=umap)."""
import ctypes as C

import numpy as np

from . import capi

PATTERNS = ("rggb", "bggr", "grbg", "gbrg")  # DFVO_BAYER_*: the colours of sites (0,0), (0,1), (1,0), (1,1)
BORDERS = ("reflect", "mirror")              # DFVO_BORDER_*


def pattern_code(pattern):
    p = pattern.lower() if isinstance(pattern, str) else pattern
    if p not in PATTERNS:
        raise ValueError("pattern: %r: one of %s" % (pattern, ", ".join(PATTERNS)))
    return PATTERNS.index(p)


def border_code(border):
    if border not in BORDERS:
        raise ValueError("border: %r: one of %s" % (border, ", ".join(BORDERS)))
    return BORDERS.index(border)


def read_lut_file(path, h, w):
    """float64 [2][h * w], x coordinates then y coordinates, of the SDK's <camera>_distortion_lut.bin: CameraModel.__load_lut
    reads the file as float64 [2][n], and undistort's slicing (bilinear_lut[:, 1::-1].T) hands map_coordinates row 1 as the y
    and row 0 as the x coordinate"""
    lut = np.fromfile(str(path), np.float64)
    if lut.size != 2 * h * w:
        raise ValueError("%s: %d values; a table for %d x %d frames has %d" % (path, lut.size, h, w, 2 * h * w))
    return lut.reshape(2, h * w)


class UndistortMap:
    """UndistortMap(h, w, map_xy): the table on the device.  map_xy float64 [2][h * w] (or [2, h, w]): for every pixel of the
    undistorted frame the x, then the y coordinates of its sample in the raw frame.  A non-finite entry raises DfvoError.
    close() frees it -- after the last frame that was submitted with it is complete."""

    def __init__(self, h, w, map_xy):
        capi.require_gpu()
        self.h, self.w = int(h), int(w)
        m = np.ascontiguousarray(np.asarray(map_xy, np.float64).reshape(2, -1))
        if m.shape[1] != self.h * self.w:
            raise ValueError("map_xy: %d samples; %d x %d frames have %d" % (m.shape[1], self.h, self.w, self.h * self.w))
        self.lib = capi.lib()
        handle = C.c_void_p()
        capi.check(self.lib.dfvo_undistort_create(self.h, self.w, capi.as_ptr(m), C.byref(handle)))
        self.handle = handle

    @classmethod
    def from_lut_file(cls, path, h, w):
        return cls(h, w, read_lut_file(path, h, w))

    def close(self):
        if self.handle is not None:
            self.lib.dfvo_undistort_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _box(h, w, crop):
    if crop is None:
        return 0, h, 0, w
    return int(h * crop[0][0]), int(h * crop[0][1]), int(w * crop[1][0]), int(w * crop[1][1])  # utils.py:46-50


def mosaic_to_device(mosaic, h, w, umap, pattern, crop=None, border="reflect"):
    """the resident-frame twin of sequence.image_to_device for a raw frame: mosaic uint8 [img_h, img_w] as decoded ->
    demosaic (+ undistortion when umap is an UndistortMap, None for none) of the crop's pixels -> read_image's crop
    ([[y0, y1], [x0, x1]] fractions) and resize to (h, w).  Returns a device uint8 tensor [h, w, 3] (RGB), drained as
    image_to_device drains its own (the pipeline's ordering contract for frames)."""
    import torch
    m = np.ascontiguousarray(mosaic)
    if m.ndim != 2 or m.dtype != np.uint8:
        raise ValueError("mosaic: %s %s: a uint8 [h, w] plane" % (m.dtype, m.shape))
    ih, iw = m.shape
    y0, y1, x0, x1 = _box(ih, iw, crop)
    lib = capi.lib()
    src = torch.from_numpy(m).cuda()
    rgb = torch.empty((ih, iw, 3), dtype=torch.uint8, device="cuda")
    dst = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    capi.check(lib.dfvo_undistort_mosaic_u8(None if umap is None else umap.handle, src.data_ptr(), ih, iw, pattern_code(pattern),
                                            border_code(border), y0, y1, x0, x1, rgb.data_ptr(), stream.cuda_stream))
    capi.check(lib.dfvo_read_image_tail_u8(rgb.data_ptr(), ih, iw, 0, y0, y1, x0, x1, dst.data_ptr(), h, w, stream.cuda_stream))
    stream.synchronize()
    return dst


def undistort_mosaic(mosaic_dev, umap, pattern, border="reflect", box=None, out=None):
    """dfvo_undistort_mosaic_u8 on device tensors: mosaic uint8 [h, w] -> `out` uint8 [h, w, 3] (allocated when None), only
    inside box (y0, y1, x0, x1); asynchronous on torch's current stream"""
    import torch
    ih, iw = mosaic_dev.shape
    if out is None:
        out = torch.empty((ih, iw, 3), dtype=torch.uint8, device="cuda")
    y0, y1, x0, x1 = (0, ih, 0, iw) if box is None else box
    capi.check(capi.lib().dfvo_undistort_mosaic_u8(None if umap is None else umap.handle, mosaic_dev.data_ptr(), ih, iw,
                                                   pattern_code(pattern), border_code(border), y0, y1, x0, x1, out.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream))
    return out


def undistort_rgb(rgb_dev, umap, box=None, out=None):
    """dfvo_undistort_rgb_u8 on device tensors: a distorted uint8 [h, w, 3] frame of the map's size -> `out`"""
    import torch
    if tuple(rgb_dev.shape) != (umap.h, umap.w, 3):
        raise ValueError("frame %s: the map is for %d x %d x 3" % (tuple(rgb_dev.shape), umap.h, umap.w))
    if out is None:
        out = torch.empty((umap.h, umap.w, 3), dtype=torch.uint8, device="cuda")
    y0, y1, x0, x1 = (0, umap.h, 0, umap.w) if box is None else box
    capi.check(capi.lib().dfvo_undistort_rgb_u8(umap.handle, rgb_dev.data_ptr(), y0, y1, x0, x1, out.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream))
    return out
