"""Baseline JPEG frames decoded on the device (csrc/jpeg_entropy.h, csrc/jpeg.hip; include/dfvo_hip.h, dfvo_jpeg_*): the
bit-serial Huffman pass on the host, dequantisation, IDCT, chroma upsampling and YCbCr -> RGB on the device, with the arithmetic
of Pillow's decoder (libjpeg-turbo's default path) restated exactly -- the pixels are Pillow's byte for byte for files a
conforming encoder wrote (docs/parity.md).  Parity with OpenCV's decoder is not established.

probe / entropy_decode need no device.  A refused or corrupt file raises JpegError, whose message names the reason."""
import ctypes as C

import numpy as np

from . import capi


class JpegError(ValueError):
    """a JPEG that is refused (progressive, CMYK, ...) or corrupt; the message names the reason"""


def is_jpeg(data):
    return len(data) >= 2 and data[0] == 0xFF and data[1] == 0xD8


def _bytes(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview, np.ndarray)):
        return np.frombuffer(bytes(path_or_bytes), np.uint8)
    with open(path_or_bytes, "rb") as f:
        return np.frombuffer(f.read(), np.uint8)


def _check(rc):
    if rc == capi.ERR_JPEG:
        raise JpegError(capi.lib().dfvo_last_error().decode())
    capi.check(rc)


def probe(data):
    """the capi.JpegInfo header of the file's bytes (size, components, sampling, block grids, .bytes of the staged buffer)"""
    a = _bytes(data)
    info = capi.JpegInfo()
    _check(capi.lib().dfvo_jpeg_probe(capi.as_ptr(a), a.size, C.byref(info)))
    return info


def entropy_decode_into(data, dst):
    """the host pass of the file's bytes (a uint8 array) into the flat uint8 array `dst`, which may be pinned staging memory;
    the header.  The C call runs without the GIL."""
    info = capi.JpegInfo()
    _check(capi.lib().dfvo_jpeg_entropy_decode(capi.as_ptr(data), data.size, dst.ctypes.data_as(C.c_void_p), dst.size, C.byref(info)))
    return info


def entropy_decode(data):
    """(info, buffer, coeffs): the header, the whole staged buffer (uint8, the header at byte 0) and per component the quantised
    coefficients as an int16 view [blocks_h, blocks_w, 64] of it, natural order"""
    a = _bytes(data)
    buf = np.zeros(int(probe(a).bytes), np.uint8)
    info = entropy_decode_into(a, buf)
    coeffs = []
    for c in range(info.components):
        n = info.blocks_h[c] * info.blocks_w[c]
        coeffs.append(buf[info.plane_offset[c]:info.plane_offset[c] + n * 128].view(np.int16).reshape(info.blocks_h[c], info.blocks_w[c], 64))
    return info, buf, coeffs


def decode_to_device(path_or_bytes):
    """the file's pixels as a device uint8 tensor, [h, w, 3] RGB or [h, w] for a one-component file (dfvo_jpeg_decode_u8 on
    torch's current stream, drained)"""
    import torch
    capi.require_gpu()
    info, buf, _ = entropy_decode(path_or_bytes)
    d_buf = torch.from_numpy(buf).cuda()
    shape = (info.height, info.width) if info.components == 1 else (info.height, info.width, 3)
    dst = torch.empty(shape, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    capi.check(capi.lib().dfvo_jpeg_decode_u8(d_buf.data_ptr(), C.byref(info), dst.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    return dst


def jpeg_to_device(path_or_bytes, h, w, crop=None):
    """sequence.image_to_device for a JPEG file that is decoded on the device: read_image's crop and resize of the decoded frame
    as the device uint8 tensor [h, w, 3], complete on return (the same ordering contract)"""
    import torch
    img = decode_to_device(path_or_bytes)
    ih, iw = img.shape[:2]
    y0, y1, x0, x1 = 0, ih, 0, iw
    if crop is not None:
        y0, y1 = int(ih * crop[0][0]), int(ih * crop[0][1])
        x0, x1 = int(iw * crop[1][0]), int(iw * crop[1][1])
    dst = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    lib = capi.lib()
    if img.ndim == 2:
        capi.check(lib.dfvo_read_image_tail_gray_u8(img.data_ptr(), ih, iw, y0, y1, x0, x1, dst.data_ptr(), h, w, stream.cuda_stream))
    else:
        capi.check(lib.dfvo_read_image_tail_u8(img.data_ptr(), ih, iw, 0, y0, y1, x0, x1, dst.data_ptr(), h, w, stream.cuda_stream))
    stream.synchronize()
    return dst
