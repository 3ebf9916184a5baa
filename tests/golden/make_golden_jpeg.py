"""Regenerates tests/golden/jpeg_cases.npz, byte for byte with the Pillow, zlib and numpy it was made with (Pillow 12.2.0,
libjpeg-turbo 3.1): every case of tests/jpeg_cases.py as the JPEG file Pillow writes and the pixels Pillow decodes from it.

    python tests/golden/make_golden_jpeg.py [--check]

The archive is written member by member with a fixed timestamp (numpy's savez stamps the time of day).  Members: meta (JSON:
name, offsets, shape per case), jpg (all files, concatenated), px (all decoded frames, concatenated)."""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cases  # noqa: E402


def build():
    meta, jpg, px = [], [], []
    j0 = p0 = 0
    for c in jpeg_cases.CASES:
        data = jpeg_cases.encode(c)
        pix = jpeg_cases.pillow_decode(data)
        assert pix.shape[:2] == (c.h, c.w)
        meta.append({"name": c.name, "jpg0": j0, "jpg_n": len(data), "px0": p0, "shape": list(pix.shape)})
        jpg.append(np.frombuffer(data, np.uint8))
        px.append(pix.reshape(-1))
        j0 += len(data)
        p0 += pix.size
    arrays = {"meta": np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8), "jpg": np.concatenate(jpg),
              "px": np.concatenate(px)}
    out = io.BytesIO()
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in ("meta", "jpg", "px"):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[name]), version=(1, 0))
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue(), compresslevel=9)
    return out.getvalue()


if __name__ == "__main__":
    blob = build()
    if "--check" in sys.argv:
        same = open(jpeg_cases.FIXTURE, "rb").read() == blob
        print("identical" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
    with open(jpeg_cases.FIXTURE, "wb") as f:
        f.write(blob)
    print("%s: %d cases, %d bytes" % (jpeg_cases.FIXTURE, len(jpeg_cases.CASES), len(blob)))
