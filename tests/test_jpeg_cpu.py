"""CPU: the host half of the JPEG decode and its oracles.
  1. tests/jpeg_ref.py (numpy) equals live Pillow and tests/golden/jpeg_cases.npz byte for byte on the whole case matrix;
  2. dfvo_jpeg_entropy_decode through the built library: header and every coefficient equal the restatement's;
  3. refusals by name: progressive, CMYK, files cut short, a capacity one byte too small, a PNG handed in as bytes;
  4. the entropy pass alone (csrc/jpeg_entropy.h) in tests/host_harness/jpeg_entropy_check.cpp under AddressSanitizer and UBSan:
     prefixes and seeded corruptions return a code, touch nothing outside their buffers."""
import ctypes as C
import importlib
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_cases
import jpeg_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "jpeg_entropy_check.cpp")
HDRS = [os.path.join(HERE, "..", "df-vo_amd", "csrc", "jpeg_entropy.h"), os.path.join(HERE, "..", "include", "dfvo_hip.h")]
IDS = [c.name for c in jpeg_cases.CASES]
ERR_JPEG = -7


@pytest.fixture(scope="module")
def jpeg(capi):
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("df-vo_amd.jpeg")


_parsed = {}


def parsed(name):
    """the restatement's parse of a fixture file, once"""
    if name not in _parsed:
        _parsed[name] = jpeg_ref.parse(jpeg_cases.fixture()[name][0])
    return _parsed[name]


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------
def test_the_matrix_is_the_one_the_fixture_holds():
    assert sorted(jpeg_cases.fixture()) == sorted(IDS)
    subs = {(c.sub, c.quality) for c in jpeg_cases.CASES}
    assert subs == {(s, q) for s in jpeg_cases.SUBS for q in jpeg_cases.QUALITIES}
    assert {(c.h, c.w) for c in jpeg_cases.CASES} == set(jpeg_cases.SMALL + jpeg_cases.LARGE)
    assert os.path.getsize(jpeg_cases.FIXTURE) < 600 * 1024


@pytest.mark.parametrize("case", jpeg_cases.CASES, ids=IDS)
def test_restatement_equals_pillow_and_the_fixture(case):
    data, want = jpeg_cases.fixture()[case.name]
    got = jpeg_ref.pixels(parsed(case.name))
    assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(jpeg_cases.pillow_decode(data), want), "the installed Pillow decodes the fixture's file differently"
    live = jpeg_cases.encode(case)  # (the installed Pillow may write other bytes than the fixture's: the restatement follows it)
    assert np.array_equal(jpeg_ref.decode(live), jpeg_cases.pillow_decode(live))


@pytest.mark.parametrize("case", jpeg_cases.RESTART_CASES, ids=[c.name for c in jpeg_cases.RESTART_CASES])
def test_restart_cases_carry_a_dri_marker(case):
    data = jpeg_cases.fixture()[case.name][0]
    p = parsed(case.name)
    mcus_x = p.blocks_w[0] // p.h_samp
    assert b"\xff\xdd\x00\x04" in data and p.dri == (case.rst_blocks or mcus_x * case.rst_rows)
    assert sum(data.count(bytes([0xFF, 0xD0 + i])) for i in range(8)) >= 1 or p.dri >= mcus_x * (p.blocks_h[0] // p.v_samp)


def test_upsampling_reads_the_downsampled_size_not_the_padded_one():
    """the restatement's own seeded check.  An even size whose chroma size is no multiple of 8 (24 x 520: 12 x 260 in a 16 x 264
    grid) ends on a pixel that looks at the chroma sample beyond the last real one: replicating the edge and reading the
    padding give different pixels there.  (At an odd size the last pixel looks the other way, and nothing shows.)"""
    p = parsed("24x520-420-q100")
    plane = jpeg_ref.idct_plane(p.coeffs[1], p.quant[1], p.blocks_h[1], p.blocks_w[1])
    own = jpeg_ref.upsample(plane[:p.comp_h[1], :p.comp_w[1]], 2, 2)[:24, :520]
    padded = jpeg_ref.upsample(plane, 2, 2)[:24, :520]
    assert not np.array_equal(own[:, -1], padded[:, -1]) and not np.array_equal(own[-1], padded[-1])
    assert np.array_equal(own[:-1, :-1], padded[:-1, :-1])


# ---- 2. the entropy pass through the library ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", jpeg_cases.CASES, ids=IDS)
def test_entropy_decode_equals_the_restatement(jpeg, case):
    data = jpeg_cases.fixture()[case.name][0]
    p = parsed(case.name)
    info, buf, coeffs = jpeg.entropy_decode(data)
    assert (info.width, info.height, info.components, info.h_samp, info.v_samp) == (p.width, p.height, p.components, p.h_samp, p.v_samp)
    n = p.components
    for field in ("blocks_w", "blocks_h", "comp_w", "comp_h", "plane_offset"):
        assert list(getattr(info, field))[:n] == getattr(p, field), field
    assert info.bytes == p.bytes == buf.size
    for c in range(n):
        assert np.array_equal(np.array(info.quant[c]), p.quant[c])
        assert coeffs[c].dtype == np.int16 and np.array_equal(coeffs[c].reshape(-1, 64), p.coeffs[c]), "component %d" % c
    head = jpeg.probe(data)
    assert bytes(head) == bytes(info) and bytes(buf[:C.sizeof(info)]) == bytes(info)


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------
def saved(img, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, **kw) if isinstance(img, np.ndarray) else img.save(b, **kw)
    return b.getvalue()


def refused(jpeg, data, reason, capacity=None, header=True):
    """header: the reason is one the header alone shows, so dfvo_jpeg_probe refuses too"""
    if capacity is not None:
        with pytest.raises(jpeg.JpegError, match=reason):
            jpeg.entropy_decode_into(np.frombuffer(data, np.uint8), np.zeros(capacity, np.uint8))
        return
    if header:
        with pytest.raises(jpeg.JpegError, match=reason):
            jpeg.probe(data)
    with pytest.raises(jpeg.JpegError, match=reason):
        jpeg.entropy_decode_into(np.frombuffer(data, np.uint8), np.zeros(1 << 16, np.uint8))


def test_refusals_name_their_reason(jpeg, capi):
    from PIL import Image
    case = jpeg_cases.CASES[IDS.index("37x53-420-q50")]
    img = jpeg_cases.make_image(case)
    refused(jpeg, saved(img, format="JPEG", progressive=True), "progressive")
    refused(jpeg, saved(Image.fromarray(img).convert("CMYK"), format="JPEG"), "four components")
    refused(jpeg, saved(img, format="PNG"), "not a JPEG")
    refused(jpeg, b"", "not a JPEG")
    data = jpeg_cases.fixture()[case.name][0]
    need = int(jpeg.probe(data).bytes)
    refused(jpeg, data, "capacity too small", capacity=need - 1)
    jpeg.entropy_decode_into(np.frombuffer(data, np.uint8), np.zeros(need, np.uint8))
    sos = data.index(b"\xff\xda")
    for n in (1, 2, 3, 20, sos, sos + 5, sos + 14, (sos + len(data)) // 2, len(data) - 3, len(data) - 2, len(data) - 1):
        with pytest.raises(jpeg.JpegError, match="data ends early|not a JPEG"):
            jpeg.entropy_decode_into(np.frombuffer(data[:n], np.uint8), np.zeros(need, np.uint8))
    assert capi.lib().dfvo_jpeg_probe(None, 10, C.byref(capi.JpegInfo())) == ERR_JPEG
    assert capi.lib().dfvo_jpeg_probe(capi.as_ptr(np.frombuffer(data, np.uint8)), len(data), None) == ERR_JPEG


def patched(data, marker, offset, value):
    i = data.index(marker)
    return data[:i + offset] + bytes([value]) + data[i + offset + 1:]


def test_refusals_of_patched_headers(jpeg):
    """what Pillow cannot write: the marker or field is patched into a valid file"""
    data = jpeg_cases.fixture()["37x53-420-q50"][0]
    refused(jpeg, patched(data, b"\xff\xc0", 1, 0xC9), "arithmetic coding")
    refused(jpeg, patched(data, b"\xff\xc0", 1, 0xC1), "only baseline sequential")
    refused(jpeg, patched(data, b"\xff\xc0", 4, 12), "12-bit samples")
    refused(jpeg, patched(data, b"\xff\xc0", 11, 0x41), "sampling")
    refused(jpeg, patched(data, b"\xff\xc0", 11, 0x12), "sampling")
    refused(jpeg, patched(data, b"\xff\xdb", 4, 0x10), "16-bit quantisation tables")
    refused(jpeg, patched(data, b"\xff\xc0", 12, 3), "missing table")
    refused(jpeg, patched(data, b"\xff\xda", 6, 0x33), "missing table", header=False)
    refused(jpeg, patched(data, b"\xff\xda", 4, 1), "more than one scan")
    rst = jpeg_cases.fixture()["37x53-420-q50-rst1"][0]
    i = rst.index(b"\xff\xd1")
    refused(jpeg, rst[:i + 1] + b"\xd5" + rst[i + 2:], "bad restart marker", header=False)


def test_device_entry_points_check_their_arguments_before_the_device(capi):
    lib = capi.lib()
    assert lib.dfvo_frame_ring_submit_jpeg(None, 0, 0, 1, 0, 1, None, 1, 1) == -2 and b"dfvo_frame_ring_submit_jpeg: null ring" in lib.dfvo_last_error()
    assert lib.dfvo_jpeg_decode_u8(None, C.byref(capi.JpegInfo()), None, None) == -2 and b"dfvo_jpeg_decode_u8" in lib.dfvo_last_error()
    assert C.sizeof(capi.JpegInfo) == 488 <= capi.JPEG_HEADER_BYTES


def test_stream_refuses_jpeg_device_with_a_mosaic_or_a_depth_stream(capi):
    fs = importlib.import_module("df-vo_amd.frame_stream")
    for kw in (dict(mosaic="gbrg"), dict(kind="depth_u16")):
        with pytest.raises(ValueError, match="jpeg"):
            fs.FrameStream(["a.jpg"], 8, 8, jpeg="device", **kw)
    with pytest.raises(ValueError, match="jpeg"):
        fs.FrameStream(["a.jpg"], 8, 8, jpeg="gpu")
    assert fs.jpeg_capacity(376, 1241) == 512 + 6 * 384 * 1248


# ---- 4. the sanitized harness -------------------------------------------------------------------------------------------------
HARNESS_CASES = ["1x1-420-q50", "17x23-420-q50", "33x15-422-q92-rst3", "17x23-grey-q50-rst1", "16x16-444-q100", "37x53-422-q92-opt"]


@pytest.fixture(scope="module")
def checker():
    out_dir = os.path.join(HERE, "host_harness", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "jpeg_entropy_check")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    return exe


def test_entropy_pass_on_prefixes_and_corruptions_under_sanitizers(checker, tmp_path):
    paths = []
    for name in HARNESS_CASES:
        paths.append(str(tmp_path / (name + ".jpg")))
        with open(paths[-1], "wb") as f:
            f.write(jpeg_cases.fixture()[name][0])
    r = subprocess.run([checker] + paths, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.strip().endswith("jpeg_entropy_check: ok") and r.stdout.count("corruptions") == len(HARNESS_CASES)
