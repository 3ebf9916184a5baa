"""CPU: the fp32 Winograd F(2x2,3x3) path without a device -- the fp32 emulation of the algorithm against its float64 bound on
every operator shape of tests/test_wino_gpu.py, the host packer (df-vo_amd/csrc/conv_pack_wino_f32.h) built into a
stand-alone program under the address and undefined-behaviour sanitizers against numpy's float64 G g G^T bit for bit, and
the three C-ABI symbols."""
import os
import subprocess

import numpy as np
import pytest
import torch

import wino_bounds as WB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_switch_is_exported_and_off_by_default(capi):
    lib = capi.lib()
    for n in ("dfvo_set_fp32_winograd", "dfvo_get_fp32_winograd", "dfvo_fp32_winograd_launches"):
        assert hasattr(lib, n)
    if "DFVO_FP32_WINOGRAD" not in os.environ:
        assert lib.dfvo_get_fp32_winograd() == 0
    before = lib.dfvo_get_fp32_winograd()
    try:
        for m in (1, 2, 0):
            capi.check(lib.dfvo_set_fp32_winograd(m))
            assert lib.dfvo_get_fp32_winograd() == m
        assert lib.dfvo_set_fp32_winograd(3) != 0 and lib.dfvo_get_fp32_winograd() == 0
    finally:
        lib.dfvo_set_fp32_winograd(before)


def test_mirror_option_is_passed_through_only_when_given(capi):
    import importlib
    dm = importlib.import_module("df-vo_amd.libs.deep_models.deep_models")
    assert "fp32_winograd" not in dm.hip_options({"dfvo_hip": {"conv_precision": "fp32"}})
    assert dm.hip_options({"dfvo_hip": {"conv_precision": "fp32", "fp32_winograd": True}})["fp32_winograd"] is True


@pytest.mark.parametrize("case", WB.CASES, ids=[c["name"] for c in WB.CASES])
def test_fp32_emulation_is_within_the_bound(case):
    x, w, b, res = WB.case_tensors(case)
    y64, bound = WB.wino_bound(x, w, b, res)
    y = WB.wino_conv_f32(x, w, b)
    if res is not None:
        y = y + res
    err = (y.double() - y64).abs()
    ratio = float((err / bound).max())
    print("WINO-EMU %s: max err / bound %.4f (max |y| %.3e)" % (case["name"], ratio, float(y64.abs().max())))
    assert torch.isfinite(y).all() and ratio <= 1.0
    # the bound is one that a wrong coefficient breaks: one flipped sign of A^T is far outside it
    bad = WB._winograd(x, WB.filter_transform(w.double()).float(), WB.BT, WB.AT.abs()) + b.view(1, -1, 1, 1)
    if res is not None:
        bad = bad + res
    assert float(((bad.double() - y64).abs() / bound).max()) > 100.0


_MAIN = r"""
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "conv_pack_wino_f32.h"
// argv: cout c0 c1 weights.bin out.bin -- packs the OIHW weights of the file, writes the packed floats
int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const int cout = atoi(argv[1]), c0 = atoi(argv[2]), c1 = atoi(argv[3]);
    std::vector<float> w((size_t)cout * (c0 + c1) * 9);
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(w.data(), sizeof(float), w.size(), f) != w.size()) return 3;
    fclose(f);
    std::vector<float> out(conv_wino_f32_floats(cout, c0, c1));  // exactly the size the packer states: a write past it is caught
    conv_pack_wino_f32(w.data(), cout, c0, c1, nullptr, out.data());
    f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) return 4;
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def pack_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("wino_pack")
    src, exe = d / "wino_pack_main.cpp", d / "wino_pack_main"
    src.write_text(_MAIN)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # the runtimes inside the program: nothing depends on load order
                        "-I", os.path.join(ROOT, "df-vo_amd", "csrc"), str(src), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return str(exe)


@pytest.mark.parametrize("cout,c0,c1", [(9, 32, 0), (48, 128, 2), (128, 386, 0)])
def test_packer_under_sanitizers_equals_numpy_float64(pack_program, tmp_path, cout, c0, c1):
    rng = np.random.RandomState(cout * 1000 + c0 + c1)
    cin = c0 + c1
    w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    wf, of = tmp_path / "w.bin", tmp_path / "u.bin"
    w.tofile(str(wf))
    r = subprocess.run([pack_program, str(cout), str(c0), str(c1), str(wf), str(of)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    nch0, nch1, cp = (c0 + 7) // 8, (c1 + 7) // 8, (cout + 31) // 32 * 32
    got = np.fromfile(str(of), dtype=np.float32)
    assert got.size == (nch0 + nch1) * 16 * 8 * cp
    got = got.reshape(nch0 + nch1, 16, 2, cp, 4)
    # numpy float64 G g G^T, rounded to fp32 once
    g64 = w.astype(np.float64)
    Gm = WB.G.numpy()
    t = np.stack([g64[:, :, 0, :], 0.5 * ((g64[:, :, 0, :] + g64[:, :, 1, :]) + g64[:, :, 2, :]),
                  0.5 * ((g64[:, :, 0, :] - g64[:, :, 1, :]) + g64[:, :, 2, :]), g64[:, :, 2, :]], axis=2)   # G g: [o, c, 4, 3]
    U = np.stack([t[..., 0], 0.5 * ((t[..., 0] + t[..., 1]) + t[..., 2]), 0.5 * ((t[..., 0] - t[..., 1]) + t[..., 2]), t[..., 2]], axis=3)
    assert np.allclose(U, Gm @ g64 @ Gm.T, rtol=1e-14, atol=1e-300)    # the same matrix product, whatever the order of its sums
    U32 = U.astype(np.float32).reshape(cout, cin, 16)
    want = np.zeros_like(got)
    for ci in range(cin):
        s1 = ci >= c0
        ch = ci - c0 if s1 else ci
        chunk = (nch0 if s1 else 0) + ch // 8
        want[chunk, :, (ch % 8) // 4, :cout, ch % 4] = U32[:, ci, :].T
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))   # bit for bit, the padding rows (zero in `want`) included
    assert not got[:, :, :, cout:, :].any()
