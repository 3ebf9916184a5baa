"""The f16 range edge, end to end.

Under the f16x3 / f16 packings every conv operand is split into f16 planes, so an activation beyond +-65504 becomes inf in
the hi plane and inf / NaN in the layer's output; the device counts such activations (capi.f16s_overflow_count) and every
net entry point raises / returns DFVO_ERR_RANGE instead of handing the map out silently.  Checked here:
  * kernel level, the f16 conv families (profile rows 19 window, 20 streaming, 21 K-sliced): exact +-65504 is in range and
    fp32-class accurate; anything strictly above counts (65504 < |x| < 65520 conservatively: the split is still exact
    there); under f16x3 one hot activation makes exactly the outputs whose receptive field holds it non-finite, and leaves
    every other output bit-identical to the run without it;
  * non-finite inputs follow torch's float64 semantics through the exact-fp32 kernel families and every activation.
Every test that overflows resets the counter before it returns and restores the exact-fp32 packing."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import ref_act, run_conv

pytestmark = pytest.mark.gpu

F16_MAX = 65504.0
ACTS = {"none": (0, 0.0), "leaky": (1, 0.1), "relu": (2, 0.0), "elu": (3, 1.0), "sigmoid": (4, 0.0)}

# name, N, H, W, c0, c1, cout, kh, kw, stride, pad, pad_mode, up0, profile row of the f16 family that must serve it
FAMILIES = [
    ("win_128_128", 2, 96, 312, 128, 0, 128, 3, 3, 1, (1, 1), 0, 0, 19),           # F16_CASES 128_128_leaky
    ("win_cat_128_4_to_128", 2, 96, 168, 128, 4, 128, 3, 3, 1, (1, 1), 0, 0, 19),  # two sources, 4-channel tail
    ("win_mixed_height_a", 2, 176, 608, 128, 0, 64, 3, 3, 1, (1, 1), 0, 0, 19),     # _MIX_WORKER shape "a"
    ("win_L4_128_128", 2, 48, 156, 128, 0, 128, 3, 3, 1, (1, 1), 0, 0, 19),        # first window skeleton
    ("ksliced_flow_L6_192_6x19_cat", 2, 6, 19, 192, 52, 128, 3, 3, 1, (1, 1), 0, 0, 21),
    ("ksliced_resnet_256_12x40", 1, 12, 40, 256, 0, 256, 3, 3, 1, (1, 1), 0, 0, 21),
    ("stream_1x1_32_64", 2, 33, 47, 32, 0, 64, 1, 1, 1, (0, 0), 0, 0, 20),
    ("stream_3x3s2_32_64", 2, 256, 320, 32, 0, 64, 3, 3, 2, (1, 1), 0, 0, 20),     # stride 2: never the tap window
    # tap-window kernel (conv_taps_f16s.hip): multi-tap, stride 1, one source, couts padded to 32 / 64, a map large enough
    # that K is not sliced -- profile row 20 as well
    ("taps_dist7x1_32_49", 2, 128, 160, 32, 0, 49, 7, 1, 1, (3, 0), 0, 0, 20),
    ("taps_7x7_32_64", 2, 128, 160, 32, 0, 64, 7, 7, 1, (3, 3), 0, 0, 20),
    # the depth decoder's form: reflection padding, nearest-x2 upsampled first source, two sources (H, W: the layer's map)
    ("win_dec_refl_up_cat", 1, 192, 640, 32, 64, 32, 3, 3, 1, (1, 1), 1, 1, 19),
]
FAM = {f[0]: f for f in FAMILIES}
MODES = [b"f16x3", b"f16"]


def _conv(gpu, mode, fam, x0, x1, wt, b, act=0, a=0.0):
    """one dfvo_conv2d under packing `mode`; returns (output NCHW float32, launches per profile row, counter)"""
    name, n, h, w, c0, c1, cout, kh, kw, stride, pad, pad_mode, up0, _ = fam
    lib = gpu.lib()
    ms, fl, ln = np.zeros(24), np.zeros(24), np.zeros(24, np.int32)
    gpu.check(lib.dfvo_set_conv_precision(mode))
    gpu.f16s_overflow_count(reset=True)
    try:
        gpu.check(lib.dfvo_conv_profile_begin())
        try:
            out = run_conv(gpu, x0, wt, b, stride, pad, pad_mode, act, a, x1, up0)
        finally:
            gpu.check(lib.dfvo_conv_profile_end(gpu.as_ptr(ms), gpu.as_ptr(fl), gpu.as_ptr(ln)))
    finally:
        gpu.check(lib.dfvo_set_conv_precision(b"fp32"))
        n_ovf = gpu.f16s_overflow_count(reset=True)
    return out, ln, n_ovf


def _data(fam, seed):
    name, n, h, w, c0, c1, cout, kh, kw, stride, pad, pad_mode, up0, _ = fam
    g = torch.Generator().manual_seed(seed)
    hs, ws = (h // 2, w // 2) if up0 else (h, w)
    x0 = torch.randn(n, c0, hs, ws, generator=g)
    x1 = torch.randn(n, c1, h, w, generator=g) if c1 else None
    wt = torch.randn(cout, c0 + c1, kh, kw, generator=g) / np.sqrt((c0 + c1) * kh * kw)
    b = torch.randn(cout, generator=g) * 0.1
    return x0, x1, wt, b


def _full_input(fam, x0, x1):
    """the layer's input as the reference sees it: nearest x2 of source 0 (when up0), concatenated with source 1"""
    xin = F.interpolate(x0, scale_factor=2, mode="nearest") if fam[12] else x0
    return torch.cat([xin, x1], 1) if x1 is not None else xin


def _conv64(fam, xin, wt, b):
    name, n, h, w, c0, c1, cout, kh, kw, stride, pad, pad_mode, up0, _ = fam
    if pad_mode == 1:
        return F.conv2d(F.pad(xin, (pad[1], pad[1], pad[0], pad[0]), mode="reflect"), wt, b, stride=stride)
    return F.conv2d(xin, wt, b, stride=stride, padding=pad)


# ---- A. in range at the edge --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=[m.decode() for m in MODES])
@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_exact_f16_max_is_in_range_and_accurate(gpu, fam, mode):
    """inputs holding exactly +-65504 and values near 6e4 (every 97th element): no event, and the result is what the mode
    defines -- f16x3 within test_f16x3_dynamic_range's bound (2^-22 + 2^-20) sum|w x| of the float64 convolution, f16 within
    2^-20 sum|w x| (accumulation only) of the float64 convolution of the f16-ROUNDED operands"""
    x0, x1, wt, b = _data(fam, 7)
    for x in (x0, x1):
        if x is None:
            continue
        flat = x.view(-1)
        flat[0::97] = 6.0e4 * torch.sign(flat[0::97])
        flat[1::97] = F16_MAX
        flat[2::97] = -F16_MAX
        flat[3::97] = 65503.0                                   # (rounds to 65504 in f16)
    out, ln, n_ovf = _conv(gpu, mode, fam, x0, x1, wt, b)
    assert ln[fam[13]] >= 1, "profile rows %s: %s did not run on the family it names" % (np.nonzero(ln)[0].tolist(), fam[0])
    assert n_ovf == 0
    xin = _full_input(fam, x0, x1).double()
    w64 = wt.double()
    if mode == b"f16":
        xin, w64 = xin.half().double(), wt.half().double()
    ref = _conv64(fam, xin, w64, b.double())
    sabs = _conv64(fam, xin.abs(), w64.abs(), None) + b.double().abs().view(1, -1, 1, 1)
    bound = (2.0 ** -22 + 2.0 ** -20) * sabs if mode == b"f16x3" else 2.0 ** -20 * sabs
    err = (out.double() - ref).abs()
    print("   %-30s %-5s max|ref| %.3e  worst err / bound %.3f" % (fam[0], mode.decode(), float(ref.abs().max()),
                                                                  float((err / bound).max())))
    assert bool((err <= bound).all())


# ---- A. just above the edge ---------------------------------------------------------------------------------------------
ABOVE = [float(np.nextafter(np.float32(F16_MAX), np.float32(np.inf))), 65519.0, 7.0e4, 1.0e5, float("inf")]


@pytest.mark.parametrize("mode", MODES, ids=[m.decode() for m in MODES])
@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_strictly_above_f16_max_is_counted(gpu, fam, mode):
    """one activation strictly above 65504 (either sign) raises the counter.  The threshold is |x| > 65504, pinned as it is:
    65504 < |x| < 65520 rounds to a FINITE hi plane (65504) and the split stays exact there, so those events are counted
    conservatively; from 65520 on the hi plane is inf"""
    x0, x1, wt, b = _data(fam, 8)
    src = x1 if x1 is not None else x0
    for i, v in enumerate(ABOVE):
        s = src.clone()
        s[0, 0, s.shape[2] // 2, s.shape[3] // 2] = v if i % 2 == 0 else -v
        args = (x0, s) if x1 is not None else (s, None)
        out, ln, n_ovf = _conv(gpu, mode, fam, args[0], args[1], wt, b)
        assert n_ovf >= 1, "%s %s: %r not counted" % (fam[0], mode.decode(), v)
        if v < 65520.0:
            assert bool(torch.isfinite(out).all()), "%r: the hi plane is 65504, the output must stay finite" % v


# ---- A. containment ------------------------------------------------------------------------------------------------------
# (family, which source, position (n, c, y, x) in that source)
HOT_SPOTS = [
    ("win_128_128", 0, (1, 5, 40, 31)), ("win_128_128", 0, (0, 127, 47, 32)),   # columns 31 / 32: tile edge
    ("win_128_128", 0, (1, 0, 31, 200)), ("win_128_128", 0, (0, 3, 0, 0)),      # a row on a tile edge; the corner
    ("win_cat_128_4_to_128", 1, (1, 3, 50, 100)),                                  # the 4-channel tail of source 1
    ("win_mixed_height_a", 0, (1, 9, 175, 300)), ("win_mixed_height_a", 0, (0, 100, 88, 607)),
    ("win_L4_128_128", 0, (1, 64, 24, 127)),
    ("ksliced_flow_L6_192_6x19_cat", 1, (1, 51, 5, 18)), ("ksliced_flow_L6_192_6x19_cat", 0, (0, 100, 3, 9)),
    ("ksliced_resnet_256_12x40", 0, (0, 255, 11, 0)),
    ("stream_1x1_32_64", 0, (1, 31, 32, 46)),
    ("stream_3x3s2_32_64", 0, (0, 17, 255, 319)), ("stream_3x3s2_32_64", 0, (1, 2, 24, 33)),
    ("taps_dist7x1_32_49", 0, (1, 30, 2, 43)), ("taps_dist7x1_32_49", 0, (0, 0, 127, 31)),
    ("taps_7x7_32_64", 0, (0, 31, 127, 3)), ("taps_7x7_32_64", 0, (1, 8, 64, 159)),
    ("win_dec_refl_up_cat", 0, (0, 7, 0, 17)),                                     # border row under reflection + x2
    ("win_dec_refl_up_cat", 1, (0, 40, 191, 639)), ("win_dec_refl_up_cat", 1, (0, 5, 100, 0)),  # reflected corner / column
]
CONTAIN_ACTS = ["none", "leaky", "elu", "relu"]


def _affected(fam, src, pos, wt):
    """float64: the outputs whose receptive field holds the hot element -- the indicator convolved with |w| > 0 over the
    hot input channel (F.pad's reflection and F.interpolate's x2 replicate it as the device must)"""
    name, n, h, w, c0, c1, cout, kh, kw, stride, pad, pad_mode, up0, _ = fam
    nn, c, y, x = pos
    hs, ws = ((h // 2, w // 2) if (up0 and src == 0) else (h, w))
    ind = torch.zeros(n, 1, hs, ws, dtype=torch.float64)
    ind[nn, 0, y, x] = 1.0
    if up0 and src == 0:
        ind = F.interpolate(ind, scale_factor=2, mode="nearest")
    ci = c if src == 0 else c0 + c
    k = (wt[:, ci:ci + 1].abs() > 0).double()
    fam1 = fam[:4] + (1, 0, cout) + fam[7:12] + (0, fam[13])
    return _conv64(fam1, ind, k, None) > 0


@pytest.mark.parametrize("spot", HOT_SPOTS, ids=["%s-src%d-%s" % (s[0], s[1], "_".join(map(str, s[2]))) for s in HOT_SPOTS])
def test_one_hot_activation_is_contained(gpu, spot):
    """f16x3: 1e5 at one element: the output is non-finite EXACTLY on the outputs whose receptive field holds it, for every
    activation (ReLU included: NaN propagates as in torch), and bit-identical elsewhere to the run with that element at 0 --
    halo, tile, split-K and mixed-height indexing checked where finite-data tolerances cannot see them"""
    fname, src, pos = spot
    fam, mode = FAM[fname], b"f16x3"
    x0, x1, wt, b = _data(fam, 9)
    aff = _affected(fam, src, pos, wt)
    assert 0 < int(aff.sum()) < aff.numel()
    for act in CONTAIN_ACTS:
        code, a = ACTS[act]
        outs = {}
        for tag, v in (("hot", 1.0e5), ("zero", 0.0)):
            xs = [x0.clone(), x1.clone() if x1 is not None else None]
            xs[src][pos] = v
            outs[tag], ln, n_ovf = _conv(gpu, mode, fam, xs[0], xs[1], wt, b, code, a)
            assert ln[fam[13]] >= 1
            assert (n_ovf >= 1) == (tag == "hot"), (tag, n_ovf)
        bad = ~torch.isfinite(outs["hot"])
        miss, extra = int((aff & ~bad).sum()), int((bad & ~aff).sum())
        assert miss == 0 and extra == 0, "%s %s act %s: %d affected outputs finite, %d outside non-finite" % (
            fname, mode.decode(), act, miss, extra)
        assert torch.equal(outs["hot"][~aff], outs["zero"][~aff]), "%s %s act %s: outputs outside the receptive field moved" % (
            fname, mode.decode(), act)


# ---- A. weights at pack time ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=[m.decode() for m in MODES])
@pytest.mark.parametrize("fname", ["stream_1x1_32_64", "taps_dist7x1_32_49"])
def test_weights_beyond_f16_max_are_counted_once_each(gpu, fname, mode):
    """the packer (f16s_split_host) clamps a weight beyond +-65504 and counts it once; exactly 65504 is not counted, and
    the clamped weight computes exactly what 65504 does"""
    fam = FAM[fname]
    x0, _, wt, b = _data(fam, 10)
    x0 = x0 * 1e-3
    w_edge = wt.clone()
    w_edge[3, 5, 0, 0], w_edge[10, 0, -1, 0] = F16_MAX, -F16_MAX
    out_edge, _, n_edge = _conv(gpu, mode, fam, x0, None, w_edge, b)
    assert n_edge == 0
    w_over = wt.clone()
    w_over[3, 5, 0, 0], w_over[10, 0, -1, 0] = 65505.0, -65505.0
    w_over[20, 7, 0, 0] = 1.0e6
    out_over, _, n_over = _conv(gpu, mode, fam, x0, None, w_over, b)
    assert n_over == 3
    w_edge[20, 7, 0, 0] = F16_MAX
    out_clamped, _, _ = _conv(gpu, mode, fam, x0, None, w_edge, b)
    assert torch.equal(out_over, out_clamped)


def test_k_sliced_families_with_k_divided_over_more_workgroups(gpu):
    """DFVO_F16G_NZ=-1 (read once per process): the K-sliced cases of this module again in a child pytest"""
    env = dict(os.environ, DFVO_F16G_NZ="-1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k", "ksliced and not more_workgroups"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:]
    n_fam = sum(f[0].startswith("ksliced") for f in FAMILIES)
    want = 2 * len(MODES) * n_fam + sum(h[0].startswith("ksliced") for h in HOT_SPOTS)  # (edge + above) per mode, hot spots
    assert re.search(r"\b%d passed" % want, r.stdout) and " failed" not in r.stdout, r.stdout[-500:]


# ---- B. non-finite inputs through the exact-fp32 families -----------------------------------------------------------------
FP32_FAMILIES = [
    # name, N, H, W, c0, c1, cout, kh, kw, stride, pad, pad_mode, up0, allowed profile rows
    ("igemm_1x1_32_64", 2, 96, 160, 32, 0, 64, 1, 1, 1, (0, 0), 0, 0, tuple(range(12))),
    ("win3_128_64", 2, 96, 160, 128, 0, 64, 3, 3, 1, (1, 1), 0, 0, (12, 13, 14, 15)),
    ("head3_cat_32_4_to_2", 2, 45, 77, 32, 4, 2, 3, 3, 1, (1, 1), 0, 0, (18,)),
    ("f32g_flow_L6_192_6x19_cat", 2, 6, 19, 192, 52, 128, 3, 3, 1, (1, 1), 0, 0, (22, 23)),
]


@pytest.mark.parametrize("fam", FP32_FAMILIES, ids=[f[0] for f in FP32_FAMILIES])
def test_non_finite_inputs_follow_torch_in_exact_fp32(gpu, fam):
    """a NaN, a +inf and a -inf activation (separate pixels, separate samples where there are two) through every activation:
    the NaN / +-inf positions and values equal torch's float64 result; the finite outputs stay at the fp32 tolerance"""
    x0, x1, wt, b = _data(fam[:13] + (0,), 11)
    n, h, w = fam[1], fam[2], fam[3]
    x0[0, 1, h // 3, w // 4] = float("nan")
    x0[-1, 2, h // 2, w // 2] = float("inf")
    (x1 if x1 is not None else x0)[0, 0, h - 1, w - 2] = float("-inf")
    ref_lin = _conv64(fam, _full_input(fam, x0, x1).double(), wt.double(), b.double())
    for act, (code, a) in ACTS.items():
        ref = ref_act(ref_lin, code, a)
        out, ln, _ = _conv(gpu, b"fp32", fam[:13] + (0,), x0, x1, wt, b, code, a)
        assert any(ln[r] for r in fam[13]), "profile rows %s for %s" % (np.nonzero(ln)[0].tolist(), fam[0])
        out = out.double()
        for pred in (torch.isnan, torch.isposinf, torch.isneginf):
            assert torch.equal(pred(out), pred(ref)), "%s act %s: %s positions differ from torch (%d vs %d)" % (
                fam[0], act, pred.__name__, int(pred(out).sum()), int(pred(ref).sum()))
        fin = torch.isfinite(ref)
        e = float((out[fin] - ref[fin]).abs().max())
        assert e <= 2e-5 * max(1.0, float(ref[fin].abs().max())), (act, e)


@pytest.mark.parametrize("mode", MODES, ids=[m.decode() for m in MODES])
def test_nan_input_propagates_under_the_split(gpu, mode):
    """a NaN activation is not a range event (the counter measures |x|; it stays 0), but it must not be lost either: the
    outputs whose receptive field holds it are NaN -- through ReLU too -- and nothing else changes"""
    fam = FAM["win_128_128"]
    x0, x1, wt, b = _data(fam, 12)
    pos = (1, 9, 50, 31)
    aff = _affected(fam, 0, pos, wt)
    for act in ("leaky", "relu"):
        code, a = ACTS[act]
        xs = x0.clone()
        xs[pos] = float("nan")
        out, _, n_ovf = _conv(gpu, mode, fam, xs, None, wt, b, code, a)
        xs[pos] = 0.0
        out0, _, _ = _conv(gpu, mode, fam, xs, None, wt, b, code, a)
        print("   NaN input, %s %s: counter %d" % (mode.decode(), act, n_ovf))
        assert torch.equal(torch.isnan(out), aff)
        assert torch.equal(out[~aff], out0[~aff])


# ---- B. max-pool: NaN and +-inf as torch.max_pool2d -----------------------------------------------------------------------
def test_maxpool_follows_torch_on_non_finite_values(gpu):
    """dfvo_maxpool3x3s2 (the monodepth2 encoder's pool) against F.max_pool2d(3, 2, 1): bit for bit on finite data, NaN
    wherever a window holds one (also next to +inf and finite values), +-inf as torch"""
    lib = gpu.lib()
    g = torch.Generator().manual_seed(13)
    n, c, h, w = 2, 64, 95, 161
    x = torch.randn(n, c, h, w, generator=g)
    x[0, 3, 10, 10] = float("nan")
    x[0, 3, 10, 11] = float("inf")                              # NaN and +inf in one window: NaN
    x[1, 60, 0, 0] = float("nan")                               # corner (padding)
    x[1, 7, 50:53, 80:83] = float("-inf")                       # a whole window of -inf
    x[0, 63, h - 1, w - 1] = float("inf")
    x[1, 0, 33, 70] = float("nan")
    x[1, 0, 33, 71] = 1.0e30
    ref = F.max_pool2d(x.double(), 3, 2, 1).float()
    src = x.permute(0, 2, 3, 1).contiguous().cuda()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dst = torch.full((n, ho, wo, c), 7.0, device="cuda")
    gpu.check(lib.dfvo_maxpool3x3s2(C.c_void_p(src.data_ptr()), n, h, w, c, C.c_void_p(dst.data_ptr()), None))
    got = dst.permute(0, 3, 1, 2).cpu()
    assert ref.shape == got.shape
    for pred in (torch.isnan, torch.isposinf, torch.isneginf):
        assert torch.equal(pred(got), pred(ref)), pred.__name__
    fin = torch.isfinite(ref)
    assert torch.equal(got[fin], ref[fin])
    assert int(torch.isnan(ref).sum()) >= 3


# ---- C. the guard through the mirrors and the C session --------------------------------------------------------------------
def _dropin():
    return importlib.import_module("test_dropin_gpu")


def _hot_depth_on_bright_blue(fsd, dsd):
    """the crafted depth decoder reads conv1's +B channel (ReLU of the normalised blue, <= 2.44) at upconv(1,1): at a gain
    of 3e4 a frame whose blue is >= 240 drives that layer's output beyond 65504, split by upconv(0,0); blue <= 200 stays at
    4.5e4.  Nothing else of either net changes"""
    dsd["decoder.7.conv.conv.weight"][0, 32 + 0, 1, 1] = 3.0e4


def _hot_flow_on_bright(fsd, dsd):
    """Features.moduleOne channel 2: 3e4 on the centre tap of R, G and B, no bias.  The flow net reads u8 / 255: a white
    frame gives 9e4 there, beyond f16 at the next split; a black frame gives 0"""
    wt, b = fsd["moduleFeatures.moduleOne.0.weight"], fsd["moduleFeatures.moduleOne.0.bias"]
    wt[2] = 0.0
    wt[2, :, 3, 3] = 3.0e4
    b[2] = 0.0


def _cold_frames(seq, n):
    out = []
    for k in range(n):
        f = seq["frames"][k].copy()
        f[..., 2] = np.minimum(f[..., 2], 200)
        out.append(f)
    return out


def _hot(f):
    f = f.copy()
    f[..., 2] = 255
    return f


@pytest.mark.parametrize("sess", ["0", "1"])
def test_mirror_guard_is_per_call(gpu, tmp_path, monkeypatch, sess):
    """in range -> hot -> in range -> external reset -> hot through forward_depth (and the plain forward_flow): the hot calls
    raise; every in-range call returns bit for bit what a fresh model of the same weights returns for that frame"""
    capi = importlib.import_module("df-vo_amd.capi")
    D = _dropin()
    monkeypatch.setenv("DFVO_SESSION", sess)
    try:
        h, w, seq, cfg = D._small_world(tmp_path, tweak=_hot_depth_on_bright_blue)
        cold = _cold_frames(seq, 4)

        def fresh_depth(f):
            m = D._build_mirrors(cfg, seq["K"])[0]
            return np.array(m.forward_depth(imgs=[f.copy()]))
        want = [fresh_depth(f) for f in cold[:3]]
        assert all(np.isfinite(d).all() for d in want)
        dm = D._build_mirrors(cfg, seq["K"])[0]
        assert (dm.session is not None) == (sess == "1") and dm.conv_precision == "f16x3"
        assert np.array_equal(np.array(dm.forward_depth(imgs=[cold[0].copy()])), want[0])
        with pytest.raises(capi.DfvoError, match="out of range"):
            dm.forward_depth(imgs=[_hot(cold[1])])
        assert np.array_equal(np.array(dm.forward_depth(imgs=[cold[1].copy()])), want[1])
        if sess == "0":
            fl = dm.forward_flow({"id": 1, "img": cold[1]}, {"id": 0, "img": cold[0]}, True)
            assert all(np.isfinite(v).all() for v in fl.values())
        capi.f16s_overflow_count(reset=True)                    # somebody else resets the process-wide counter
        assert np.array_equal(np.array(dm.forward_depth(imgs=[cold[2].copy()])), want[2])
        with pytest.raises(capi.DfvoError, match="out of range"):
            dm.forward_depth(imgs=[_hot(cold[3])])
    finally:
        capi.f16s_overflow_count(reset=True)


class _CSession:
    """dfvo_session_* through ctypes on the session a DeepModel mirror created"""

    def __init__(self, capi, dm, h, w):
        self.capi, self.lib, self.hnd = capi, dm.session.lib, dm.session.handle
        self.h, self.w, self.fh, self.fw = h, w, dm.session.fh, dm.session.fw
        capi.check(self.lib.dfvo_session_reset(self.hnd))

    def push(self, img, flags=0):
        g = C.c_longlong()
        self.capi.check(self.lib.dfvo_session_push_frame(self.hnd, self.capi.as_ptr(np.ascontiguousarray(img)), None, None, flags,
                                                         C.byref(g)))
        return g.value

    def depth(self, g):
        p = C.c_void_p()
        rc = self.lib.dfvo_session_depth(self.hnd, g, C.byref(p))
        return rc, (np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (self.fh * self.fw,)).copy() if p.value else None)

    def flow(self, g):
        pf, pb, pd = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.lib.dfvo_session_flow(self.hnd, g, C.byref(pf), C.byref(pb), C.byref(pd))
        return rc, (np.ctypeslib.as_array(C.cast(pf, C.POINTER(C.c_float)), (2 * self.h * self.w,)).copy() if pf.value else None)


def test_c_session_reports_a_bad_generation_on_every_read(gpu, tmp_path, monkeypatch):
    """dfvo_session_depth / dfvo_session_flow of a hot generation return DFVO_ERR_RANGE on EVERY read, the pointer set and the
    map non-finite; the next in-range generations return DFVO_OK with finite maps"""
    capi = importlib.import_module("df-vo_amd.capi")
    D = _dropin()
    monkeypatch.setenv("DFVO_SESSION", "1")

    def both(fsd, dsd):
        _hot_depth_on_bright_blue(fsd, dsd)
        _hot_flow_on_bright(fsd, dsd)
    try:
        h, w, seq, cfg = D._small_world(tmp_path, tweak=both)
        s = _CSession(capi, D._build_mirrors(cfg, seq["K"])[0], h, w)
        black, white = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
        capi.f16s_overflow_count(reset=True)
        g = s.push(black)
        assert s.depth(g)[0] == 0
        g = s.push(black)
        (rc_d, d), (rc_f, f) = s.depth(g), s.flow(g)
        assert rc_d == 0 and rc_f == 0 and np.isfinite(d).all() and np.isfinite(f).all(), "precondition: black is in range"
        g = s.push(white)
        for _ in range(3):
            rc, d = s.depth(g)
            assert rc == capi.ERR_RANGE and d is not None and not np.isfinite(d).all()
            rc, f = s.flow(g)
            assert rc == capi.ERR_RANGE and f is not None and not np.isfinite(f).all()
        g = s.push(black, capi.PUSH_NO_FLOW)                    # (depth only: both frames of the next pair go through Features)
        rc, d = s.depth(g)
        assert rc == 0 and np.isfinite(d).all()
        g = s.push(black)
        (rc_d, d), (rc_f, f) = s.depth(g), s.flow(g)
        assert rc_d == 0 and rc_f == 0 and np.isfinite(d).all() and np.isfinite(f).all()
    finally:
        capi.f16s_overflow_count(reset=True)


def test_c_session_pair_after_a_hot_frame_is_never_nan_with_success(gpu, tmp_path, monkeypatch):
    """the session carries frame g's flow pyramids into the pair (g, g + 1); when frame g overflowed they hold inf / NaN, and
    NaN is not a range event.  The pair right after a hot frame must fail or be finite -- never NaN with DFVO_OK"""
    capi = importlib.import_module("df-vo_amd.capi")
    D = _dropin()
    monkeypatch.setenv("DFVO_SESSION", "1")
    try:
        h, w, seq, cfg = D._small_world(tmp_path, tweak=_hot_flow_on_bright)
        s = _CSession(capi, D._build_mirrors(cfg, seq["K"])[0], h, w)
        black, white = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
        capi.f16s_overflow_count(reset=True)
        s.push(black)
        g = s.push(white)
        assert s.flow(g)[0] == capi.ERR_RANGE
        g = s.push(black)
        rc, f = s.flow(g)
        print("   pair after a hot frame: rc %d, finite %s" % (rc, bool(np.isfinite(f).all())))
        assert rc == capi.ERR_RANGE or np.isfinite(f).all(), "flow of the pair after a hot frame: NaN with DFVO_OK"
        g = s.push(black)
        rc, f = s.flow(g)
        assert rc == 0 and np.isfinite(f).all()                 # (two in-range frames again)
    finally:
        capi.f16s_overflow_count(reset=True)


def test_depth_map_next_to_err_range_is_not_finite(gpu, tmp_path, monkeypatch):
    """hot encoder (conv1 + BN + ReLU ~1e5, the first residual block splits it): the map dfvo_session_depth hands out with
    DFVO_ERR_RANGE holds non-finite values, as the header says -- the encoder's ReLUs and max-pool must not turn the NaN into
    a finite, plausible depth"""
    capi = importlib.import_module("df-vo_amd.capi")
    D = _dropin()
    monkeypatch.setenv("DFVO_SESSION", "1")

    def hot_encoder(fsd, dsd):
        dsd["encoder.bn1.bias"][:] = 1.0e5
    try:
        h, w, seq, cfg = D._small_world(tmp_path, tweak=hot_encoder)
        s = _CSession(capi, D._build_mirrors(cfg, seq["K"])[0], h, w)
        g = s.push(seq["frames"][0].copy(), capi.PUSH_NO_FLOW)
        rc, d = s.depth(g)
        assert rc == capi.ERR_RANGE and d is not None
        assert not np.isfinite(d).all(), "DFVO_ERR_RANGE with a finite depth map: the overflow was laundered"
    finally:
        capi.f16s_overflow_count(reset=True)
