"""The flow net launch by launch against float64, so that a failure of the net's whole-map gates names its layer.

Every entry of tests/flow_world.py's FLOW_LAYERS runs through the C ABI on its real input: the float64 walk's values
rounded to fp32, in the views (floats per pixel, appended channels, batch swap) the net passes.  Each output element is
compared with the float64 result of the same fp32 operands.
  conv       all three packings, random world (224x672): tests/layer_bounds.py's bounds; the two-channel heads that the
             device runs on its exact fp32 head kernel (N*Ho*Wo >= 1024, square k = 3 / 5 / 7) take the fp32 bound in every
             mode.  No case may raise an f16 range event.
  non-conv   both worlds (the tunnel's 10-27 px flows carry samples across the zero-padding border), with the bounds of
             tests/flow_bounds.py, derived from each kernel's arithmetic.
Exact by construction and checked bit for bit: the flow the sub-pixel warp appends (and its two zero channels), the zero
channel of reg prep, the padding channels [k*k, kkp) the distance convolutions zero, and the pixels a stride-2 warp leaves
alone.  test_inventory_runs_the_conv_families_the_net_runs sums the conv launches per profile row over the inventory and
compares them with one dfvo_flownet_forward_host (graphs off) in each packing."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_bounds as B
import flow_world as FW
from layer_bounds import conv_bound
from oracle import nets_torch as O
from util import ptr

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "f16x3", "f16"]
CONVS = [L for L in FW.FLOW_LAYERS if L["op"] == "conv"]
OPS = [L for L in FW.FLOW_LAYERS if L["op"] != "conv"]
SENTINEL = 7.0
_cache = {}


def _world(name):
    if name not in _cache:
        sd, ref, cur = FW.world(name)
        acts = FW.walk64(name)
        _cache[name] = sd, ref, cur, {k: v.float() for k, v in acts.items()}
    return _cache[name]


def _dev(t, cs):
    """NCHW fp32 -> NHWC device buffer with cs floats per pixel (logical channels first, zeros behind)"""
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, cs, dtype=torch.float32)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out.cuda().contiguous()


def _host(d, c0, c1):
    return d[..., c0:c1].permute(0, 3, 1, 2).contiguous().cpu()


def _exact_head(L, n, ho, wo):
    """launch_conv's conv_use_head: the exact fp32 head kernel in every packing"""
    cout = 2 if L["dst_cs"] == 4 else None
    return (cout == 2 and L["kh"] == L["kw"] and L["kh"] in (3, 5, 7) and L["stride"] == 1
            and L["pad"] == (L["kh"] // 2, L["kw"] // 2) and n * ho * wo >= 1024)


def _run_conv(gpu, precision, L):
    key = ("conv", precision, L["id"])
    if key in _cache:
        return _cache[key]
    sd, _, _, a32 = _world("random")
    lib = gpu.lib()
    x0 = a32[L["src"]]
    if L["frame"] is not None:
        x0 = x0[L["frame"]:L["frame"] + 1]
    x1 = a32[L["src1"]] if L["src1"] else None
    res = a32[L["res"]] if L["res"] else None
    wt, b = sd[L["name"] + ".weight"].float().contiguous(), sd[L["name"] + ".bias"].float().contiguous()
    cout = wt.shape[0]
    n, _, h, w = x0.shape
    ho = (h + 2 * L["pad"][0] - L["kh"]) // L["stride"] + 1
    wo = (w + 2 * L["pad"][1] - L["kw"]) // L["stride"] + 1
    d0 = _dev(x0, L["cs0"])
    d1 = _dev(x1, L["cs1"]) if x1 is not None else None
    dres = _dev(res, 4) if res is not None else None
    dst = torch.full((n, ho, wo, L["dst_cs"]), SENTINEL, device="cuda")
    desc = gpu.ConvDesc(N=n, H=h, W=w, kh=L["kh"], kw=L["kw"], stride=L["stride"], pad_h=L["pad"][0], pad_w=L["pad"][1],
                        pad_mode=0, c0=L["c0"], cs0=L["cs0"], co0=0, up0=0, c1=L["c1"], cs1=L["cs1"], co1=0, cout=cout,
                        act=1 if L["act"] == "leaky" else 0, act_param=0.1, res_cs=4 if res is not None else 0, res_co=0,
                        dst_cs=L["dst_cs"], dst_co=0, dst_zero_to=L["dst_zero_to"])
    wn, bn = wt.numpy(), b.numpy()
    ms, fl, ln = np.zeros(24), np.zeros(24), np.zeros(24, np.int32)
    gpu.check(lib.dfvo_set_conv_precision(precision.encode()))
    gpu.f16s_overflow_count(reset=True)
    try:
        gpu.check(lib.dfvo_conv_profile_begin())
        try:
            gpu.check(lib.dfvo_conv2d(C.byref(desc), ptr(d0), ptr(d1), gpu.as_ptr(wn), gpu.as_ptr(bn), ptr(dres), ptr(dst), None))
            torch.cuda.synchronize()
        finally:
            gpu.check(lib.dfvo_conv_profile_end(gpu.as_ptr(ms), gpu.as_ptr(fl), gpu.as_ptr(ln)))
    finally:
        gpu.check(lib.dfvo_set_conv_precision(b"fp32"))
        n_ovf = gpu.f16s_overflow_count(reset=True)
    xin = torch.cat([x0, x1], 1) if x1 is not None else x0
    head = _exact_head(L, n, ho, wo)
    _, _, y, bound = conv_bound(lambda x, ww, bb: FW.conv_ref(L, x, ww, bb), xin.double(), wt.double(), b.double(),
                                res.double() if res is not None else None, precision, exact_fp32=head)
    ref = F.leaky_relu(y, 0.1) if L["act"] == "leaky" else y
    out = _host(dst, 0, cout)
    pad = _host(dst, cout, L["dst_zero_to"]) if L["dst_zero_to"] else None
    _cache[key] = (out, ref, bound, pad, n_ovf, ln.copy(), head)
    return _cache[key]


def _rows(ln):
    return " ".join("%d:%d" % (r, ln[r]) for r in np.nonzero(ln)[0])


def _report(tag, out, ref, bound):
    assert out.shape == ref.shape, (tag, out.shape, ref.shape)
    err = (out.double() - ref).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())  # (a zero bound admits only zero error)
    print("   %-52s max|ref| %.2e  max err %.2e  worst err / bound %.3f" % (tag, float(ref.abs().max()), float(err.max()), ratio))
    assert bool(torch.isfinite(out).all()), tag
    assert bool((err <= bound).all()), "%s: worst err / bound %.3f" % (tag, ratio)


@pytest.mark.parametrize("layer", [L["id"] for L in CONVS])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_flownet_conv_layers_vs_float64(gpu, precision, layer):
    L = next(L for L in CONVS if L["id"] == layer)
    out, ref, bound, pad, n_ovf, ln, head = _run_conv(gpu, precision, L)
    assert n_ovf == 0, "%s %s: %d f16 range events" % (precision, layer, n_ovf)
    _report("%-5s %s%s rows %s" % (precision, layer, " (fp32 head)" if head else "", _rows(ln)), out, ref, bound)
    if pad is not None:
        assert bool((pad == 0).all()), "%s: channels [k*k, kkp) not zeroed" % layer


def _lin(n):
    return torch.linspace(-1.0, 1.0, n).numpy()


def _run_op(gpu, world, L):
    """the device output(s) of non-conv entry L and their float64 reference(s) and bounds: [(tag, out, ref, bound)], plus
    the exact checks [(tag, got, want)]"""
    sd, ref_u8, cur_u8, a32 = _world(world)
    lib = gpu.lib()
    a64 = {k: v.double() for k, v in a32.items()}
    op = L["op"]
    checks, exact = [], []
    if op == "input":
        u8 = np.ascontiguousarray(ref_u8 if L["frame"] == 0 else cur_u8)
        th, tw = a32["img1"].shape[2:]
        du8 = torch.from_numpy(u8).cuda()
        dst = torch.full((th, tw, 4), SENTINEL, device="cuda")
        gpu.check(lib.dfvo_img_u8_to_flow_input(ptr(du8), u8.shape[0], u8.shape[1], ptr(dst), th, tw, None))
        img = torch.from_numpy(np.transpose(u8 / 255, (2, 0, 1))).unsqueeze(0).float().double()
        r = F.interpolate(img, (th, tw), mode="bilinear", align_corners=True)
        out = dst.unsqueeze(0)
        checks.append(("input", _host(out, 0, 3), r, B.input_bound(img)(th, tw)))
        exact.append(("input channel 3", _host(out, 3, 4), torch.zeros(1, 1, th, tw)))
    elif op == "resize":
        f = L["frame"]
        x = a32[L["src"]][f:f + 1]
        n, c, h, w = x.shape
        dx = _dev(x, 4)
        dst = torch.full((1, h // 2, w // 2, 4), SENTINEL, device="cuda")
        gpu.check(lib.dfvo_resize_bilinear(ptr(dx), 1, h, w, 4, ptr(dst), h // 2, w // 2, 0, None))
        torch.cuda.synchronize()
        checks.append(("resize", _host(dst, 0, 3), FW.resize_ref(x.double(), (h // 2, w // 2)), B.resize_half_bound(x.double())))
    elif op == "deconv":
        x = a32[L["src"]]
        n, c, h, w = x.shape
        wt = sd[L["w"]].float().contiguous()
        dx = _dev(x, L["cs"])
        dst = torch.full((n, 2 * h, 2 * w, L["cs"]), SENTINEL, device="cuda")
        gpu.check(lib.dfvo_deconv_dw4x4s2(ptr(dx), n, h, w, c, L["cs"], gpu.as_ptr(wt.numpy()), ptr(dst), None))
        checks.append(("deconv", _host(dst, 0, c), FW.deconv_ref(x.double(), wt.double()), B.deconv_bound(x.double(), wt.double())))
    elif op == "warp":
        src, flow = a32[L["src"]], a32[L["flow"]]
        n, c, h, w = src.shape
        ds, dfl = _dev(src, L["scs"]), _dev(flow, 4)
        dst = torch.full((n, h, w, L["dcs"]), SENTINEL, device="cuda")
        lx, ly = _lin(w), _lin(h)
        gpu.check(lib.dfvo_warp_view(ptr(ds), L["scs"], 0, L["swap"], ptr(dfl), 4, 0, L["mult"], n, h, w, c, gpu.as_ptr(lx),
                                     gpu.as_ptr(ly), ptr(dst), L["dcs"], 0, L["append_flow"], L["step"], None))
        s64, f64 = src.double(), flow.double()
        r = FW.warp_ref(s64, f64, L["mult"], L["swap"])
        bnd = B.warp_bound(s64, f64, L["mult"], L["swap"])
        out = _host(dst, 0, L["dcs"])
        st = L["step"]
        checks.append(("warp swap=%d step=%d" % (L["swap"], st), out[:, :c, ::st, ::st], r[:, :, ::st, ::st], bnd[:, :, ::st, ::st]))
        if st > 1:
            keep = torch.ones(h, w, dtype=torch.bool)
            keep[::st, ::st] = False
            exact.append(("pixels a step-%d warp leaves alone" % st, out[:, :, keep], torch.full_like(out[:, :, keep], SENTINEL)))
        if L["append_flow"]:
            exact.append(("appended flow", out[:, c:c + 2], flow))
            exact.append(("appended zero channels", out[:, c + 2:c + 4], torch.zeros(n, 2, h, w)))
    elif op == "corr":
        f1, f2 = a32[L["src1"]], a32[L["src2"]]
        n, c, h, w = f1.shape
        s = L["stride"]
        ho, wo = -(-h // s), -(-w // s)
        d1, d2 = _dev(f1, L["cs1"]), _dev(f2, L["cs2"])
        dst = torch.full((n, ho, wo, 52), SENTINEL, device="cuda")
        gpu.check(lib.dfvo_correlation_view(ptr(d1), L["cs1"], 0, ptr(d2), L["cs2"], 0, L["swap2"], n, h, w, c, s, 0.1, ptr(dst),
                                            52, None))
        r = FW.corr_ref(f1.double(), f2.double(), s, L["swap2"])
        checks.append(("corr swap2=%d stride=%d C=%d" % (L["swap2"], s, c), _host(dst, 0, 49), r,
                       B.corr_bound(f1.double(), f2.double(), s, L["swap2"], O.correlation)))
    elif op == "mean":
        fl = a32[L["src"]]
        n, _, h, w = fl.shape
        dfl = _dev(fl, 4)
        mean = torch.full((n, 2), SENTINEL, device="cuda")
        gpu.check(lib.dfvo_flow_mean(ptr(dfl), 4, 0, n, h * w, ptr(mean), None))
        m64 = FW.mean_ref(fl.double()).view(n, 2)
        checks.append(("flow mean (1 ulp)", mean.cpu().view(n, 2, 1, 1), m64.view(n, 2, 1, 1), B.mean_ulp(m64).view(n, 2, 1, 1)))
    elif op == "reg_prep":
        img, fl, mean = a32[L["img"]], a32[L["flow"]], a32[L["mean"]]
        n, _, h, w = fl.shape
        di, dfl = _dev(img, 4), _dev(fl, 4)
        dmean = mean.view(n, 2).contiguous().cuda()
        dst = torch.full((n, h, w, 4), SENTINEL, device="cuda")
        gpu.check(lib.dfvo_reg_prep(ptr(di), ptr(dfl), 4, 0, L["mult"], ptr(dmean), n, h, w, gpu.as_ptr(_lin(w)),
                                    gpu.as_ptr(_lin(h)), ptr(dst), None))
        r = FW.reg_prep_ref(img.double(), fl.double(), mean.double(), L["mult"])
        out = _host(dst, 0, 4)
        checks.append(("reg prep", out[:, :3], r, B.reg_prep_bound(img.double(), fl.double(), mean.double(), L["mult"], r)))
        exact.append(("reg prep channel 3", out[:, 3:4], torch.zeros(n, 1, h, w)))
    elif op == "reg_head":
        dist, fl = a32[L["dist"]], a32[L["flow"]]
        n, kk, h, w = dist.shape
        k = L["k"]
        wx, bx = sd[L["wx"] + ".weight"].float(), float(sd[L["wx"] + ".bias"][0])
        wy, by = sd[L["wy"] + ".weight"].float(), float(sd[L["wy"] + ".bias"][0])
        dd, dfl = _dev(dist, L["dist_cs"]), _dev(fl, 4)
        dst = torch.full((n, h, w, 4), SENTINEL, device="cuda")
        gpu.check(lib.dfvo_reg_head(ptr(dd), L["dist_cs"], k, ptr(dfl), 4, 0, gpu.as_ptr(wx.contiguous().numpy().ravel()), bx,
                                    gpu.as_ptr(wy.contiguous().numpy().ravel()), by, n, h, w, ptr(dst), 4, 0, None))
        d64, f64 = dist.double(), fl.double()
        b64 = [torch.tensor([float(np.float32(v))], dtype=torch.float64) for v in (bx, by)]
        r = FW.reg_head_ref(d64, f64, wx.double(), b64[0], wy.double(), b64[1], k)
        checks.append(("reg head k=%d" % k, _host(dst, 0, 2), r,
                       B.reg_head_bound(d64, f64, wx.double(), bx, wy.double(), by, k, r)))
    elif op == "post":
        fl = a32[L["src"]]
        H, W = ref_u8.shape[:2]
        _, _, h, w = fl.shape
        dfl = _dev(fl, 4)
        fwd = torch.full((2, H, W), SENTINEL, device="cuda")
        bwd = torch.full((2, H, W), SENTINEL, device="cuda")
        diff = torch.full((H, W), SENTINEL, device="cuda")
        gpu.check(lib.dfvo_flow_post(ptr(dfl), 4, 0, h, w, L["scale"], H, W, ptr(fwd), ptr(bwd), ptr(diff), None))
        f64 = fl.double()
        rf, rb = FW.post_resize_ref(f64, L["scale"], H, W)
        bf, bb = B.post_resize_bound(f64, L["scale"], H, W)
        checks.append(("flow post resize fwd", fwd.cpu().unsqueeze(0), rf, bf))
        checks.append(("flow post resize bwd", bwd.cpu().unsqueeze(0), rb, bb))
        # the consistency kernel against float64 on the fp32 maps it read
        fd, bd = fwd.cpu().unsqueeze(0).double(), bwd.cpu().unsqueeze(0).double()
        rc = FW.consistency_ref(fd, bd)
        checks.append(("flow post consistency", diff.cpu().view(1, 1, H, W), rc.permute(0, 3, 1, 2), B.consistency_bound(fd, bd, rc)))
    torch.cuda.synchronize()
    return checks, exact


@pytest.mark.parametrize("layer", [L["id"] for L in OPS])
@pytest.mark.parametrize("world", FW.WORLDS)
def test_flownet_operators_vs_float64(gpu, world, layer):
    L = next(L for L in OPS if L["id"] == layer)
    checks, exact = _run_op(gpu, world, L)
    for tag, out, ref, bound in checks:
        _report("%-6s %s %s" % (world, layer, tag), out, ref, bound)
    for tag, got, want in exact:
        assert torch.equal(got, want.float()), "%s %s: %s not exact" % (world, layer, tag)


def _net_rows(gpu, precision):
    """launches per profile row of one flow-net forward (graphs off), packed under `precision`"""
    from test_nets_gpu import make_flownet
    sd, ref, cur, _ = _world("random")
    lib = gpu.lib()
    h, w = ref.shape[:2]
    gpu.check(lib.dfvo_set_conv_precision(precision.encode()))
    try:
        net, _, _ = make_flownet(gpu, h, w, sd)
    finally:
        gpu.check(lib.dfvo_set_conv_precision(b"fp32"))
    fwd, bwd, diff = np.zeros((2, h, w), np.float32), np.zeros((2, h, w), np.float32), np.zeros((h, w), np.float32)
    args = [gpu.as_ptr(a) for a in (ref, cur, fwd, bwd, diff)]
    ms, fl, ln = np.zeros(24), np.zeros(24), np.zeros(24, np.int32)
    try:
        gpu.check(lib.dfvo_flownet_forward_host(net, *args))  # the one eager tuning run
        gpu.check(lib.dfvo_conv_profile_begin())
        try:
            gpu.check(lib.dfvo_flownet_forward_host(net, *args))
        finally:
            gpu.check(lib.dfvo_conv_profile_end(gpu.as_ptr(ms), gpu.as_ptr(fl), gpu.as_ptr(ln)))
    finally:
        lib.dfvo_flownet_destroy(net)
    assert gpu.f16s_overflow_count(reset=True) == 0
    return ln


@pytest.mark.parametrize("precision", PRECISIONS)
def test_inventory_runs_the_conv_families_the_net_runs(gpu, precision):
    """the inventory's conv launches, summed per profile row, equal one forward of the net: every conv family the net uses
    at 224x672 was checked above, as often as the net launches it"""
    inv = np.zeros(24, np.int32)
    print("\n   layer -> profile row:launches (%s)" % precision)
    for L in CONVS:
        ln = _run_conv(gpu, precision, L)[5]
        print("   %-52s %s" % (L["id"], _rows(ln)))
        inv += ln
    net = _net_rows(gpu, precision)
    print("   inventory %s | net %s" % (_rows(inv), _rows(net)))
    assert np.array_equal(inv, net)
