"""Every instantiation launch_conv can reach, on one ragged layer each, against float64 -- tests/conv_variants.py holds the table.

One test per (case, packing).  A case runs dfvo_conv2d once under the per-launch profile and asserts:
  (a) the profile's variant tag of the single launch is the case's declared one (a retuned dispatch rule fails here instead
      of silently testing another kernel);
  (b) every output element is within tests/layer_bounds.py's derived bound of the float64 convolution of the same fp32
      operands (the head kernels: the fp32 bound in every packing; the two Winograd cases: tests/wino_bounds.py's), and no
      f16 range event was counted;
  (c) the writes stay inside the destination view: the destination lies inside a larger buffer of sentinels, and afterwards
      the bands before and behind it and every channel outside [dst_co, dst_co + max(cout, dst_zero_to)) still hold the
      sentinel, nothing else does, and channels [cout, dst_zero_to) are exactly 0;
  (d) nothing outside the source and residual views enters a result: both sources and the residual lie inside buffers whose
      bands and out-of-view channels hold NaN (the pad channels of a source's last group of four hold 0: the nets' contract),
      and the output is finite.
test_the_nets_run_only_covered_variants is the counterpart of the two row-level inventory tests at variant granularity, at
the workload's own sizes.  The last test prints, per variant tag, the cases that reached it and their worst err / bound."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_variants as V
from layer_bounds import conv_bound
from wino_bounds import wino_bound

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
BAND = 64  # floats in front of and behind every view (a multiple of 4: the views keep their 16-byte alignment)
_operands = {}  # the operands and references of the case under test (one case at a time: the big maps are 100s of MB)
_seen = {}      # profile tag -> [(case id, packing, worst err / bound)]

PARAMS = [(c["id"], p) for c in V.CASES for p in V.PRECISIONS if p in c["tags"]]


def _tensors(case):
    if _operands.get("id") != case["id"]:
        _operands.clear()
        g = torch.Generator().manual_seed(sum(map(ord, case["id"])))
        H, W, ho, wo = V.out_size(case)
        cin = case["c0"] + case["c1"]
        x0 = torch.randn(case["N"], case["c0"], case["h"], case["w"], generator=g)  # (different data in every sample)
        x1 = torch.randn(case["N"], case["c1"], H, W, generator=g) if case["c1"] else None
        w = torch.randn(case["cout"], cin, case["kh"], case["kw"], generator=g) / np.sqrt(cin * case["kh"] * case["kw"])
        b = torch.randn(case["cout"], generator=g) * 0.1
        res = torch.randn(case["N"], case["cout"], ho, wo, generator=g) if case["res"] else None
        _operands.update(id=case["id"], x0=x0, x1=x1, w=w, b=b, res=res, ref={})
    return _operands


def _conv64(case):
    ph, pw = case["pad"]

    def conv(x, w, b):
        if case["pad_mode"] == 1:
            return F.conv2d(F.pad(x, (pw, pw, ph, ph), mode="reflect"), w, b, stride=case["stride"])
        return F.conv2d(x, w, b, stride=case["stride"], padding=(ph, pw))
    return conv


def _reference(case, precision):
    """(float64 reference after the activation, per-output bound): computed once per case and arithmetic"""
    t = _tensors(case)
    exact = V.family_of(case["tags"][precision]) == "head"
    key = "fp32" if exact else precision
    if key not in t["ref"]:
        xin = F.interpolate(t["x0"], scale_factor=2, mode="nearest") if case["up0"] else t["x0"]
        if t["x1"] is not None:
            xin = torch.cat([xin, t["x1"]], 1)
        if case["wino"]:
            y, bound = wino_bound(xin, t["w"], t["b"], t["res"])
        else:
            _, _, y, bound = conv_bound(_conv64(case), xin.double(), t["w"].double(), t["b"].double(),
                                        t["res"].double() if t["res"] is not None else None, precision, exact_fp32=exact)
        a = case["act_param"]
        ref = {0: lambda v: v, 1: lambda v: F.leaky_relu(v, a), 2: F.relu, 3: lambda v: F.elu(v, a), 4: torch.sigmoid}[case["act"]](y)
        t["ref"][key] = ref, bound
    return t["ref"][key]


def _banded(x, cs, co, fill):
    """NCHW x as a view (cs floats per pixel, channel offset co) of a device buffer that holds `fill` everywhere else; the
    pad channels of the last group of four hold 0.  Returns (buffer, pointer to the view's first pixel)"""
    n, c, h, w = x.shape
    inner = torch.full((n, h, w, cs), fill, dtype=torch.float32)
    inner[..., co:co + (c + 3) // 4 * 4] = 0.0
    inner[..., co:co + c] = x.permute(0, 2, 3, 1)
    buf = torch.full((2 * BAND + inner.numel(),), fill, dtype=torch.float32)
    buf[BAND:BAND + inner.numel()] = inner.reshape(-1)
    buf = buf.cuda()
    return buf, C.c_void_p(buf.data_ptr() + 4 * BAND)


def _profile_tags(path):
    """the variant column of the launches in a DFVO_CONV_PROFILE_CSV file (the tag holds commas: it is the last column)"""
    lines = [ln for ln in path.read_text().splitlines() if ln and not ln.startswith("cfg,")]
    return [ln.split(",", 15)[15] for ln in lines]


def _run(gpu, case, precision, csv):
    lib = gpu.lib()
    t = _tensors(case)
    v = case["view"]
    H, W, ho, wo = V.out_size(case)
    nan = float("nan")
    b0, p0 = _banded(t["x0"], v["cs0"], v["co0"], nan)
    b1, p1 = _banded(t["x1"], v["cs1"], v["co1"], nan) if t["x1"] is not None else (None, None)
    # (the residual's view is [res_co, res_co + cout): no pad channels of its own)
    br, pr = (None, None)
    if t["res"] is not None:
        inner = torch.full((case["N"], ho, wo, v["res_cs"]), nan)
        inner[..., v["res_co"]:v["res_co"] + case["cout"]] = t["res"].permute(0, 2, 3, 1)
        br = torch.full((2 * BAND + inner.numel(),), nan)
        br[BAND:BAND + inner.numel()] = inner.reshape(-1)
        br = br.cuda()
        pr = C.c_void_p(br.data_ptr() + 4 * BAND)
    n_dst = case["N"] * ho * wo * v["dst_cs"]
    dst = torch.full((2 * BAND + n_dst,), SENTINEL, device="cuda")
    desc = gpu.ConvDesc(N=case["N"], H=H, W=W, kh=case["kh"], kw=case["kw"], stride=case["stride"], pad_h=case["pad"][0],
                        pad_w=case["pad"][1], pad_mode=case["pad_mode"], c0=case["c0"], cs0=v["cs0"], co0=v["co0"], up0=case["up0"],
                        c1=case["c1"], cs1=v["cs1"] if case["c1"] else 0, co1=v["co1"] if case["c1"] else 0, cout=case["cout"],
                        act=case["act"], act_param=case["act_param"], res_cs=v["res_cs"] if case["res"] else 0,
                        res_co=v["res_co"] if case["res"] else 0, dst_cs=v["dst_cs"], dst_co=v["dst_co"], dst_zero_to=case["zero_to"])
    wn, bn = np.ascontiguousarray(t["w"].numpy()), np.ascontiguousarray(t["b"].numpy())
    ms, fl, ln = np.zeros(24), np.zeros(24), np.zeros(24, np.int32)
    gpu.check(lib.dfvo_set_conv_precision(precision.encode()))
    if case["wino"]:
        gpu.check(lib.dfvo_set_fp32_winograd(2))
    gpu.f16s_overflow_count(reset=True)
    try:
        gpu.check(lib.dfvo_conv_profile_begin())
        try:
            gpu.check(lib.dfvo_conv2d(C.byref(desc), p0, p1, gpu.as_ptr(wn), gpu.as_ptr(bn), pr, C.c_void_p(dst.data_ptr() + 4 * BAND),
                                      None))
            torch.cuda.synchronize()
        finally:
            gpu.check(lib.dfvo_conv_profile_end(gpu.as_ptr(ms), gpu.as_ptr(fl), gpu.as_ptr(ln)))
    finally:
        if case["wino"]:
            gpu.check(lib.dfvo_set_fp32_winograd(0))
        gpu.check(lib.dfvo_set_conv_precision(b"fp32"))
        n_ovf = gpu.f16s_overflow_count(reset=True)
    host = dst.cpu()
    return _profile_tags(csv), n_ovf, host[:BAND], host[BAND + n_dst:], host[BAND:BAND + n_dst].view(case["N"], ho, wo, v["dst_cs"])


@pytest.mark.parametrize("cid,precision", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_conv_variant(gpu, monkeypatch, tmp_path, cid, precision):
    case = next(c for c in V.CASES if c["id"] == cid)
    csv = tmp_path / "conv_profile.csv"
    monkeypatch.setenv("DFVO_CONV_PROFILE_CSV", str(csv))
    tags, n_ovf, front, back, out = _run(gpu, case, precision, csv)
    want = V.profile_tag(case, precision)
    # (a) the instantiation
    assert tags == [want], "%s %s: the dispatcher ran %s, the case declares %s" % (cid, precision, tags, want)
    assert n_ovf == 0, "%s %s: %d f16 range events" % (cid, precision, n_ovf)
    # (c) the writes
    v, cout = case["view"], case["cout"]
    lo, hi, end = v["dst_co"], v["dst_co"] + cout, v["dst_co"] + max(cout, case["zero_to"])
    assert bool((front == SENTINEL).all()) and bool((back == SENTINEL).all()), "%s %s: wrote outside the destination buffer" % (cid, precision)
    assert bool((out[..., :lo] == SENTINEL).all()) and bool((out[..., end:] == SENTINEL).all()), \
        "%s %s: wrote outside channels [%d, %d) of the destination view" % (cid, precision, lo, end)
    assert bool((out[..., hi:end] == 0).all()), "%s %s: channels [cout, dst_zero_to) not zeroed" % (cid, precision)
    got = out[..., lo:hi].permute(0, 3, 1, 2)
    assert not bool((got == SENTINEL).any()), "%s %s: output elements never written" % (cid, precision)
    # (d) and (b)
    assert bool(torch.isfinite(got).all()), "%s %s: an out-of-view value (NaN) entered a result" % (cid, precision)
    ref, bound = _reference(case, precision)
    assert got.shape == ref.shape
    err = (got.double() - ref).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    print("   %-34s %-5s %-30s max|ref| %.2e  max err %.2e  worst err / bound %.3f"
          % (cid, precision, want, float(ref.abs().max()), float(err.max()), ratio))
    _seen.setdefault(want, []).append((cid, precision, ratio))
    assert bool((err <= bound).all()), "%s %s %s: worst err / bound %.3f" % (cid, precision, want, ratio)


# ---- the nets at the workload's sizes, at variant granularity ---------------------------------------------------------------
def _covered(precision):
    return {V.profile_tag(c, precision) for c in V.CASES if precision in c["tags"] and not c["wino"]}


def _flow_tags(gpu, precision, h, w, csv):
    import flow_world as FW
    from synth import image_pair
    from test_nets_gpu import make_flownet
    lib = gpu.lib()
    sd = FW.world("random")[0]
    ref, cur = image_pair(h, w, seed=1193)
    gpu.check(lib.dfvo_set_conv_precision(precision.encode()))
    try:
        net, _, _ = make_flownet(gpu, h, w, sd)
    finally:
        gpu.check(lib.dfvo_set_conv_precision(b"fp32"))
    fwd, bwd, diff = np.zeros((2, h, w), np.float32), np.zeros((2, h, w), np.float32), np.zeros((h, w), np.float32)
    args = [gpu.as_ptr(a) for a in (ref, cur, fwd, bwd, diff)]
    ms, fl, ln = np.zeros(24), np.zeros(24), np.zeros(24, np.int32)
    try:
        gpu.check(lib.dfvo_conv_profile_begin())
        try:
            gpu.check(lib.dfvo_flownet_forward_host(net, *args))
        finally:
            gpu.check(lib.dfvo_conv_profile_end(gpu.as_ptr(ms), gpu.as_ptr(fl), gpu.as_ptr(ln)))
    finally:
        lib.dfvo_flownet_destroy(net)
    return set(_profile_tags(csv))


def _depth_tags(gpu, precision, h, w, csv):
    import depth_world as DW
    from synth import image_pair
    lib = gpu.lib()
    sd = DW.calibrated_monodepth2_state_dict(4869, h, w)
    img, _ = image_pair(h, w, seed=55)
    net = C.c_void_p()
    gpu.check(lib.dfvo_set_conv_precision(precision.encode()))
    try:
        gpu.check(lib.dfvo_depthnet_create(h, w, 0.1, 100.0, 5.4, None, C.byref(net)))
        gpu.set_params(lib.dfvo_depthnet_set_param, net, {k: t.numpy() for k, t in sd.items()})
        gpu.check(lib.dfvo_depthnet_finalize(net))
    finally:
        gpu.check(lib.dfvo_set_conv_precision(b"fp32"))
    depth = np.zeros((h, w), np.float32)
    ms, fl, ln = np.zeros(24), np.zeros(24), np.zeros(24, np.int32)
    try:
        gpu.check(lib.dfvo_depthnet_set_graph(net, 0))
        gpu.check(lib.dfvo_conv_profile_begin())
        try:
            gpu.check(lib.dfvo_depthnet_forward_host(net, gpu.as_ptr(img), gpu.as_ptr(depth)))
        finally:
            gpu.check(lib.dfvo_conv_profile_end(gpu.as_ptr(ms), gpu.as_ptr(fl), gpu.as_ptr(ln)))
    finally:
        lib.dfvo_depthnet_destroy(net)
    return set(_profile_tags(csv))


# the flagship size, the depth net's feed size, and the two large benchmark configurations (1280x960, 1920x1280)
NET_RUNS = [("flow", 376, 1241), ("flow", 192, 640), ("depth", 192, 640), ("flow", 960, 1280), ("flow", 1280, 1920)]


@pytest.mark.parametrize("precision", V.PRECISIONS)
@pytest.mark.parametrize("net,h,w", NET_RUNS, ids=["%s_%dx%d" % r for r in NET_RUNS])
def test_the_nets_run_only_covered_variants(gpu, monkeypatch, tmp_path, net, h, w, precision):
    """one forward (graphs off) of the net at a workload size: every variant tag its conv launches record has a case above in
    that packing -- no instantiation runs in the workload that is only seen through whole-net tolerances"""
    csv = tmp_path / "conv_profile.csv"
    monkeypatch.setenv("DFVO_CONV_PROFILE_CSV", str(csv))
    gpu.f16s_overflow_count(reset=True)
    tags = (_flow_tags if net == "flow" else _depth_tags)(gpu, precision, h, w, csv)
    assert gpu.f16s_overflow_count(reset=True) == 0
    covered = _covered(precision)
    print("\n   %s net %dx%d %s runs: %s" % (net, h, w, precision, "  ".join(sorted(tags))))
    print("   covered by cases in %s: %s" % (precision, "  ".join(sorted(covered))))
    assert tags, "no conv launch was profiled"
    assert tags <= covered, "%s net %dx%d %s runs variants without a case: %s" % (net, h, w, precision, sorted(tags - covered))


def test_report_of_the_variants_reached():
    """the per-variant report of this run (pytest -s): tag, the cases that reached it, their worst err / bound"""
    print("\n   variant tag -> case (packing) worst err / bound")
    for tag in sorted(_seen):
        print("   %-30s %s" % (tag, "  ".join("%s (%s) %.3f" % r for r in _seen[tag])))
