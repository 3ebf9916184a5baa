"""The non-conv operators of df-vo_amd/csrc/ops.hip at ragged maps and views: the table behind tests/test_op_cases_gpu.py
(device) and tests/test_op_cases_cpu.py (the table, its references and its bounds, without a device).  Plain data, seeded
float32 inputs and float64 references; nothing here touches the GPU.

CASES[op] is a list of dicts.  Every case has an `id`, the map (`N`, `h`, `w`), the views as the C entry point takes them
(floats per pixel and channel offsets) and, for the three dispatching launchers, the `variant` code that
dfvo_deconv_variant / dfvo_correlation_variant / dfvo_reg_head_variant must return for it (include/dfvo_hip.h):
    deconv     0 k_deconv_dw4_blk, 1 k_deconv_dw4, 2 k_deconv_dw
    corr       100 K + 10 TH + TW, K = C / 32 for k_correlation_rt<K>, 0 for k_correlation (`variant_rt0`: the code of the
               same case in a process started with DFVO_CORR_RT=0)
    reg_head   k for k_reg_head_v<k>, 0 for k_reg_head
The smallest map the product can make is 2 x 2 (FlowNet refuses images under 64 x 64; level 6 is the net size / 32).

tensors(case)            the seeded float32 operands (NCHW, logical channels only), cached
reference(case, t, ...)  the operator on them in `dtype` (float64: the anchor; float32: the CPU restatement), from the
                         references of tests/flow_world.py; `bug` names one seeded mutation of the restatement
bound(case, t, ref)      the per-element bound of tests/flow_bounds.py (None: the operator is exact)
REFUSALS                 argument sets every entry point must refuse with DFVO_ERR_ARG, naming itself

Flow categories of warp and reg_prep (`flow`): "random" sub-pixel flows of a few pixels; "integer" flows that land on pixel
centres; "edge" flows that land on column -1 / W and row -1 / H; "far" flows of 1e6 and 1e10 (x mult: beyond the int range);
"nan" a NaN in single components (torch's grid_sample and the kernel both answer NaN there, and nowhere else)."""
import functools
import zlib

import torch
import torch.nn.functional as F

import flow_bounds as B
import flow_world as FW
from oracle import nets_torch as O

OPS = ("corr", "deconv", "warp", "reg_prep", "reg_head", "mean", "resize", "maxpool")
MAPS = [(2, 2), (2, 5), (7, 9)]            # warp, reg_prep
FLOW_KINDS = ("random", "integer", "edge", "far", "nan")
FM_G = 64                                  # k_flow_mean's workgroups per sample

# ---- correlation ------------------------------------------------------------------------------------------------------
CORR_RT_C = (32, 64, 96, 128, 192)             # one per k_correlation_rt instantiation
# k_correlation: C no multiple of 32, C = 160, C > 192.  8 x 8 tiles up to C = 64, 4 x 8 up to 96, 4 x 4 above: C = 80 is
# the only way to the 4 x 8 tile in a default process (C = 96 takes it under DFVO_CORR_RT=0).  C = 352 is the last count
# whose 4 x 4 tile fits the 160 KB LDS check: (16 + 100) * 353 * 4 = 163 792 B
CORR_GEN_C = (4, 48, 80, 100, 160, 224, 352)
CORR_VARIANT = {32: 188, 64: 288, 96: 388, 128: 488, 192: 648, 4: 88, 48: 88, 80: 48, 100: 44, 160: 44, 224: 44, 352: 44}
CORR_VARIANT_RT0 = {32: 88, 64: 88, 96: 48, 128: 44, 192: 44}
CORR_MAPS = [(2, 2), (3, 2), (7, 9), (9, 17), (5, 13)]
_SWAP_N = [(0, 1), (1, 1), (0, 2), (1, 2), (0, 3), (1, 3)]


def _corr_cases():
    L, i = [], 0
    for c in CORR_RT_C + CORR_GEN_C:
        for h, w in CORR_MAPS:
            for stride in (1, 2):
                swap2, n = _SWAP_N[i % 6]
                i += 1
                L.append(dict(op="corr", id="corr_c%d_%dx%d_s%d_swap%d_n%d" % (c, h, w, stride, swap2, n), C=c, cs1=c, co1=0, cs2=c,
                              co2=0, dcs=52, N=n, h=h, w=w, stride=stride, swap2=swap2))
    # views: a 64-channel slice at offset 32 of a 128-stride buffer; different strides and offsets on the two sides; the
    # generic kernel on a slice; a destination wider than one quad behind the 49 values
    for cid, kw in [("slice32of128", dict(C=64, cs1=128, co1=32, cs2=128, co2=32, h=7, w=9, stride=1, swap2=1, N=3)),
                    ("cs1_ne_cs2", dict(C=64, cs1=64, co1=0, cs2=96, co2=16, h=9, w=17, stride=2, swap2=0, N=2)),
                    ("co1_ne_co2", dict(C=32, cs1=48, co1=16, cs2=40, co2=4, h=5, w=13, stride=1, swap2=1, N=2, dcs=56)),
                    ("generic_slice", dict(C=48, cs1=64, co1=12, cs2=52, co2=4, h=7, w=9, stride=2, swap2=1, N=3))]:
        L.append(dict(dict(op="corr", id="corr_view_" + cid, dcs=52), **kw))
    for c in L:
        c["variant"] = CORR_VARIANT[c["C"]]
        c["variant_rt0"] = CORR_VARIANT_RT0.get(c["C"], c["variant"])
        c["view"] = c["id"].startswith("corr_view_")
    return L


# ---- deconv -----------------------------------------------------------------------------------------------------------
DECONV_VARIANT = {(2, 4): 0, (49, 52): 0, (2, 8): 0, (64, 64): 0, (49, 49): 2, (3, 3): 2, (516, 516): 1}
DECONV_MAPS = [(1, 1), (2, 3), (7, 5)]


def _deconv_cases():
    L = []
    for (c, cs), v in DECONV_VARIANT.items():
        for j, (h, w) in enumerate([(2, 3)] if c == 516 else DECONV_MAPS):
            n = 1 + (j + c) % 3
            twin = "deconv_c%d_%dx%d_n%d" % (c, h, w, n)  # (C = 49 at cs 49 and 52: the same values through two kernels)
            L.append(dict(op="deconv", id="%s_cs%d" % (twin, cs), twin=twin, C=c, cs=cs, N=n, h=h, w=w, variant=v))
    return L


# ---- warp / reg_prep --------------------------------------------------------------------------------------------------
MULTS = (0.625, 1.25, 5.0)


def _warp_cases():
    L = []
    for mi, (h, w) in enumerate(MAPS):
        i = mi  # (the three maps start at different categories and views)
        for c in (4, 8, 64):
            for step in (1, 2, 3):
                swap = i % 2
                n = 3 if swap else 1 + (i // 2) % 2
                app = (i // 2) % 2
                off = (i // 3) % 2 == 0  # views with every offset non-zero: flow at fco = 2 of fcs = 4, dst at dco = 4 of C + 8
                v = dict(scs=c + 8, sco=4, fcs=4, fco=2, dcs=c + 8 + 4 * app, dco=4) if off else \
                    dict(scs=c, sco=0, fcs=2, fco=0, dcs=c + 4 * app, dco=0)
                kind = FLOW_KINDS[i % 5]
                L.append(dict(dict(op="warp", id="warp_c%d_%dx%d_step%d_swap%d_n%d_app%d_%s_%s" % (c, h, w, step, swap, n, app, kind,
                                                                                                  "off" if off else "dense"),
                                   C=c, N=n, h=h, w=w, step=step, swap=swap, append_flow=app, flow=kind, mult=MULTS[i % 3]), **v))
                i += 1
    return L


def _reg_prep_cases():
    L, i = [], 0
    for h, w in MAPS:
        for kind in FLOW_KINDS:
            n = 1 + i % 3
            fcs, fco = ((4, 2), (4, 0), (2, 0))[i % 3 if kind != "random" else 0]
            L.append(dict(op="reg_prep", id="reg_prep_%dx%d_n%d_%s_fco%dof%d" % (h, w, n, kind, fco, fcs), N=n, h=h, w=w, flow=kind,
                          fcs=fcs, fco=fco, mult=MULTS[i % 3]))
            i += 1
    return L


# ---- reg_head ---------------------------------------------------------------------------------------------------------
REG_HEAD_MAPS = [(2, 2), (3, 7), (9, 5)]   # each smaller than one kernel radius of k = 7 / 9 in at least one direction
REG_HEAD_PAIRS = {3: (12, 9), 5: (28, 25), 7: (52, 49)}  # k: (dist_cs of k_reg_head_v<k>, dist_cs of k_reg_head)


def _reg_head_cases():
    L, i = [], 0
    for k, pair in REG_HEAD_PAIRS.items():
        for h, w in REG_HEAD_MAPS:
            for steep in (0, 1):
                n = 1 + i % 3
                fcs, fco, dcs, dco = ((4, 2, 4, 2), (4, 0, 4, 0), (2, 0, 2, 0))[i % 3]
                for cs in pair:  # the same values through both strides: `twin` names the pair
                    twin = "reg_head_k%d_%dx%d_n%d_%s" % (k, h, w, n, "steep" if steep else "mild")
                    L.append(dict(op="reg_head", id="%s_cs%d" % (twin, cs), twin=twin, k=k, dist_cs=cs, N=n, h=h, w=w, steep=steep,
                                  fcs=fcs, fco=fco, dcs=dcs, dco=dco, variant=k if cs % 4 == 0 else 0))
                i += 1
    for k, cs in ((1, 4), (1, 1), (9, 84), (9, 81)):
        for j, (h, w) in enumerate(REG_HEAD_MAPS):
            twin = "reg_head_k%d_%dx%d_n%d_%s" % (k, h, w, 1 + j, "steep" if j == 1 else "mild")
            L.append(dict(op="reg_head", id="%s_cs%d" % (twin, cs), twin=twin, k=k, dist_cs=cs, N=1 + j, h=h, w=w, steep=int(j == 1),
                          fcs=4, fco=2, dcs=4, dco=2, variant=0))
    return L


# ---- flow mean, resize, max pool --------------------------------------------------------------------------------------
MEAN_HW = (1, 4, 63, 64, 65, 147, 4097)
RESIZES = [((7, 9), (3, 4)), ((3, 4), (7, 9)), ((5, 5), (1, 1)), ((1, 1), (4, 5)), ((9, 6), (9, 3))]
POOL_MAPS = [(1, 1), (2, 2), (7, 9), (8, 5)]


def _mean_cases():
    L = []
    for i, hw in enumerate(MEAN_HW):
        for n in (1, 2, 3):
            fcs, fco = ((4, 2), (2, 0), (4, 0))[(i + n) % 3] if hw != 4097 else (4, 2)
            L.append(dict(op="mean", id="mean_hw%d_n%d_fco%dof%d" % (hw, n, fco, fcs), N=n, h=hw, w=1, fcs=fcs, fco=fco))
    return L


def _resize_cases():
    L, i = [], 0
    for c in (4, 8, 12):
        for ac in (0, 1):
            for (h, w), (ho, wo) in RESIZES:
                n = 1 + i % 3
                i += 1
                L.append(dict(op="resize", id="resize_c%d_%dx%d_to_%dx%d_ac%d_n%d" % (c, h, w, ho, wo, ac, n), C=c, N=n, h=h, w=w,
                              ho=ho, wo=wo, align_corners=ac))
    return L


def _maxpool_cases():
    L, i = [], 0
    for c in (4, 8):
        for h, w in POOL_MAPS:
            n = 1 + i % 3
            i += 1
            L.append(dict(op="maxpool", id="maxpool_c%d_%dx%d_n%d" % (c, h, w, n), C=c, N=n, h=h, w=w))
    return L


CASES = {"corr": _corr_cases(), "deconv": _deconv_cases(), "warp": _warp_cases(), "reg_prep": _reg_prep_cases(),
         "reg_head": _reg_head_cases(), "mean": _mean_cases(), "resize": _resize_cases(), "maxpool": _maxpool_cases()}
ALL = [c for op in OPS for c in CASES[op]]
BY_ID = {c["id"]: c for c in ALL}
assert len(BY_ID) == len(ALL)

# what every entry point must refuse: (id, entry point, the word its message must hold)
REFUSALS = [
    dict(id="corr_c6", op="corr", name=b"correlation", C=6, cs=8),
    dict(id="corr_c356_lds", op="corr", name=b"correlation", C=356, cs=356),
    dict(id="warp_scs6", op="warp", name=b"warp", scs=6, dco=0, h=3, w=3),
    dict(id="warp_dco2", op="warp", name=b"warp", scs=4, dco=2, h=3, w=3),
    dict(id="warp_1wide", op="warp", name=b"warp", scs=4, dco=0, h=3, w=1),
    dict(id="warp_1high", op="warp", name=b"warp", scs=4, dco=0, h=1, w=3),
    dict(id="reg_prep_1wide", op="reg_prep", name=b"reg_prep", h=3, w=1),
    dict(id="reg_prep_1high", op="reg_prep", name=b"reg_prep", h=1, w=3),
    dict(id="mean_odd_fcs", op="mean", name=b"flow_mean", fcs=3),
    dict(id="resize_c6", op="resize", name=b"resize_bilinear", C=6),
]


# ---- seeded operands --------------------------------------------------------------------------------------------------
def twins(op):
    """the pairs of case ids of `op` that run the same values through two kernels"""
    by = {}
    for c in CASES[op]:
        by.setdefault(c["twin"], []).append(c["id"])
    return sorted(tuple(v) for v in by.values() if len(v) == 2)


def _gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def _flow(kind, n, h, w, mult, g):
    """[n,2,h,w] float32 flows of one category (module docstring): the displacement is flow * mult pixels"""
    f = (torch.rand(n, 2, h, w, generator=g) * 2 - 1) * 2.5 / mult
    if kind == "random":
        return f
    if kind == "integer":  # whole pixels, inside and just outside the map (mult is a power of two times 5: exact)
        return torch.randint(-2, 3, (n, 2, h, w), generator=g).float() / mult
    x = torch.arange(w, dtype=torch.float32).view(1, w).expand(h, w)
    y = torch.arange(h, dtype=torch.float32).view(h, 1).expand(h, w)
    if kind == "edge":  # alternate pixels land on column -1 / W, the rows behind them on row -1 / H
        odd = ((torch.arange(h).view(h, 1) + torch.arange(w).view(1, w)) % 2).bool()
        f[:, 0] = torch.where(odd, -1 - x, w - x) / mult
        f[:, 1] = torch.where(odd, h - y, -1 - y) / mult
        f[:, 1, 0, :] = 0.0  # (row 0: on the column alone, so that the border column's values enter)
        return f
    if kind == "far":
        f[:, 0, 0, 0] = 1e6
        f[:, 1, -1, -1] = -1e10
        f[:, 0, -1, 0] = 1e10
        return f
    if kind == "nan":
        f[:, 0, 0, 0] = float("nan")
        f[:, 1, -1, -1] = float("nan")
        return f
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def tensors(cid):
    """the float32 operands of case `cid` (NCHW, logical channels) -- computed once, never written"""
    c = BY_ID[cid]
    g = _gen(c.get("twin", cid))  # (the cases of a twin pair take the same values)
    op, n, h, w = c["op"], c["N"], c["h"], c["w"]
    t = {}
    if op == "corr":
        t["f1"] = torch.randn(n, c["C"], h, w, generator=g)
        t["f2"] = torch.randn(n, c["C"], h, w, generator=g)
    elif op == "deconv":
        t["x"] = torch.randn(n, c["C"], h, w, generator=g)
        t["w"] = torch.randn(c["C"], 1, 4, 4, generator=g) * 0.5
    elif op == "warp":
        t["src"] = torch.randn(n, c["C"], h, w, generator=g)
        t["flow"] = _flow(c["flow"], n, h, w, c["mult"], g)
    elif op == "reg_prep":
        t["img"] = torch.rand(n, 3, h, w, generator=g)
        t["flow"] = _flow(c["flow"], n, h, w, c["mult"], g)
        t["mean"] = torch.randn(n, 2, 1, 1, generator=g)
    elif op == "reg_head":
        k = c["k"]
        # steep: |dist| up to ~60, so that -dist^2 spans thousands and most of the k*k softmax weights underflow in fp32
        t["dist"] = torch.randn(n, k * k, h, w, generator=g) * (20.0 if c["steep"] else 1.0)
        t["flow"] = torch.randn(n, 2, h, w, generator=g) * 4.0
        t["wx"] = torch.randn(1, k * k, 1, 1, generator=g)
        t["wy"] = torch.randn(1, k * k, 1, 1, generator=g)
        t["bx"], t["by"] = [torch.randn(1, generator=g) * 0.1 for _ in range(2)]
    elif op == "mean":
        t["flow"] = torch.randn(n, 2, h, w, generator=g) * 3.0 + torch.tensor([1.5, -0.75]).view(1, 2, 1, 1)
    elif op == "resize":
        t["x"] = torch.randn(n, c["C"], h, w, generator=g)
    elif op == "maxpool":
        x = torch.randn(n, c["C"], h, w, generator=g)
        r = torch.rand(n, c["C"], h, w, generator=g)
        x[r < 0.15] = float("-inf")
        x[r > 0.93] = float("nan")
        x[:, 0] = float("-inf")  # a channel whose every window is -inf
        x[:, 1, 0, 0] = float("nan")  # (the smallest maps hold both kinds too)
        x[:, 2, -1, -1] = float("-inf")
        t["x"] = x
    # what a kernel that ignored a channel offset would read instead: other values of the same shape
    for k_ in ("f1", "src", "flow"):
        if k_ in t:
            t["other_" + k_] = torch.randn(t[k_].shape, generator=g) * (1.0 if k_ != "flow" else 2.0)
    return t


# ---- references -------------------------------------------------------------------------------------------------------
def maxpool_ref(x):
    """MaxPool2d(3, 2, 1) spelled out: -inf padding, the maximum of each window with NaN propagating (torch.max's rule)"""
    n, c, h, w = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    cols = F.unfold(F.pad(x.double(), (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(n, c, 9, -1)
    return cols.max(2)[0].view(n, c, ho, wo).to(x.dtype)


def reg_head_f32(dist, flow, wx, bx, wy, by, k):
    """the kernels' arithmetic restated: -dist^2, its maximum and the exponentials in fp32, the weighted mean in double"""
    r = (k - 1) // 2
    v = -dist.float().pow(2)
    e = (v - v.max(1, True)[0]).exp().double()
    out = []
    for ch, (wt, b) in enumerate(((wx, bx), (wy, by))):
        uf = F.unfold(flow[:, ch:ch + 1].double(), k, padding=r).view_as(e)
        out.append((F.conv2d(e * uf, wt.double(), b.double()) / e.sum(1, True)).float())
    return torch.cat(out, 1)


BUGS = {  # mutation -> the operators whose float32 restatement can take it
    "last_tile_row_dropped": ("corr",), "offset_ignored": ("corr", "warp", "reg_prep", "reg_head", "mean"),
    "swap_ignored": ("corr", "warp"), "divided_by_c_plus_1": ("corr",), "step2_samples_at_half": ("warp",),
    "mean_over_padded_count": ("mean",),
}


def bug_applies(case, bug):
    """whether `bug` changes what the restatement of `case` computes"""
    op = case["op"]
    if op not in BUGS[bug]:
        return False
    if bug == "last_tile_row_dropped":
        return -(-case["h"] // case["stride"]) % 2 == 1  # (the rt kernel's second row of a lane pair is the tile's last)
    if bug == "offset_ignored":
        return {"corr": case.get("co1", 0), "warp": case.get("sco", 0), "reg_prep": case.get("fco", 0),
                "reg_head": case.get("fco", 0), "mean": case.get("fco", 0)}[op] != 0
    if bug == "swap_ignored":
        return case["N"] > 1 and bool(case["swap2"] if op == "corr" else case["swap"])
    if bug == "step2_samples_at_half":
        return case["step"] == 2 and case["flow"] in ("random", "integer") and case["w"] > 2
    if bug == "mean_over_padded_count":
        return case["h"] % FM_G != 0
    return True


def reference(case, t, dtype=torch.float64, bug=None):
    """the operator of `case` on operands t in `dtype`; NCHW.  warp: every pixel (a step-k launch writes the pixels
    [::k, ::k] of it), the appended flow and zero channels behind the C warped ones"""
    op = case["op"]
    x = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in t.items()}
    if bug == "offset_ignored":
        key = {"corr": "f1", "warp": "src"}.get(op, "flow")
        x[key] = x["other_" + key]
    if op == "corr":
        y = FW.corr_ref(x["f1"], x["f2"], case["stride"], 0 if bug == "swap_ignored" else case["swap2"])
        if bug == "divided_by_c_plus_1":
            y = y * (case["C"] / (case["C"] + 1.0))
        if bug == "last_tile_row_dropped":
            y = y.clone()
            y[:, :, -1] = 0.0
        return y
    if op == "deconv":
        return FW.deconv_ref(x["x"], x["w"])
    if op == "warp":
        O._grid_cache.clear()
        y = FW.warp_ref(x["src"], x["flow"], case["mult"], 0 if bug == "swap_ignored" else case["swap"])
        if bug == "step2_samples_at_half":  # the pixel index on the stepped grid taken for the pixel: (y, x) reads (y / 2, x / 2)
            hs, ws = -(-case["h"] // 2), -(-case["w"] // 2)
            y = y.clone()
            y[:, :, ::2, ::2] = y[:, :, :hs, :ws].clone()
        if case["append_flow"]:
            y = torch.cat([y, x["flow"], torch.zeros_like(x["flow"])], 1)
        return y
    if op == "reg_prep":
        O._grid_cache.clear()
        return FW.reg_prep_ref(x["img"], x["flow"], x["mean"], case["mult"])
    if op == "reg_head":
        if dtype == torch.float32:
            return reg_head_f32(x["dist"], x["flow"], x["wx"], x["bx"], x["wy"], x["by"], case["k"])
        return FW.reg_head_ref(x["dist"], x["flow"], x["wx"], x["bx"], x["wy"], x["by"], case["k"])
    if op == "mean":
        if dtype == torch.float32:  # the kernel's arithmetic: a sum of floats in double, rounded once
            hw = case["h"] * case["w"]
            cnt = -(-hw // FM_G) * FM_G if bug == "mean_over_padded_count" else hw
            return (x["flow"].double().view(case["N"], 2, -1).sum(2) / cnt).float().view(case["N"], 2, 1, 1)
        return FW.mean_ref(x["flow"])
    if op == "resize":
        return FW.resize_ref(x["x"], (case["ho"], case["wo"]), bool(case["align_corners"]))
    if op == "maxpool":
        return maxpool_ref(x["x"])
    raise ValueError(op)


def bound(case, t, ref):
    """per-element bound of the device result against `ref` (= reference(case, t) in float64), from tests/flow_bounds.py;
    None for the exact operator (max pool).  NaN where the reference is NaN"""
    op = case["op"]
    x = {k: (v.double() if torch.is_tensor(v) else v) for k, v in t.items()}
    if "flow" in x:  # (the bounds at a NaN flow are never read: the reference is NaN there)
        x["flow"] = torch.nan_to_num(x["flow"], nan=0.0)
    if op == "corr":
        return B.corr_bound(x["f1"], x["f2"], case["stride"], case["swap2"], O.correlation)
    if op == "deconv":
        return B.deconv_bound(x["x"], x["w"])
    if op == "warp":
        b = B.warp_bound(x["src"], x["flow"], case["mult"], case["swap"])
        return torch.cat([b, torch.zeros(case["N"], 4, case["h"], case["w"], dtype=torch.float64)], 1) if case["append_flow"] else b
    if op == "reg_prep":
        O._grid_cache.clear()
        return B.reg_prep_bound(x["img"], x["flow"], x["mean"], case["mult"], ref)
    if op == "reg_head":
        return B.reg_head_bound(x["dist"], x["flow"], x["wx"], float(x["bx"]), x["wy"], float(x["by"]), case["k"], ref)
    if op == "mean":
        return B.mean_ulp(ref)
    if op == "resize":
        return B.resize_bound(x["x"], case["ho"], case["wo"], bool(case["align_corners"]))
    if op == "maxpool":
        return None
    raise ValueError(op)


def ratio(got, ref, bnd):
    """worst err / bound over the elements whose reference is a number; the NaN patterns must be the same.  An exact
    operator (bnd None) answers 0 for bit-equality and inf otherwise"""
    nan = torch.isnan(ref)
    if not torch.equal(torch.isnan(got), nan):
        return float("inf")
    if bnd is None:
        same = torch.equal(torch.nan_to_num(got.double(), nan=0.0), torch.nan_to_num(ref.double(), nan=0.0))
        return 0.0 if same else float("inf")
    err = (got.double() - ref).abs()[~nan]
    b = bnd[~nan]
    if err.numel() == 0:
        return 0.0
    if bool(torch.isnan(b).any()):
        return float("inf")
    r = torch.where(err == 0, torch.zeros_like(err), err / b)  # (a zero bound admits only zero error)
    return float(r.max())
