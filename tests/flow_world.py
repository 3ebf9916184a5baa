"""The flow net's launch inventory and its float64 walk, for the per-layer and per-operator tests.

FLOW_LAYERS lists every launch of FlowNet::enqueue_input, enqueue_features and enqueue_levels (df-vo_amd/csrc/nets.hip) in
launch order.  The image input, the image pyramid and the feature convolutions are listed once per frame at N=1 (`frame`
0 = ref, 1 = cur), as enqueue_features_both launches them; the level launches run at N=2, sample 0 = ref, sample 1 = cur,
"the second image" being the other sample (`swap`).  Each entry names its operands as the net passes them:

  conv      weight prefix, source view(s) (channels, floats per pixel, channel offset), residual, activation, (kh, kw),
            padding, output floats per pixel and dst_zero_to (the distance convolutions pad k*k to kkp = round_up(k*k, 4))
  input     launch_img_u8_to_flow_input of one frame
  resize    launch_resize_bilinear (align_corners=False), one pyramid step of one frame
  deconv    launch_deconv_dw (depthwise 4x4, stride 2, pad 1) with its weight and view
  warp      launch_warp: swap, step, append_flow, mult = kDbl[l]
  corr      launch_correlation: swap2, stride, channel views
  mean      launch_flow_mean
  reg_prep  launch_reg_prep: mult = kDbl[l]
  reg_head  launch_reg_head: k, the moduleScaleX / Y weights
  post      launch_flow_post (k_flow_resize + k_flow_consistency), scale 10

activations(sd, ref, cur, dtype) walks the list with the oracle's own primitives (oracle/nets_torch.py) and records every
input and output (NCHW; a view's logical channels only).  In float64 its raw level flows and its fwd / bwd / diff equal
oracle.nets_torch.flow_inference(..., dtype=float64, return_levels=True) bit for bit: torch's float64 convolution adds in
the same order at batch 1 as at batch 2 (tests/test_flow_world_cpu.py checks it)."""
import functools
import importlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets_torch as O
from synth import image_pair

KDBL = O.DBL
KER = O.KER
FEAT_C = [0, 32, 32, 64, 96, 128, 192]
WORLDS = ("random", "tunnel")


def _feature_layers(frame):
    # (name, cin, stride, pad, level of the input map, source, output, output floats per pixel)
    fcs = [("moduleOne.0", 3, 1, 3, 1, "img1", "feat1", 32), ("moduleTwo.0", 32, 2, 1, 1, "feat1", "f.two0", 32),
           ("moduleTwo.2", 32, 1, 1, 2, "f.two0", "f.two2", 32), ("moduleTwo.4", 32, 1, 1, 2, "f.two2", "feat2", 32),
           ("moduleThr.0", 32, 2, 1, 2, "feat2", "f.thr0", 64), ("moduleThr.2", 64, 1, 1, 3, "f.thr0", "feat3", 64),
           ("moduleFou.0", 64, 2, 1, 3, "feat3", "f.fou0", 96), ("moduleFou.2", 96, 1, 1, 4, "f.fou0", "feat4", 96),
           ("moduleFiv.0", 96, 2, 1, 4, "feat4", "feat5", 128), ("moduleSix.0", 128, 2, 1, 5, "feat5", "feat6", 192)]
    L = [dict(op="resize", frame=frame, src="img%d" % (l - 1), out="img%d" % l, level=l) for l in range(2, 7)]
    for name, cin, stride, pad, lin, src, out, ocs in fcs:
        k = 7 if name == "moduleOne.0" else 3
        L.append(conv("moduleFeatures." + name, src, cin, 4 if src == "img1" else cin, out, ocs, k, k, pad, pad, "leaky",
                      stride=stride, frame=frame, level=lin))
    return L


def conv(name, src, c0, cs0, out, dst_cs, kh, kw, ph, pw, act, stride=1, frame=None, level=None, src1=None, c1=0, cs1=0,
         res=None, dst_zero_to=0, cout=None):
    return dict(op="conv", name=name, src=src, c0=c0, cs0=cs0, src1=src1, c1=c1, cs1=cs1, res=res, out=out, dst_cs=dst_cs,
                kh=kh, kw=kw, pad=(ph, pw), stride=stride, act=act, frame=frame, level=level, dst_zero_to=dst_zero_to)


def _level_layers(l):
    k, C = KER[l], FEAT_C[l]
    r, kkp = (k - 1) // 2, (k * k + 3) // 4 * 4
    Cm = 64 if l == 2 else C
    Cr = 128 if l < 5 else C
    stride = 2 if l < 4 else 1
    P = "L%d." % l
    mm, sm, rm = ("moduleMatching.%d." % (l - 2), "moduleSubpixel.%d." % (l - 2), "moduleRegularization.%d." % (l - 2))
    L = []
    mf = sf = "feat%d" % l
    if l == 2:
        L.append(conv(mm + "moduleFeat.0", mf, C, C, P + "mfeat", 64, 1, 1, 0, 0, "leaky", level=l))
        L.append(conv(sm + "moduleFeat.0", sf, C, C, P + "sfeat", 64, 1, 1, 0, 0, "leaky", level=l))
        mf, sf = P + "mfeat", P + "sfeat"
    flow_up = None
    if l < 6:
        flow_up = P + "flow_up"
        L.append(dict(op="deconv", w=mm + "moduleUpflow.weight", src="L%d.flow" % (l + 1), C=2, cs=4, out=flow_up, level=l))
        L.append(dict(op="warp", src=mf, C=Cm, scs=Cm, swap=1, flow=flow_up, mult=KDBL[l], step=stride, append_flow=0,
                      dcs=Cm, out=P + "warped", level=l))
        L.append(dict(op="corr", src1=mf, cs1=Cm, src2=P + "warped", cs2=Cm, swap2=0, C=Cm, stride=stride, out=P + "corr",
                      level=l))
    else:
        L.append(dict(op="corr", src1=mf, cs1=Cm, src2=mf, cs2=Cm, swap2=1, C=Cm, stride=stride, out=P + "corr", level=l))
    corr = P + "corr"
    if l < 4:
        L.append(dict(op="deconv", w=mm + "moduleUpcorr.weight", src=corr, C=49, cs=52, out=P + "corr_up", level=l))
        corr = P + "corr_up"
    L.append(conv(mm + "moduleMain.0", corr, 49, 52, P + "m0", 128, 3, 3, 1, 1, "leaky", level=l))
    L.append(conv(mm + "moduleMain.2", P + "m0", 128, 128, P + "m2", 64, 3, 3, 1, 1, "leaky", level=l))
    L.append(conv(mm + "moduleMain.4", P + "m2", 64, 64, P + "m4", 32, 3, 3, 1, 1, "leaky", level=l))
    L.append(conv(mm + "moduleMain.6", P + "m4", 32, 32, P + "flowM", 4, k, k, r, r, "none", level=l, res=flow_up))
    L.append(dict(op="warp", src=sf, C=Cm, scs=Cm, swap=1, flow=P + "flowM", mult=KDBL[l], step=1, append_flow=1,
                  dcs=Cm + 4, out=P + "b1", level=l))
    L.append(conv(sm + "moduleMain.0", sf, Cm, Cm, P + "s0", 128, 3, 3, 1, 1, "leaky", level=l, src1=P + "b1", c1=Cm + 2,
                  cs1=Cm + 4))
    L.append(conv(sm + "moduleMain.2", P + "s0", 128, 128, P + "s2", 64, 3, 3, 1, 1, "leaky", level=l))
    L.append(conv(sm + "moduleMain.4", P + "s2", 64, 64, P + "s4", 32, 3, 3, 1, 1, "leaky", level=l))
    L.append(conv(sm + "moduleMain.6", P + "s4", 32, 32, P + "flowS", 4, k, k, r, r, "none", level=l, res=P + "flowM"))
    L.append(dict(op="mean", src=P + "flowS", out=P + "mean", level=l))
    L.append(dict(op="reg_prep", img="img%d" % l, flow=P + "flowS", mean=P + "mean", mult=KDBL[l], out=P + "r0", level=l))
    rf, rcs = "feat%d" % l, C
    if l < 5:
        L.append(conv(rm + "moduleFeat.0", rf, C, C, P + "rfeat", 128, 1, 1, 0, 0, "leaky", level=l))
        rf, rcs = P + "rfeat", 128
    L.append(conv(rm + "moduleMain.0", P + "r0", 3, 4, P + "x0", 128, 3, 3, 1, 1, "leaky", level=l, src1=rf, c1=Cr, cs1=rcs))
    chans = [128, 128, 64, 64, 32, 32]
    for i in range(1, 6):
        L.append(conv(rm + "moduleMain.%d" % (2 * i), P + "x%d" % (i - 1), chans[i - 1], chans[i - 1], P + "x%d" % i,
                      chans[i], 3, 3, 1, 1, "leaky", level=l))
    if l < 5:
        L.append(conv(rm + "moduleDist.0", P + "x5", 32, 32, P + "dist_a", kkp, k, 1, r, 0, "none", level=l, dst_zero_to=kkp))
        L.append(conv(rm + "moduleDist.1", P + "dist_a", k * k, kkp, P + "dist_b", kkp, 1, k, 0, r, "none", level=l,
                      dst_zero_to=kkp))
        dist = P + "dist_b"
    else:
        L.append(conv(rm + "moduleDist.0", P + "x5", 32, 32, P + "dist_a", kkp, k, k, r, r, "none", level=l, dst_zero_to=kkp))
        dist = P + "dist_a"
    L.append(dict(op="reg_head", dist=dist, dist_cs=kkp, k=k, flow=P + "flowS", wx=rm + "moduleScaleX", wy=rm + "moduleScaleY",
                  out=P + "flow", level=l))
    return L


def _layers():
    L = [dict(op="input", frame=f, out="img1", level=1) for f in (0, 1)]
    for f in (0, 1):
        L += _feature_layers(f)
    for l in range(6, 1, -1):
        L += _level_layers(l)
    L.append(dict(op="post", src="L2.flow", scale=10.0, out="post", level=2))
    for i, d in enumerate(L):
        d.setdefault("frame", None)
        d["id"] = "%02d.%s.%s%s" % (i, d["op"], d.get("name", d["out"]), "" if d["frame"] is None else ".f%d" % d["frame"])
    return L


FLOW_LAYERS = _layers()


# ---- the operators, as the oracle states them (float64 anchor, or any dtype) ------------------------------------------
def lrelu(x):
    return F.leaky_relu(x, 0.1)


def conv_ref(L, x, w, b):
    return F.conv2d(x, w, b, stride=L["stride"], padding=L["pad"] if L["pad"][0] != L["pad"][1] else L["pad"][0])


def net_input(u8, th, tw, dtype=torch.float64):
    """flow_inference's input: float32(u8 / 255) widened, bilinear (align_corners=True) to the net size"""
    x = torch.from_numpy(np.transpose(u8 / 255, (2, 0, 1))).unsqueeze(0).float().to(dtype)
    return F.interpolate(x, (th, tw), mode="bilinear", align_corners=True)


def resize_ref(x, size, align_corners=False):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=align_corners)


def deconv_ref(x, w):
    return F.conv_transpose2d(x, w, None, stride=2, padding=1, groups=x.shape[1])


def warp_ref(src, flow, mult, swap):
    """Backward() of the other sample (swap) or the same one at (x, y) + flow * mult"""
    return O.backward_warp(src.flip(0) if swap else src, flow * mult)


def corr_ref(f1, f2, stride, swap2):
    return lrelu(O.correlation(f1, f2.flip(0) if swap2 else f2, stride))


def mean_ref(flow):
    return flow.view(flow.size(0), 2, -1).mean(2, True).view(flow.size(0), 2, 1, 1)


def reg_prep_ref(img, flow, mean, mult):
    """(brightness error, flow - mean): the first three channels of the regularisation input"""
    diff = img - O.backward_warp(img.flip(0), flow * mult)
    diff = (diff.pow(2.0).sum(1, True) + 1e-6).sqrt()
    return torch.cat([diff, flow - mean], 1)


def reg_head_ref(dist, flow, wx, bx, wy, by, k):
    r = (k - 1) // 2
    dist = dist.pow(2.0).neg()
    dist = (dist - dist.max(1, True)[0]).exp()
    div = dist.sum(1, True).reciprocal()
    sx = F.conv2d(dist * F.unfold(flow[:, 0:1], k, stride=1, padding=r).view_as(dist), wx, bx) * div
    sy = F.conv2d(dist * F.unfold(flow[:, 1:2], k, stride=1, padding=r).view_as(dist), wy, by) * div
    return torch.cat([sx, sy], 1)


def post_resize_ref(flow, scale, H, W):
    """flows[1] = raw[2] * 10, resize_dense_flow: (fwd, bwd) [1,2,H,W] each"""
    f = O.resize_dense_flow(flow * scale, H, W)
    return f[0:1], f[1:2]


def consistency_ref(fwd, bwd):
    return O.forward_backward_consistency(fwd, bwd, O.flow_to_pix(fwd))


def _cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()} if any(v.dtype != dtype for v in sd.values()) else sd


def run_op(L, sd, acts):
    """the output of entry L from the recorded activations (every operand in their dtype)"""
    op = L["op"]
    if op == "conv":
        x = acts[L["src"]]
        if L["frame"] is not None:
            x = x[L["frame"]:L["frame"] + 1]
        if L["src1"]:
            x = torch.cat([x, acts[L["src1"]]], 1)
        y = conv_ref(L, x, sd[L["name"] + ".weight"], sd[L["name"] + ".bias"])
        if L["res"]:
            y = acts[L["res"]] + y
        return lrelu(y) if L["act"] == "leaky" else y
    if op == "resize":
        f = L["frame"]
        x = acts[L["src"]][f:f + 1]
        return resize_ref(x, (x.shape[2] // 2, x.shape[3] // 2))
    if op == "deconv":
        return deconv_ref(acts[L["src"]], sd[L["w"]])
    if op == "warp":
        y = warp_ref(acts[L["src"]], acts[L["flow"]], L["mult"], L["swap"])
        return torch.cat([y, acts[L["flow"]]], 1) if L["append_flow"] else y
    if op == "corr":
        return corr_ref(acts[L["src1"]], acts[L["src2"]], L["stride"], L["swap2"])
    if op == "mean":
        return mean_ref(acts[L["src"]])
    if op == "reg_prep":
        return reg_prep_ref(acts[L["img"]], acts[L["flow"]], acts[L["mean"]], L["mult"])
    if op == "reg_head":
        return reg_head_ref(acts[L["dist"]], acts[L["flow"]], sd[L["wx"] + ".weight"], sd[L["wx"] + ".bias"],
                            sd[L["wy"] + ".weight"], sd[L["wy"] + ".bias"], L["k"])
    raise ValueError(op)


def activations(sd, ref, cur, dtype=torch.float64):
    """every input and output of FLOW_LAYERS: {"img1".."img6", "feat1".."feat6", "L<l>.<name>", "fwd", "bwd", "diff"}.
    Per-frame entries fill sample `frame` of a batch-2 activation."""
    sd = _cast(sd, dtype)
    h, w = ref.shape[:2]
    th, tw = O.get_target_size(h, w)
    O._grid_cache.clear()
    acts = {}
    frames = {}
    for L in FLOW_LAYERS:
        op, f = L["op"], L["frame"]
        if op == "input":
            y = net_input(ref if f == 0 else cur, th, tw, dtype)
        elif op == "post":
            fwd, bwd = post_resize_ref(acts[L["src"]], L["scale"], h, w)
            acts["fwd"], acts["bwd"], acts["diff"] = fwd, bwd, consistency_ref(fwd, bwd)
            continue
        else:
            y = run_op(L, sd, acts)
        if f is None:
            acts[L["out"]] = y
        else:
            frames.setdefault(L["out"], [None, None])[f] = y
            if f == 1:
                acts[L["out"]] = torch.cat(frames[L["out"]], 0)
            elif L["out"] not in acts:
                acts[L["out"]] = y  # frame 0 alone until frame 1 arrives (the frame-0 chain reads only sample 0)
    O._grid_cache.clear()
    return acts


@functools.lru_cache(maxsize=2)
def world(name):
    """(state dict, ref u8, cur u8) of the two worlds: the seeded random net on image_pair(192, 640) (net size 224x672) and
    the coded tunnel with the crafted net (256x640, flows of 10-27 px that carry samples across the zero-padding border)"""
    if name == "random":
        ref, cur = image_pair(192, 640, seed=1193)
        return O.liteflownet_state_dict(4869), ref, cur
    syn = importlib.import_module("df-vo_amd.synthetic")
    seq = syn.coded_tunnel_sequence(256, 640, 3, mode="mux", step=1.0, seed=21)
    return syn.crafted_liteflownet_state_dict(256, 640, "mux"), seq["frames"][1], seq["frames"][2]


@functools.lru_cache(maxsize=2)
def walk64(name):
    """the float64 walk of a world (cached: ~10 s)"""
    sd, ref, cur = world(name)
    return activations(sd, ref, cur, torch.float64)
