"""A well-conditioned monodepth2 world for the depth net's accuracy tests, and the net's layer inventory.

monodepth2_state_dict's batch-norm statistics are near identity (every folded scale ~1) and its sigmoid head saturates:
on a 192x640 frame the median disparity is 0.9985, so the depth sits at min_depth and barely responds to any layer above
it.  calibrated_monodepth2_state_dict starts from the same weights and gives them what a trained encoder has:

  * conv filters whose norms differ per output channel by 10^U(-1.5, 1.5) (every conv that feeds a batch norm);
  * batch-norm statistics measured on a calibration frame (image_pair(h, w, seed=999), never a test frame) in float64,
    layer by layer: running_mean = channel mean + 0.1 std noise, running_var = channel variance x 10^U(-0.3, 0.3),
    gamma ~ U(0.2, 2), beta ~ U(-0.5, 0.5); the walk continues with the activations those statistics normalise;
  * one dead filter (zero weights, running_var 0, mean 0: folded scale gamma / sqrt(1e-5)) and one near-dead channel
    (gamma 1e-3: folded weights in f16's subnormal range);
  * a head rescaled so that its logits on the calibration frame have mean 0 and std 1.5 (>= 90 % of the disparities in
    [0.02, 0.98]).

DEPTH_LAYERS lists every convolution of DepthNet::enqueue (df-vo_amd/csrc/nets.hip) in launch order; activations()
walks it, with the unfolded batch norm, and equals oracle/nets_torch.depth_decoder's scale-0 disparity."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets_torch as O
from synth import image_pair

DEAD = ("encoder.layer1.0.conv1", "encoder.layer1.0.bn1", 5)   # conv, its batch norm, channel
NEAR_DEAD = ("encoder.layer4.1.bn1", 7, 1e-3)                  # batch norm, channel, gamma
HEAD_LOGIT_STD = 1.5
CALIBRATION_SEED = 999


def _layers():
    L = [dict(name="encoder.conv1", bn="encoder.bn1", k=7, stride=2, pad=3, act="relu", src="input", out="stem")]
    prev = "pool"
    for li in range(1, 5):
        for b in range(2):
            p = "encoder.layer%d.%d" % (li, b)
            s = 2 if (li > 1 and b == 0) else 1
            L.append(dict(name=p + ".conv1", bn=p + ".bn1", k=3, stride=s, pad=1, act="relu", src=prev, out=p + ".conv1"))
            res = prev
            if s == 2:
                L.append(dict(name=p + ".downsample.0", bn=p + ".downsample.1", k=1, stride=2, pad=0, act="none", src=prev,
                              out=p + ".downsample"))
                res = p + ".downsample"
            L.append(dict(name=p + ".conv2", bn=p + ".bn2", k=3, stride=1, pad=1, act="relu", src=p + ".conv1", res=res,
                          out=p))
            prev = p
    feats = ["stem"] + ["encoder.layer%d.1" % li for li in range(1, 5)]
    cur = feats[4]
    for i in range(4, -1, -1):
        i0, i1 = (4 - i) * 2, (4 - i) * 2 + 1
        L.append(dict(name="decoder.%d.conv.conv" % i0, k=3, stride=1, pad=1, reflect=1, act="elu", src=cur,
                      out="decoder.%d" % i0))
        L.append(dict(name="decoder.%d.conv.conv" % i1, k=3, stride=1, pad=1, reflect=1, act="elu", src="decoder.%d" % i0,
                      up0=1, skip=feats[i - 1] if i > 0 else None, out="decoder.%d" % i1))
        cur = "decoder.%d" % i1
    L.append(dict(name="decoder.10.conv", k=3, stride=1, pad=1, reflect=1, act="sigmoid", src=cur, out="disp"))
    for d in L:
        d.setdefault("bn", None)
        d.setdefault("reflect", 0)
        d.setdefault("up0", 0)
        d.setdefault("skip", None)
        d.setdefault("res", None)
    return L


DEPTH_LAYERS = _layers()
ACT = {"none": lambda t: t, "relu": F.relu, "elu": F.elu, "sigmoid": torch.sigmoid}


def layer_input(L, acts):
    """the layer's full input as the reference sees it: nearest x2 of source 0 (up0), concatenated with the skip"""
    x = acts[L["src"]]
    if L["up0"]:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return torch.cat([x, acts[L["skip"]]], 1) if L["skip"] else x


def conv(L, x, w, b=None):
    if L["reflect"]:
        return F.conv2d(F.pad(x, (L["pad"],) * 4, mode="reflect"), w, b, stride=L["stride"])
    return F.conv2d(x, w, b, stride=L["stride"], padding=L["pad"])


def net_input(img_u8, dtype=torch.float64):
    """depth_inference's normalised input, (img / 255 - 0.45) / 0.225, computed in `dtype`"""
    x = torch.from_numpy(img_u8).permute(2, 0, 1).contiguous().float().div(255).unsqueeze(0).to(dtype)
    return (x - 0.45) / 0.225


def activations(sd, img_u8, dtype=torch.float64, on_bn=None):
    """every activation of the net: {"input", "stem", "pool", <layer out>...}.  on_bn(L, y) is called with each batch norm's
    input before the norm is applied (the calibration walk sets the statistics there)"""
    if any(v.dtype != dtype for v in sd.values()):
        sd = {k: v.to(dtype) for k, v in sd.items()}
    acts = {"input": net_input(img_u8, dtype)}
    for L in DEPTH_LAYERS:
        y = conv(L, layer_input(L, acts), sd[L["name"] + ".weight"], sd.get(L["name"] + ".bias"))
        if L["bn"]:
            if on_bn:
                on_bn(L, y)
            y = O._bn(sd, L["bn"], y)
        if L["res"]:
            y = y + acts[L["res"]]
        acts[L["out"]] = ACT[L["act"]](y)
        if L["out"] == "stem":
            acts["pool"] = F.max_pool2d(acts["stem"], 3, 2, 1)
    return acts


def fold(sd, bn):
    """DepthNet::finalize's bn_fold in float32: (scale, shift) per channel"""
    g, b, m, v = (sd[bn + k].numpy().astype(np.float32) for k in (".weight", ".bias", ".running_mean", ".running_var"))
    inv = np.float32(1.0) / np.sqrt(v + np.float32(1e-5))
    scale = g * inv
    return scale, b - m * scale


def folded_params(sd, L):
    """the fp32 operands the device packs for layer L: (weight OIHW, bias) as float32 torch tensors"""
    w = sd[L["name"] + ".weight"].numpy().astype(np.float32)
    if L["bn"]:
        scale, shift = fold(sd, L["bn"])
        return torch.from_numpy(w * scale[:, None, None, None]), torch.from_numpy(shift)
    b = sd.get(L["name"] + ".bias")
    return torch.from_numpy(w), (b.float() if b is not None else torch.zeros(w.shape[0]))


@functools.lru_cache(maxsize=4)
def _calibrated(seed, h, w):
    sd = {k: v.double().clone() for k, v in O.monodepth2_state_dict(seed).items()}
    g = torch.Generator().manual_seed(seed + 12345)
    for L in DEPTH_LAYERS:
        if L["bn"]:
            wt = sd[L["name"] + ".weight"]
            wt *= torch.pow(10.0, torch.rand(wt.shape[0], generator=g, dtype=torch.float64) * 3 - 1.5).view(-1, 1, 1, 1)
    sd[DEAD[0] + ".weight"][DEAD[2]] = 0

    def on_bn(L, y):
        bn, c = L["bn"], y.shape[1]
        mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        sd[bn + ".running_mean"] = mean + 0.1 * var.sqrt() * torch.randn(c, generator=g, dtype=torch.float64)
        sd[bn + ".running_var"] = var * torch.pow(10.0, torch.rand(c, generator=g, dtype=torch.float64) * 0.6 - 0.3)
        sd[bn + ".weight"] = 0.2 + 1.8 * torch.rand(c, generator=g, dtype=torch.float64)
        sd[bn + ".bias"] = torch.rand(c, generator=g, dtype=torch.float64) - 0.5
        if bn == DEAD[1]:
            sd[bn + ".running_mean"][DEAD[2]] = 0
            sd[bn + ".running_var"][DEAD[2]] = 0
        if bn == NEAR_DEAD[0]:
            sd[bn + ".weight"][NEAR_DEAD[1]] = NEAR_DEAD[2]

    img, _ = image_pair(h, w, seed=CALIBRATION_SEED)
    acts = activations(sd, img, torch.float64, on_bn)
    head = DEPTH_LAYERS[-1]
    hw, hb = sd[head["name"] + ".weight"], sd[head["name"] + ".bias"]
    z = conv(head, acts[head["src"]], hw, hb)
    a = HEAD_LOGIT_STD / float(z.std())
    sd[head["name"] + ".weight"] = hw * a
    sd[head["name"] + ".bias"] = (hb - float(z.mean())) * a
    return {k: v.float() for k, v in sd.items()}


def calibrated_monodepth2_state_dict(seed=4869, h=192, w=640):
    """monodepth2_state_dict(seed) with spread filters, calibrated batch-norm statistics, a dead and a near-dead channel
    and an unsaturated head (module docstring); float32, deterministic per (seed, h, w)"""
    return dict(_calibrated(seed, h, w))


def unsaturated_fraction(disp):
    """share of the pixels whose sigmoid disparity lies in [0.02, 0.98]"""
    d = np.asarray(disp)
    return float(((d >= 0.02) & (d <= 0.98)).mean())


def disparity(depth, min_depth=0.1, max_depth=100.0, mult=5.4):
    """the sigmoid disparity behind a depth map (depth_inference's disp_to_depth, inverted)"""
    return (mult / np.asarray(depth, np.float64) - 1.0 / max_depth) / (1.0 / min_depth - 1.0 / max_depth)


def rel_err_stats(depth, exact):
    """(max, p99, median) of the per-pixel relative error |d - d64| / d64"""
    e = np.abs(np.asarray(depth, np.float64) - exact) / exact
    return float(e.max()), float(np.quantile(e, 0.99)), float(np.median(e))


# Gate of the float64-anchor test (test_nets_gpu.py::test_depthnet_distance_to_the_exact_function): per statistic
# (max, p99, median) of the per-pixel relative depth error, the device may be at most DEPTH_ANCHOR_FACTOR times further
# from the exact function than the oracle's own fp32 arithmetic, plus an absolute floor of about an fp32 ulp.  Measured on
# the MI355X (device / oracle per statistic, over both worlds and 64x96, 192x640, 320x1024): fp32 0.60-1.43 (the 1.43 is the
# max of random_weights 320x1024, 3.74e-5 vs 2.61e-5), f16x3 0.37-1.12.
DEPTH_ANCHOR_FACTOR = (1.5, 1.5, 1.5)
DEPTH_ANCHOR_FLOOR = (1e-6, 2.5e-7, 1.2e-7)


def anchor_gate(oracle_stats, factor=DEPTH_ANCHOR_FACTOR, floor=DEPTH_ANCHOR_FLOOR):
    return tuple(f * o + a for f, o, a in zip(factor, oracle_stats, floor))
