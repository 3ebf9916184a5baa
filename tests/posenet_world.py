"""A well-conditioned world for the pose net's accuracy tests, and the net's layer inventory.

synthetic.posenet_state_dict takes its encoder from monodepth2_state_dict: every folded batch-norm scale is about 1, no
filter norm differs from its neighbour's and no channel is dead (tests/depth_world.py says why that is ill-conditioned for an
accuracy gate).  calibrated_posenet_state_dict follows depth_world._calibrated step by step on the pose net:

  * conv filters whose norms differ per output channel by 10^U(-1.5, 1.5) (every conv that feeds a batch norm);
  * batch-norm statistics measured in float64 on a calibration pair (image_pair(h, w, seed=999), never a test pair), layer by
    layer, with depth_world's noise, gamma and beta;
  * depth_world's dead filter (DEAD) and near-dead channel (NEAR_DEAD);
  * the head net.3 rescaled per output channel so that on the calibration pair the six parameters of either predicted frame
    have the magnitudes HEAD_TARGETS (the net's own signs): 1.2e-3 .. 5e-2, the scale posenet_ref.MATH_CASES states for a
    trained net and tests/test_pose_math_cpu.py tests pose_math.h at.  Each row's weights are scaled so that a change of the
    map's channel mean by the rms of the twelve means moves the parameter by HEAD_RESPONSE of its target, and its bias
    supplies the rest: the parameters follow the frames, and stay within [1e-4, 1e-1] from pair to pair.

POSE_LAYERS lists every convolution of PoseNet::enqueue (df-vo_amd/csrc/nets.hip) in launch order, in DEPTH_LAYERS' record
format: ResNetEncoder::enqueue's twenty (depth_world's own entries, conv1 over six channels here) and PoseDecoder's four.
activations() walks it with the unfolded batch norm and equals posenet_ref.posenet_parameters; with emulate="f16" it walks the
folded float32 parameters with every conv's input and weight rounded to f16, the definition of the single-product mode
(tests/test_ops_gpu.py::test_conv_f16_mode) applied layer by layer."""
import functools
import importlib

import numpy as np
import torch
import torch.nn.functional as F

import depth_world as W
from depth_world import ACT, DEAD, NEAR_DEAD, conv, fold, folded_params  # noqa: F401  (the pose tests take them from here)
from oracle import nets_torch as O
from posenet_ref import pair_tensor
from synth import image_pair

CALIBRATION_SEED = W.CALIBRATION_SEED
# |parameter| per head channel on the calibration pair (axis-angle, translation; both predicted frames): MATH_CASES' scale
HEAD_TARGETS = (3.1e-3, 1.2e-3, 4.7e-3, 2.3e-2, 4.1e-3, 5.0e-2)
HEAD_RESPONSE = 1.0
# conv layers that launch_conv (conv_dispatch.hip) keeps in exact fp32 under the f16 packings: only conv_use_head's one- and
# two-channel square heads.  The pose net has none -- net.3 (cout 12) is padded to a 16-wide tile and runs on the f16 ring
# kernel like every other layer
EXACT_FP32 = frozenset()


def _layers():
    L = [dict(d) for d in W.DEPTH_LAYERS if d["name"].startswith("encoder.")]
    src = L[-1]["out"]
    for i, (k, act) in enumerate([(1, "relu"), (3, "relu"), (3, "relu"), (1, "none")]):
        L.append(dict(name="net.%d" % i, bn=None, k=k, stride=1, pad=k // 2, reflect=0, up0=0, skip=None, res=None, act=act,
                      src=src, out="net.%d" % i))
        src = "net.%d" % i
    return L


POSE_LAYERS = _layers()


def net_input(img6, dtype=torch.float64):
    """resnet_encoder.py:89 on forward_pose's [1, 6, H, W] tensor of k / 255 values, computed in `dtype`"""
    return (img6.to(dtype) - 0.45) / 0.225


def _f16(t):
    return t.half().to(t.dtype)


def activations(sd, img6, dtype=torch.float64, emulate=None, on_bn=None, on_act=None):
    """(every activation of the net: {"input", "stem", "pool", <layer out>...}, "net.3" being the head's map; the six raw
    parameters of frame 0, 0.01 * map.mean(3).mean(2), as a numpy vector).  img6 is posenet_ref.pair_tensor's tensor.
    emulate=None: the unfolded batch norm in `dtype`; on_bn(L, y) is called with each batch norm's input before the norm
    is applied.  emulate="f16": the folded float32 parameters (folded_params) widened to `dtype`, each conv's input and
    weight rounded to f16 first (layers in EXACT_FP32 excepted); bias, residual and activation function unrounded.
    on_act(name, tensor) may return a replacement for the activation `name` as it is produced (the mutation tests)."""
    assert emulate in (None, "f16")
    if emulate is None and any(v.dtype != dtype for v in sd.values()):
        sd = {k: v.to(dtype) for k, v in sd.items()}
    acts = {"input": net_input(img6, dtype)}
    keep = on_act or (lambda name, t: t)
    with torch.no_grad():
        for L in POSE_LAYERS:
            x = acts[L["src"]]
            if emulate:
                wt, b = (t.to(dtype) for t in folded_params(sd, L))
                if L["name"] not in EXACT_FP32:
                    x, wt = _f16(x), _f16(wt)
                y = conv(L, x, wt, b)
            else:
                y = conv(L, x, sd[L["name"] + ".weight"], sd.get(L["name"] + ".bias"))
                if L["bn"]:
                    if on_bn:
                        on_bn(L, y)
                    y = O._bn(sd, L["bn"], y)
            if L["res"]:
                y = y + acts[L["res"]]
            acts[L["out"]] = keep(L["out"], ACT[L["act"]](y))
            if L["out"] == "stem":
                acts["pool"] = keep("pool", F.max_pool2d(acts["stem"], 3, 2, 1))
        params = 0.01 * acts["net.3"].mean(3).mean(2)
    return acts, params[0, :6].numpy()


def pair(h, w, seed):
    """(frame 0, frame 1, pair_tensor of them) of image_pair(h, w, seed)"""
    img0, img1 = image_pair(h, w, seed=seed)
    return img0, img1, pair_tensor(img0, img1)


@functools.lru_cache(maxsize=4)
def _calibrated(seed, h, w):
    base = importlib.import_module("df-vo_amd.synthetic").posenet_state_dict(seed)
    sd = {k: v.double().clone() for k, v in base.items()}
    g = torch.Generator().manual_seed(seed + 12345)
    for L in POSE_LAYERS:
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

    activations(sd, pair(h, w, CALIBRATION_SEED)[2], torch.float64, on_bn=on_bn)
    return sd


@functools.lru_cache(maxsize=8)
def _with_head(seed, h, w, head_hw):
    sd = dict(_calibrated(seed, h, w))
    acts, _ = activations(sd, pair(head_hw[0], head_hw[1], CALIBRATION_SEED)[2], torch.float64)
    z = acts["net.3"].mean(3).mean(2)[0]  # the twelve channel means on the calibration pair, bias included
    target = torch.tensor(HEAD_TARGETS * 2, dtype=torch.float64) * torch.where(z < 0, -1.0, 1.0)
    a = HEAD_RESPONSE * target.abs() / (0.01 * z.pow(2).mean().sqrt())
    sd["net.3.weight"] = sd["net.3.weight"] * a.view(-1, 1, 1, 1)
    sd["net.3.bias"] = sd["net.3.bias"] * a + (target / 0.01 - a * z)
    return {k: v.float() for k, v in sd.items()}


def calibrated_posenet_state_dict(seed=4869, h=192, w=640, head_hw=None):
    """posenet_state_dict(seed) with spread filters, calibrated batch-norm statistics, a dead and a near-dead channel and a
    head that emits parameters of a trained net's scale (module docstring); float32, deterministic per (seed, h, w, head_hw).
    The batch-norm statistics are measured at h x w; the head is rescaled on the calibration pair of head_hw (default: h, w),
    so that one set of statistics can serve feeds whose final map is too small to measure a variance on."""
    return dict(_with_head(seed, h, w, tuple(head_hw) if head_hw else (h, w)))


# ---- the pooled end-to-end gate (tests/test_posenet_world_gpu.py, part B) ------------------------------------------------------
# feed size -> number of frame pairs.  The smallest sizes that still reach each mechanism: the smallest legal net (a 1 x 1
# final map), a 1 x 2 and a 2 x 3 map, a 17-row map (the second trip of k_pose_head's loop over 16-row chunks) and the
# deployed feed.  Six numbers from one pair are too small a sample for a ratio rule (the fp32 walk's own max-of-six distance
# to float64 varies four-fold between pairs), so the distances are pooled over 6 x pairs values per size.
POOLS = {(32, 32): 8, (32, 64): 4, (64, 96): 8, (544, 64): 4, (192, 640): 4}
POOL_SEED = 300
WORLD_SEED = 4869
WORLD_HW = (192, 640)
POOL_FACTOR = 1.5  # the project's rule for another summation order (test_nets_gpu.py, depth_world.DEPTH_ANCHOR_FACTOR)


def pool_world(h, w):
    """the calibrated weights of the pooled tests at feed h x w: batch-norm statistics once, at 192 x 640 (a 1 x 1 or 1 x 2
    final map has no variance to measure), the head rescaled on the calibration pair of the feed's own size, so that the
    conditions of tests/test_posenet_world_cpu.py hold at every size"""
    return calibrated_posenet_state_dict(WORLD_SEED, WORLD_HW[0], WORLD_HW[1], head_hw=(h, w))


def pool_pairs(h, w):
    """the test pairs of feed h x w: [(frame 0, frame 1, pair_tensor)], seeds distinct over all sizes"""
    first = POOL_SEED + 16 * list(POOLS).index((h, w))
    return [pair(h, w, first + i) for i in range(POOLS[(h, w)])]


def pooled(got, exact):
    """(rms, max) of |got - exact| over a pool: both [pairs, 6]"""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(exact, np.float64))
    return float(np.sqrt((d * d).mean())), float(d.max())


def pool_floor(exact):
    """one fp32 ulp of the pool's largest parameter (DEPTH_ANCHOR_FLOOR's class)"""
    return 2.0 ** -23 * float(np.abs(exact).max())


def pool_gate(oracle_stats, floor, factor=POOL_FACTOR):
    return tuple(factor * o + floor for o in oracle_stats)
