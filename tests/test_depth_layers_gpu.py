"""The depth net layer by layer against float64, so that a failure of the net's float64-anchor gate names its layer.

Every convolution of DepthNet::enqueue (tests/depth_world.py: DEPTH_LAYERS) runs as one dfvo_conv2d on the layer's real
input in the calibrated world at 192x640: the float64 oracle's activations, rounded to fp32, with the batch norm folded as
bn_fold does it in float32.  The result is compared with the float64 convolution of the same fp32 operands, per output,
with test_f16x3_dynamic_range's bounds (tests/layer_bounds.py; the one-channel head stays exact fp32 in the f16 modes).
The encoder's max-pool runs on the real stem output and must equal F.max_pool2d bit for bit.
test_inventory_runs_the_families_the_net_runs proves the inventory exercised the kernel families the net itself launches,
profile row by profile row."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import depth_world as W
from oracle import nets_torch as O
from synth import image_pair
from layer_bounds import conv_bound
from test_ops_gpu import run_conv

pytestmark = pytest.mark.gpu

H, W_ = 192, 640
PRECISIONS = ["fp32", "f16x3", "f16"]
LAYERS = {L["name"]: L for L in W.DEPTH_LAYERS}
_cache = {}


def _world():
    if "world" not in _cache:
        sd = W.calibrated_monodepth2_state_dict(4869, H, W_)
        img, _ = image_pair(H, W_, seed=55)
        acts = W.activations(sd, img, torch.float64)
        _cache["world"] = sd, img, {k: v.float() for k, v in acts.items()}
    return _cache["world"]


def _run_layer(gpu, precision, L):
    """one dfvo_conv2d of layer L under `precision`: (device output, float64 reference, bound, launches per profile row)"""
    key = (precision, L["name"])
    if key in _cache:
        return _cache[key]
    sd, _, a32 = _world()
    lib = gpu.lib()
    wt, b = W.folded_params(sd, L)
    x0, x1 = a32[L["src"]], (a32[L["skip"]] if L["skip"] else None)
    res = a32[L["res"]] if L["res"] else None
    act = {"none": (0, 0.0), "relu": (2, 0.0), "elu": (3, 1.0), "sigmoid": (4, 0.0)}[L["act"]]
    ms, fl, ln = np.zeros(24), np.zeros(24), np.zeros(24, np.int32)
    gpu.check(lib.dfvo_set_conv_precision(precision.encode()))
    gpu.f16s_overflow_count(reset=True)
    try:
        gpu.check(lib.dfvo_conv_profile_begin())
        try:
            out = run_conv(gpu, x0, wt, b, L["stride"], (L["pad"], L["pad"]), L["reflect"], act[0], act[1], x1, L["up0"], res)
        finally:
            gpu.check(lib.dfvo_conv_profile_end(gpu.as_ptr(ms), gpu.as_ptr(fl), gpu.as_ptr(ln)))
    finally:
        gpu.check(lib.dfvo_set_conv_precision(b"fp32"))
        n_ovf = gpu.f16s_overflow_count(reset=True)
    assert n_ovf == 0, "%s %s: %d f16 range events" % (precision, L["name"], n_ovf)
    head = L["name"] == "decoder.10.conv"
    _, _, y, bound = conv_bound(lambda x, w, bb: W.conv(L, x, w, bb), W.layer_input(L, a32).double(), wt.double(), b.double(),
                                res.double() if res is not None else None, precision, exact_fp32=head)
    _cache[key] = (out, W.ACT[L["act"]](y), bound, ln.copy())
    return _cache[key]


def _rows(ln):
    return " ".join("%d:%d" % (r, ln[r]) for r in np.nonzero(ln)[0])


@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_depthnet_layers_vs_float64(gpu, precision, layer):
    L = LAYERS[layer]
    out, ref, bound, ln = _run_layer(gpu, precision, L)
    assert out.shape == ref.shape
    err = (out.double() - ref).abs()
    ratio = float((err / bound).max())
    print("   %-5s %-30s rows %-8s max|ref| %.2e  max err %.2e  worst err / bound %.3f"
          % (precision, layer, _rows(ln), float(ref.abs().max()), float(err.max()), ratio))
    assert bool(torch.isfinite(out).all())
    assert bool((err <= bound).all()), "%s %s: worst err / bound %.3f" % (precision, layer, ratio)


def test_depthnet_maxpool_on_the_stem_output_is_exact(gpu):
    _, _, a32 = _world()
    x = a32["stem"]
    n, c, h, w = x.shape
    src = x.permute(0, 2, 3, 1).contiguous().cuda()
    dst = torch.full((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), 7.0, device="cuda")
    gpu.check(gpu.lib().dfvo_maxpool3x3s2(C.c_void_p(src.data_ptr()), n, h, w, c, C.c_void_p(dst.data_ptr()), None))
    torch.cuda.synchronize()
    assert torch.equal(dst.permute(0, 3, 1, 2).cpu(), F.max_pool2d(x, 3, 2, 1))


def _net_rows(gpu, precision):
    """launches per profile row of one depth-net forward (graphs off), packed under `precision`"""
    sd, img, _ = _world()
    lib = gpu.lib()
    net = C.c_void_p()
    gpu.check(lib.dfvo_set_conv_precision(precision.encode()))
    try:
        gpu.check(lib.dfvo_depthnet_create(H, W_, 0.1, 100.0, 5.4, None, C.byref(net)))
        gpu.set_params(lib.dfvo_depthnet_set_param, net, {k: v.numpy() for k, v in sd.items()})
        gpu.check(lib.dfvo_depthnet_finalize(net))
    finally:
        gpu.check(lib.dfvo_set_conv_precision(b"fp32"))
    gpu.check(lib.dfvo_depthnet_set_graph(net, 0))
    depth = np.zeros((H, W_), np.float32)
    gpu.check(lib.dfvo_depthnet_forward_host(net, gpu.as_ptr(img), gpu.as_ptr(depth)))  # the one eager tuning run
    ms, fl, ln = np.zeros(24), np.zeros(24), np.zeros(24, np.int32)
    gpu.check(lib.dfvo_conv_profile_begin())
    try:
        gpu.check(lib.dfvo_depthnet_forward_host(net, gpu.as_ptr(img), gpu.as_ptr(depth)))
    finally:
        gpu.check(lib.dfvo_conv_profile_end(gpu.as_ptr(ms), gpu.as_ptr(fl), gpu.as_ptr(ln)))
        lib.dfvo_depthnet_destroy(net)
    assert gpu.f16s_overflow_count(reset=True) == 0
    return ln


@pytest.mark.parametrize("precision", PRECISIONS)
def test_inventory_runs_the_families_the_net_runs(gpu, precision):
    """the inventory's launches, summed per profile row, equal one forward of the net: every conv family the net uses at
    192x640 was checked above, as often as the net launches it"""
    inv = np.zeros(24, np.int32)
    print("\n   layer -> profile row:launches (%s)" % precision)
    for name, L in LAYERS.items():
        ln = _run_layer(gpu, precision, L)[3]
        print("   %-30s %s" % (name, _rows(ln)))
        inv += ln
    net = _net_rows(gpu, precision)
    print("   inventory %s | net %s" % (_rows(inv), _rows(net)))
    assert np.array_equal(inv, net)
