"""GPU: the pose net against float64 in the calibrated world (tests/posenet_world.py), per layer and on pooled outputs.

Part A -- every convolution of PoseNet::enqueue (POSE_LAYERS) runs as one dfvo_conv2d on the layer's real input at the
deployed 192x640 feed, in fp32, f16x3 and f16: the float64 walk's activations rounded to fp32, the batch norm folded in
float32 as bn_fold does it, the residual where the block has one.  The result is compared per output with the float64
convolution of the same fp32 operands under tests/layer_bounds.py's bound for the precision.  No layer takes exact_fp32:
the dispatcher (conv_dispatch.hip: conv_use_head) keeps only one- and two-channel square heads in fp32 under the f16
packings, and net.3 (cout 12, a 16-wide tile) runs on the f16 ring kernel like the rest.  encoder.layer4.* and the decoder
run again at the 32x32 feed's maps (2x2 -> 1x1 with stride 2, 3x3 windows on a 1x1 map).  The max-pool on the real stem output
equals F.max_pool2d bit for bit, and test_inventory_runs_the_families_the_net_runs proves that the inventory ran the kernel
families the executor launches, profile row by profile row.

Part B -- dfvo_posenet_forward, the whole executor (input kernel, bn_fold, packing, every launch, k_pose_head), on the pools
of posenet_world.POOLS: per feed size and per precision of the conv_precision fixture the 6 x pairs parameters' distance to the
float64 walk, as rms and as max, may be at most POOL_FACTOR = 1.5 times the torch-CPU float32 walk's, plus one fp32 ulp of the
largest parameter.  The weights are posenet_world.pool_world's: batch-norm statistics calibrated once, at 192x640 (a 1x1 map
has no variance to measure), the head rescaled per size; tests/test_posenet_world_cpu.py checks the world's conditions at
every size.  Every 4x4 is pose_math.h's arithmetic on its own parameters, and a captured-graph replay of the last pair equals
its eager run bit for bit.

Part C -- the single-product f16 mode against its own definition (test_ops_gpu.py::test_conv_f16_mode, layer by layer:
posenet_world.activations(emulate="f16")): the device's pooled distance to the float64 emulated walk may be at most 1.5 times
the float32 emulated walk's, plus the same floor.  "F16-MODE POSENET" lines say what the mode costs against the unrounded
float64 anchor; nothing is gated on that figure.

Set DFVO_POSENET_PARITY_JSON to a path to have the pooled figures written there (profiles/posenet_parity.json, section
"posenet_world")."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import posenet_ref as PR
import posenet_world as PW
from layer_bounds import conv_bound
from test_ops_gpu import run_conv
from test_posenet_gpu import _forward, check_pose_of_parameters, make_posenet

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "f16x3", "f16"]
LAYERS = {L["name"]: L for L in PW.POSE_LAYERS}
FEED, SMALL = (192, 640), (32, 32)
SMALL_LAYERS = [n for n in LAYERS if n.startswith("encoder.layer4.") or n.startswith("net.")]
MULT = 5.4
_cache = {}


# ---- part A ----------------------------------------------------------------------------------------------------------------------
def _world(hw):
    """(weights, the pool's first pair, its float64 activations rounded to fp32), once per feed size"""
    if ("world", hw) not in _cache:
        sd = PW.pool_world(*hw)
        pair = PW.pool_pairs(*hw)[0]
        acts, _ = PW.activations(sd, pair[2], torch.float64)
        _cache[("world", hw)] = sd, pair, {k: v.float() for k, v in acts.items()}
    return _cache[("world", hw)]


def _run_layer(gpu, precision, L, hw=FEED):
    """one dfvo_conv2d of layer L under `precision`: (device output, float64 reference, bound, launches per profile row)"""
    key = (precision, L["name"], hw)
    if key in _cache:
        return _cache[key]
    sd, _, a32 = _world(hw)
    lib = gpu.lib()
    wt, b = PW.folded_params(sd, L)
    x, res = a32[L["src"]], (a32[L["res"]] if L["res"] else None)
    act = {"none": 0, "relu": 2}[L["act"]]
    ms, fl, ln = np.zeros(24), np.zeros(24), np.zeros(24, np.int32)
    gpu.check(lib.dfvo_set_conv_precision(precision.encode()))
    gpu.f16s_overflow_count(reset=True)
    try:
        gpu.check(lib.dfvo_conv_profile_begin())
        try:
            out = run_conv(gpu, x, wt, b, L["stride"], (L["pad"], L["pad"]), 0, act, 0.0, None, 0, res)
        finally:
            gpu.check(lib.dfvo_conv_profile_end(gpu.as_ptr(ms), gpu.as_ptr(fl), gpu.as_ptr(ln)))
    finally:
        gpu.check(lib.dfvo_set_conv_precision(b"fp32"))
        n_ovf = gpu.f16s_overflow_count(reset=True)
    assert n_ovf == 0, "%s %s: %d f16 range events" % (precision, L["name"], n_ovf)
    _, _, y, bound = conv_bound(lambda xx, w, bb: PW.conv(L, xx, w, bb), x.double(), wt.double(), b.double(),
                                res.double() if res is not None else None, precision, exact_fp32=L["name"] in PW.EXACT_FP32)
    _cache[key] = (out, PW.ACT[L["act"]](y), bound, ln.copy())
    return _cache[key]


def _rows(ln):
    return " ".join("%d:%d" % (r, ln[r]) for r in np.nonzero(ln)[0])


def _check_layer(gpu, precision, layer, hw):
    L = LAYERS[layer]
    out, ref, bound, ln = _run_layer(gpu, precision, L, hw)
    assert out.shape == ref.shape
    err = (out.double() - ref).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    print("   %-5s %dx%d %-30s map %dx%d rows %-8s max|ref| %.2e  max err %.2e  worst err / bound %.3f"
          % (precision, hw[0], hw[1], layer, ref.shape[2], ref.shape[3], _rows(ln), float(ref.abs().max()), float(err.max()), ratio))
    assert bool(torch.isfinite(out).all())
    assert bool((err <= bound).all()), "%s %s: worst err / bound %.3f" % (precision, layer, ratio)


@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_posenet_layers_vs_float64(gpu, precision, layer):
    _check_layer(gpu, precision, layer, FEED)


@pytest.mark.parametrize("layer", SMALL_LAYERS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_posenet_layers_vs_float64_smallest_feed(gpu, precision, layer):
    """the 32x32 feed: layer4.0's stride-2 convs from a 2x2 map to one pixel, every later 3x3 window on a 1x1 map"""
    a32 = _world(SMALL)[2]
    assert tuple(a32["encoder.layer3.1"].shape[2:]) == (2, 2) and tuple(a32["net.3"].shape[2:]) == (1, 1)
    _check_layer(gpu, precision, layer, SMALL)


@pytest.mark.parametrize("hw", [FEED, SMALL])
def test_posenet_maxpool_on_the_stem_output_is_exact(gpu, hw):
    _, _, a32 = _world(hw)
    x = a32["stem"]
    n, c, h, w = x.shape
    src = x.permute(0, 2, 3, 1).contiguous().cuda()
    dst = torch.full((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), 7.0, device="cuda")
    gpu.check(gpu.lib().dfvo_maxpool3x3s2(C.c_void_p(src.data_ptr()), n, h, w, c, C.c_void_p(dst.data_ptr()), None))
    torch.cuda.synchronize()
    assert torch.equal(dst.permute(0, 3, 1, 2).cpu(), F.max_pool2d(x, 3, 2, 1))


def _net_rows(gpu, precision):
    """launches per profile row of one eager pose-net forward at 192x640 (graphs off), packed under `precision`"""
    sd, (img0, img1, _), _ = _world(FEED)
    lib = gpu.lib()
    gpu.check(lib.dfvo_set_conv_precision(precision.encode()))
    try:
        net = make_posenet(gpu, FEED[0], FEED[1], sd, mult=MULT, graph=0)
    finally:
        gpu.check(lib.dfvo_set_conv_precision(b"fp32"))
    ms, fl, ln = np.zeros(24), np.zeros(24), np.zeros(24, np.int32)
    try:
        d0, d1 = torch.from_numpy(img0).cuda(), torch.from_numpy(img1).cuda()
        _forward(gpu, net, d0, d1)  # the first call holds the eager tuning run
        gpu.check(lib.dfvo_conv_profile_begin())
        try:
            _forward(gpu, net, d0, d1)
        finally:
            gpu.check(lib.dfvo_conv_profile_end(gpu.as_ptr(ms), gpu.as_ptr(fl), gpu.as_ptr(ln)))
    finally:
        lib.dfvo_posenet_destroy(net)
    assert gpu.f16s_overflow_count(reset=True) == 0
    return ln


@pytest.mark.parametrize("precision", PRECISIONS)
def test_inventory_runs_the_families_the_net_runs(gpu, precision):
    """the inventory's launches, summed per profile row, equal one forward of the net: every conv family the pose net uses
    at 192x640 was checked above, as often as the net launches it"""
    inv = np.zeros(24, np.int32)
    print("\n   layer -> profile row:launches (%s)" % precision)
    for name, L in LAYERS.items():
        ln = _run_layer(gpu, precision, L)[3]
        print("   %-30s %s" % (name, _rows(ln)))
        inv += ln
    net = _net_rows(gpu, precision)
    print("   inventory %s | net %s" % (_rows(inv), _rows(net)))
    assert int(inv.sum()) == len(LAYERS)
    assert np.array_equal(inv, net)


# ---- parts B and C ---------------------------------------------------------------------------------------------------------------
def _pool(hw, emulate=None):
    """(weights, pairs, float64 walk's parameters [pairs, 6], float32 walk's), once per feed size and kind of walk"""
    key = ("pool", hw, emulate)
    if key not in _cache:
        sd, pairs = PW.pool_world(*hw), PW.pool_pairs(*hw)
        p64 = np.array([PW.activations(sd, q[2], torch.float64, emulate)[1] for q in pairs])
        p32 = np.array([PW.activations(sd, q[2], torch.float32, emulate)[1] for q in pairs])
        _cache[key] = sd, pairs, p64, p32
    return _cache[key]


def _device_pool(gpu, hw, sd, pairs):
    """every pair of the pool through one net of the current packing, eagerly: the parameters [pairs, 6].  Each 4x4 is checked
    against its own parameters; the last pair is replayed from a captured graph"""
    lib = gpu.lib()
    net = make_posenet(gpu, hw[0], hw[1], sd, mult=MULT, graph=0)
    got = []
    try:
        for img0, img1, _ in pairs:
            d0, d1 = torch.from_numpy(img0).cuda(), torch.from_numpy(img1).cuda()
            pose, par = _forward(gpu, net, d0, d1)
            assert np.isfinite(pose).all() and np.isfinite(par).all()
            check_pose_of_parameters(pose, par, MULT)
            got.append(par)
        gpu.check(lib.dfvo_posenet_set_graph(net, 1))
        replays = [_forward(gpu, net, d0, d1) for _ in range(2)]  # capture, then replay
    finally:
        lib.dfvo_posenet_destroy(net)
    for r in replays:
        assert np.array_equal(r[0], pose) and np.array_equal(r[1], par), "graph replay differs from the eager pass"
    return np.array(got)


@pytest.mark.parametrize("h,w", list(PW.POOLS))
def test_posenet_pooled_distance_to_the_exact_function(gpu, conv_precision, h, w):
    """rms and max of |parameter - float64 walk| over the pool: device <= 1.5 x torch-CPU float32 + 2^-23 max |parameter|.
    Measured on the MI355X, device / gate: fp32 0.23-0.69 (rms) and 0.24-0.96 (max, the 0.96 at 32x64: 6.9e-8 against torch's
    4.3e-8), f16x3 0.19-0.57 and 0.18-0.62 -- f16x3 holds the 1.5 rule on this net (profiles/posenet_parity.json)"""
    sd, pairs, p64, p32 = _pool((h, w))
    dev = _device_pool(gpu, (h, w), sd, pairs)
    d, o, floor = PW.pooled(dev, p64), PW.pooled(p32, p64), PW.pool_floor(p64)
    gate = PW.pool_gate(o, floor)
    print("POSENET POOLED %dx%d %s (%d pairs): |device - exact| rms %.3e max %.3e | |torch fp32 - exact| rms %.3e max %.3e | "
          "floor %.3e | device / gate rms %.2f max %.2f | max |param| %.3e"
          % (h, w, conv_precision, len(pairs), d[0], d[1], o[0], o[1], floor, d[0] / gate[0], d[1] / gate[1], float(np.abs(p64).max())))
    PR.record_parity("posenet_world", {"pooled %dx%d %s" % (h, w, conv_precision): {
        "pairs": len(pairs), "device_to_exact_rms": d[0], "device_to_exact_max": d[1], "torch_fp32_to_exact_rms": o[0],
        "torch_fp32_to_exact_max": o[1], "floor": floor, "factor": PW.POOL_FACTOR, "max_abs_parameter": float(np.abs(p64).max())}})
    assert d[0] <= gate[0] and d[1] <= gate[1], (d, o, floor)


@pytest.mark.parametrize("h,w", [(64, 96), (192, 640)])
def test_posenet_f16_mode_pooled_distance_to_its_definition(gpu, f16_mode, h, w):
    """the f16 mode computes the net of f16-rounded conv operands: the device's pooled distance to the float64 evaluation of
    that net is at most 1.5 x the float32 evaluation's, plus the floor.  Both distances are the noise of f16 roundings that
    flip on an fp32 ulp (measured rms 8.0e-6 vs 9.4e-6 at 64x96, 2.7e-6 vs 2.7e-6 at 192x640), a thousand times the fp32
    walks' distance to each other: this gate sees a wrong f16 kernel, not a 1e-7 slip.  Reported, not gated: what the mode
    costs against the unrounded float64 walk (max 4.5e-5 and 3.6e-5, 7e-4 of the largest parameter)"""
    sd, pairs, p64, _ = _pool((h, w))
    _, _, e64, e32 = _pool((h, w), "f16")
    dev = _device_pool(gpu, (h, w), sd, pairs)
    d, o, floor = PW.pooled(dev, e64), PW.pooled(e32, e64), PW.pool_floor(e64)
    gate = PW.pool_gate(o, floor)
    cost_dev, cost_emu, pmax = PW.pooled(dev, p64), PW.pooled(e64, p64), float(np.abs(p64).max())
    print("F16-MODE POSENET %dx%d (%d pairs): |device - emulation64| rms %.3e max %.3e | |emulation32 - emulation64| rms %.3e max %.3e | "
          "floor %.3e | device / gate rms %.2f max %.2f" % (h, w, len(pairs), d[0], d[1], o[0], o[1], floor, d[0] / gate[0], d[1] / gate[1]))
    print("F16-MODE POSENET %dx%d cost of the mode: |device - exact| rms %.3e max %.3e (%.2e of max |param| %.3e) | "
          "|emulation64 - exact| rms %.3e max %.3e (%.2e)"
          % (h, w, cost_dev[0], cost_dev[1], cost_dev[1] / pmax, pmax, cost_emu[0], cost_emu[1], cost_emu[1] / pmax))
    PR.record_parity("posenet_world", {"f16 mode %dx%d" % (h, w): {
        "pairs": len(pairs), "device_to_emulation64_rms": d[0], "device_to_emulation64_max": d[1], "emulation32_to_emulation64_rms": o[0],
        "emulation32_to_emulation64_max": o[1], "floor": floor, "factor": PW.POOL_FACTOR, "device_to_exact_rms": cost_dev[0],
        "device_to_exact_max": cost_dev[1], "emulation64_to_exact_rms": cost_emu[0], "emulation64_to_exact_max": cost_emu[1],
        "max_abs_parameter": pmax}})
    assert d[0] <= gate[0] and d[1] <= gate[1], (d, o, floor)
