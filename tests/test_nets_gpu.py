"""GPU parity of the two CNN executors (C ABI: dfvo_flownet_*, dfvo_depthnet_*) against the torch-CPU
oracle (oracle/nets_torch.py, itself pinned to the reference by tests/golden).

Tolerance: the nets are ~60 fp32 convolutions deep with data-dependent warps; the HIP path differs
from torch-CPU only in fp32 summation order (MFMA fmaf chains vs oneDNN), so errors are reported
relative to the flow magnitude.  Stated bound: max|dflow| <= 2e-3 px on the final maps with the
seeded random weights (which amplify noise far more than trained weights do)."""
import ctypes as C

import numpy as np
import pytest
import torch

import depth_world as DW
from oracle import nets_torch as O
from synth import image_pair
from util import report

pytestmark = pytest.mark.gpu


def make_flownet(capi, h, w, sd, graph=0):
    lib = capi.lib()
    net = C.c_void_p()
    capi.check(lib.dfvo_flownet_create(h, w, None, C.byref(net)))
    nh, nw = C.c_int(), C.c_int()
    capi.check(lib.dfvo_flownet_net_size(net, C.byref(nh), C.byref(nw)))
    params = {k: v.numpy() for k, v in sd.items()}
    for l in range(1, 7):
        params["aux.linspace_x.%d" % l] = torch.linspace(-1.0, 1.0, nw.value >> (l - 1)).numpy()
        params["aux.linspace_y.%d" % l] = torch.linspace(-1.0, 1.0, nh.value >> (l - 1)).numpy()
    capi.set_params(lib.dfvo_flownet_set_param, net, params)
    capi.check(lib.dfvo_flownet_finalize(net))
    capi.check(lib.dfvo_flownet_set_graph(net, graph))
    return net, nh.value, nw.value


_oracle_cache = {}


def _oracle_flow(sd, ref_img, cur_img, key, levels=False):
    """torch-CPU oracle, computed once per input (the tests are parametrised over the conv precision)"""
    if key not in _oracle_cache:
        O._grid_cache.clear()
        _oracle_cache[key] = O.flow_inference(sd, ref_img, cur_img, return_levels=levels)
    return _oracle_cache[key]


def _flow_gate(name, got, want, tol=2e-3):
    """absolute pixel error of a flow field; the bound is absolute up to 10 px of flow and relative (tol/10 per px) beyond"""
    e, s = report(name, got, want)
    bound = tol * max(1.0, s / 10)
    assert e <= bound, "%s: max |HIP - oracle| = %.3e px exceeds %.3e px (max |flow| %.1f px)" % (name, e, bound, s)
    return e


# (64 x 64: the smallest image FlowNet accepts -- level 6 is a 2 x 2 map, level 5 a 4 x 4 one)
@pytest.mark.parametrize("h,w", [(64, 64), (70, 100), (192, 640), (376, 1241)])
def test_flownet_vs_oracle(gpu, conv_precision, h, w):
    lib = gpu.lib()
    sd = O.liteflownet_state_dict(4869)
    ref_img, cur_img = image_pair(h, w, seed=1001 + h)
    net, nh, nw = make_flownet(gpu, h, w, sd)
    assert (nh, nw) == O.get_target_size(h, w)
    fwd = np.zeros((2, h, w), np.float32)
    bwd = np.zeros((2, h, w), np.float32)
    diff = np.zeros((h, w), np.float32)
    gpu.check(lib.dfvo_flownet_forward_host(net, gpu.as_ptr(ref_img), gpu.as_ptr(cur_img), gpu.as_ptr(fwd),
                                            gpu.as_ptr(bwd), gpu.as_ptr(diff)))
    ofwd, obwd, odiff, raw = _oracle_flow(sd, ref_img, cur_img, ("vs", h, w), levels=True)
    for lvl in (6, 5, 4, 3, 2):
        lh, lw = nh >> (lvl - 1), nw >> (lvl - 1)
        buf = np.zeros((2, lh, lw, 2), np.float32)
        gpu.check(lib.dfvo_flownet_get_level_flow(net, lvl, gpu.as_ptr(buf), None, None))
        _flow_gate("flow level %d (%dx%d) %s" % (lvl, h, w, conv_precision), np.transpose(buf, (0, 3, 1, 2)), raw[lvl].numpy())
    print("   useful GFLOP per forward: %.1f (%s)" % (lib.dfvo_flownet_last_flops(net) / 1e9, conv_precision))
    lib.dfvo_flownet_destroy(net)
    assert np.isfinite(fwd).all() and np.isfinite(bwd).all() and np.isfinite(diff).all()
    _flow_gate("fwd flow %dx%d %s" % (h, w, conv_precision), fwd, ofwd)
    _flow_gate("bwd flow %dx%d %s" % (h, w, conv_precision), bwd, obwd)
    _flow_gate("flow diff %dx%d %s" % (h, w, conv_precision), diff, odiff[..., 0], tol=4e-3)


def _err_stats(x, exact):
    e = np.abs(x.astype(np.float64) - exact)
    return float(e.max()), float(np.quantile(e, 0.99)), float(np.median(e))


# Gates of the float64-anchor test, set from the measured runs (profiles/r4u_anchor.txt, printed lines "ANCHOR").
# Random weights (every layer a dense sum, the realistic case): the device may be at most ANCHOR_FACTOR times further from
# the exact function than the reference's own fp32 arithmetic (torch CPU) is -- (max, 99th percentile, median) of
# |flow - anchor| over the map; measured 0.5-1.1 (fp32) and 0.75-1.03 (f16x3: consistent with the f16 MFMA adding its 16 exact
# products before one rounding into the accumulator -- shorter float chains than oneDNN's).  Coded tunnel world: the oracle sits at the REPRESENTATION floor there (median
# 9e-7 px = half an ulp of a 10-27 px flow: its decode layers have at most three non-zero products, summed in one fixed order)
# and the device's forward flow carries a uniform +7e-6 px offset -- one ulp of the constant 1.0 the crafted "later frame"
# selector computes as 255 * (c2 - c1): 1 + 0.992 * 2^-24 for frame counters 1 and 2, next to the midpoint of two floats, where the
# two summation orders land on different sides
# (tools/flow_error_by_level.py; the oracle has the same offset against the anchor at other frame counters).  Absolute
# gates there: (max, median) px.
ANCHOR_FACTOR = {"fp32": (1.5, 1.5, 1.5), "f16x3": (1.5, 1.5, 1.5)}
ANCHOR_TUNNEL_ABS = {"fwd": (1e-4, 2.5e-5), "bwd": (1e-4, 2.5e-5), "diff": (3e-3, 2.5e-5)}


@pytest.mark.parametrize("world", ["random_weights_192x640", "coded_tunnel_256x640"])
def test_flownet_distance_to_the_exact_function(gpu, conv_precision, world):
    """The yardstick for "results identical to the reference's" in floating point: the flow net evaluated in DOUBLE on the
    same fp32 inputs, weights and grid constants (oracle/nets_torch.py, dtype=float64) is the function every fp32 execution
    approximates.  The reference's own arithmetic (torch CPU fp32, the oracle) sits ~5e-4 px (max) / ~1e-5 px (median) from
    it; two CPU executions of the oracle are 50 times closer to EACH OTHER than that only because they add in the same
    order.  Gate: the device is no further from the function than a small multiple of the oracle's own distance."""
    import importlib
    lib = gpu.lib()
    if world.startswith("random"):
        h, w = 192, 640
        sd = O.liteflownet_state_dict(4869)
        ref_img, cur_img = image_pair(h, w, seed=1001 + h)
    else:
        h, w = 256, 640
        syn = importlib.import_module("df-vo_amd.synthetic")
        seq = syn.coded_tunnel_sequence(h, w, 3, mode="mux", step=1.0, seed=21)
        sd = syn.crafted_liteflownet_state_dict(h, w, "mux")
        ref_img, cur_img = seq["frames"][1], seq["frames"][2]
    net, nh, nw = make_flownet(gpu, h, w, sd)
    fwd = np.zeros((2, h, w), np.float32)
    bwd = np.zeros((2, h, w), np.float32)
    diff = np.zeros((h, w), np.float32)
    gpu.check(lib.dfvo_flownet_forward_host(net, gpu.as_ptr(ref_img), gpu.as_ptr(cur_img), gpu.as_ptr(fwd), gpu.as_ptr(bwd),
                                            gpu.as_ptr(diff)))
    lib.dfvo_flownet_destroy(net)
    o32 = _oracle_flow(sd, ref_img, cur_img, ("anchor32", world))
    key = ("anchor64", world)
    if key not in _oracle_cache:
        O._grid_cache.clear()
        _oracle_cache[key] = O.flow_inference(sd, ref_img, cur_img, dtype=torch.float64)
    o64 = _oracle_cache[key]
    fmax, f99, fmed = ANCHOR_FACTOR[conv_precision]
    for name, dev, a32, a64 in (("fwd", fwd, o32[0], o64[0]), ("bwd", bwd, o32[1], o64[1]), ("diff", diff, o32[2][..., 0], o64[2][..., 0])):
        d, o, x = _err_stats(dev, a64), _err_stats(a32, a64), _err_stats(dev, a32.astype(np.float64))
        print("ANCHOR %s %s %s: |device - exact| max %.2e p99 %.2e median %.2e | |oracle fp32 - exact| max %.2e p99 %.2e median %.2e | "
              "|device - oracle fp32| max %.2e p99 %.2e median %.2e px" % ((world, conv_precision, name) + d + o + x))
        if world.startswith("random"):
            assert d[0] <= fmax * o[0] + 1e-5, "%s %s: max distance to the exact flow %.2e px vs the oracle's own %.2e" % (world, name, d[0], o[0])
            assert d[1] <= f99 * o[1] + 2e-6 and d[2] <= fmed * o[2] + 5e-7, (world, name, d, o)
        else:
            amax, amed = ANCHOR_TUNNEL_ABS[name]
            assert d[0] <= max(amax, 1.5 * o[0]) and d[2] <= amed, (world, name, d, o)


_SPLITK_AB = r"""
import ctypes as C, importlib, sys, numpy as np, torch
sys.path.insert(0, %(tests)r); sys.path.insert(0, %(root)r)
from oracle import nets_torch as O
from synth import image_pair
import test_nets_gpu as T
capi = importlib.import_module("df-vo_amd.capi")
lib = capi.lib()
h, w = 192, 640
sd = O.liteflownet_state_dict(4869)
ref_img, cur_img = image_pair(h, w, seed=77)
net, nh, nw = T.make_flownet(capi, h, w, sd)
out = {}
for rep in range(3):
    fwd, bwd, diff = np.zeros((2, h, w), np.float32), np.zeros((2, h, w), np.float32), np.zeros((h, w), np.float32)
    capi.check(lib.dfvo_flownet_forward_host(net, capi.as_ptr(ref_img), capi.as_ptr(cur_img), capi.as_ptr(fwd), capi.as_ptr(bwd),
                                             capi.as_ptr(diff)))
    out["fwd%%d" %% rep], out["bwd%%d" %% rep], out["diff%%d" %% rep] = fwd, bwd, diff
dsd = O.monodepth2_state_dict(4869)
np.savez(%(out)r, **out)
"""


def test_splitk_in_kernel_finish_equals_two_launch_reduction(gpu, tmp_path):
    """the split-K layers (pyramid levels 3-6) reduced by the last-arriving workgroup inside the contracting kernel
    (tile tickets) against the separate ordered-reduction launch (DFVO_SPLITK_FUSED=0): same slice order, so the flow
    fields are identical bit for bit, and repeated passes reproduce themselves (no ordering race)"""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    res = {}
    for fused in ("0", "1"):
        out = str(tmp_path / ("splitk_%s.npz" % fused))
        env = dict(os.environ, DFVO_SPLITK_FUSED=fused, DFVO_CONV_PRECISION="fp32")
        code = _SPLITK_AB % {"tests": tests, "root": os.path.dirname(tests), "out": out}
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[fused] = np.load(out)
    for k in ("fwd", "bwd", "diff"):
        for rep in (1, 2):
            assert np.array_equal(res["1"][k + "0"], res["1"]["%s%d" % (k, rep)]), "fused finish not repeatable: %s" % k
        assert np.array_equal(res["0"][k + "0"], res["1"][k + "0"]), "fused finish differs from the two-launch reduction: %s" % k
    assert np.abs(res["1"]["fwd0"]).max() > 0.1


@pytest.mark.parametrize("knob", ["DFVO_REG_HEAD_V", "DFVO_CORR_RT"])
def test_rewritten_kernels_leave_the_flow_bit_identical(gpu, tmp_path, knob):
    """the register-tiled correlation kernel and the vectorised regularisation head keep the operation order of the plain
    restatements they replaced (kept compiled as test references behind DFVO_CORR_RT=0 / DFVO_REG_HEAD_V=0): the whole flow
    net's output with the knob off / on, bit for bit"""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    res = {}
    for on in ("0", "1"):
        out = str(tmp_path / ("%s_%s.npz" % (knob, on)))
        env = dict(os.environ, DFVO_CONV_PRECISION="fp32")
        env[knob] = on
        code = _SPLITK_AB % {"tests": tests, "root": os.path.dirname(tests), "out": out}
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[on] = np.load(out)
    for k in ("fwd0", "bwd0", "diff0"):
        assert np.array_equal(res["0"][k], res["1"][k]), "%s changes %s" % (knob, k)
    assert np.abs(res["1"]["fwd0"]).max() > 0.1


def test_tap_window_kernel_leaves_the_f16x3_flow_bit_identical(gpu, tmp_path):
    """f16x3 mode: the multi-tap streaming layers (7x7 first layer, 7x1 / 1x7 / 5x5 distance layers) on the tap-window
    kernel (conv_taps_f16s.hip: window split once into LDS planes) against the generic register-ring kernel
    (DFVO_TAPS=0): same weights, table, operand positions and step order -- the whole flow net's output bit for bit"""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    res = {}
    for on in ("0", "1"):
        out = str(tmp_path / ("taps_%s.npz" % on))
        env = dict(os.environ, DFVO_CONV_PRECISION="f16x3", DFVO_TAPS=on)
        code = _SPLITK_AB % {"tests": tests, "root": os.path.dirname(tests), "out": out}
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[on] = np.load(out)
    for k in ("fwd0", "bwd0", "diff0"):
        assert np.array_equal(res["0"][k], res["1"][k]), "the tap-window kernel changes %s" % k
    assert np.abs(res["1"]["fwd0"]).max() > 0.1


_SPLITK_LOAD = """
import importlib, sys, zlib
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
importlib.import_module("df-vo_amd")
pmod = importlib.import_module("df-vo_amd.pipeline")
smod = importlib.import_module("df-vo_amd.sequence")
from oracle import nets_torch as O
from synth import image_pair, rigid_scene
h, w = 192, 640
K = rigid_scene(64, 64, seed=1)["K"]
pipe = pmod.TrackingPipeline(h, w, 192, 640, K, O.liteflownet_state_dict(4869), O.monodepth2_state_dict(4869), seed=4869)
frames = []
for i in range(5):
    a, b = image_pair(h, w, seed=100 + i)
    frames += [a, b]
frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
crc = []
def collect(j, out):
    fwd, bwd, diff, raw, dep = pipe.get_outputs(j %% 4)
    crc.append([zlib.crc32(fwd.tobytes()), zlib.crc32(bwd.tobytes()), zlib.crc32(diff.tobytes()), zlib.crc32(raw.tobytes())])
for rep in range(2):  # two flow-net instances, the depth net and the solver stage of the pairs behind run concurrently
    smod.track_chunk(pipe, frames, 0, len(frames) - 1, collect=collect)
pipe.close()
np.save(%(out)r, np.array(crc, np.int64))
"""


def test_splitk_in_kernel_finish_under_pipeline_load(gpu, tmp_path):
    """the same A/B inside the fused pipeline in exact fp32: two flow-net instances three pairs ahead, the depth net and the
    solver stages on their own streams while the split-K layers hand their partials over across XCDs -- flow / depth of
    every pair of two passes over a 10-frame sequence, fused finish vs the separate reduction launch, CRC-equal"""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    res = {}
    for fused in ("0", "1"):
        out = str(tmp_path / ("splitk_load_%s.npy" % fused))
        env = dict(os.environ, DFVO_SPLITK_FUSED=fused, DFVO_CONV_PRECISION="fp32")
        code = _SPLITK_LOAD % {"tests": tests, "root": os.path.dirname(tests), "out": out}
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        res[fused] = np.load(out)
    assert res["0"].shape == (18, 4)
    assert np.array_equal(res["0"], res["1"]), "fused split-K finish differs under load: rows %s" % np.nonzero((res["0"] != res["1"]).any(1))[0]
    assert np.array_equal(res["1"][:9], res["1"][9:]), "second pass over the sequence differs from the first"


def test_flownet_graph_replay_is_identical(gpu):
    """graph replay equals the eager pass bit for bit, on ANOTHER pair in every pass (the net's output buffers still hold the
    pass before, so a replay that does nothing or reads a stale frame differs) and into host arrays that hold NaN before the
    call; the first pair again at the end.  tests/test_graph_replay_gpu.py has the caller's buffers, the depth net, the
    pipeline and the session."""
    lib = gpu.lib()
    h, w = 128, 224
    sd = O.liteflownet_state_dict(4869)
    pairs = [image_pair(h, w, seed=s) for s in (7, 8, 9, 7)]
    outs = {}
    for graph in (0, 1):
        net, _, _ = make_flownet(gpu, h, w, sd, graph=graph)
        outs[graph] = []
        for ref_img, cur_img in pairs:  # graphs on: eager + capture, then replays
            fwd = np.full((2, h, w), np.nan, np.float32)
            bwd = np.full((2, h, w), np.nan, np.float32)
            diff = np.full((h, w), np.nan, np.float32)
            gpu.check(lib.dfvo_flownet_forward_host(net, gpu.as_ptr(ref_img), gpu.as_ptr(cur_img), gpu.as_ptr(fwd),
                                                    gpu.as_ptr(bwd), gpu.as_ptr(diff)))
            outs[graph].append((fwd, bwd, diff))
        lib.dfvo_flownet_destroy(net)
    for k, (eager, replay) in enumerate(zip(outs[0], outs[1])):
        for a, b in zip(eager, replay):
            assert np.isfinite(a).all() and np.array_equal(a, b), "pass %d" % k
    for a, b in zip(outs[0][0], outs[0][3]):
        assert np.array_equal(a, b)
    assert not any(np.array_equal(outs[0][k][0], outs[0][k + 1][0]) for k in range(3))


@pytest.mark.parametrize("h,w", [(64, 96), (192, 640)])
def test_depthnet_vs_oracle(gpu, conv_precision, h, w):
    lib = gpu.lib()
    sd = O.monodepth2_state_dict(4869)
    img, _ = image_pair(h, w, seed=55)
    net = C.c_void_p()
    gpu.check(lib.dfvo_depthnet_create(h, w, 0.1, 100.0, 5.4, None, C.byref(net)))
    gpu.set_params(lib.dfvo_depthnet_set_param, net, {k: v.numpy() for k, v in sd.items()})
    gpu.check(lib.dfvo_depthnet_finalize(net))
    depth = np.zeros((h, w), np.float32)
    for _ in range(2):
        gpu.check(lib.dfvo_depthnet_forward_host(net, gpu.as_ptr(img), gpu.as_ptr(depth)))
    ref = O.depth_inference(sd, img)
    e, s = report("depth %dx%d" % (h, w), depth, ref)
    print("   useful GFLOP per forward: %.2f" % (lib.dfvo_depthnet_last_flops(net) / 1e9))
    lib.dfvo_depthnet_destroy(net)
    assert np.isfinite(depth).all()
    assert e <= 1e-3 * max(1.0, s)
    # per pixel: the bound above scales with the FARTHEST depth (0.1 m at 100 m allows 20 % at the nearest 0.5 m)
    rel = float((np.abs(depth.astype(np.float64) - ref) / ref).max())
    print("   max per-pixel |d - oracle| / oracle: %.2e" % rel)
    assert rel <= 1e-4


def _depthnet_forward(capi, h, w, sd, img):
    lib = capi.lib()
    net = C.c_void_p()
    capi.check(lib.dfvo_depthnet_create(h, w, 0.1, 100.0, 5.4, None, C.byref(net)))
    try:
        capi.set_params(lib.dfvo_depthnet_set_param, net, {k: v.numpy() for k, v in sd.items()})
        capi.check(lib.dfvo_depthnet_finalize(net))
        depth = np.zeros((h, w), np.float32)
        capi.check(lib.dfvo_depthnet_forward_host(net, capi.as_ptr(img), capi.as_ptr(depth)))
    finally:
        lib.dfvo_depthnet_destroy(net)
    assert np.isfinite(depth).all()
    return depth


_depth_cache = {}


def _depth_world(world, h, w):
    """(weights, frame, oracle fp32 depth, float64 depth) of a depth-anchor world, computed once per (world, size)"""
    key = (world, h, w)
    if key not in _depth_cache:
        sd = O.monodepth2_state_dict(4869) if world == "random_weights" else DW.calibrated_monodepth2_state_dict(4869, h, w)
        img, _ = image_pair(h, w, seed=55)
        d64 = O.depth_inference(sd, img, dtype=torch.float64)
        if world == "calibrated":  # the precondition of the test's power (tests/test_depth_world_cpu.py)
            frac = DW.unsaturated_fraction(DW.disparity(d64))
            assert frac >= 0.9, "calibrated world %dx%d: only %.3f of the disparities in [0.02, 0.98]" % (h, w, frac)
        _depth_cache[key] = sd, img, O.depth_inference(sd, img), d64
    return _depth_cache[key]


DEPTH_WORLDS = ["random_weights", "calibrated"]
# 320x1024: monodepth2's high-resolution model (the feed size is read from the encoder file); larger maps move layers onto
# other conv families
DEPTH_SIZES = [(64, 96), (192, 640), (320, 1024)]


@pytest.mark.parametrize("h,w", DEPTH_SIZES)
@pytest.mark.parametrize("world", DEPTH_WORLDS)
def test_depthnet_distance_to_the_exact_function(gpu, conv_precision, world, h, w):
    """The depth net's float64 anchor (the flow net's test_flownet_distance_to_the_exact_function, per pixel): the device
    depth's relative error |d - d64| / d64 against the net evaluated in DOUBLE on the same fp32 weights and frame, gated per
    statistic (max, p99, median) at DEPTH_ANCHOR_FACTOR times the oracle fp32's own distance plus an ulp-sized floor
    (tests/depth_world.py).  The calibrated world (trained-like batch-norm scales 1.7e-4 .. 478, 96-99 % unsaturated disparities)
    is where the encoder, the fold and every decoder level reach the depth; tests/test_depth_world_cpu.py shows on the CPU
    that a lost f16x3 lo plane in one decoder layer lands about 50x outside this gate, a wrong fold scale in one channel
    about 220x."""
    sd, img, o32, d64 = _depth_world(world, h, w)
    depth = _depthnet_forward(gpu, h, w, sd, img)
    d, o, x = DW.rel_err_stats(depth, d64), DW.rel_err_stats(o32, d64), DW.rel_err_stats(depth, o32.astype(np.float64))
    print("ANCHOR depth %s_%dx%d %s: |device - exact| / exact max %.2e p99 %.2e median %.2e | |oracle fp32 - exact| max %.2e "
          "p99 %.2e median %.2e | |device - oracle fp32| max %.2e p99 %.2e median %.2e" % ((world, h, w, conv_precision) + d + o + x))
    gate = DW.anchor_gate(o)
    assert all(a <= g for a, g in zip(d, gate)), "%s %dx%d %s: device %s vs gate %s" % (world, h, w, conv_precision, d, gate)


# f16 mode (operands rounded to f16, one product per term; not fp32-class): absolute gates on (max, p99, median) of the
# per-pixel relative depth error at 2.5x the first device measurement (printed lines "ANCHOR depth ... f16"), which was
#   random_weights 64x96 1.76e-2 1.04e-2 1.13e-4 | 192x640 2.66e-2 5.10e-3 9.48e-6 | 320x1024 3.93e-2 5.63e-3 1.04e-5
#   calibrated     64x96 3.53e-2 1.96e-2 2.42e-3 | 192x640 2.93e-2 1.02e-2 1.34e-3 | 320x1024 2.79e-2 9.80e-3 1.35e-3
# (a float64 simulation of the mode on the CPU, f16-rounded operands layer by layer, lands within 1.3x of these)
F16_DEPTH_ANCHOR_GATE = {
    ("random_weights", 64, 96): (4.4e-2, 2.6e-2, 2.8e-4), ("random_weights", 192, 640): (6.7e-2, 1.3e-2, 2.4e-5),
    ("random_weights", 320, 1024): (9.8e-2, 1.4e-2, 2.6e-5), ("calibrated", 64, 96): (8.8e-2, 4.9e-2, 6e-3),
    ("calibrated", 192, 640): (7.3e-2, 2.6e-2, 3.4e-3), ("calibrated", 320, 1024): (7e-2, 2.5e-2, 3.4e-3)}


@pytest.mark.parametrize("h,w", DEPTH_SIZES)
@pytest.mark.parametrize("world", DEPTH_WORLDS)
def test_depthnet_f16_distance_to_the_exact_function(gpu, f16_mode, world, h, w):
    """the same anchor under the f16 packing: reported and gated at F16_DEPTH_ANCHOR_GATE"""
    sd, img, o32, d64 = _depth_world(world, h, w)
    depth = _depthnet_forward(gpu, h, w, sd, img)
    d, o = DW.rel_err_stats(depth, d64), DW.rel_err_stats(o32, d64)
    print("ANCHOR depth %s_%dx%d f16: |device - exact| / exact max %.2e p99 %.2e median %.2e | |oracle fp32 - exact| max %.2e "
          "p99 %.2e median %.2e" % ((world, h, w) + d + o))
    gate = F16_DEPTH_ANCHOR_GATE[(world, h, w)]
    assert all(a <= g for a, g in zip(d, gate)), "%s %dx%d f16: device %s vs gate %s" % (world, h, w, d, gate)


@pytest.mark.parametrize("h,w", [(960, 1280), (1280, 1920)])
def test_flownet_large_configs(gpu, conv_precision, h, w):
    """BASELINE configs 4 / 5 (RobotCar 1280x960 frames, synthetic 1920x1280 pairs) against the torch-CPU oracle: live at
    960x1280; at 1280x1920 against the fixture the oracle wrote in the build container (tests/golden/
    make_oracle_fixtures.py: every 8th pixel of the three maps, input frames pinned by CRC).  Plus the size-independent
    property: the net runs (ref, cur) and (cur, ref) as the two samples of one batch, so swapping the inputs must swap
    the forward and backward flows bit for bit."""
    import os
    import zlib
    lib = gpu.lib()
    sd = O.liteflownet_state_dict(4869)
    ref_img, cur_img = image_pair(h, w, seed=2000 + h)
    net, nh, nw = make_flownet(gpu, h, w, sd)
    assert (nh, nw) == O.get_target_size(h, w)
    outs = []
    for a, b in ((ref_img, cur_img), (cur_img, ref_img)):
        fwd = np.zeros((2, h, w), np.float32)
        bwd = np.zeros((2, h, w), np.float32)
        diff = np.zeros((h, w), np.float32)
        gpu.check(lib.dfvo_flownet_forward_host(net, gpu.as_ptr(a), gpu.as_ptr(b), gpu.as_ptr(fwd), gpu.as_ptr(bwd),
                                                gpu.as_ptr(diff)))
        outs.append((fwd, bwd, diff))
    print("   %dx%d (net %dx%d): useful GFLOP per forward %.1f" % (h, w, nh, nw, lib.dfvo_flownet_last_flops(net) / 1e9))
    lib.dfvo_flownet_destroy(net)
    for o in outs:
        assert all(np.isfinite(x).all() for x in o)
    assert np.array_equal(outs[0][0], outs[1][1]) and np.array_equal(outs[0][1], outs[1][0])
    assert np.abs(outs[0][0]).max() > 0
    if (h, w) == (1280, 1920):
        fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flownet_1280x1920.npz"))
        crc = [zlib.crc32(np.ascontiguousarray(x).tobytes()) & 0xffffffff for x in (ref_img, cur_img)]
        assert crc == list(fx["img_crc"]), "the seeded input frames differ from the ones the oracle fixture was computed on"
        st = int(fx["step"])
        _flow_gate("fwd flow 1280x1920 %s (fixture, every %dth px)" % (conv_precision, st), outs[0][0][:, ::st, ::st], fx["fwd"])
        _flow_gate("bwd flow 1280x1920 %s (fixture)" % conv_precision, outs[0][1][:, ::st, ::st], fx["bwd"])
        _flow_gate("flow diff 1280x1920 %s (fixture)" % conv_precision, outs[0][2][::st, ::st], fx["diff"], tol=4e-3)
    else:
        ofwd, obwd, odiff = _oracle_flow(sd, ref_img, cur_img, ("large", h, w))
        _flow_gate("fwd flow %dx%d %s" % (h, w, conv_precision), outs[0][0], ofwd)
        _flow_gate("bwd flow %dx%d %s" % (h, w, conv_precision), outs[0][1], obwd)
