"""GPU: captured-graph replay of the two nets (csrc/nets.hip: FlowNet::forward, DepthNet::forward) and of their callers
(the fused pipeline, the frame session) with changing frames and changing buffers.

Both nets run as captured hipGraphs wherever the product uses them; the per-layer and per-operator tests run them eagerly.
What is checked here is not the arithmetic but that a REPLAY executes it on the current frames into the requested buffers:

  * anchor, once per module: the graphs-off flow of the first pair (70x100, the pair of test_flownet_vs_oracle) and the
    graphs-off depth of the first feed image (64x96, the image of test_depthnet_vs_oracle) against the torch-CPU oracle with
    the assertions of those two tests;
  * everything else: graphs on against graphs off on the same weights and frames, np.array_equal (graph and eager passes
    launch the same kernels with the same arguments).

Every output buffer the caller owns is filled with NaN before each pass (device buffers through dfvo_memcpy_h2d), and every
pass of a case sees another pair / image than the pass before it, so that a replay that writes nothing, writes somewhere
else or reads a stale frame cannot pass.  The nets' internal output buffers (dfvo_*_forward_host, the pipeline's slots, the
session's ring) cannot be reached from outside: there the changing frames carry the check.

Sizes: the suite's smallest -- flow net 70x100 (net size 96x128), depth net 64x96; the pipeline and the session accept the
same two."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nets_torch as O
from synth import image_pair, rigid_scene
from test_nets_gpu import _flow_gate, make_flownet
from util import report

pytestmark = pytest.mark.gpu

H, W = 70, 100       # flow net / pipeline / session frames
FH, FW = 64, 96      # depth net feed
FPX = FH * FW
PAIR_SEEDS = [1001 + H] + list(range(3101, 3112))     # pair 0: test_flownet_vs_oracle's pair at this size
FEED_SEEDS = [55, 3201, 3202, 3203, 3204]             # image 0: test_depthnet_vs_oracle's image
PRECISIONS = ["fp32", "f16x3"]


def _pairs():
    return [image_pair(H, W, seed=s) for s in PAIR_SEEDS]


def _feeds():
    out = []
    for s in FEED_SEEDS:
        out += list(image_pair(FH, FW, seed=s))
    return out


def _frames(n):
    """n distinct HxW frames (both images of consecutive seeded pairs)"""
    out = []
    for a, b in _pairs():
        out += [a, b]
    assert n <= len(out)
    return out[:n]


class _Packing:
    """nets packed inside the block use conv precision `name` (read at finalize); fp32 is restored, and no activation or
    weight of the block's nets may have been clamped (the contract of conftest's conv_precision fixture)"""

    def __init__(self, gpu, name):
        self.gpu, self.name = gpu, name

    def __enter__(self):
        self.gpu.check(self.gpu.lib().dfvo_set_conv_precision(self.name.encode()))
        self.gpu.f16s_overflow_count(reset=True)

    def __exit__(self, et, ev, tb):
        self.gpu.check(self.gpu.lib().dfvo_set_conv_precision(b"fp32"))
        clamped = self.gpu.f16s_overflow_count(reset=True)
        if et is None:
            assert clamped == 0, "%s: %d activations / weights were clamped to +-65504" % (self.name, clamped)


class _Dev:
    """device allocations through dfvo_malloc, freed together"""

    def __init__(self, gpu):
        self.gpu, self.lib, self.ptrs = gpu, gpu.lib(), []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.gpu.check(self.lib.dfvo_sync_device())
        for p in self.ptrs:
            self.lib.dfvo_free(p)

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.gpu.check(self.lib.dfvo_malloc(C.byref(p), nbytes))
        self.ptrs.append(p)
        return p

    def put(self, p, a):
        a = np.ascontiguousarray(a)
        self.gpu.check(self.lib.dfvo_memcpy_h2d(p, self.gpu.as_ptr(a), a.nbytes))

    def image(self, a):
        p = self.alloc(a.nbytes)
        self.put(p, a)
        return p

    def floats(self, n):
        p = self.alloc(4 * n)
        self.poison(p, n)
        return p

    def poison(self, p, n):
        self.put(p, np.full(n, np.nan, np.float32))

    def get(self, p, shape):
        a = np.zeros(shape, np.float32)
        self.gpu.check(self.lib.dfvo_memcpy_d2h(self.gpu.as_ptr(a), p, a.nbytes))
        return a


def _nan(*shape):
    return np.full(shape, np.nan, np.float32)


def _same(a, b):
    """bit-identical maps (no NaN may be left: NaN != NaN)"""
    return a.shape == b.shape and np.array_equal(a, b)


def _flow_host(gpu, net, ref, cur):
    fwd, bwd, diff = _nan(2, H, W), _nan(2, H, W), _nan(H, W)
    gpu.check(gpu.lib().dfvo_flownet_forward_host(net, gpu.as_ptr(ref), gpu.as_ptr(cur), gpu.as_ptr(fwd), gpu.as_ptr(bwd),
                                                  gpu.as_ptr(diff)))
    return fwd, bwd, diff


def _level_flow(gpu, net, nh, nw, lvl):
    buf = _nan(2, nh >> (lvl - 1), nw >> (lvl - 1), 2)
    gpu.check(gpu.lib().dfvo_flownet_get_level_flow(net, lvl, gpu.as_ptr(buf), None, None))
    return buf


def _make_depthnet(gpu, sd, graph):
    lib = gpu.lib()
    net = C.c_void_p()
    gpu.check(lib.dfvo_depthnet_create(FH, FW, 0.1, 100.0, 5.4, None, C.byref(net)))
    gpu.set_params(lib.dfvo_depthnet_set_param, net, {k: v.numpy() for k, v in sd.items()})
    gpu.check(lib.dfvo_depthnet_finalize(net))
    gpu.check(lib.dfvo_depthnet_set_graph(net, graph))
    return net


def _depth_host(gpu, net, img):
    d = _nan(FH, FW)
    gpu.check(gpu.lib().dfvo_depthnet_forward_host(net, gpu.as_ptr(img), gpu.as_ptr(d)))
    return d


def _depth_image_host(gpu, net, frame):
    d = _nan(FH, FW)
    gpu.check(gpu.lib().dfvo_depthnet_forward_image_host(net, gpu.as_ptr(frame), H, W, gpu.as_ptr(d)))
    return d


_eager = {}


def _flow_eager(gpu, precision):
    """graphs off, per pair of PAIR_SEEDS: (fwd, bwd, diff, level-6 flow, level-2 flow); computed once per precision and
    never changed.  The fp32 set is anchored to the oracle on its first pair with test_flownet_vs_oracle's assertions."""
    key = ("flow", precision)
    if key not in _eager:
        sd = O.liteflownet_state_dict(4869)
        with _Packing(gpu, precision):
            net, nh, nw = make_flownet(gpu, H, W, sd, graph=0)
            try:
                res = []
                for ref, cur in _pairs():
                    out = _flow_host(gpu, net, ref, cur)
                    res.append(out + (_level_flow(gpu, net, nh, nw, 6), _level_flow(gpu, net, nh, nw, 2)))
            finally:
                gpu.lib().dfvo_flownet_destroy(net)
        for r in res:
            assert all(np.isfinite(x).all() for x in r)
        if precision == "fp32":
            O._grid_cache.clear()
            ref, cur = _pairs()[0]
            ofwd, obwd, odiff = O.flow_inference(sd, ref, cur)
            _flow_gate("anchor: eager fwd flow %dx%d" % (H, W), res[0][0], ofwd)
            _flow_gate("anchor: eager bwd flow %dx%d" % (H, W), res[0][1], obwd)
            _flow_gate("anchor: eager flow diff %dx%d" % (H, W), res[0][2], odiff[..., 0], tol=4e-3)
        for a, b in zip(res, res[1:]):  # the precondition of every "follows the frame" check below
            assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[3], b[3])
        _eager[key] = res
    return _eager[key]


def _depth_eager(gpu, precision):
    """graphs off: (depth per feed image of FEED_SEEDS, depth per HxW frame through dfvo_depthnet_forward_image_host); the
    fp32 set is anchored to the oracle on its first image with test_depthnet_vs_oracle's assertions"""
    key = ("depth", precision)
    if key not in _eager:
        sd = O.monodepth2_state_dict(4869)
        with _Packing(gpu, precision):
            net = _make_depthnet(gpu, sd, 0)
            try:
                feeds = [_depth_host(gpu, net, f) for f in _feeds()]
                frames = [_depth_image_host(gpu, net, f) for f in _frames(8)]
            finally:
                gpu.lib().dfvo_depthnet_destroy(net)
        assert all(np.isfinite(d).all() for d in feeds + frames)
        if precision == "fp32":
            ref = O.depth_inference(sd, _feeds()[0])
            e, s = report("anchor: eager depth %dx%d" % (FH, FW), feeds[0], ref)
            assert e <= 1e-3 * max(1.0, s)
            assert float((np.abs(feeds[0].astype(np.float64) - ref) / ref).max()) <= 1e-4
        for a, b in zip(feeds + frames, (feeds + frames)[1:]):
            assert not np.array_equal(a, b)
        _eager[key] = feeds, frames
    return _eager[key]


# ---- 1. flow net, changing frames, the net's own buffers ----------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_flownet_replay_follows_the_frames(gpu, precision):
    """seven distinct pairs through dfvo_flownet_forward_host with graphs on (capture on the first, replays after): each the
    graphs-off result of ITS pair, and so are the per-level flows (levels 6 and 2) read after the pass; then the first pair
    again gives the first pair's result ("the last result persists" fails), and the last pair once more"""
    want = _flow_eager(gpu, precision)
    pairs = _pairs()
    K = 7
    with _Packing(gpu, precision):
        net, nh, nw = make_flownet(gpu, H, W, O.liteflownet_state_dict(4869), graph=1)
        try:
            for k in list(range(K)) + [0, K - 1]:
                got = _flow_host(gpu, net, *pairs[k])
                for name, g, w_ in zip(("fwd", "bwd", "diff"), got, want[k]):
                    assert _same(g, w_), "%s: pass on pair %d: %s differs from the eager result" % (precision, k, name)
                assert _same(_level_flow(gpu, net, nh, nw, 6), want[k][3]), "pair %d: level-6 flow" % k
                assert _same(_level_flow(gpu, net, nh, nw, 2), want[k][4]), "pair %d: level-2 flow" % k
        finally:
            gpu.lib().dfvo_flownet_destroy(net)


# ---- 2. flow net, the caller's device pointers --------------------------------------------------------------------------------
class _FlowDev:
    """dfvo_flownet_forward on device buffers with a ledger of what every output BUFFER must hold (None: the sentinel)"""

    def __init__(self, gpu, dev, net, want):
        self.gpu, self.dev, self.net, self.want = gpu, dev, net, want
        self.bufs = {}    # name -> (pointer, shape)
        self.holds = {}   # name -> expected array, or None while it holds the sentinel

    def buffer(self, name, shape):
        self.bufs[name] = (self.dev.floats(int(np.prod(shape))), shape)
        self.holds[name] = None
        return name

    def new_set(self, tag):
        return (self.buffer(tag + ".fwd", (2, H, W)), self.buffer(tag + ".bwd", (2, H, W)), self.buffer(tag + ".diff", (H, W)))

    def run(self, oset, k, d_ref, d_cur, what):
        lib = self.gpu.lib()
        for name in oset:  # the target set is poisoned before the pass
            p, shape = self.bufs[name]
            self.dev.poison(p, int(np.prod(shape)))
            self.holds[name] = None
        self.gpu.check(lib.dfvo_flownet_forward(self.net, d_ref, d_cur, *[self.bufs[n][0] for n in oset]))
        self.gpu.check(lib.dfvo_flownet_sync(self.net))
        for name, w_ in zip(oset, self.want[k][:3]):
            self.holds[name] = w_
        for name, (p, shape) in self.bufs.items():
            got = self.dev.get(p, shape)
            if self.holds[name] is None:
                assert np.isnan(got).all(), "%s: buffer %s was written although no pass targeted it" % (what, name)
            else:
                assert _same(got, self.holds[name]), "%s: buffer %s does not hold the eager result of its last pass" % (what, name)


def test_flownet_replay_reads_frames_at_new_addresses(gpu):
    """one output set, the two frames at another device address in every call (the earlier frames stay allocated, with their
    contents): the frames are not part of the captured graphs, so the flow must follow the frame handed over"""
    want = _flow_eager(gpu, "fp32")
    pairs = _pairs()
    net, _, _ = make_flownet(gpu, H, W, O.liteflownet_state_dict(4869), graph=1)
    try:
        with _Dev(gpu) as dev:
            fd = _FlowDev(gpu, dev, net, want)
            oset = fd.new_set("O")
            seen = set()
            for k in (3, 4, 5, 6, 3):
                d_ref, d_cur = dev.image(pairs[k][0]), dev.image(pairs[k][1])
                assert d_ref.value not in seen and d_cur.value not in seen
                seen |= {d_ref.value, d_cur.value}
                fd.run(oset, k, d_ref, d_cur, "frames at a new address, pair %d" % k)
    finally:
        gpu.lib().dfvo_flownet_destroy(net)


def test_flownet_levels_graph_cache_over_many_output_sets(gpu):
    """the four-entry round-robin cache of levels graphs (keyed by the three output pointers): six output sets in the order
    A B C D E F A C F B -- four fills, evictions of A and B, re-capture of evicted sets, hits on entries that are not the
    latest --, then G, which shares its forward-flow buffer with A and nothing else, and A again.  After every call the
    target set holds the eager result of that call's pair and every other buffer still holds what was last written to it
    (or the sentinel): a hit on the wrong entry writes into another set and fails here"""
    want = _flow_eager(gpu, "fp32")
    pairs = _pairs()
    net, _, _ = make_flownet(gpu, H, W, O.liteflownet_state_dict(4869), graph=1)
    try:
        with _Dev(gpu) as dev:
            fd = _FlowDev(gpu, dev, net, want)
            sets = {t: fd.new_set(t) for t in "ABCDEF"}
            sets["G"] = (sets["A"][0], fd.buffer("G.bwd", (2, H, W)), fd.buffer("G.diff", (H, W)))
            frames = [(dev.image(a), dev.image(b)) for a, b in pairs]
            for k, t in enumerate("ABCDEFACFBGA"):
                fd.run(sets[t], k, frames[k][0], frames[k][1], "call %d on set %s" % (k, t))
    finally:
        gpu.lib().dfvo_flownet_destroy(net)


# ---- 3. depth net --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_depthnet_replay_follows_image_and_buffers(gpu, precision):
    """dfvo_depthnet_forward with graphs on; d_img and d_depth are baked into the one captured graph, which is re-captured
    when either changes (and the capturing call itself relies on the eager pass before the capture):
    (a) fixed buffers, the image's CONTENTS change; (b) the image at a new address per call, the old ones kept with their
    contents; (c) a new depth buffer per call, every earlier one poisoned again and required to stay so; (d) two
    (image, depth) pairs alternating, contents changing.  Each result is the graphs-off depth of the image handed over."""
    want, _ = _depth_eager(gpu, precision)
    feeds = _feeds()
    lib = gpu.lib()
    with _Packing(gpu, precision):
        net = _make_depthnet(gpu, O.monodepth2_state_dict(4869), 1)
        try:
            with _Dev(gpu) as dev:
                def run(d_img, d_depth, k, what, untouched=()):
                    dev.poison(d_depth, FPX)
                    for p in untouched:
                        dev.poison(p, FPX)
                    gpu.check(lib.dfvo_depthnet_forward(net, d_img, d_depth))
                    gpu.check(lib.dfvo_depthnet_sync(net))
                    assert _same(dev.get(d_depth, (FH, FW)), want[k]), "%s %s: not the eager depth of image %d" % (precision, what, k)
                    for p in untouched:
                        assert np.isnan(dev.get(p, (FH, FW))).all(), "%s %s: an earlier call's depth buffer was written" % (precision, what)

                d_img, d_depth = dev.image(feeds[0]), dev.floats(FPX)
                for k in (0, 1, 2, 3, 1):                                     # (a)
                    dev.put(d_img, feeds[k])
                    run(d_img, d_depth, k, "(a) call on image %d" % k)
                for k in (4, 5, 6):                                           # (b)
                    run(dev.image(feeds[k]), d_depth, k, "(b) image at a new address")
                d_img, old = dev.image(feeds[7]), [d_depth]
                for k in (7, 8, 9):                                           # (c)
                    dev.put(d_img, feeds[k])
                    d_new = dev.floats(FPX)
                    run(d_img, d_new, k, "(c) depth at a new address", untouched=old)
                    old.append(d_new)
                two = [(dev.image(feeds[0]), dev.floats(FPX)), (dev.image(feeds[1]), dev.floats(FPX))]
                for i, k in enumerate((2, 3, 4, 5, 6, 7)):                    # (d)
                    im, dp = two[i % 2]
                    dev.put(im, feeds[k])
                    run(im, dp, k, "(d) alternating pairs, call %d" % i, untouched=[two[1 - i % 2][1]])
        finally:
            lib.dfvo_depthnet_destroy(net)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_depthnet_graph_switch_and_host_entries(gpu, precision):
    """one net switched between graphs on and off between calls (fixed buffers, changing contents) keeps giving the eager
    result in both directions; K images through dfvo_depthnet_forward_host and K frames through
    dfvo_depthnet_forward_image_host (device LANCZOS resize in front of the replay) with graphs on"""
    want, want_frames = _depth_eager(gpu, precision)
    feeds, frames = _feeds(), _frames(8)
    lib = gpu.lib()
    with _Packing(gpu, precision):
        net = _make_depthnet(gpu, O.monodepth2_state_dict(4869), 1)
        try:
            with _Dev(gpu) as dev:
                d_img, d_depth = dev.image(feeds[0]), dev.floats(FPX)
                for k, graph in enumerate((1, 1, 0, 1, 1, 0, 0, 1, 1)):
                    gpu.check(lib.dfvo_depthnet_set_graph(net, graph))
                    dev.put(d_img, feeds[k])
                    dev.poison(d_depth, FPX)
                    gpu.check(lib.dfvo_depthnet_forward(net, d_img, d_depth))
                    gpu.check(lib.dfvo_depthnet_sync(net))
                    assert _same(dev.get(d_depth, (FH, FW)), want[k]), "%s call %d (graphs %d): not the eager depth" % (precision, k, graph)
            gpu.check(lib.dfvo_depthnet_set_graph(net, 1))
            for k in (0, 1, 2, 3, 4, 0):
                assert _same(_depth_host(gpu, net, feeds[k]), want[k]), "%s forward_host on image %d" % (precision, k)
            for k in (0, 1, 2, 3, 4, 0):
                assert _same(_depth_image_host(gpu, net, frames[k]), want_frames[k]), "%s forward_image_host on frame %d" % (precision, k)
            assert _same(_depth_host(gpu, net, feeds[5]), want[5])
        finally:
            lib.dfvo_depthnet_destroy(net)


# ---- 4 / 5. the fused pipeline: carry path under graphs, and end to end ---------------------------------------------------------
TRACK_FIELDS = ("R", "t", "scale", "status", "n_kp", "good_kp_found", "best_inlier_cnt", "num_valid", "cheirality",
                "scale_n_valid", "scale_n_trials", "scale_n_inliers", "pnp_found", "pnp_inliers", "pnp_n_filtered")
# pair j: (slot, carried?, caller's feed image?) -- the first pair full, then carried, a full pass, carried again (the order
# pattern of test_feature_carry_equals_recomputed_features); every slot twice; the feed alternates between the pipeline's own
# resize buffer and a caller's tensor, so that the depth graph is re-captured on the way
SEQUENCE = [(0, False, False), (1, True, False), (2, True, True), (3, False, False), (0, True, True), (1, True, False),
            (2, False, False), (3, True, True), (1, True, False)]
# then four pairs enqueued back to back with no wait between them (the nets running ahead, as in a sequence): (slot, carried?)
BURST = [(0, False), (1, True), (2, False), (3, True)]


def _run_sequence(pipe_mod, graph):
    K = rigid_scene(64, 64, seed=1)["K"]
    # (kp_thre: the seeded random weights give no forward-backward consistent flow; with the default 0.1 px no pair has a
    # keypoint and track returns the constant-motion status before any solver runs)
    pipe = pipe_mod.TrackingPipeline(H, W, FH, FW, K, O.liteflownet_state_dict(4869), O.monodepth2_state_dict(4869), seed=4869,
                                     kp_thre=1.0e3)
    try:
        pipe.set_graph(graph)  # before the first enqueue
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        frames = [d(f) for f in _frames(len(SEQUENCE) + len(BURST) + 1)]
        feeds = [d(f) for f in _feeds()]
        pipe.set_ref_image(frames[0])
        res = []
        for j, (slot, carried, own_feed) in enumerate(SEQUENCE):
            pipe.enqueue_nets(slot, None if carried else frames[j], frames[j + 1], feeds[j] if own_feed else None)
            pipe.sync()
            maps = pipe.get_outputs(slot)
            out = pipe.track(slot)
            track = {f: (np.array(getattr(out, f)[:]) if f in ("R", "t") else getattr(out, f)) for f in TRACK_FIELDS}
            res.append((maps, track, pipe.get_rng_state()))
        for j, (slot, carried) in enumerate(BURST, len(SEQUENCE)):
            pipe.enqueue_nets(slot, None if carried else frames[j], frames[j + 1])
        pipe.sync()
        return res, [pipe.get_outputs(slot) for slot, _ in BURST]
    finally:
        pipe.close()


@pytest.mark.parametrize("instances", ["1", "2"])
def test_pipeline_graphs_on_equals_graphs_off(gpu, monkeypatch, instances):
    """two fresh pipelines (70x100 frames, 64x96 feed), dfvo_pipeline_set_graph 1 / 0 before the first enqueue, the same nine
    distinct pairs (SEQUENCE) through enqueue_nets / get_outputs / track: forward flow, backward flow, consistency map, raw
    and processed depth of every pair bit for bit, and the returned pose, scale, counts and the RandomState after every
    pair exactly; then four pairs enqueued back to back without a wait (BURST), their maps bit for bit.  With one flow-net
    instance the carry-over comes from the same instance's last pass, with two from the other instance (whose feature graph
    bakes the source in and is re-captured when it changes)."""
    monkeypatch.setenv("DFVO_FLOW_INSTANCES", instances)
    pipe_mod = importlib.import_module("df-vo_amd.pipeline")
    (on, burst_on), (off, burst_off) = _run_sequence(pipe_mod, 1), _run_sequence(pipe_mod, 0)
    print("   graphs off: status %s, keypoints %s, E inliers %s" % tuple([r[1][f] for r in off] for f in ("status", "n_kp", "best_inlier_cnt")))
    assert all(r[1]["n_kp"] > 0 for r in off), "a pair without keypoints compares nothing of the solver stage"
    for j, ((m1, t1, r1), (m0, t0, r0)) in enumerate(zip(on, off)):
        for name, a, b in zip(("fwd", "bwd", "diff", "raw depth", "processed depth"), m1, m0):
            assert np.isfinite(b).all(), "pair %d: graphs-off %s is not finite" % (j, name)
            assert _same(a, b), "pair %d (slot %d): %s differs between graphs on and off" % (j, SEQUENCE[j][0], name)
        for f in TRACK_FIELDS:
            assert np.array_equal(t1[f], t0[f]), "pair %d: track output %s: %r with graphs, %r without" % (j, f, t1[f], t0[f])
        assert np.array_equal(r1[1], r0[1]) and r1[2] == r0[2], "pair %d: RandomState differs between graphs on and off" % j
    for j, (m1, m0) in enumerate(zip(burst_on, burst_off)):
        for name, a, b in zip(("fwd", "bwd", "diff", "raw depth", "processed depth"), m1, m0):
            assert np.isfinite(b).all() and _same(a, b), "burst pair %d: %s differs between graphs on and off" % (j, name)
    maps = [r[0] for r in off] + burst_off
    for a, b in zip(maps, maps[1:]):  # distinct pairs give distinct maps: a stale replay cannot equal the eager run
        assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[3], b[3])


# ---- 6. the f16 range counter under replay -----------------------------------------------------------------------------------
def test_f16_range_counter_counts_every_replay(gpu):
    """f16 packing, the guard-tripping input of tests/test_f16_range_gpu.py (_hot_flow_on_bright: Features.moduleOne channel 2
    at 3e4 per colour, a white frame gives 9e4 there) at 70x100.  Both nets are warmed by one pass on the hot pair (the first
    pass of a net runs its layers twice, eagerly: lazy allocations before any capture) and the counter reset; then one eager
    call plus two replays of the pair on the graph net count three times what one call on the graphs-off net counts."""
    lib = gpu.lib()
    sd = O.liteflownet_state_dict(4869)
    wt, b = sd["moduleFeatures.moduleOne.0.weight"], sd["moduleFeatures.moduleOne.0.bias"]
    wt[2] = 0.0
    wt[2, :, 3, 3] = 3.0e4
    b[2] = 0.0
    white, black = np.full((H, W, 3), 255, np.uint8), np.zeros((H, W, 3), np.uint8)
    nets = []
    try:
        gpu.check(lib.dfvo_set_conv_precision(b"f16"))
        for graph in (0, 1):
            nets.append(make_flownet(gpu, H, W, sd, graph=graph)[0])
        for net in nets:
            _flow_host(gpu, net, white, black)
        gpu.f16s_overflow_count(reset=True)
        _flow_host(gpu, nets[0], white, black)
        one = gpu.f16s_overflow_count(reset=True)
        print("   f16 range events of one graphs-off pass on the hot pair: %d" % one)
        assert one > 0, "the hot pair does not trip the range guard at %dx%d" % (H, W)
        gpu.check(lib.dfvo_flownet_set_graph(nets[1], 0))
        _flow_host(gpu, nets[1], white, black)
        assert gpu.f16s_overflow_count() == one
        gpu.check(lib.dfvo_flownet_set_graph(nets[1], 1))
        for rep in (2, 3):
            _flow_host(gpu, nets[1], white, black)
            assert gpu.f16s_overflow_count() == rep * one, "replay %d: the counter stands at %d, one pass counts %d" % (
                rep - 1, gpu.f16s_overflow_count(), one)
    finally:
        for net in nets:
            lib.dfvo_flownet_destroy(net)
        gpu.check(lib.dfvo_set_conv_precision(b"fp32"))
        gpu.f16s_overflow_count(reset=True)


# ---- 7. the frame session's stream orders ------------------------------------------------------------------------------------
# frame g: flags of its push.  Pair (0, 1) runs both frames through Features, (1, 2) carries frame 1's pyramids over, frame 3
# is pushed without a flow pass, so that (3, 4) is a full pass again and (4, 5) a carried one
SESSION_FLAGS = [0, 0, 0, 1, 0, 0]

_SESSION_CHILD = r"""
import ctypes as C, importlib, sys
import numpy as np
sys.path.insert(0, %(tests)r); sys.path.insert(0, %(root)r)
from oracle import nets_torch as O
import test_graph_replay_gpu as T
capi = importlib.import_module("df-vo_amd.capi")
capi.require_gpu()
lib = capi.lib()
H, W, FH, FW = T.H, T.W, T.FH, T.FW
flow, _, _ = T.make_flownet(capi, H, W, O.liteflownet_state_dict(4869), graph=1)
depth = T._make_depthnet(capi, O.monodepth2_state_dict(4869), 1)
sess = C.c_void_p()
capi.check(lib.dfvo_session_create(flow, depth, None, H, W, C.byref(sess)))
out = {}
def view(p, n):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (n,))
for g, (frame, flags) in enumerate(zip(T._frames(len(T.SESSION_FLAGS)), T.SESSION_FLAGS)):
    gen = C.c_longlong(-1)
    capi.check(lib.dfvo_session_push_frame(sess, capi.as_ptr(np.ascontiguousarray(frame)), None, None, flags, C.byref(gen)))
    assert gen.value == g
    p = C.c_void_p()
    capi.check(lib.dfvo_session_depth(sess, g, C.byref(p)))
    v = view(p, FH * FW)
    out["depth%%d" %% g] = v.copy()
    v[:] = np.nan  # the ring slot comes round again three frames on: it must have been written by then
    if g >= 1 and not flags:
        pf, pb, pd = C.c_void_p(), C.c_void_p(), C.c_void_p()
        capi.check(lib.dfvo_session_flow(sess, g, C.byref(pf), C.byref(pb), C.byref(pd)))
        for name, q, n in (("fwd", pf, 2 * H * W), ("bwd", pb, 2 * H * W), ("diff", pd, H * W)):
            v = view(q, n)
            out["%%s%%d" %% (name, g)] = v.copy()
            v[:] = np.nan
lib.dfvo_session_destroy(sess)
lib.dfvo_depthnet_destroy(depth)
lib.dfvo_flownet_destroy(flow)
np.savez(%(out)r, **out)
"""


def _session_eager(gpu):
    """what the session must hand out per generation, from graphs-off nets on the same frames"""
    if "session" not in _eager:
        lib = gpu.lib()
        frames = _frames(len(SESSION_FLAGS))
        want = {}
        dnet = _make_depthnet(gpu, O.monodepth2_state_dict(4869), 0)
        try:
            for g, f in enumerate(frames):
                want["depth%d" % g] = _depth_image_host(gpu, dnet, f).ravel()
        finally:
            lib.dfvo_depthnet_destroy(dnet)
        fnet, _, _ = make_flownet(gpu, H, W, O.liteflownet_state_dict(4869), graph=0)
        try:
            for g in range(1, len(frames)):
                if not SESSION_FLAGS[g]:
                    for name, a in zip(("fwd", "bwd", "diff"), _flow_host(gpu, fnet, frames[g - 1], frames[g])):
                        want["%s%d" % (name, g)] = a.ravel()
        finally:
            lib.dfvo_flownet_destroy(fnet)
        assert all(np.isfinite(a).all() for a in want.values())
        _eager["session"] = want
    return _eager["session"]


@pytest.mark.parametrize("order", ["0", "1", "2", "3"])
def test_session_stream_orders_equal_the_eager_nets(gpu, tmp_path, order):
    """DFVO_SESSION_ORDER (read at dfvo_session_create) 0 flow net enqueued first | 1 depth net first | 2 / 3 the depth net's
    captured graph launched into the flow net's stream, before / behind the flow net: six distinct frames through
    dfvo_session_push_frame in a fresh process with graphs on; the depth of every generation and the flow of every pair are
    bit-identical to graphs-off nets on the same frames -- hence to each other across the four orders"""
    want = _session_eager(gpu)
    tests = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / ("session_order_%s.npz" % order))
    env = dict(os.environ, DFVO_SESSION_ORDER=order, DFVO_CONV_PRECISION="fp32")
    code = _SESSION_CHILD % {"tests": tests, "root": os.path.dirname(tests), "out": out}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert sorted(got.files) == sorted(want)
    for k in sorted(want):
        assert _same(got[k], want[k]), "session order %s: %s differs from the graphs-off net" % (order, k)
