"""Child process of tests/test_stream_layout_gpu.py: one 192 x 640 fused pipeline in the stream layout this process's
environment selects (GPU_MAX_HW_QUEUES is read once, when HIP starts; DFVO_STREAM_LAYOUT by dfvo_pipeline_create), driven
the way bench.py drives it.  Prints the layout and, per tracked pair, one JSON line of everything a layout could disturb."""
import importlib
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SLOTS, AHEAD, H, W = 4, 3, 192, 640


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def main():
    import torch
    torch.cuda.set_device(0)
    importlib.import_module("df-vo_amd")
    capi = importlib.import_module("df-vo_amd.capi")
    syn = importlib.import_module("df-vo_amd.synthetic")
    pmod = importlib.import_module("df-vo_amd.pipeline")
    capi.check(capi.lib().dfvo_set_conv_precision(b"f16x3"))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    mode = "mux" if syn._net_size(H, W) == (H, W) else "pot"
    seq = syn.coded_tunnel_sequence(H, W, 2, mode=mode, step=1.0, seed=7,
                                    poses=None if mode == "mux" else syn.tunnel_poses_lateral(2, 0.4))
    pipe = pmod.TrackingPipeline(H, W, 192, 640, seq["K"], syn.crafted_liteflownet_state_dict(H, W, mode),
                                 syn.crafted_monodepth2_state_dict(), seed=4869)
    print("LAYOUT " + json.dumps(pipe.stream_layout()), flush=True)
    d_frames = [dev(f) for f in seq["frames"][:2]]

    def report(tag, k, pipe, out, rel):
        fwd, bwd, diff, _, dep = pipe.get_outputs(k % SLOTS)  # (device-wide sync: the slot is reused four pairs later)
        print("PAIR " + json.dumps(dict(
            run=tag, pair=k, pose=rel.astype(np.float64).tobytes().hex(), status=int(out.status), n_kp=int(out.n_kp),
            inliers=int(out.best_inlier_cnt), scale_inliers=int(out.scale_n_inliers), scale_trials=int(out.scale_n_trials),
            pnp_inliers=int(out.pnp_inliers), crc_fwd=crc(fwd), crc_bwd=crc(bwd), crc_diff=crc(diff), crc_depth=crc(dep))),
            flush=True)

    # (a) bench.py's software pipeline on the coded sequence A, B, A, B ...: nets three pairs ahead with the pre-part right
    # behind them, carried features from the second pair on; SLOTS + 3 pairs, so every slot is reused and both flow-net
    # instances carry
    n = SLOTS + 3
    pipe.set_ref_image(d_frames[0])

    def feed(j):
        pipe.enqueue_nets(j % SLOTS, None if j > 0 else d_frames[j % 2], d_frames[1 - j % 2], None)
        pipe.prefetch_track(j % SLOTS)

    fed, prev = 0, np.eye(4)
    feed(0)
    fed = 1
    for k in range(n):
        pipe.track_begin(k % SLOTS)
        while fed < n and fed <= k + AHEAD:
            feed(fed)
            fed += 1
        out = pipe.track_end(k % SLOTS)
        rel, _ = pipe.hybrid_pose(out, prev)
        prev = rel
        report("coded", k, pipe, out, rel)
    pipe.sync()
    print("RNG coded %08x" % crc(pipe.get_rng_state()[1]), flush=True)

    # (b) the solver stage on a synthetic rigid scene handed in as overrides (pairs that take the PnP fallback among them),
    # once with the pre-part prefetched behind the nets and once left to track_begin (the late pre-part)
    sc = syn.rigid_scene(H, W, seed=3 + H)
    dflow, ddiff, ddepth, dref_depth = dev(sc["flow"]), dev(sc["diff"]), dev(sc["depth_cur"]), dev(sc["depth_ref"])
    for tag, prefetch in (("rigid_prefetch", True), ("rigid_late", False)):
        pipe.seed(4869)
        pipe.set_ref_depth(depth=dref_depth)
        prev = np.eye(4)
        for k in range(3):
            pipe.enqueue_nets(k % SLOTS, d_frames[k % 2], d_frames[1 - k % 2], None)
            if prefetch:
                pipe.prefetch_track(k % SLOTS, dflow, ddiff)
            pipe.track_begin(k % SLOTS, dflow, ddiff, ddepth)
            out = pipe.track_end(k % SLOTS)
            rel, _ = pipe.hybrid_pose(out, prev)
            prev = rel
            report(tag, k, pipe, out, rel)
        pipe.sync()
        print("RNG %s %08x" % (tag, crc(pipe.get_rng_state()[1])), flush=True)
    pipe.close()
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
