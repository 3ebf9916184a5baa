"""What reading a sequence from disk costs the fused pipeline (df-vo_amd/frame_stream.py), measured in one process:
    python tools/bench_stream.py [--frames 200] [--out profiles/stream_rates.json]
  decode_only   frames/s of the host decode alone (Pillow -> a host buffer, frame_stream.decode) at 1 / 2 / 4 / 8 / 12 worker
                threads, for the files that are streamed and for KITTI-like files (band-limited noise, about 1 MB each: the
                tunnel world's frames compress better than a camera's and decode faster)
  resident      sequence.run_sequence over the frames resident on the device (what bench.py measures: 376 x 1241, the coded tunnel
                world, two frames in turn, f16x3)
  streamed      the same run over a FrameStream of the PNG files at each worker count and ring size (--slots), with the
                consumer's wait times (for a decode / for a slot's event) per frame
  resident_idle_ring   the resident run again with an idle frame ring alive: what the extra stream costs
Writes about --frames PNG files of 376 x 1241 into a temporary directory.  Nothing is gated on the rates."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 376, 1241
WORKERS = (1, 2, 4, 8, 12)


def decode_rate(fs, paths, workers, reps):
    """frames/s of `workers` threads decoding paths (each `reps` times) into host buffers of their own"""
    jobs = list(paths) * reps
    stages = [np.zeros(H * W * 3, np.uint8) for _ in range(workers)]

    def work(i):
        for p in jobs[i::workers]:
            fs.decode(p, "image", stages[i])

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=workers) as ex:
        list(ex.map(work, range(workers)))
    dt = time.perf_counter() - t0
    return dict(workers=workers, frames=len(jobs), frames_per_s=len(jobs) / dt, ms_per_frame_per_thread=dt * 1e3 * workers / len(jobs))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--slots", default="8,12,16", help="ring sizes to stream with (the first one also sizes the idle ring)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_rates.json"))
    a = ap.parse_args(argv)
    os.environ.setdefault("DFVO_CONV_PRECISION", "f16x3")  # bench.py's headline arithmetic, read when the layers are packed
    from PIL import Image
    import torch
    syn = importlib.import_module("df-vo_amd.synthetic")
    pmod = importlib.import_module("df-vo_amd.pipeline")
    smod = importlib.import_module("df-vo_amd.sequence")
    fs = importlib.import_module("df-vo_amd.frame_stream")
    n = a.frames
    slot_counts = [int(v) for v in a.slots.split(",")]
    # bench.py's workload: the coded tunnel world at 376 x 1241 (potential encoding, the sideways drive), two frames in turn
    seq = syn.coded_tunnel_sequence(H, W, 2, mode="pot", step=1.0, seed=7, poses=syn.tunnel_poses_lateral(2, 0.4))
    fsd, dsd = syn.crafted_liteflownet_state_dict(H, W, "pot"), syn.crafted_monodepth2_state_dict()
    res = dict(tool="bench_stream", height=H, width=W, frames=n, slots=slot_counts, conv_precision=os.environ["DFVO_CONV_PRECISION"],
               cpus=len(os.sched_getaffinity(0)))
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for k in range(n):
            p = os.path.join(tmp, "%06d.png" % k)
            Image.fromarray(seq["frames"][k % 2]).save(p, compress_level=6)
            paths.append(p)
        rng = np.random.Generator(np.random.PCG64(5))
        noise = []
        for k in range(16):
            img = np.clip(128.0 + 40.0 * syn.smooth_noise(rng, H, W, sigmas=(0.7, 1.5, 3, 8)) / 2.0, 0, 255)
            p = os.path.join(tmp, "noise_%02d.png" % k)
            Image.fromarray(img.astype(np.uint8)).save(p, compress_level=6)
            noise.append(p)
        res["png_bytes_streamed"] = int(np.mean([os.path.getsize(p) for p in paths]))
        res["png_bytes_kitti_like"] = int(np.mean([os.path.getsize(p) for p in noise]))
        res["decode_only_streamed_files"] = [decode_rate(fs, paths, w, 1) for w in WORKERS]
        res["decode_only_kitti_like_files"] = [decode_rate(fs, noise, w, max(1, n // (2 * len(noise)))) for w in WORKERS]
        for r in res["decode_only_streamed_files"] + res["decode_only_kitti_like_files"]:
            print(json.dumps(r), flush=True)

        pipe = pmod.TrackingPipeline(H, W, 192, 640, seq["K"], fsd, dsd, seed=4869)
        try:
            two = smod.frames_to_device([seq["frames"][0], seq["frames"][1]])
            frames = [two[k % 2] for k in range(n)]
            torch.cuda.synchronize()
            smod.track_chunk(pipe, frames, 0, 10, rng_mode="per_pair")  # warm-up (clocks, autotuned layer configurations)

            def timed(fr):
                t0 = time.perf_counter()
                traj, rows = smod.run_sequence(pipe, fr, n, rng_mode="per_pair")
                torch.cuda.synchronize()
                return (n - 1) / (time.perf_counter() - t0), rows

            rate, want = timed(frames)
            res["resident"] = dict(frames_per_s=rate, status=np.bincount(want[:, 16].astype(int), minlength=5).tolist())
            print(json.dumps(res["resident"]), flush=True)
            res["streamed"] = []
            for slots, w in [(c, w) for c in slot_counts for w in WORKERS]:
                with fs.FrameStream(paths, H, W, slots=slots, workers=w) as s:
                    rate, rows = timed(s)
                    r = dict(slots=slots, workers=w, frames_per_s=rate, equal_to_resident=bool(np.array_equal(rows, want)),
                             wait_decode_ms_per_frame=s.wait_decode_s * 1e3 / n, wait_device_ms_per_frame=s.wait_device_s * 1e3 / n,
                             max_live=s.max_live)
                res["streamed"].append(r)
                print(json.dumps(r), flush=True)
            ring = fs.FrameRing(slot_counts[0], H * W * 3)
            try:
                rate, rows = timed(frames)
            finally:
                ring.close()
            res["resident_idle_ring"] = dict(frames_per_s=rate, equal_to_resident=bool(np.array_equal(rows, want)))
            rate, _ = timed(frames)
            res["resident_again"] = dict(frames_per_s=rate)
            # the same comparison under a camera's decode load: the KITTI-like files in turn (another workload for the solvers
            # -- noise frames -- so its resident rate is its own).  Last, and kept apart: a pair the crafted nets cannot track
            # on noise ends this leg only
            try:
                sixteen = smod.frames_to_device([np.array(Image.open(p)) for p in noise])
                torch.cuda.synchronize()
                rate, want = timed([sixteen[k % len(noise)] for k in range(n)])
                leg = dict(resident=dict(frames_per_s=rate, status=np.bincount(want[:, 16].astype(int), minlength=5).tolist()), streamed=[])
                for w in (2, 4, 6, 8, 12):
                    with fs.FrameStream([noise[k % len(noise)] for k in range(n)], H, W, slots=12, workers=w) as s:
                        try:
                            rate, rows = timed(s)
                        except Exception:
                            pipe.sync()  # before the stream closes: the pipeline may still read its frames
                            raise
                        leg["streamed"].append(dict(slots=12, workers=w, frames_per_s=rate, equal_to_resident=bool(np.array_equal(rows, want)),
                                                    wait_decode_ms_per_frame=s.wait_decode_s * 1e3 / n,
                                                    wait_device_ms_per_frame=s.wait_device_s * 1e3 / n))
                    print(json.dumps(leg["streamed"][-1]), flush=True)
                res["kitti_like_files"] = leg
            except Exception as e:
                res["kitti_like_files"] = dict(error="%s: %s" % (type(e).__name__, e))
            print(json.dumps(res["kitti_like_files"].get("resident", res["kitti_like_files"])), flush=True)
        finally:
            pipe.sync()
            pipe.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(resident=res["resident"], resident_idle_ring=res["resident_idle_ring"], resident_again=res["resident_again"])))


if __name__ == "__main__":
    main()
