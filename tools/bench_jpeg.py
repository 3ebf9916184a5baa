"""What decoding JPEG frames costs, on the host and on the device (df-vo_amd/jpeg.py, FrameStream(jpeg=)), in one process:
    python tools/bench_jpeg.py [--frames 200] [--out profiles/jpeg_rates.json]
Two sets of 376 x 1241 4:2:0 quality-95 files: KITTI-like ones (band-limited noise, as tools/bench_stream.py makes them) and the
coded tunnel world's two frames in turn (bench.py's workload).  For each set:
  host_ms_per_frame     one thread: Pillow's whole decode (frame_stream.decode) against the entropy pass alone
                        (dfvo_jpeg_entropy_decode), both into a host buffer
  device_decode_us      dfvo_jpeg_decode_u8 between two HIP events, median and spread of 200 (the coefficients are restored by
                        a device copy outside the events: the operator overwrites them)
  resident / streamed   sequence.run_sequence over frames resident on the device, and over FrameStream(jpeg="host") and
                        FrameStream(jpeg="device") at 1 / 2 / 4 workers and 12 slots, with whether the rows equal the resident
                        run's bit for bit and the consumer's waits per frame
Nothing is gated on the rates."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 376, 1241
WORKERS = (1, 2, 4)
SLOTS = 12


def host_ms(fs, jp, paths, reps):
    stage = np.zeros(fs.jpeg_capacity(H, W), np.uint8)
    blobs = [np.frombuffer(open(p, "rb").read(), np.uint8) for p in paths]
    out = {}
    t0 = time.perf_counter()
    for _ in range(reps):
        for p in paths:
            fs.decode(p, "image", stage)
    out["pillow_whole_decode"] = (time.perf_counter() - t0) * 1e3 / (reps * len(paths))
    t0 = time.perf_counter()
    for _ in range(reps):
        for b in blobs:
            jp.entropy_decode_into(b, stage)
    out["entropy_pass_alone"] = (time.perf_counter() - t0) * 1e3 / (reps * len(paths))
    t0 = time.perf_counter()
    for _ in range(reps):
        for p in paths:
            fs.decode_any(p, stage)
    out["entropy_pass_with_file_read"] = (time.perf_counter() - t0) * 1e3 / (reps * len(paths))
    return out


def device_us(torch, capi, jp, path, reps=200):
    info, buf, _ = jp.entropy_decode(path)
    keep = torch.from_numpy(buf).cuda()
    work = torch.empty_like(keep)
    dst = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    times = []
    for i in range(reps + 20):
        work.copy_(keep)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        capi.check(capi.lib().dfvo_jpeg_decode_u8(work.data_ptr(), C.byref(info), dst.data_ptr(), stream.cuda_stream))
        b.record(stream)
        b.synchronize()
        if i >= 20:
            times.append(a.elapsed_time(b) * 1e3)
    t = np.sort(np.array(times))
    return dict(reps=reps, median=float(np.median(t)), p10=float(t[len(t) // 10]), p90=float(t[len(t) * 9 // 10]), min=float(t[0]),
                max=float(t[-1]), blocks=int(sum(info.blocks_w[c] * info.blocks_h[c] for c in range(3))), upload_bytes=int(info.bytes))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_rates.json"))
    a = ap.parse_args(argv)
    os.environ.setdefault("DFVO_CONV_PRECISION", "f16x3")  # bench.py's headline arithmetic, read when the layers are packed
    from PIL import Image
    import torch
    syn = importlib.import_module("df-vo_amd.synthetic")
    pmod = importlib.import_module("df-vo_amd.pipeline")
    smod = importlib.import_module("df-vo_amd.sequence")
    fs = importlib.import_module("df-vo_amd.frame_stream")
    jp = importlib.import_module("df-vo_amd.jpeg")
    capi = importlib.import_module("df-vo_amd.capi")
    n = a.frames
    seq = syn.coded_tunnel_sequence(H, W, 2, mode="pot", step=1.0, seed=7, poses=syn.tunnel_poses_lateral(2, 0.4))
    fsd, dsd = syn.crafted_liteflownet_state_dict(H, W, "pot"), syn.crafted_monodepth2_state_dict()
    res = dict(tool="bench_jpeg", height=H, width=W, frames=n, slots=SLOTS, quality=95, subsampling="4:2:0",
               conv_precision=os.environ["DFVO_CONV_PRECISION"], cpus=len(os.sched_getaffinity(0)))
    with tempfile.TemporaryDirectory() as tmp:
        sets = {"tunnel_world": [], "kitti_like": []}
        for k in range(2):
            p = os.path.join(tmp, "tunnel_%d.jpg" % k)
            Image.fromarray(seq["frames"][k]).save(p, quality=95, subsampling=2)
            sets["tunnel_world"].append(p)
        rng = np.random.Generator(np.random.PCG64(5))
        for k in range(16):
            img = np.clip(128.0 + 40.0 * syn.smooth_noise(rng, H, W, sigmas=(0.7, 1.5, 3, 8)) / 2.0, 0, 255)
            p = os.path.join(tmp, "noise_%02d.jpg" % k)
            Image.fromarray(img.astype(np.uint8)).save(p, quality=95, subsampling=2)
            sets["kitti_like"].append(p)
        pipe = pmod.TrackingPipeline(H, W, 192, 640, seq["K"], fsd, dsd, seed=4869)
        try:
            warm = smod.frames_to_device([seq["frames"][0], seq["frames"][1]])
            torch.cuda.synchronize()
            smod.track_chunk(pipe, [warm[k % 2] for k in range(12)], 0, 10, rng_mode="per_pair")  # warm-up

            def timed(fr):
                t0 = time.perf_counter()
                _, rows = smod.run_sequence(pipe, fr, n, rng_mode="per_pair")
                torch.cuda.synchronize()
                return (n - 1) / (time.perf_counter() - t0), rows

            for name, files in sets.items():
                leg = dict(jpeg_bytes=int(np.mean([os.path.getsize(p) for p in files])))
                leg["host_ms_per_frame"] = host_ms(fs, jp, files, max(1, 64 // len(files)))
                leg["device_decode_us"] = device_us(torch, capi, jp, files[0])
                print(json.dumps({name: leg}), flush=True)
                paths = [files[k % len(files)] for k in range(n)]
                try:
                    some = smod.frames_to_device([np.array(Image.open(p)) for p in files])
                    torch.cuda.synchronize()
                    rate, want = timed([some[k % len(files)] for k in range(n)])
                    leg["resident"] = dict(frames_per_s=rate, status=np.bincount(want[:, 16].astype(int), minlength=5).tolist())
                    leg["streamed"] = []
                    for mode in ("host", "device"):
                        for w in WORKERS:
                            with fs.FrameStream(paths, H, W, slots=SLOTS, workers=w, jpeg=mode) as s:
                                try:
                                    rate, rows = timed(s)
                                except Exception:
                                    pipe.sync()  # before the stream closes: the pipeline may still read its frames
                                    raise
                                leg["streamed"].append(dict(jpeg=mode, workers=w, frames_per_s=rate,
                                                            equal_to_resident=bool(np.array_equal(rows, want)),
                                                            wait_decode_ms_per_frame=s.wait_decode_s * 1e3 / n,
                                                            wait_device_ms_per_frame=s.wait_device_s * 1e3 / n))
                            print(json.dumps(leg["streamed"][-1]), flush=True)
                    rate, _ = timed([some[k % len(files)] for k in range(n)])
                    leg["resident_again"] = dict(frames_per_s=rate)
                except Exception as e:  # (a pair the crafted nets cannot track on noise ends this leg only)
                    leg["error"] = "%s: %s" % (type(e).__name__, e)
                res[name] = leg
                print(json.dumps({name: {k: v for k, v in leg.items() if k != "streamed"}}), flush=True)
        finally:
            pipe.sync()
            pipe.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
