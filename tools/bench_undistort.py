"""What the raw-frame input stage costs (df-vo_amd/undistort.py, csrc/undistort.hip), measured in one process:
    python tools/bench_undistort.py [--frames 120] [--out profiles/undistort_rates.json]
  kernel        HIP-event time of one launch at RobotCar's 960 x 1280: demosaic + remap inside the runner's crop (rows 0 .. 768) and on
                the whole frame, demosaic alone, the remap of an RGB frame; median of --reps launches, with the bytes each must move
  decode        Pillow's cost per frame and thread for a 1-channel 960 x 1280 mosaic PNG against the same content demosaiced and
                stored as an RGB PNG (frame_stream.decode into a host buffer, 1 and 4 threads)
  pairs         tools/bench_stream.py's protocol at 256 x 640: sequence.run_sequence over frames resident on the device against the
                same run over a FrameStream of the mosaic files (960 x 1280, crop rows 0 .. 768, the barrel table), f16x3
Nothing is gated on the rates."""
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

RAW_H, RAW_W = 960, 1280
H, W = 256, 640
CROP = [[0.0, 0.8], [0.0, 1.0]]


def barrel_map(h, w, k=-0.05):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cy, cx = (h - 1) / 2, (w - 1) / 2
    r2 = ((yy - cy) ** 2 + (xx - cx) ** 2) / (cy * cy + cx * cx)
    return np.stack([(cx + (xx - cx) * (1 + k * r2)).reshape(-1), (cy + (yy - cy) * (1 + k * r2)).reshape(-1)])


def mosaic_gbrg(rgb):
    """the gbrg Bayer mosaic (G B / R G) of an RGB frame"""
    site = np.zeros(rgb.shape[:2], np.int64)
    site[0::2, 0::2], site[0::2, 1::2], site[1::2, 0::2], site[1::2, 1::2] = 1, 2, 0, 1
    return np.ascontiguousarray(np.take_along_axis(rgb, site[..., None], 2)[..., 0])


def camera_like(syn, rng):
    """band-limited noise, uint8 [RAW_H, RAW_W, 3]: compresses like a camera frame (tools/bench_stream.py)"""
    return np.clip(128.0 + 40.0 * syn.smooth_noise(rng, RAW_H, RAW_W, sigmas=(0.7, 1.5, 3, 8)) / 2.0, 0, 255).astype(np.uint8)


def event_ms(torch, launch, reps):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def decode_ms(fs, paths, workers, reps, nbytes):
    jobs = list(paths) * reps
    stages = [np.zeros(nbytes, np.uint8) for _ in range(workers)]

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
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_rates.json"))
    a = ap.parse_args(argv)
    os.environ.setdefault("DFVO_CONV_PRECISION", "f16x3")
    from PIL import Image
    import torch
    syn = importlib.import_module("df-vo_amd.synthetic")
    pmod = importlib.import_module("df-vo_amd.pipeline")
    smod = importlib.import_module("df-vo_amd.sequence")
    fs = importlib.import_module("df-vo_amd.frame_stream")
    ud = importlib.import_module("df-vo_amd.undistort")
    n = a.frames
    res = dict(tool="bench_undistort", raw_size=[RAW_H, RAW_W], size=[H, W], frames=n, conv_precision=os.environ["DFVO_CONV_PRECISION"],
               cpus=len(os.sched_getaffinity(0)))
    rng = np.random.Generator(np.random.PCG64(5))
    umap = ud.UndistortMap(RAW_H, RAW_W, barrel_map(RAW_H, RAW_W))
    try:
        # ---- kernel ----
        d_m = torch.from_numpy(mosaic_gbrg(camera_like(syn, rng))).cuda()
        d_rgb = torch.empty((RAW_H, RAW_W, 3), dtype=torch.uint8, device="cuda")
        d_out = torch.empty((RAW_H, RAW_W, 3), dtype=torch.uint8, device="cuda")
        crop_box = (0, int(RAW_H * 0.8), 0, RAW_W)
        full = (0, RAW_H, 0, RAW_W)
        px = RAW_H * RAW_W
        legs = [("mosaic_remap_crop", lambda: ud.undistort_mosaic(d_m, umap, "gbrg", "reflect", crop_box, d_rgb), crop_box[1] * RAW_W * 19 + px),
                ("mosaic_remap_full", lambda: ud.undistort_mosaic(d_m, umap, "gbrg", "reflect", full, d_rgb), px * 20),
                ("demosaic_only_full", lambda: ud.undistort_mosaic(d_m, None, "gbrg", "reflect", full, d_rgb), px * 4),
                ("rgb_remap_full", lambda: ud.undistort_rgb(d_rgb, umap, full, d_out), px * 22)]
        res["kernel"] = {}
        for name, launch, nbytes in legs:
            med, best = event_ms(torch, launch, a.reps)
            res["kernel"][name] = dict(median_ms=med, min_ms=best, bytes=nbytes, gb_per_s_at_median=nbytes / med / 1e6)
            print(json.dumps({name: res["kernel"][name]}), flush=True)
        with tempfile.TemporaryDirectory() as tmp:
            # ---- decode: camera-like content (band-limited noise), as a mosaic and as its demosaiced RGB frame ----
            mono, colour = [], []
            for k in range(8):
                m = mosaic_gbrg(camera_like(syn, rng))
                rgb = ud.undistort_mosaic(torch.from_numpy(m).cuda(), None, "gbrg").cpu().numpy()
                mono.append(os.path.join(tmp, "m_%02d.png" % k))
                colour.append(os.path.join(tmp, "c_%02d.png" % k))
                Image.fromarray(m).save(mono[-1], compress_level=6)
                Image.fromarray(rgb).save(colour[-1], compress_level=6)
            res["decode"] = dict(png_bytes_mosaic=int(np.mean([os.path.getsize(p) for p in mono])),
                                 png_bytes_rgb=int(np.mean([os.path.getsize(p) for p in colour])),
                                 mosaic=[decode_ms(fs, mono, w, 4, px * 3) for w in (1, 4)],
                                 rgb=[decode_ms(fs, colour, w, 4, px * 3) for w in (1, 4)])
            print(json.dumps(res["decode"]), flush=True)
            # ---- pairs: the pot world at the raw size, mosaicked, two frames in turn ----
            seq = syn.coded_tunnel_sequence(RAW_H, RAW_W, 2, mode="pot", step=1.0, seed=7, poses=syn.tunnel_poses_lateral(2, 0.4))
            mosaics = [mosaic_gbrg(f) for f in seq["frames"]]
            paths = []
            for k in range(n):
                p = os.path.join(tmp, "%d.png" % (10 ** 15 + k))
                Image.fromarray(mosaics[k % 2]).save(p, compress_level=6)
                paths.append(p)
            res["png_bytes_streamed"] = int(np.mean([os.path.getsize(p) for p in paths]))
            K = np.array(seq["K"], np.float64)
            K[0] *= W / RAW_W
            K[1] *= H / int(RAW_H * 0.8)
            fsd, dsd = syn.crafted_liteflownet_state_dict(H, W, "pot"), syn.crafted_monodepth2_state_dict()
            pipe = pmod.TrackingPipeline(H, W, 192, 640, K, fsd, dsd, seed=4869)
            try:
                two = [ud.mosaic_to_device(m, H, W, umap, "gbrg", CROP) for m in mosaics]
                frames = [two[k % 2] for k in range(n)]
                smod.track_chunk(pipe, frames, 0, 10, rng_mode="per_pair")  # warm-up

                def timed(fr):
                    t0 = time.perf_counter()
                    traj, rows = smod.run_sequence(pipe, fr, n, rng_mode="per_pair")
                    torch.cuda.synchronize()
                    return (n - 1) / (time.perf_counter() - t0), rows

                rate, want = timed(frames)
                res["resident"] = dict(pairs_per_s=rate, status=np.bincount(want[:, 16].astype(int), minlength=5).tolist())
                print(json.dumps(res["resident"]), flush=True)
                res["streamed"] = []
                for slots, w in ((12, 2), (12, 4), (12, 6)):
                    with fs.FrameStream(paths, H, W, crop=CROP, slots=slots, workers=w, mosaic="gbrg", undistort=umap) as s:
                        try:
                            rate, rows = timed(s)
                        except Exception:
                            pipe.sync()
                            raise
                        r = dict(slots=slots, workers=w, pairs_per_s=rate, equal_to_resident=bool(np.array_equal(rows, want)),
                                 wait_decode_ms_per_frame=s.wait_decode_s * 1e3 / n, wait_device_ms_per_frame=s.wait_device_s * 1e3 / n)
                    res["streamed"].append(r)
                    print(json.dumps(r), flush=True)
                rate, _ = timed(frames)
                res["resident_again"] = dict(pairs_per_s=rate)
            finally:
                pipe.sync()
                pipe.close()
    finally:
        umap.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(kernel=res["kernel"], resident=res.get("resident"), streamed=res.get("streamed"))))


if __name__ == "__main__":
    main()
