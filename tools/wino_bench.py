"""fp32 Winograd F(2x2,3x3) against the direct fp32 kernels, layer by layer: the record launch_conv's size rule for
dfvo_set_fp32_winograd(1) is derived from.

Every 3x3 / stride-1 shape of the flow net's large maps (level 2 at the 352 x 1216 and 384 x 1248 net sizes, batch of two; 128 /
64 / 32 wide) runs through dfvo_conv2d with the switch off and with it forced on (mode 2), each launch under its own HIP events
(dfvo_conv_profile_*; the weights are packed per call, outside the events).  Prints ONE JSON table: per shape the profile row
(= the window kernel's tile class), us per launch of both, their ratio, and both rates in algorithmic TFLOP/s (the direct
convolution's FLOP count: with the switch on that is an effective rate and may exceed the matrix peak).
usage: python tools/wino_bench.py [--iters 10] [--out FILE]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
capi = importlib.import_module("df-vo_amd.capi")

# (c0, c1, cout) of the level-2 layers: matching 52 (49 + pad) -> 128 -> 64 -> 32, sub-pixel 128 + 4 -> 128 -> 64 -> 32,
# regularisation 128 + 4 -> 128 -> 128 -> 64 -> 64 -> 32 -> 32; features 32 -> 32
LAYERS = [(52, 0, 128), (128, 4, 128), (128, 0, 128), (128, 0, 64), (64, 0, 64), (64, 0, 32), (32, 0, 32)]
MAPS = [(2, 176, 608), (2, 192, 624)]


def time_layer(lib, N, H, W, c0, c1, cout, mode, iters):
    capi.check(lib.dfvo_set_fp32_winograd(mode))
    cs0, cs1, dcs = (c0 + 3) // 4 * 4, (c1 + 3) // 4 * 4, (cout + 3) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(1)
    x0 = torch.randn(N, H, W, cs0, device="cuda", generator=g)
    x1 = torch.randn(N, H, W, cs1, device="cuda", generator=g) if c1 else None
    dst = torch.zeros(N, H, W, dcs, device="cuda")
    w = (np.random.RandomState(2).randn(cout, c0 + c1, 3, 3) * 0.05).astype(np.float32)
    b = np.zeros(cout, np.float32)
    desc = capi.ConvDesc(N=N, H=H, W=W, kh=3, kw=3, stride=1, pad_h=1, pad_w=1, pad_mode=0, c0=c0, cs0=cs0, co0=0, up0=0, c1=c1,
                         cs1=cs1, co1=0, cout=cout, act=1, act_param=0.1, res_cs=0, res_co=0, dst_cs=dcs, dst_co=0)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    call = lambda: capi.check(lib.dfvo_conv2d(C.byref(desc), p(x0), p(x1), capi.as_ptr(w), capi.as_ptr(b), None, p(dst), None))
    for _ in range(2):
        call()
    n = C.c_ulonglong(0)
    capi.check(lib.dfvo_fp32_winograd_launches(C.byref(n), 1))
    ms, fl, ln = np.zeros(24), np.zeros(24), np.zeros(24, np.int32)
    capi.check(lib.dfvo_conv_profile_begin())
    for _ in range(iters):
        call()
    capi.check(lib.dfvo_conv_profile_end(capi.as_ptr(ms), capi.as_ptr(fl), capi.as_ptr(ln)))
    capi.check(lib.dfvo_fp32_winograd_launches(C.byref(n), 1))
    assert n.value == (iters if mode else 0), "the layer did not take the expected kernel"
    i = int(np.argmax(ms))
    assert ln[i] == iters
    return i, ms[i] * 1e3 / iters, fl[i] / (ms[i] * 1e-3) / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = capi.lib()
    capi.require_gpu()
    capi.check(lib.dfvo_set_conv_precision(b"fp32"))
    before = lib.dfvo_get_fp32_winograd()
    rows = []
    try:
        for (N, H, W) in MAPS:
            for (c0, c1, cout) in LAYERS:
                cfg, us0, tf0 = time_layer(lib, N, H, W, c0, c1, cout, 0, a.iters)
                cfg2, us1, tf1 = time_layer(lib, N, H, W, c0, c1, cout, 2, a.iters)
                assert cfg == cfg2, "Winograd launches are filed under the row of the class they replace"
                rows.append({"N": N, "H": H, "W": W, "c0": c0, "c1": c1, "cout": cout, "cfg": cfg, "direct_us": round(us0, 1),
                             "winograd_us": round(us1, 1), "ratio": round(us1 / us0, 3), "direct_tflops": round(tf0, 1),
                             "winograd_effective_tflops": round(tf1, 1)})
    finally:
        capi.check(lib.dfvo_set_fp32_winograd(before))
    by_cfg = {}
    for r in rows:
        c = by_cfg.setdefault(str(r["cfg"]), {"direct_us": 0.0, "winograd_us": 0.0})
        c["direct_us"] += r["direct_us"]
        c["winograd_us"] += r["winograd_us"]
    for c in by_cfg.values():
        c["ratio"] = round(c["winograd_us"] / c["direct_us"], 3)
    line = json.dumps({"tool": "wino_bench", "iters": a.iters, "layers": rows, "by_class": by_cfg})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
