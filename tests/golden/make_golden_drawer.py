"""Writes tests/golden/frame_drawer.npz: what the REFERENCE's drawer computes for the dense panels, on seeded inputs.

Needs the reference checkout (default /root/reference, or argv[1]) and matplotlib; cv2 is a stand-in made here:
`oracle.cv2_shim.resize` (the restatement of OpenCV 3.4.3's 8-bit INTER_LINEAR) and a channel flip for cvtColor.  The
reference's own FrameDrawer.draw_depth / draw_flow / draw_flow_consistency / draw_rigid_flow_consistency and
flowlib.flow_to_image run unmodified; the RGB image each hands to update_data is recorded where cvtColor receives it.

Stored: img/<case>@<h>x<w> (full-resolution RGB the reference computed; the tests resize it into the cell themselves),
flow_rgb/<flow>@<h>x<w> (+ flow_after_idx / _val: the entries of the caller's array the call changed, `specials` flow), pct/<case> (np.percentile of the
disparity), raises (JSON: case -> exception type name).  Inputs come from tests/drawer_np.py by name."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, REF)

import drawer_np as D  # noqa: E402
from oracle import cv2_shim  # noqa: E402

recorded = []


def _cvt(img, code):
    recorded.append(np.array(img))
    return np.ascontiguousarray(img[..., ::-1])


cv2 = types.ModuleType("cv2")
cv2.COLOR_RGB2BGR = 4
cv2.INTER_LINEAR = cv2_shim.INTER_LINEAR
cv2.INTER_NEAREST = cv2_shim.INTER_NEAREST
cv2.cvtColor = _cvt
cv2.resize = cv2_shim.resize
sys.modules["cv2"] = cv2

import matplotlib.cm  # noqa: E402,F401  (frame_drawer.py uses mpl.cm after `import matplotlib as mpl`)
from libs.flowlib.flowlib import flow_to_image  # noqa: E402
from libs.general.frame_drawer import FrameDrawer  # noqa: E402


class NS(dict):
    __getattr__ = dict.__getitem__


def make_vo(cur_data, depth_disp="disp", tracking=False, ratio=False):
    cfg = NS(visualization=NS(depth=NS(use_tracking_depth=tracking, depth_disp=depth_disp)),
             depth=NS(max_depth=D.MAX_DEPTH),
             kp_selection=NS(local_bestN=NS(enable=True, score_method="flow_ratio" if ratio else "flow"),
                             rigid_flow_kp=NS(rigid_flow_thre=D.RIGID_FLOW_THRE)))
    return NS(cfg=cfg, cur_data=cur_data)


def main():
    out, raises = {}, {}
    drawer = FrameDrawer(NS(window_h=600, window_w=1000, trajectory=NS(vis_scale=1)))
    for (h, w), specs in D.PANELS_BY_MAP.items():
        for spec in specs:
            kind = spec.split(":")[0]
            x = D.panel_input(spec, h, w)
            del recorded[:]
            try:
                if kind == "flow":
                    drawer.draw_flow(x.copy(), "flow1")
                elif kind in ("disp", "depth"):
                    f8 = spec.endswith("f8")  # the float64 map is the tracking depth (use_tracking_depth)
                    drawer.draw_depth(make_vo({"depth" if f8 else "raw_depth": x}, depth_disp=kind, tracking=f8))
                elif spec.endswith("rigid"):
                    drawer.draw_rigid_flow_consistency(make_vo({"rigid_flow_mask": x}))
                else:
                    drawer.draw_flow_consistency(make_vo({"fb_flow_mask": x}, ratio=spec.endswith("ratio")))
            except Exception as e:  # noqa: BLE001
                raises[D.panel_key(spec, h, w)] = type(e).__name__
                continue
            assert len(recorded) == 1 and recorded[0].shape == (h, w, 3) and recorded[0].dtype == np.uint8, spec
            key = D.panel_key(spec, h, w)
            assert key not in out or np.array_equal(out[key], recorded[0])
            out[key] = recorded[0]
    for h, w in ((37, 53), (96, 160)):
        for name in D.FLOW_GENERIC + D.FLOW_LATTICE:
            f = D.flow_case(name, h, w)
            with np.errstate(all="ignore"):
                img = flow_to_image(f.transpose(1, 2, 0))
            key = "flow_rgb/%s@%dx%d" % (name, h, w)
            assert key not in out or np.array_equal(out[key], img)  # (draw_flow handed update_data the same image)
            out[key] = img
            if name == "specials":  # flow_to_image zeroed the unknown entries in the caller's array: where, and to what
                f0 = D.flow_case(name, h, w)
                changed = np.argwhere(f.view(np.uint32) != f0.view(np.uint32))
                out["flow_after_idx/%s@%dx%d" % (name, h, w)] = changed
                out["flow_after_val/%s@%dx%d" % (name, h, w)] = f[tuple(changed.T)]
    for name, d in D.percentile_cases() + [("map192x640_float32", D.depth_case("rand", 192, 640).ravel()),
                                           ("map192x640_float64", D.depth_case("rand", 192, 640, np.float64).ravel())]:
        disp = 1 / (d + 1e-3)
        disp[d == 0] = 0
        p = np.percentile(disp, 90)
        assert p.dtype == d.dtype
        out["pct/" + name] = np.float64(p)
    out["raises"] = np.array(json.dumps(raises))
    out["versions"] = np.array(json.dumps({"numpy": np.__version__, "matplotlib": __import__("matplotlib").__version__}))
    path = os.path.join(HERE, "frame_drawer.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "entries; raises:", raises)


if __name__ == "__main__":
    main()
