"""CPU: the arithmetic contract of the dense drawer panels and the drawer overlay.

tests/drawer_np.py restates, operation for operation, what df-vo_amd/csrc/vis.hip computes.  Here that restatement is pinned,
bit for bit, against (a) the reference's own flow_to_image and drawer methods (their output on seeded inputs is the fixture
tests/golden/frame_drawer.npz, written by tests/golden/make_golden_drawer.py under the installed numpy), (b) live matplotlib
and (c) np.percentile.  The GPU tests then compare the kernels with the same fixture."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import drawer_np as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = "/root/reference"


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "frame_drawer.npz"))


def test_tables_are_matplotlibs(fx):
    matplotlib = pytest.importorskip("matplotlib")
    t = D.load_tables()
    for name in ("magma", "jet"):
        want = (matplotlib.colormaps[name](np.arange(256))[:, :3] * 255).astype(np.uint8)
        assert np.array_equal(t[name], want), name
    assert t["wheel"].shape == (55, 3) and tuple(t["wheel"][0]) == (255, 0, 0) and tuple(t["wheel"][15]) == (255, 255, 0)


@pytest.mark.parametrize("h,w", [(37, 53), (96, 160)])
@pytest.mark.parametrize("name", D.FLOW_GENERIC + D.FLOW_LATTICE)
def test_wheel_restatement_equals_flow_to_image(fx, name, h, w):
    flow = D.flow_case(name, h, w)
    img, n_unknown = D.flow_to_image_np(flow)
    ref = fx["flow_rgb/%s@%dx%d" % (name, h, w)]
    assert (img != ref).any(-1).sum() == 0
    assert n_unknown == (2 if name == "specials" else 0)
    if name == "specials":  # the entries flow_to_image zeroes in its caller's array are the unknown ones, both components
        idx = fx["flow_after_idx/%s@%dx%d" % (name, h, w)]
        _, unknown = D.flow_max_radius(flow)
        changed = {(int(c), int(y), int(x)) for c, y, x in idx}
        want = {(c, int(y), int(x)) for y, x in np.argwhere(unknown) for c in (0, 1) if flow[c, y, x] != 0}
        assert changed == want and np.all(fx["flow_after_val/%s@%dx%d" % (name, h, w)] == 0)


def test_signed_zero_pixels_are_on_the_references_side(fx):
    """arctan2(-v, -u) honours the sign of a zero: in the REFERENCE's own image of the lattice_axes flow, u = 1 with v = -0
    (x = 5) and u = 1 with v = +0 (x = 14) on an even row are different wheel entries -- and u = -1 (x = 3, x = 12) is the same
    entry for both zeros.  The restatement gives the reference's pixel at each of them."""
    h, w = 37, 53
    flow = D.flow_case("lattice_axes", h, w)
    ref = fx["flow_rgb/lattice_axes@%dx%d" % (h, w)]
    assert flow[0, 0, 5] == flow[0, 0, 14] == 1 and np.signbit(flow[1, 0, 5]) and not np.signbit(flow[1, 0, 14]) and flow[1, 0, 5] == 0
    assert flow[0, 0, 3] == flow[0, 0, 12] == -1 and np.signbit(flow[1, 0, 3]) != np.signbit(flow[1, 0, 12])
    assert not np.array_equal(ref[0, 5], ref[0, 14]) and np.abs(ref[0, 5].astype(int) - ref[0, 14]).max() > 10
    assert np.array_equal(ref[0, 3], ref[0, 12])
    img, _ = D.flow_to_image_np(flow)
    for x in (3, 5, 12, 14):
        assert np.array_equal(img[0, x], ref[0, x])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["magma", "jet"])
def test_colour_map_restatement_equals_matplotlib(name, dtype):
    mpl = pytest.importorskip("matplotlib")
    import matplotlib.cm  # noqa: F401
    rng = np.random.RandomState(5)
    x = (rng.rand(64, 96) * 1.3 - 0.1).astype(dtype)
    x[0, :8] = [0, -0.0, 1, 1.0000001, np.inf, -np.inf, np.nan, 0.99999994]
    x[1, :] = np.linspace(0, 1, 96)
    for vmax in (1, 0.1, 3.0, 50.0, 0.0, np.float32(0.7351), np.nan):
        with np.errstate(all="ignore"):
            mapper = mpl.cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=0, vmax=vmax), cmap=name)
            want = (mapper.to_rgba(x)[:, :, :3] * 255).astype(np.uint8)
        got = D.cmap_np(x, float(vmax), name)
        assert (got != want).any(-1).sum() == 0, (name, dtype, vmax)


def test_panel_restatement_equals_the_references_methods(fx):
    """every panel case of the fixture: the image the reference's draw_* handed to update_data"""
    for (h, w), specs in D.PANELS_BY_MAP.items():
        for spec in specs:
            kind = spec.split(":")[0]
            x = D.panel_input(spec, h, w)
            if kind == "flow":
                img = D.flow_to_image_np(x)[0]
            elif kind in ("disp", "depth"):
                img = D.depth_panel_np(x, kind, D.MAX_DEPTH)[0]
            else:
                img = D.cmap_np(x, D.JET_VMAX[spec.split(":")[2]], "jet")
            assert (img != fx[D.panel_key(spec, h, w)]).any(-1).sum() == 0, (spec, h, w)
    assert json.loads(str(fx["raises"])) == {}  # (matplotlib colours a map with a NaN, and a NaN vmax, without raising)


@pytest.mark.parametrize("name,depth", D.percentile_cases(), ids=[c[0] for c in D.percentile_cases()])
def test_percentile_restatement_equals_numpy(fx, name, depth):
    disp = 1 / (depth + 1e-3)
    disp[depth == 0] = 0
    assert np.array_equal(disp, D.disparity_np(depth)) and disp.dtype == depth.dtype
    want = np.percentile(disp, 90)
    got = D.percentile90_np(disp)
    assert got.dtype == want.dtype == depth.dtype and got.tobytes() == want.tobytes(), (name, got, want)
    assert np.float64(want) == fx["pct/" + name]
    with_nan = np.concatenate([disp, [np.nan]]).astype(depth.dtype)
    assert np.isnan(D.percentile90_np(with_nan)) and np.isnan(np.percentile(with_nan, 90))


_OVERLAY_SCRIPT = r"""
import importlib, json, sys, types
sys.path.insert(0, %(root)r); sys.path.insert(0, %(ref)r)
import __graft_entry__ as g
g.dfvo_amd()
importlib.import_module("df-vo_amd.overlay").install()
assert "cv2" not in sys.modules
cv2 = types.ModuleType("cv2")   # the stub: frame_drawer.py and libs.general.utils only import it
sys.modules["cv2"] = cv2
from libs.general.frame_drawer import FrameDrawer, draw_match_temporal
import libs.general.frame_drawer as stand_in
ref = sys.modules["libs.general._dfvo_reference_frame_drawer"]
ours = importlib.import_module("df-vo_amd.libs.general.frame_drawer")
class NS(dict):
    __getattr__ = dict.__getitem__
d = FrameDrawer(NS(window_h=600, window_w=1000, trajectory=NS(vis_scale=1)))
print(json.dumps({
    "mro_has_reference": ref.FrameDrawer in FrameDrawer.__mro__,
    "draw_traj_is_reference": FrameDrawer.draw_traj is ref.FrameDrawer.draw_traj,
    "main_is_reference": FrameDrawer.main is ref.FrameDrawer.main,
    "dense_are_ours": all(getattr(FrameDrawer, m) is getattr(ours.DenseMixin, m) for m in
                          ("draw_depth", "draw_flow", "draw_flow_consistency", "draw_rigid_flow_consistency")),
    "module_passthrough": draw_match_temporal is ref.draw_match_temporal and stand_in.draw_match_side is ref.draw_match_side,
    "ref_file": ref.__file__,
    "layout": {k: [int(v.__array_interface__["data"][0] - d.img.__array_interface__["data"][0]), list(v.shape)] for k, v in d.data.items()},
    "display": d.display, "traj0": [d.traj_y0, d.traj_x0], "img": list(d.img.shape),
}))
"""


def test_overlay_resolves_the_drawer_to_a_subclass_of_the_references():
    if not os.path.isdir(os.path.join(REFERENCE, "libs", "general")):
        pytest.skip("the reference checkout is not on this machine")
    pytest.importorskip("matplotlib")
    r = subprocess.run([sys.executable, "-W", "ignore", "-c", _OVERLAY_SCRIPT % {"root": ROOT, "ref": REFERENCE}], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mro_has_reference"] and out["draw_traj_is_reference"] and out["main_is_reference"]
    assert out["dense_are_ours"] and out["module_passthrough"]
    assert out["ref_file"] == os.path.join(REFERENCE, "libs", "general", "frame_drawer.py")
    # the reference's layout: every item a view of the 600 x 1000 window at its quarter-grid rectangle
    assert out["img"] == [600, 1000, 3] and out["traj0"] == [270, 250] and all(out["display"].values())
    rect = {"traj": (0, 0, 600, 500), "match_temp": (0, 500, 150, 1000), "match_side": (150, 500, 300, 1000),
            "depth": (300, 500, 450, 750), "flow1": (300, 750, 450, 1000), "flow2": (450, 500, 600, 750),
            "rigid_flow_diff": (450, 500, 600, 750), "opt_flow_diff": (450, 750, 600, 1000), "warp_diff": (450, 500, 600, 750)}
    assert set(out["layout"]) == set(rect)
    for k, (y0, x0, y1, x1) in rect.items():
        assert out["layout"][k] == [(y0 * 1000 + x0) * 3, [y1 - y0, x1 - x0, 3]], k
    cells = D.layout(600, 1000)
    for item, cell in D.CELLS.items():
        assert tuple(rect[item]) == cells[cell]


def test_consistency_map_as_kp_selection_hands_it_over_is_recognised(capi):
    """kp_selection returns np.asarray(copy, float32).reshape(h, w): a plain view of a plain view of the token-carrying copy.
    The drawer's test must find the owner's token through that chain, and must still compare the contents."""
    import importlib
    import types
    sess = importlib.import_module("df-vo_amd.libs.deep_models.session")
    h, w = 6, 8
    mine = np.arange(h * w, dtype=np.float32).reshape(h, w, 1).view(sess.SessionArray)
    mine._dfvo_tok = (3, 5, "diff")
    fake = types.SimpleNamespace(sid=3, gen=5, flow_views=(5, None, None, mine))
    check = lambda a, name="diff": sess.FrameSession.vis_is_buffer(fake, a, name)  # noqa: E731
    copy = mine.copy()
    mask = np.asarray(copy, dtype=np.float32).reshape(h, w)
    assert type(mask) is np.ndarray and getattr(mask, "_dfvo_tok", None) is None
    assert check(copy) and check(mask)
    assert not check(np.array(mask))          # an owned plain copy carries no token: uploaded
    assert not check(mask, "fwd")
    np.asarray(copy)[2, 3, 0] = -1.0          # written through a plain view: token intact, contents differ
    assert not check(mask) and not check(copy)
    copy2 = mine.copy()
    copy2[0, 0, 0] = copy2[0, 0, 0]           # a write through the array object drops the token, whatever was written
    assert not check(np.asarray(copy2).reshape(h, w))
    fake.gen = 6
    assert not check(mine.copy())
