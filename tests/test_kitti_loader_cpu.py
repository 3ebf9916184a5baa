"""CPU: the KITTI dataset layer of df-vo_amd/kitti.py -- intrinsics, file names and the yaml merge -- against what the
reference's own loaders returned (tests/golden/kitti_loader.json, written by tests/golden/make_golden_kitti_loader.py), and the
runner's refusals that need no device."""
import importlib
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kmod():
    import __graft_entry__ as g
    g.dfvo_amd()
    return importlib.import_module("df-vo_amd.kitti")


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(HERE, "golden", "kitti_loader.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["seq00", "skewed"])
def test_intrinsics_equal_the_reference_loaders(kmod, fx, tmp_path, name):
    rec = fx["intrinsics"][name]
    p = tmp_path / "calib.txt"
    p.write_text(rec["text"])
    assert len(rec["sizes"]) == 2
    for s in rec["sizes"]:
        K = kmod.kitti_odom_intrinsics(str(p), s["h"], s["w"])
        cx, cy, fx_, fy = s["cx_cy_fx_fy"]
        assert K.shape == (3, 3) and K.dtype == np.float64
        assert np.array_equal(K, np.array([[fx_, 0, cx], [0, fy, cy], [0, 0, 1.0]])), (name, s)  # the same doubles


def test_intrinsics_scale_from_the_hard_coded_raw_size_not_the_files(kmod, fx, tmp_path):
    """1226 x 370 whatever the sequence's images are (seq 00's are 1241 x 376)"""
    p = tmp_path / "calib.txt"
    p.write_text(fx["intrinsics"]["seq00"]["text"])
    K = kmod.kitti_odom_intrinsics(str(p), 370, 1226)
    want = [718.856 / 1226.0 * 1226, 718.856 / 370.0 * 370, 607.1928 / 1226.0 * 1226, 185.2157 / 370.0 * 370]
    assert [K[0, 0], K[1, 1], K[0, 2], K[1, 2]] == want and np.allclose(want, [718.856, 718.856, 607.1928, 185.2157], rtol=1e-15)
    short = tmp_path / "short.txt"
    short.write_text("P0: 1 0 2 0 0 3 4 0 0 0 1 0\n")
    with pytest.raises(ValueError, match="short.txt"):
        kmod.kitti_odom_intrinsics(str(short), 192, 640)


@pytest.mark.parametrize("src", [None, "gt"])
def test_paths_are_the_ones_kitti_odom_builds(kmod, fx, tmp_path, src):
    rec = fx["paths"]
    want = rec["depth_src_%s" % src]
    root = tmp_path / "odom_data"
    img_dir = root / rec["seq"] / "image_2"
    img_dir.mkdir(parents=True)
    for i in range(rec["n_images"]):
        (img_dir / ("%06d.%s" % (i, rec["ext"]))).write_bytes(b"")
    (img_dir / "notes.txt").write_bytes(b"")
    got = kmod.kitti_odom_paths(str(root), rec["seq"], rec["ext"], str(tmp_path / "depth") if src == "gt" else None)
    rel = lambda ps: [os.path.relpath(p, str(tmp_path)) for p in ps]
    assert want["len"] == rec["n_images"] == len(got["images"])
    assert rel(got["images"]) == want["images"]
    assert os.path.relpath(got["calib"], str(tmp_path)) == os.path.join("odom_data", rec["seq"], "calib.txt")
    if src == "gt":
        assert rel(got["depths"]) == want["depths"] and got["depth_scale"] == want["depth_scale"] == 500
    else:
        assert got["depths"] is None and got["depth_scale"] is None and want["depths"] == []


def plain(node):
    if isinstance(node, dict):
        return {k: plain(v) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [plain(v) for v in node]
    return node


def test_yaml_merge_equals_config_loader(kmod, fx, tmp_path):
    rec = fx["merge"]
    d, o = tmp_path / "default.yml", tmp_path / "overlay.yml"
    d.write_text(rec["default_yml"])
    o.write_text(rec["overlay_yml"])
    cfg = kmod.cfg_from_yaml(str(d), str(o))
    assert plain(cfg) == rec["merged"]
    assert plain(kmod.cfg_from_yaml(str(d))) == rec["default_alone"] == plain(kmod.cfg_from_yaml(str(d), None))
    # a default_cfg.Cfg all the way down, dictionaries inside lists included (EasyDict's conversion)
    Cfg = importlib.import_module("df-vo_amd.default_cfg").Cfg
    assert isinstance(cfg, Cfg) and isinstance(cfg.depth.deep_depth, Cfg) and isinstance(cfg.new_top[1], Cfg)
    assert cfg.depth.depth_src == "gt" and cfg.image.ext == "png" and cfg.image.height == 192 and cfg.seq == "09"
    assert cfg.kp_selection.local_bestN.num_bestN == 2000 and cfg.kp_selection.local_bestN.enable is False
    assert cfg.sentinel == {"now": "a table"} and cfg.replaced_table == {"a": 1}


def test_the_runner_keeps_options_from_cfgs_refusals(kmod, fx, tmp_path):
    """a configuration the fused pipeline does not run is refused with options_from_cfg's own message, before any file of the
    sequence but calib.txt and the folder listing is read and before the device is touched"""
    dc = importlib.import_module("df-vo_amd.default_cfg")
    root = tmp_path / "odom_data"
    (root / "04" / "image_2").mkdir(parents=True)
    for i in range(3):
        (root / "04" / "image_2" / ("%06d.png" % i)).write_bytes(b"")
    (root / "04" / "calib.txt").write_text(fx["intrinsics"]["seq00"]["text"])
    cfg = dc.default_configuration(128, 416, None, None)
    cfg.seq = "04"
    cfg.image.ext = "png"
    cfg.directory = dc.Cfg(img_seq_dir=str(root), depth_dir=None, gt_pose_dir=None)
    cfg.online_finetune.enable = True
    with pytest.raises(NotImplementedError, match="online_finetune.enable"):
        kmod.run_kitti_odom(cfg, {}, {})
    cfg.online_finetune.enable = False
    cfg.depth.depth_src = "lidar"
    with pytest.raises(NotImplementedError, match="depth.depth_src"):
        kmod.run_kitti_odom(cfg, {}, {})
    cfg.depth.depth_src = None
    cfg.seq = "05"  # no such folder
    with pytest.raises(ValueError, match="05"):
        kmod.run_kitti_odom(cfg, {}, {})
