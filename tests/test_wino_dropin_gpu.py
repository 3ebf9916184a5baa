"""GPU: the drop-in key `dfvo_hip.fp32_winograd` -- DeepModel packs its nets with the switch on and puts it back."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_deepmodel_packs_with_the_switch_and_restores_it(gpu, tmp_path, monkeypatch):
    from synth import coded_tunnel_sequence, crafted_liteflownet_state_dict, crafted_monodepth2_state_dict, write_weight_files
    import test_dropin_gpu as D
    monkeypatch.delenv("DFVO_CONV_PRECISION", raising=False)
    h, w = 256, 640
    seq = coded_tunnel_sequence(h, w, 2, mode="mux", step=1.0, seed=33)
    flow_path, depth_dir = write_weight_files(str(tmp_path), crafted_liteflownet_state_dict(h, w, "mux"), crafted_monodepth2_state_dict())
    cfg = D.full_cfg(h, w, flow_path, depth_dir)
    cfg["dfvo_hip"] = {"conv_precision": "fp32", "fp32_winograd": True, "session": False}
    lib = gpu.lib()
    n = C.c_ulonglong(0)
    gpu.check(lib.dfvo_fp32_winograd_launches(C.byref(n), 1))
    before = lib.dfvo_get_fp32_winograd()
    dm_mod = importlib.import_module("df-vo_amd.libs.deep_models.deep_models")
    dm = dm_mod.DeepModel(cfg)
    dm.initialize_models()
    assert lib.dfvo_get_fp32_winograd() == before
    flows = dm.forward_flow({"id": 1, "img": seq["frames"][1]}, {"id": 0, "img": seq["frames"][0]}, True)
    assert lib.dfvo_get_fp32_winograd() == before
    for k, v in flows.items():
        assert np.isfinite(np.asarray(v)).all(), k
    gpu.check(lib.dfvo_fp32_winograd_launches(C.byref(n), 0))
    assert n.value > 0, "no layer of the nets ran as Winograd"
