"""Fixture of the trackers' iterative keypoint refinement: the REFERENCE's own DFVO.tracking() (libs/dfvo.py:121-262) with its own
KeypointSampler, EssTracker and PnpTracker, on CPU torch over the rigid scenes, with the iterative_kp blocks switched on.

    python tests/golden/make_golden_iterative_kp.py       # (re)writes tests/golden/iterative_kp.npz

Inputs (rigid_case) and the compatibility patches are those of make_golden.py; like make_golden_rigid_iter.py, numpy runs with its
SIMD dispatch off so that np.argpartition's order is the scalar introselect's.  The DFVO object is made without its constructor (no
dataset, no nets): the configuration is the reference's default file with the case's keys edited, cur_data / ref_data are filled
from the scene.  Two consecutive calls per case, the current depths rolled over to the reference side in between, so the
RandomState carries.  Per call: the pose, tracking_mode, kp_depth of the reference frame (int16 pixels; the current frame's are
those plus the flow there, stored as a CRC), the inlier mask, the CRC of rigid_flow_diff, the RandomState afterwards.
"""
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

_SIMD_OFF = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR AVX2 FMA3"
if __name__ == "__main__" and os.environ.get("NPY_DISABLE_CPU_FEATURES") is None:
    import subprocess
    sys.exit(subprocess.call([sys.executable] + sys.argv, env=dict(os.environ, NPY_DISABLE_CPU_FEATURES=_SIMD_OFF)))

import numpy as np  # noqa: E402

SCENES = [(60, 100, 64), (120, 200, 63)]  # (h, w, seed); np.random.seed(4869 + seed) before a case's first call
# name -> (e, scale, pnp iterative_kp.enable, tracking_method, current depth zeroed).  "minus_one": no valid depth ratio, so pass
# one's scale is -1, the E refinement runs on [R | 0] and the PnP branch refines
CONFIGS = {"e": (True, False, False, "hybrid", False), "e_scale": (True, True, False, "hybrid", False),
           "pnp": (False, False, True, "PnP", False), "minus_one": (True, True, True, "hybrid", True)}
SCORES = ["opt_flow", "rigid_flow"]
# the rigid scenes are close to a plane: GRIC rejects E there, the 'flow' validity of ablation_model_sel_flow.yml tracks them
VALIDITY = ("flow", 1.0)
RIGID_FLOW_THRE = 0.5


def cases():
    """[(tag, h, w, seed, config name, score_method)] -- also imported by the tests"""
    return [("s%d_%s_%s" % (si, name, score), h, w, seed, name, score)
            for si, (h, w, seed) in enumerate(SCENES) for name in CONFIGS for score in SCORES]


def edit_cfg(cfg, h, w, name, score):
    """the case's keys on the reference's configuration object"""
    e, s, p, method, _ = CONFIGS[name]
    cfg.image.height, cfg.image.width = h, w
    cfg.tracking_method = method
    cfg.e_tracker.validity.method, cfg.e_tracker.validity.thre = VALIDITY
    cfg.kp_selection.rigid_flow_kp.enable = True
    cfg.kp_selection.rigid_flow_kp.rigid_flow_thre = RIGID_FLOW_THRE
    cfg.e_tracker.iterative_kp.enable, cfg.e_tracker.iterative_kp.score_method = e, score
    cfg.scale_recovery.iterative_kp.enable = s
    cfg.pnp_tracker.iterative_kp.enable, cfg.pnp_tracker.iterative_kp.score_method = p, score


def main():
    import torch
    import make_golden as G  # (imported, not run: its fixtures are not rewritten)
    G.apply_compat()
    from oracle import cv2_shim
    sys.modules["cv2"] = cv2_shim
    G._stub_matplotlib()
    import sklearn.linear_model as lm
    if not getattr(lm.RANSACRegressor, "_dfvo_compat", False):
        _RR = lm.RANSACRegressor

        def ransac_regressor_compat(base_estimator=None, **kw):  # sklearn 0.20 spelling
            return _RR(estimator=base_estimator, **kw)
        ransac_regressor_compat._dfvo_compat = True
        lm.RANSACRegressor = ransac_regressor_compat
    torch.nn.Module.to = lambda self, *a, **k: self  # the layers are moved "to cuda" in their constructors
    from libs.general.configuration import ConfigLoader
    from libs.general.timer import Timer
    from libs.geometry.camera_modules import Intrinsics, SE3
    from libs.matching.keypoint_sampler import KeypointSampler
    from libs.tracker.E_tracker import EssTracker
    from libs.tracker.pnp_tracker import PnpTracker
    from libs.dfvo import DFVO
    out = {}
    for tag, h, w, seed, name, score in cases():
        c = G.rigid_case(h, w, seed)
        K = c["K"]
        cfg = ConfigLoader().merge_cfg([os.path.join(G.REF, "options/examples/default_configuration.yml")])
        edit_cfg(cfg, h, w, name, score)
        intr = Intrinsics([K[0, 2], K[1, 2], K[0, 0], K[1, 1]])
        vo = DFVO.__new__(DFVO)
        vo.cfg, vo.tracking_stage, vo.global_poses, vo.timers = cfg, 1, {0: SE3()}, Timer()
        vo.tracking_method = cfg.tracking_method
        vo.kp_sampler = KeypointSampler(cfg)
        vo.pnp_tracker = PnpTracker(cfg, intr)
        if cfg.tracking_method == "hybrid":
            vo.e_tracker = EssTracker(cfg, intr, vo.timers)
        depth_cur = np.zeros_like(c["depth_cur"]) if CONFIGS[name][4] else c["depth_cur"]
        ref_depth, ref_raw = c["raw_depth"].astype(np.float64), c["raw_depth"]
        np.random.seed(4869 + seed)
        for call in range(2):
            vo.tracking_mode = "Ess. Mat."
            vo.ref_data = {"id": call, "flow": c["flow"], "flow_diff": c["diff"][..., None], "raw_depth": ref_raw, "depth": ref_depth,
                           "motion": SE3()}
            vo.cur_data = {"id": call + 1, "depth": depth_cur, "pose": SE3()}
            vo.tracking()
            k = "%s_c%d" % (tag, call)
            out[k + "_pose"] = np.asarray(vo.ref_data["pose"].pose, np.float64)
            out[k + "_pnp"] = np.array(vo.tracking_mode == "PnP")
            kr, kc = np.asarray(vo.ref_data["kp_depth"]), np.asarray(vo.cur_data["kp_depth"])
            assert np.array_equal(kr, kr.astype(np.int16))
            out[k + "_kp_ref"] = kr.astype(np.int16)
            out[k + "_kp_cur_crc"] = np.array(zlib.crc32(np.ascontiguousarray(kc, np.float64).tobytes()), np.uint32)
            out[k + "_inliers"] = np.packbits(np.asarray(vo.ref_data["inliers"]).astype(bool)) if "inliers" in vo.ref_data else np.zeros(0, np.uint8)
            out[k + "_n_inliers"] = np.array(len(vo.ref_data["inliers"]) if "inliers" in vo.ref_data else -1)
            m = np.ascontiguousarray(vo.ref_data["rigid_flow_diff"][..., 0], np.float32)
            out[k + "_mask_crc"] = np.array(zlib.crc32(m.tobytes()), np.uint32)
            st = np.random.get_state()
            out[k + "_rng_after"] = np.r_[st[1].astype(np.uint32), np.uint32(st[2])]
            print("  iterative_kp", k, vo.tracking_mode, "kp_depth", len(kr), "t", np.round(out[k + "_pose"][:3, 3], 4))
            ref_depth, ref_raw = depth_cur, c["depth_cur"].astype(np.float32)  # (the raw map stays the scene's where the processed is zeroed)
    np.savez_compressed(os.path.join(HERE, "iterative_kp.npz"), **out)


if __name__ == "__main__":
    main()
