"""Fixture of the iterative scale recovery: the REFERENCE's own EssTracker.scale_recovery_iterative (E_tracker.py:509-569) on CPU
torch over the rigid scenes, round by round.

    python tests/golden/make_golden_rigid_iter.py       # (re)writes tests/golden/rigid_iter.npz

Inputs (rigid_case) and the compatibility patches are those of make_golden.py's golden_rigid_flow; like there, numpy runs with
its SIMD dispatch off so that np.argpartition's order is the scalar introselect's.  Per case: the scale, the rounds taken
(calls of find_scale_from_depth), each round's keypoint count and scale, both keypoint arrays, the CRC of the final distance
map and the RandomState afterwards.
"""
import os
import sys
import types
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

_SIMD_OFF = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR AVX2 FMA3"
if __name__ == "__main__" and os.environ.get("NPY_DISABLE_CPU_FEATURES") is None:
    import subprocess
    sys.exit(subprocess.call([sys.executable] + sys.argv, env=dict(os.environ, NPY_DISABLE_CPU_FEATURES=_SIMD_OFF)))

import numpy as np  # noqa: E402

# (h, w, seed, score_method) x rigid_flow_thre x prev_scale; np.random.seed(4869 + seed) before each
SCENES = [(120, 200, 63, "opt_flow"), (60, 100, 64, "opt_flow"), (48, 64, 65, "rigid_flow")]
THRES = [0.2, 0.5]
PREV_SCALES = [0, 0.7, 3.0]


def cases():
    """[(tag, h, w, seed, score, rigid_flow_thre, prev_scale)] -- also imported by the tests"""
    out = []
    for si, (h, w, seed, score) in enumerate(SCENES):
        for ti, thre in enumerate(THRES):
            for pi, prev in enumerate(PREV_SCALES):
                out.append(("s%dt%dp%d" % (si, ti, pi), h, w, seed, score, thre, prev))
    return out


def tracker_cfg(score, thre, h, w, kp_src="kp_depth"):
    """the configuration tree of golden_rigid_flow with the rigid-flow threshold of the case (plain dicts)"""
    return {
        "kp_selection": {"rigid_flow_kp": {"enable": True, "num_bestN": 2000, "num_row": 10, "num_col": 10,
                                           "score_method": score, "rigid_flow_thre": thre, "optical_flow_thre": 0.1}},
        "e_tracker": {"ransac": {"reproj_thre": 0.2, "repeat": 5}, "validity": {"method": "GRIC", "thre": None},
                      "kp_src": "kp_best", "iterative_kp": {"enable": False, "kp_src": "kp_depth", "score_method": score}},
        "scale_recovery": {"method": "iterative", "kp_src": kp_src,
                           "iterative_kp": {"enable": False, "kp_src": "kp_depth", "score_method": score},
                           "ransac": {"method": "depth_ratio", "min_samples": 3, "max_trials": 100, "stop_prob": 0.99,
                                      "thre": 0.1}},
        "image": {"height": h, "width": w}}


def unit_E_pose(T_ref_to_cur):
    """the E-tracker's pose: cur -> ref with unit translation"""
    E = np.linalg.inv(T_ref_to_cur)
    E[:3, 3] = E[:3, 3] / np.linalg.norm(E[:3, 3])
    return E


def main():
    import torch
    import make_golden as G  # (imported, not run: its fixtures are not rewritten)
    G.apply_compat()
    from oracle import cv2_shim
    sys.modules["cv2"] = cv2_shim
    import sklearn.linear_model as lm
    if getattr(lm.RANSACRegressor, "__name__", "") != "ransac_regressor_compat":
        _RR = lm.RANSACRegressor

        def ransac_regressor_compat(base_estimator=None, **kw):
            return _RR(estimator=base_estimator, **kw)
        lm.RANSACRegressor = ransac_regressor_compat
    torch.nn.Module.to = lambda self, *a, **k: self  # the layers are moved "to cuda" in their constructors
    try:
        import matplotlib.pyplot  # noqa: F401
    except Exception:
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"] = mpl
        sys.modules["matplotlib.pyplot"] = mpl.pyplot
    from easydict import EasyDict
    from libs.tracker.E_tracker import EssTracker
    from libs.general.timer import Timer
    from libs.geometry.camera_modules import Intrinsics, SE3
    out = {}
    for tag, h, w, seed, score, thre, prev in cases():
        c = G.rigid_case(h, w, seed)
        K = c["K"]
        trk = EssTracker(EasyDict(tracker_cfg(score, thre, h, w)), Intrinsics([K[0, 2], K[1, 2], K[0, 0], K[1, 1]]), Timer())
        ref = {"flow": c["flow"], "flow_diff": c["diff"][..., None], "raw_depth": c["raw_depth"]}
        cur = {"depth": c["depth_cur"]}
        rounds = []
        find = trk.find_scale_from_depth

        def counted(kp1, kp2, T_21, depth2, _find=find, _rounds=rounds):
            s = _find(kp1, kp2, T_21, depth2)
            _rounds.append((len(kp1), float(s)))
            return s
        trk.find_scale_from_depth = counted
        np.random.seed(4869 + seed)
        trk.prev_scale = prev
        it = trk.scale_recovery_iterative(cur, ref, SE3(unit_E_pose(c["T_ref_to_cur"])))
        out[tag + "_spec"] = np.array([h, w, seed, 0 if score == "opt_flow" else 1, thre, prev], np.float64)
        out[tag + "_scale"] = np.array(float(it["scale"]))
        out[tag + "_n_iter"] = np.array(len(rounds))
        out[tag + "_n_kp"] = np.array([r[0] for r in rounds], np.int64)
        out[tag + "_scale_out"] = np.array([r[1] for r in rounds], np.float64)
        out[tag + "_cur_kp"] = np.asarray(it["cur_kp"])
        out[tag + "_ref_kp"] = np.asarray(it["ref_kp"])
        m = np.ascontiguousarray(it["rigid_flow_mask"], np.float32)
        out[tag + "_mask_crc"] = np.array(zlib.crc32(m.tobytes()), np.uint32)
        st = np.random.get_state()
        out[tag + "_rng_after"] = np.r_[st[1].astype(np.uint32), np.uint32(st[2])]
        print("  rigid_iter", tag, (h, w), thre, prev, "rounds", len(rounds), "n_kp", [r[0] for r in rounds],
              "scales", ["%.6g" % r[1] for r in rounds])
    np.savez_compressed(os.path.join(HERE, "rigid_iter.npz"), **out)


if __name__ == "__main__":
    main()
