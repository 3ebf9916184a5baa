"""GPU: scale_recovery_iterative as one call (dfvo_scale_recovery_iterative: all five rounds enqueued at once, the loop state on
the device) against the fixture produced by the reference's own loop (tests/golden/rigid_iter.npz, make_golden_rigid_iter.py),
against the oracle (oracle/tracker_np.py scale_recovery_iterative) and against the mirror's host loop.  Bit-exact: rounds taken,
keypoint counts of every round, keypoints, the distance map of the last round, the RandomState afterwards -- the equal
RandomState of the cases that stop after two rounds is the proof that the three rounds behind them drew nothing.  Scales:
1e-12 relative (the final least squares goes through LAPACK in sklearn), the bound test_tracker_gpu.py holds for the scale.
The shapes are the smallest at which a 10 x 10 grid still has uneven cells."""
import ctypes as C
import importlib
import os
import zlib
from types import SimpleNamespace as NS

import numpy as np
import pytest

from golden.make_golden import rigid_case
from golden.make_golden_rigid_iter import cases, tracker_cfg, unit_E_pose
from oracle import tracker_np as T

pytestmark = pytest.mark.gpu

CASES = {c[0]: c[1:] for c in cases()}
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rigid_iter.npz"))
ERR_ARG, ERR_EMPTY = -2, -5


@pytest.fixture(scope="module")
def trk(gpu):
    t = C.c_void_p()
    gpu.check(gpu.lib().dfvo_tracker_create(None, C.byref(t)))
    yield t
    gpu.lib().dfvo_tracker_destroy(t)


_scenes, _oracle = {}, {}


def scene(h, w, seed):
    if (h, w, seed) not in _scenes:
        _scenes[(h, w, seed)] = rigid_case(h, w, seed)
    return _scenes[(h, w, seed)]


def rng_words():
    st = np.random.get_state()
    return np.ascontiguousarray(np.r_[st[1].astype(np.uint32), np.uint32(st[2])])


def oracle_run(tag, kp_best=None):
    """the oracle's loop for a case (once per module): (result dict, RandomState words afterwards)"""
    key = (tag, kp_best is not None)
    if key not in _oracle:
        h, w, seed, score, thre, prev = CASES[tag]
        c = scene(h, w, seed)
        np.random.seed(4869 + seed)
        kw = dict(kp_src="kp_best", kp_best=kp_best) if kp_best is not None else {}
        res = T.scale_recovery_iterative(c["flow"], c["diff"][..., None], c["raw_depth"], c["depth_cur"],
                                         unit_E_pose(c["T_ref_to_cur"]), c["K"], prev_scale=prev, score_method=score,
                                         rigid_thre=thre, **kw)
        _oracle[key] = (res, rng_words())
    return _oracle[key]


def c_call(gpu, trk, c, h, w, score, thre, prev, seed_words, kp_best=None, num_row=10, num_col=10, num_bestN=2000, want_map=True):
    """dfvo_scale_recovery_iterative on a scene -> (return code, out struct, kp_ref, kp_cur, map, RandomState words)"""
    K = c["K"]
    kcfg = gpu.RigidKpCfg(num_row=num_row, num_col=num_col, num_bestN=num_bestN, rigid_flow_thre=thre, optical_flow_thre=0.1,
                          score_method=1 if score == "rigid_flow" else 0)
    Kinv = np.linalg.inv(K)
    for i in range(9):
        kcfg.K[i], kcfg.Kinv[i] = K.flat[i], Kinv.flat[i]
    scfg = gpu.ScaleCfg(cx=K[0, 2], cy=K[1, 2], fx=K[0, 0], fy=K[1, 1], min_samples=3, max_trials=100, stop_prob=0.99, thre=0.1,
                        method=0)
    E = np.ascontiguousarray(unit_E_pose(c["T_ref_to_cur"]))
    T21 = np.ascontiguousarray(np.linalg.inv(E))
    out = gpu.ScaleIterOut()
    out.n_iter = out.n_kp = -77  # (sentinels: an error in the first round writes nothing)
    kp_ref, kp_cur = np.full((num_bestN, 2), -7.0), np.full((num_bestN, 2), -7.0)
    m = np.full((h, w), -7.0, np.float32) if want_map else None
    rng = seed_words.copy()
    b_ref = b_cur = None
    if kp_best is not None:
        b_ref, b_cur = np.ascontiguousarray(kp_best[0], np.float64), np.ascontiguousarray(kp_best[1], np.float64)
    code = gpu.lib().dfvo_scale_recovery_iterative(
        trk, gpu.as_ptr(np.ascontiguousarray(c["flow"])), gpu.as_ptr(np.ascontiguousarray(c["diff"].reshape(h, w))),
        gpu.as_ptr(np.ascontiguousarray(c["raw_depth"])), gpu.as_ptr(np.ascontiguousarray(c["depth_cur"], np.float64)), h, w,
        C.byref(kcfg), C.byref(scfg), gpu.as_ptr(E), gpu.as_ptr(T21), float(prev), 0 if kp_best is None else 1, gpu.as_ptr(b_ref),
        gpu.as_ptr(b_cur), 0 if kp_best is None else b_ref.shape[0], gpu.as_ptr(rng), C.byref(out), gpu.as_ptr(kp_ref),
        gpu.as_ptr(kp_cur), gpu.as_ptr(m))
    return code, out, kp_ref, kp_cur, m, rng


def rel(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


def test_the_cases_cover_every_round_count_and_the_minus_one_scale():
    """what the parity test below stands on: the fixture's loops stop after 2, 3, 4 and 5 rounds, the keypoint count changes
    from round to round, and one case carries the scale -1 through both of its rounds"""
    iters = {int(GOLD[t + "_n_iter"]) for t in CASES}
    assert iters == {2, 3, 4, 5}
    assert any(len(set(GOLD[t + "_n_kp"].tolist())) == int(GOLD[t + "_n_iter"]) == 5 for t in CASES)
    assert GOLD["s1t0p2_n_kp"].tolist() == [4, 6] and GOLD["s1t0p2_scale_out"].tolist() == [-1.0, -1.0]


@pytest.mark.parametrize("tag", list(CASES))
def test_parity_with_the_reference_fixture_and_the_oracle(gpu, trk, tag):
    h, w, seed, score, thre, prev = CASES[tag]
    c = scene(h, w, seed)
    np.random.seed(4869 + seed)
    code, out, kp_ref, kp_cur, m, rng = c_call(gpu, trk, c, h, w, score, thre, prev, rng_words())
    assert code == 0, gpu.lib().dfvo_last_error()
    n_iter = int(GOLD[tag + "_n_iter"])
    print("%s: rounds %d (fixture %d), n_kp %s, scale_in %s, scale_out %s | fixture n_kp %s scale_out %s" % (
        tag, out.n_iter, n_iter, out.n_kp_round[:], out.scale_in[:], out.scale_out[:], GOLD[tag + "_n_kp"].tolist(),
        GOLD[tag + "_scale_out"].tolist()))
    # against the reference's own loop
    assert out.n_iter == n_iter and out.status == 0 and out.kp_round == n_iter - 1
    assert out.n_kp_round[:n_iter] == GOLD[tag + "_n_kp"].tolist() and all(v == -1 for v in out.n_kp_round[n_iter:])
    assert out.n_kp == GOLD[tag + "_n_kp"][-1]
    assert np.array_equal(kp_ref[:out.n_kp], GOLD[tag + "_ref_kp"]) and np.array_equal(kp_cur[:out.n_kp], GOLD[tag + "_cur_kp"])
    assert (kp_ref[out.n_kp:] == -7.0).all() and (kp_cur[out.n_kp:] == -7.0).all()
    assert zlib.crc32(m.tobytes()) == int(GOLD[tag + "_mask_crc"])
    for r in range(n_iter):
        assert rel(out.scale_out[r], GOLD[tag + "_scale_out"][r]), (r, out.scale_out[r], GOLD[tag + "_scale_out"][r])
        assert out.scale_in[r] == (float(prev) if r == 0 else out.scale_out[r - 1])
    assert out.scale == out.scale_out[n_iter - 1] and rel(out.scale, float(GOLD[tag + "_scale"]))
    assert np.array_equal(rng, GOLD[tag + "_rng_after"]), "RandomState diverged from the reference's"
    # against the oracle
    want, want_rng = oracle_run(tag)
    assert out.n_iter == want["n_iter"] and rel(out.scale, want["scale"])
    assert np.array_equal(kp_ref[:out.n_kp], want["ref_kp"]) and np.array_equal(kp_cur[:out.n_kp], want["cur_kp"])
    assert np.array_equal(m, want["rigid_flow_mask"])
    assert np.array_equal(rng, want_rng)


@pytest.mark.parametrize("tag", ["s0t0p2", "s2t1p1"])
def test_scale_from_a_fixed_keypoint_set(gpu, trk, tag):
    """scale_recovery.kp_src 'kp_best' (what the *_extend.yml configurations select): each round's scale comes from the
    local_bestN keypoints while the rigid-flow keypoints are still selected and returned"""
    h, w, seed, score, thre, prev = CASES[tag]
    c = scene(h, w, seed)
    lb = T.local_bestN(c["flow"], c["diff"][..., None])
    assert lb["good_kp_found"]
    best = (lb["kp1_best"][0], lb["kp2_best"][0])
    want, want_rng = oracle_run(tag, best)
    np.random.seed(4869 + seed)
    code, out, kp_ref, kp_cur, m, rng = c_call(gpu, trk, c, h, w, score, thre, prev, rng_words(), kp_best=best)
    print("%s kp_best (%d keypoints): rounds %d (oracle %d), scale %.15g (oracle %.15g), n_kp %s" % (
        tag, len(best[0]), out.n_iter, want["n_iter"], out.scale, want["scale"], out.n_kp_round[:]))
    assert code == 0, gpu.lib().dfvo_last_error()
    assert out.n_iter == want["n_iter"] and rel(out.scale, want["scale"])
    assert np.array_equal(kp_ref[:out.n_kp], want["ref_kp"]) and np.array_equal(kp_cur[:out.n_kp], want["cur_kp"])
    assert np.array_equal(m, want["rigid_flow_mask"])
    assert np.array_equal(rng, want_rng)


def make_mirror(h, w, score, thre, K, kp_src="kp_depth"):
    cam_mod = importlib.import_module("df-vo_amd.libs.geometry.camera_modules")
    E_mod = importlib.import_module("df-vo_amd.libs.tracker.E_tracker")

    def ns(d):
        return NS(**{k: ns(v) if isinstance(v, dict) else v for k, v in d.items()})
    cam = cam_mod.Intrinsics([K[0, 2], K[1, 2], K[0, 0], K[1, 1]])
    return E_mod.EssTracker(ns(tracker_cfg(score, thre, h, w, kp_src)), cam, None), cam_mod


def mirror_run(tag, on_device, thre=None):
    """EssTracker.scale_recovery_iterative of the drop-in class -> everything it leaves behind"""
    h, w, seed, score, thre0, prev = CASES[tag]
    c = scene(h, w, seed)
    et, cam_mod = make_mirror(h, w, score, thre0 if thre is None else thre, c["K"])
    et.iterative_on_device = on_device
    ref = {"flow": c["flow"], "flow_diff": c["diff"][..., None], "raw_depth": c["raw_depth"]}
    cur = {"depth": c["depth_cur"]}
    np.random.seed(4869 + seed)
    et.prev_scale = prev
    err = None
    out = None
    try:
        out = et.scale_recovery_iterative(cur, ref, cam_mod.SE3(unit_E_pose(c["T_ref_to_cur"])))
    except (AssertionError, ValueError) as e:
        err = e
    return dict(out=out, err=err, cur=cur, ref=ref, prev_scale=et.prev_scale, rng=rng_words())


def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and \
            np.array_equal(a, b)
    if hasattr(a, "pose"):
        return np.array_equal(a.pose, b.pose)
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("tag", ["s1t0p2", "s2t0p2", "s1t1p1"])
def test_mirror_on_the_device_leaves_what_the_host_loop_leaves(gpu, tag):
    """the scale -1 case, a five-round case and a two-round case: the returned dict, every entry written into cur_data and
    ref_data, prev_scale and np.random's state"""
    dev, host = mirror_run(tag, True), mirror_run(tag, False)
    assert dev["err"] is None and host["err"] is None
    assert sorted(dev["out"]) == sorted(host["out"]) == ["cur_kp", "ref_kp", "rigid_flow_mask", "scale"]
    print("%s: scale device %r host %r" % (tag, dev["out"]["scale"], host["out"]["scale"]))
    for k in host["out"]:
        assert same(dev["out"][k], host["out"][k]), k
    for side in ("cur", "ref"):
        assert sorted(dev[side]) == sorted(host[side]), side
        for k in host[side]:
            assert same(dev[side][k], host[side][k]), (side, k)
    assert same(dev["prev_scale"], host["prev_scale"])
    assert np.array_equal(dev["rng"], host["rng"])
    assert rel(float(dev["out"]["scale"]), float(GOLD[tag + "_scale"]))


def test_empty_selection_is_the_reference_assertion(gpu, trk):
    """rigid_flow_thre 1e-6 selects nothing: the C call answers with its own code and writes nothing, the RandomState stays,
    the mirror raises the reference's AssertionError (both loops leave the same behind), and the handle works afterwards"""
    tag = "s1t1p1"
    h, w, seed, score, thre, prev = CASES[tag]
    c = scene(h, w, seed)
    np.random.seed(4869 + seed)
    before = rng_words()
    code, out, kp_ref, kp_cur, m, rng = c_call(gpu, trk, c, h, w, score, 1e-6, prev, before)
    assert code == ERR_EMPTY, code
    assert b"sampling threshold is too small" in gpu.lib().dfvo_last_error()
    assert np.array_equal(rng, before)
    assert out.n_iter == -77 and out.n_kp == -77 and (kp_ref == -7.0).all() and (kp_cur == -7.0).all() and (m == -7.0).all()
    dev, host = mirror_run(tag, True, thre=1e-6), mirror_run(tag, False, thre=1e-6)
    for r in (dev, host):
        assert isinstance(r["err"], AssertionError) and str(r["err"]) == "sampling threshold is too small."
        assert np.array_equal(r["rng"], before) and r["prev_scale"] == prev
    assert sorted(dev["ref"]) == sorted(host["ref"]) and sorted(dev["cur"]) == sorted(host["cur"])
    assert same(dev["ref"]["rigid_flow_pose"], host["ref"]["rigid_flow_pose"])
    # the next call on the same handle
    np.random.seed(4869 + seed)
    code, out, kp_ref, kp_cur, m, rng = c_call(gpu, trk, c, h, w, score, thre, prev, rng_words())
    assert code == 0 and out.n_iter == int(GOLD[tag + "_n_iter"]) and rel(out.scale, float(GOLD[tag + "_scale"]))
    assert np.array_equal(kp_ref[:out.n_kp], GOLD[tag + "_ref_kp"]) and np.array_equal(rng, GOLD[tag + "_rng_after"])


@pytest.mark.parametrize("what,h,w,kw,msg", [
    ("grid", 48, 64, dict(num_row=40, num_col=40), b"grid too large"),
    ("n_best_zero", 48, 64, dict(num_bestN=99), b"n_best out of range"),
    ("n_best_large", 48, 64, dict(num_bestN=25700), b"n_best out of range"),
    ("cell", 300, 300, dict(num_row=1, num_col=1, num_bestN=200), b"cell larger than 65535 pixels"),
    ("lds", 200, 200, dict(num_row=1, num_col=1, num_bestN=200), b"does not fit in LDS"),
    ("ratios_lds", 48, 64, dict(num_bestN=16400), b"64 KB of LDS"),
])
def test_launcher_refusals(gpu, trk, what, h, w, kw, msg):
    """the refusals of dfvo_kp_rigid_flow's launcher (grid, n_best, LDS of a cell) hold here, and so does the bound of the
    depth-ratio kernel's dynamic LDS (one int per keypoint, 64 KB); nothing is enqueued and the handle stays usable"""
    rs = np.random.RandomState(5)
    c = dict(K=np.array([[50.0, 0, w / 2], [0, 50.0, h / 2], [0, 0, 1]]), flow=rs.rand(2, h, w).astype(np.float32),
             diff=rs.rand(h, w, 1).astype(np.float32), raw_depth=np.ones((h, w), np.float32), depth_cur=np.ones((h, w)),
             T_ref_to_cur=np.array([[1.0, 0, 0, 0.1], [0, 1, 0, 0], [0, 0, 1, 0.5], [0, 0, 0, 1]]))
    np.random.seed(1)
    before = rng_words()
    code, out, kp_ref, kp_cur, m, rng = c_call(gpu, trk, c, h, w, "opt_flow", 0.5, 0.0, before, want_map=False, **kw)
    assert code == ERR_ARG, (what, code)
    assert msg in gpu.lib().dfvo_last_error(), gpu.lib().dfvo_last_error()
    assert np.array_equal(rng, before) and out.n_iter == -77
    tag = "s2t1p1"
    hh, ww, seed, score, thre, prev = CASES[tag]
    np.random.seed(4869 + seed)
    code, out, kp_ref, kp_cur, m, rng = c_call(gpu, trk, scene(hh, ww, seed), hh, ww, score, thre, prev, rng_words())
    assert code == 0 and out.n_iter == int(GOLD[tag + "_n_iter"]) and np.array_equal(rng, GOLD[tag + "_rng_after"])
