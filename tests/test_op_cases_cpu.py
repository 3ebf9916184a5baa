"""tests/op_cases.py on the CPU: the table reaches every kernel variant and every edge category it was written for (so
that a case deleted later fails here), its variant codes are the ones the library's own dispatch functions return, its
float64 references are torch's operators, and its bounds (tests/flow_bounds.py) pass a float32 restatement of every case
and put seeded bugs of that restatement far outside."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import flow_bounds as B
import op_cases as P

F32 = torch.float32


def _by(op, **kw):
    return [c for c in P.CASES[op] if all(c.get(k) == v for k, v in kw.items())]


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_table_reaches_every_variant_code():
    assert {c["variant"] for c in P.CASES["deconv"]} == {0, 1, 2}
    assert {c["variant"] for c in P.CASES["corr"]} == {188, 288, 388, 488, 648, 88, 48, 44}  # rt<1,2,3,4,6>, three generic tiles
    assert {c["variant_rt0"] for c in P.CASES["corr"]} == {88, 48, 44}
    assert {c["variant"] for c in P.CASES["reg_head"]} == {0, 3, 5, 7}
    # every variant on every map of its operator
    for v in (188, 288, 388, 488, 648, 88, 48, 44):
        assert {(c["h"], c["w"]) for c in _by("corr", variant=v) if not c["view"]} == set(P.CORR_MAPS), v
    for k in (3, 5, 7):
        for v in (k, 0):
            assert {(c["h"], c["w"]) for c in _by("reg_head", k=k, variant=v)} == set(P.REG_HEAD_MAPS), (k, v)


def test_table_variant_codes_are_the_launchers_own(capi):
    """the three queries are the pure functions launch_deconv_dw, launch_correlation and launch_reg_head call: no device
    needed.  (The pointers of the reg-head query are only tested for alignment.)"""
    lib = capi.lib()
    for c in P.CASES["deconv"]:
        assert lib.dfvo_deconv_variant(c["C"], c["cs"]) == c["variant"], c["id"]
    for c in P.CASES["corr"]:
        assert lib.dfvo_correlation_variant(c["C"], c["cs1"], c["co1"], c["cs2"], c["co2"]) == c["variant"], c["id"]
    p = C.c_void_p(1 << 20)
    for c in P.CASES["reg_head"]:
        got = lib.dfvo_reg_head_variant(p, c["dist_cs"], c["k"], p, c["fcs"], c["fco"], p, c["dcs"], c["dco"])
        assert got == c["variant"], c["id"]
    # an unaligned pointer alone sends an otherwise vector-ready head to the scalar kernel
    assert lib.dfvo_reg_head_variant(C.c_void_p((1 << 20) + 4), 12, 3, p, 4, 0, p, 4, 0) == 0
    assert lib.dfvo_reg_head_variant(p, 12, 3, p, 4, 0, C.c_void_p((1 << 20) + 4), 4, 0) == 0
    # the refusals of the correlation launcher, and the last channel count that fits
    assert lib.dfvo_correlation_variant(6, 8, 0, 8, 0) == -1 and lib.dfvo_correlation_variant(356, 356, 0, 356, 0) == -1
    assert lib.dfvo_correlation_variant(352, 352, 0, 352, 0) == 44 and lib.dfvo_correlation_variant(64, 66, 0, 64, 0) == -1
    assert lib.dfvo_deconv_variant(512, 512) == 0 and lib.dfvo_deconv_variant(513, 516) == 1


def test_table_reaches_every_edge_category():
    corr = [c for c in P.CASES["corr"] if not c["view"]]
    assert {c["C"] for c in corr} == {32, 64, 96, 128, 192, 4, 48, 80, 100, 160, 224, 352}
    for cc in {c["C"] for c in corr}:
        assert {(c["h"], c["w"], c["stride"]) for c in corr if c["C"] == cc} == {(h, w, s) for h, w in P.CORR_MAPS for s in (1, 2)}
    assert P.CORR_MAPS == [(2, 2), (3, 2), (7, 9), (9, 17), (5, 13)]
    # Ho, Wo one below, at and one above the tile edges 4 and 8, odd Ho, stride 2 on odd maps
    ho = {-(-c["h"] // c["stride"]) for c in corr}
    wo = {-(-c["w"] // c["stride"]) for c in corr}
    assert {3, 4, 5, 7, 9} <= ho and {7, 9, 17} <= wo and {1, 2} <= ho & wo
    assert any(c["stride"] == 2 and c["h"] % 2 and c["w"] % 2 for c in corr)
    for rt in (True, False):  # both kernels see both swaps at N = 1, 2, 3
        assert {(c["swap2"], c["N"]) for c in corr if (c["variant"] >= 100) == rt} == {(s, n) for s in (0, 1) for n in (1, 2, 3)}
    views = {c["id"]: c for c in P.CASES["corr"] if c["view"]}
    assert any(c["C"] == 64 and c["co1"] == c["co2"] == 32 and c["cs1"] == c["cs2"] == 128 for c in views.values())
    assert any(c["cs1"] != c["cs2"] for c in views.values()) and any(c["co1"] != c["co2"] and c["co1"] and c["co2"] for c in views.values())
    assert any(c["variant"] < 100 and c["co1"] for c in views.values())

    assert {(c["C"], c["cs"]) for c in P.CASES["deconv"]} == {(2, 4), (49, 52), (2, 8), (64, 64), (49, 49), (3, 3), (516, 516)}
    for c, cs in [(2, 4), (49, 52), (2, 8), (64, 64), (49, 49), (3, 3)]:
        assert {(d["h"], d["w"]) for d in _by("deconv", C=c, cs=cs)} == {(1, 1), (2, 3), (7, 5)}
    assert [(d["h"], d["w"]) for d in _by("deconv", C=516)] == [(2, 3)]
    assert {d["N"] for d in P.CASES["deconv"]} == {1, 2, 3}

    warp = P.CASES["warp"]
    assert {(c["C"], c["step"], c["h"], c["w"]) for c in warp} == {(cc, s, h, w) for cc in (4, 8, 64) for s in (1, 2, 3) for h, w in P.MAPS}
    assert P.MAPS == [(2, 2), (2, 5), (7, 9)]
    assert {c["N"] for c in _by("warp", swap=1)} == {3} and _by("warp", swap=0)
    assert {c["append_flow"] for c in warp} == {0, 1}
    assert any(c["sco"] and c["dco"] and c["fco"] == 2 and c["fcs"] == 4 and c["dcs"] >= c["C"] + 8 for c in warp)
    assert any(c["sco"] == 0 and c["dco"] == 0 and c["fco"] == 0 for c in warp)
    for op in ("warp", "reg_prep"):
        assert {(c["h"], c["w"], c["flow"]) for c in P.CASES[op]} == {(h, w, k) for h, w in P.MAPS for k in P.FLOW_KINDS}, op
    for step in (2, 3):
        assert any(c["step"] == step and c["append_flow"] for c in warp) and any(c["step"] == step and c["swap"] for c in warp)
    assert any(c["fco"] for c in P.CASES["reg_prep"]) and {c["N"] for c in P.CASES["reg_prep"]} == {1, 2, 3}

    head = P.CASES["reg_head"]
    assert {(c["k"], c["dist_cs"]) for c in head} == {(3, 12), (5, 28), (7, 52), (3, 9), (5, 25), (7, 49), (1, 4), (1, 1), (9, 84), (9, 81)}
    assert all({(c["h"], c["w"]) for c in _by("reg_head", k=k)} == set(P.REG_HEAD_MAPS) for k in (1, 3, 5, 7, 9))
    assert any(c["dco"] == 2 and c["dcs"] == 4 for c in head) and any(c["fco"] == 2 for c in head)
    assert all({c["steep"] for c in _by("reg_head", k=k)} == {0, 1} for k in (3, 5, 7, 9))
    for a, b in P.REG_HEAD_PAIRS.values():  # every case of a pair has its twin on the other stride
        assert {c["twin"] for c in _by("reg_head", dist_cs=a)} == {c["twin"] for c in _by("reg_head", dist_cs=b)}

    assert {(c["h"] * c["w"], c["N"]) for c in P.CASES["mean"]} == {(hw, n) for hw in (1, 4, 63, 64, 65, 147, 4097) for n in (1, 2, 3)}
    assert all(any(c["fco"] == 2 and c["fcs"] == 4 for c in _by("mean", N=n)) for n in (1, 2, 3))
    assert {(c["C"], c["align_corners"], (c["h"], c["w"]), (c["ho"], c["wo"])) for c in P.CASES["resize"]} == \
        {(cc, ac, a, b) for cc in (4, 8, 12) for ac in (0, 1) for a, b in P.RESIZES}
    assert P.RESIZES == [((7, 9), (3, 4)), ((3, 4), (7, 9)), ((5, 5), (1, 1)), ((1, 1), (4, 5)), ((9, 6), (9, 3))]
    assert {(c["C"], c["h"], c["w"]) for c in P.CASES["maxpool"]} == {(cc, h, w) for cc in (4, 8) for h, w in [(1, 1), (2, 2), (7, 9), (8, 5)]}
    assert {r["id"] for r in P.REFUSALS} == {"corr_c6", "corr_c356_lds", "warp_scs6", "warp_dco2", "warp_1wide", "warp_1high",
                                             "reg_prep_1wide", "reg_prep_1high", "mean_odd_fcs", "resize_c6"}


def test_inputs_hold_the_values_the_categories_name():
    for c in P.CASES["maxpool"]:
        x = P.tensors(c["id"])["x"]
        assert bool(torch.isnan(x).any()) and bool(torch.isinf(x).any()), c["id"]
        assert bool(torch.isinf(P.reference(c, P.tensors(c["id"]))[:, 0]).all())
    for c in P.CASES["reg_head"]:
        if c["steep"] and c["k"] >= 3:  # several softmax weights underflow to zero in fp32, at most pixels
            v = -P.tensors(c["id"])["dist"].pow(2)
            zero = ((v - v.max(1, True)[0]).exp() == 0).sum(1)
            assert float((zero >= 3).float().mean()) > 0.5, (c["id"], zero.flatten().tolist())
            assert bool(((v - v.max(1, True)[0]).exp().sum(1) > 1).any()), c["id"]  # (and not every pixel is one-hot)
    for op in ("warp", "reg_prep"):
        for c in P.CASES[op]:
            t = P.tensors(c["id"])
            f = t["flow"]
            ix, iy, _, _ = B.warp_coords(torch.nan_to_num(f.double()), c["mult"])
            if c["flow"] == "integer":
                assert float((ix - ix.round()).abs().max()) < 1e-5 and float((iy - iy.round()).abs().max()) < 1e-5, c["id"]
            if c["flow"] == "edge":
                near = lambda v, a: bool(((v - a).abs() < 1e-5).any())  # noqa: E731
                assert near(ix, -1) and near(ix, c["w"]) and near(iy, -1) and near(iy, c["h"]), c["id"]
            if c["flow"] == "far":
                assert float(ix.abs().max()) > 2.0 ** 31 and float(iy.abs().max()) > 2.0 ** 31, c["id"]
            if c["flow"] == "nan":
                assert 0 < int(torch.isnan(f).sum()) <= 2 * c["N"]
                assert bool(torch.isnan(P.reference(c, t)).any())


# ---- the references are torch's operators --------------------------------------------------------------------------------
def _grid_sample_warp(src, flow, mult, swap):
    """Backward() written out again: the fp32 linspace grid widened, plus flow * mult in half-extents"""
    n, _, h, w = flow.shape
    gx = torch.linspace(-1.0, 1.0, w).double().view(1, 1, w).expand(n, h, w) + flow[:, 0] * mult / ((w - 1) / 2)
    gy = torch.linspace(-1.0, 1.0, h).double().view(1, h, 1).expand(n, h, w) + flow[:, 1] * mult / ((h - 1) / 2)
    return F.grid_sample(src.flip(0) if swap else src, torch.stack([gx, gy], 3), mode="bilinear", padding_mode="zeros", align_corners=True)


def _same(a, b, tol=0.0):
    nan = torch.isnan(a)
    if not torch.equal(nan, torch.isnan(b)):
        return False
    a, b = a[~nan], b[~nan]
    return torch.equal(a, b) if tol == 0 else float((a - b).abs().max() if a.numel() else 0.0) <= tol


@pytest.mark.parametrize("op", ["warp", "deconv", "resize", "maxpool", "reg_head", "mean"])
def test_float64_reference_is_torchs_operator(op):
    for c in P.CASES[op]:
        t = {k: v.double() for k, v in P.tensors(c["id"]).items()}
        ref = P.reference(c, P.tensors(c["id"]))
        if op == "warp":
            assert _same(ref[:, :c["C"]], _grid_sample_warp(t["src"], t["flow"], c["mult"], c["swap"]), 1e-12), c["id"]
        elif op == "deconv":
            assert torch.equal(ref, F.conv_transpose2d(t["x"], t["w"], None, stride=2, padding=1, groups=c["C"])), c["id"]
        elif op == "resize":
            assert torch.equal(ref, F.interpolate(t["x"], size=(c["ho"], c["wo"]), mode="bilinear", align_corners=bool(c["align_corners"])))
        elif op == "maxpool":
            for x in (t["x"], t["x"].float()):
                assert _same(P.maxpool_ref(x), F.max_pool2d(x, 3, 2, 1)), c["id"]
        elif op == "reg_head":
            k, r = c["k"], (c["k"] - 1) // 2
            # (sum w e f + b) / sum e = sum w p f + b / sum e with p = softmax(-dist^2) and e = exp(v - max v)
            v = -t["dist"].pow(2)
            p, esum = F.softmax(v, 1), (v - v.max(1, True)[0]).exp().sum(1, True)
            want = torch.cat([F.conv2d(p * F.unfold(t["flow"][:, ch:ch + 1], k, padding=r).view_as(p), wt) + b / esum
                              for ch, (wt, b) in enumerate(((t["wx"], t["bx"]), (t["wy"], t["by"])))], 1)
            assert float((ref - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max())), c["id"]
        elif op == "mean":
            assert _same(ref.view(c["N"], 2), t["flow"].mean((2, 3)), 1e-13), c["id"]


# ---- the bounds against the float32 restatement, with and without one seeded bug ---------------------------------------
@pytest.mark.parametrize("op", P.OPS)
def test_reference_and_float32_restatement_pass_the_bound(op):
    worst = worst_rounded = 0.0
    for c in P.CASES[op]:
        t = P.tensors(c["id"])
        ref = P.reference(c, t)
        bnd = P.bound(c, t, ref)
        assert P.ratio(ref, ref, bnd) == 0.0, c["id"]
        rounded = P.ratio(ref.float(), ref, bnd)  # the correctly rounded result
        r32 = P.ratio(P.reference(c, t, F32), ref, bnd)
        assert rounded < 1.0, "%s: the rounded reference is at %.3f of its bound" % (c["id"], rounded)
        assert r32 < 1.0, "%s: the float32 restatement is at %.3f of its bound (ill-conditioned inputs?)" % (c["id"], r32)
        worst, worst_rounded = max(worst, r32), max(worst_rounded, rounded)
    print("   %-9s %3d cases: float32 restatement worst err / bound %.3f, rounded reference %.3f" % (op, len(P.CASES[op]), worst, worst_rounded))


@pytest.mark.parametrize("bug,op", [(b, op) for b, ops in P.BUGS.items() for op in ops])
def test_bound_catches_the_mutation(bug, op):
    """the worst output of every case the mutation applies to.  A case whose samples all land outside the map ("edge", the
    2 x 2 maps under "far" / "integer") does not depend on its source, so a third of the cases may miss; the worst over the
    operator must be 10x outside"""
    rs = []
    for c in P.CASES[op]:
        if P.bug_applies(c, bug) and c.get("flow") != "edge":
            t = P.tensors(c["id"])
            ref = P.reference(c, t)
            rs.append((P.ratio(P.reference(c, t, F32, bug), ref, P.bound(c, t, ref)), c["id"]))
    assert rs, "no case takes this mutation"
    rs.sort()
    print("   MUTATION %-24s %-9s %3d cases: err / bound from %.3g (%s) to %.3g" % (bug, op, len(rs), rs[0][0], rs[0][1], rs[-1][0]))
    assert rs[-1][0] >= 10
    assert sum(r >= 10 for r, _ in rs) * 3 >= 2 * len(rs), rs[:len(rs) // 3 + 1]
