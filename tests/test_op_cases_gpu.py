"""Every non-conv operator variant of df-vo_amd/csrc/ops.hip at ragged maps and views, against float64 -- tests/op_cases.py
holds the table, tests/test_op_cases_cpu.py checks the table, its references and its bounds without a device.

One test per case.  A case goes through the operator's C entry point once and asserts:
  (a) for the three dispatching launchers, that the library's query (dfvo_deconv_variant, dfvo_correlation_variant,
      dfvo_reg_head_variant: the function the launcher itself calls) names the kernel the case declares, before the launch;
  (b) every output element is within tests/flow_bounds.py's derived bound of the float64 operator on the same fp32 operands
      (max pool: bit for bit), NaN exactly where the reference is NaN.  k_reg_head takes k_reg_head_v's bound: the two
      kernels run the same operations in the same order (fp32 -d^2, fmaxf, expf of the fp32 difference, the three sums in
      double, one rounding of the quotient), which is what the bound's derivation assumes;
  (c) the writes stay inside the destination view: the destination lies in a buffer of sentinels with a band in front of
      and behind it, and afterwards the bands, the channels outside the view, the pixels a step-k warp skips and the
      channels behind the last written quad still hold the sentinel.  Pinned, as read from the kernels: the two quad
      deconv kernels write the pad channels [C, round_up(C, 4)) as zeros (C = 49 in 52, C = 2 in 4) and the scalar kernel
      writes [0, C) alone; the correlation kernels write 49 channels and leave [49, dcs) alone; an appending warp writes
      the flow and two zeros; reg prep writes a zero fourth channel;
  (d) nothing outside a source view enters a result: every source lies in a buffer whose bands, out-of-view channels and
      pad channels hold NaN;
  (e) under swap the output comes from sample N - 1 - n: the device result is far outside the bound of a float64 reference
      that ignores the swap.
Twin cases run the same values through two kernels in one process (deconv C = 49 at cs 49 / 52: scalar against block
kernel; reg head at dist_cs 9 / 12, 25 / 28, 49 / 52: k_reg_head against k_reg_head_v<k>) and must agree bit for bit.  One
child process started with DFVO_CORR_RT=0 runs every case of k_correlation_rt on k_correlation, with the same checks, and
hands back its outputs: the parent's are the same bits.  The refusals of tests/op_cases.py answer DFVO_ERR_ARG naming the
function, leave the destination alone, and the next valid call is correct.  The last test prints the worst err / bound per
operator and variant (docs/parity.md)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import op_cases as P

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
NAN = float("nan")
BAND = 64  # floats in front of and behind every view (a multiple of 4: the views keep their 16-byte alignment)
_out = {}   # case id -> the device result (logical channels, NCHW, on the host)
_seen = {}  # (operator, variant) -> [worst err / bound, cases]


def _banded(x, cs, co, fill=NAN):
    """NCHW x as the view (cs floats per pixel, channel offset co) of a device buffer that holds `fill` everywhere else,
    pad channels included.  Returns (buffer, pointer to the first pixel)"""
    n, c, h, w = x.shape
    inner = torch.full((n, h, w, cs), fill, dtype=torch.float32)
    inner[..., co:co + c] = x.permute(0, 2, 3, 1)
    buf = torch.full((2 * BAND + inner.numel(),), fill, dtype=torch.float32)
    buf[BAND:BAND + inner.numel()] = inner.reshape(-1)
    buf = buf.cuda()
    return buf, C.c_void_p(buf.data_ptr() + 4 * BAND)


class _Dst:
    """a destination [n, h, w, cs] of sentinels between two bands of sentinels"""

    def __init__(self, n, h, w, cs):
        self.shape = (n, h, w, cs)
        self.numel = n * h * w * cs
        self.buf = torch.full((2 * BAND + self.numel,), SENTINEL, device="cuda")
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * BAND)

    def read(self, cid):
        """the view on the host (NHWC); the bands must be untouched"""
        host = self.buf.cpu()
        assert bool((host[:BAND] == SENTINEL).all()) and bool((host[BAND + self.numel:] == SENTINEL).all()), \
            "%s: wrote outside the destination buffer" % cid
        return host[BAND:BAND + self.numel].view(*self.shape)


def _untouched(t, cid, what):
    assert bool((t == SENTINEL).all()), "%s: wrote %s" % (cid, what)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _lin(n):
    return torch.linspace(-1.0, 1.0, n).numpy()


def run_case(capi, case, expect_variant=None):
    """the device result of `case` (logical channels, NCHW, host) after checks (a), (c) and (d)"""
    lib, cid, op = capi.lib(), case["id"], case["op"]
    t = P.tensors(cid)
    n, h, w = case["N"], case["h"], case["w"]
    want = case.get("variant") if expect_variant is None else expect_variant
    if op == "corr":
        s = case["stride"]
        ho, wo = -(-h // s), -(-w // s)
        b1, p1 = _banded(t["f1"], case["cs1"], case["co1"])
        b2, p2 = _banded(t["f2"], case["cs2"], case["co2"])
        got = lib.dfvo_correlation_variant(case["C"], case["cs1"], case["co1"], case["cs2"], case["co2"])
        assert got == want, "%s: the launcher runs variant %d, the case declares %d" % (cid, got, want)
        dst = _Dst(n, ho, wo, case["dcs"])
        capi.check(lib.dfvo_correlation_view(p1, case["cs1"], case["co1"], p2, case["cs2"], case["co2"], case["swap2"], n, h, w,
                                             case["C"], s, 0.1, dst.ptr, case["dcs"], None))
        o = dst.read(cid)
        _untouched(o[..., 49:], cid, "channels [49, dcs)")
        return _nchw(o[..., :49])
    if op == "deconv":
        c, cs = case["C"], case["cs"]
        got = lib.dfvo_deconv_variant(c, cs)
        assert got == want, "%s: the launcher runs variant %d, the case declares %d" % (cid, got, want)
        bx, px = _banded(t["x"], cs, 0)
        dst = _Dst(n, 2 * h, 2 * w, cs)
        capi.check(lib.dfvo_deconv_dw4x4s2(px, n, h, w, c, cs, capi.as_ptr(np.ascontiguousarray(t["w"].numpy())), dst.ptr, None))
        o = dst.read(cid)
        end = c if want == 2 else (c + 3) // 4 * 4
        assert bool((o[..., c:end] == 0).all()), "%s: pad channels [%d, %d) are not zero" % (cid, c, end)
        _untouched(o[..., end:], cid, "channels behind the last written quad")
        return _nchw(o[..., :c])
    if op == "warp":
        c, st, app = case["C"], case["step"], case["append_flow"]
        bs, ps = _banded(t["src"], case["scs"], case["sco"])
        bf, pf = _banded(t["flow"], case["fcs"], case["fco"])
        dst = _Dst(n, h, w, case["dcs"])
        capi.check(lib.dfvo_warp_view(ps, case["scs"], case["sco"], case["swap"], pf, case["fcs"], case["fco"], case["mult"], n, h, w, c,
                                      capi.as_ptr(_lin(w)), capi.as_ptr(_lin(h)), dst.ptr, case["dcs"], case["dco"], app, st, None))
        o = dst.read(cid)
        lo, hi = case["dco"], case["dco"] + c + 4 * app
        _untouched(o[..., :lo], cid, "channels in front of the view")
        _untouched(o[..., hi:], cid, "channels behind the view")
        keep = torch.ones(h, w, dtype=torch.bool)
        keep[::st, ::st] = False
        _untouched(o[:, keep], cid, "pixels a step-%d warp skips" % st)
        return _nchw(o[:, ::st, ::st, lo:hi])
    if op == "reg_prep":
        img4 = torch.cat([t["img"], torch.full((n, 1, h, w), NAN)], 1)  # (the fourth image channel is never used)
        bi, pi = _banded(img4, 4, 0)
        bf, pf = _banded(t["flow"], case["fcs"], case["fco"])
        bm, pm = _banded(t["mean"], 2, 0)
        dst = _Dst(n, h, w, 4)
        capi.check(lib.dfvo_reg_prep(pi, pf, case["fcs"], case["fco"], case["mult"], pm, n, h, w, capi.as_ptr(_lin(w)),
                                     capi.as_ptr(_lin(h)), dst.ptr, None))
        o = dst.read(cid)
        assert bool((o[..., 3] == 0).all()), "%s: channel 3 is not zero" % cid
        return _nchw(o[..., :3])
    if op == "reg_head":
        k = case["k"]
        bd, pd = _banded(t["dist"], case["dist_cs"], 0)
        bf, pf = _banded(t["flow"], case["fcs"], case["fco"])
        dst = _Dst(n, h, w, case["dcs"])
        got = lib.dfvo_reg_head_variant(pd, case["dist_cs"], k, pf, case["fcs"], case["fco"], dst.ptr, case["dcs"], case["dco"])
        assert got == want, "%s: the launcher runs variant %d, the case declares %d" % (cid, got, want)
        wx, wy = [np.ascontiguousarray(t[q].numpy().ravel()) for q in ("wx", "wy")]
        capi.check(lib.dfvo_reg_head(pd, case["dist_cs"], k, pf, case["fcs"], case["fco"], capi.as_ptr(wx), float(t["bx"]),
                                     capi.as_ptr(wy), float(t["by"]), n, h, w, dst.ptr, case["dcs"], case["dco"], None))
        o = dst.read(cid)
        _untouched(o[..., :case["dco"]], cid, "channels in front of the view")
        _untouched(o[..., case["dco"] + 2:], cid, "channels behind the view")
        return _nchw(o[..., case["dco"]:case["dco"] + 2])
    if op == "mean":
        bf, pf = _banded(t["flow"], case["fcs"], case["fco"])
        dst = _Dst(n, 1, 1, 2)
        capi.check(lib.dfvo_flow_mean(pf, case["fcs"], case["fco"], n, h * w, dst.ptr, None))
        return _nchw(dst.read(cid))
    if op == "resize":
        bx, px = _banded(t["x"], case["C"], 0)
        dst = _Dst(n, case["ho"], case["wo"], case["C"])
        capi.check(lib.dfvo_resize_bilinear(px, n, h, w, case["C"], dst.ptr, case["ho"], case["wo"], case["align_corners"], None))
        torch.cuda.synchronize()
        return _nchw(dst.read(cid))
    if op == "maxpool":
        bx, px = _banded(t["x"], case["C"], 0)
        dst = _Dst(n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, case["C"])
        capi.check(lib.dfvo_maxpool3x3s2(px, n, h, w, case["C"], dst.ptr, None))
        return _nchw(dst.read(cid))
    raise ValueError(op)


def check_case(capi, case, expect_variant=None):
    """run_case plus (b) and (e); returns (device result, worst err / bound)"""
    cid, op = case["id"], case["op"]
    got = run_case(capi, case, expect_variant)
    t = P.tensors(cid)
    ref = P.reference(case, t)
    bnd = P.bound(case, t, ref)
    st = case.get("step", 1)
    if st > 1:
        ref, bnd = ref[:, :, ::st, ::st], bnd[:, :, ::st, ::st]
    assert got.shape == ref.shape, (cid, got.shape, ref.shape)
    assert not bool((got == SENTINEL).any()), "%s: output elements never written" % cid
    r = P.ratio(got, ref, bnd)
    nan = torch.isnan(ref)
    err = (got.double() - ref).abs()[~nan]
    print("   %-52s max|ref| %.2e  max err %.2e  worst err / bound %.3f"
          % (cid, float(ref[~nan].abs().max()) if err.numel() else 0.0, float(err.max()) if err.numel() else 0.0, r))
    assert torch.equal(torch.isnan(got), nan), "%s: NaN where the reference has a number, or a number where it has NaN" % cid
    assert r < 1.0 if bnd is not None else r == 0.0, "%s: worst err / bound %.3f" % (cid, r)
    if P.bug_applies(case, "swap_ignored"):
        # (a case whose samples all land outside the map does not depend on its source: the rounded reference itself decides)
        wrong = P.reference(case, t, bug="swap_ignored")
        wrong = wrong[:, :, ::st, ::st] if st > 1 else wrong
        if P.ratio(ref.float(), wrong, bnd) >= 100:
            rs = P.ratio(got, wrong, bnd)
            assert rs >= 10, "%s: a reference that ignores the swap passes (err / bound %.3g)" % (cid, rs)
    return got, r


@pytest.mark.parametrize("cid", [c["id"] for c in P.ALL])
def test_op_case(gpu, cid):
    case = P.BY_ID[cid]
    got, r = check_case(gpu, case)
    _out[cid] = got
    key = (case["op"], case.get("variant", "-"))
    w = _seen.setdefault(key, [0.0, 0])
    w[0], w[1] = max(w[0], r), w[1] + 1


def _result(gpu, cid):
    if cid not in _out:
        _out[cid] = check_case(gpu, P.BY_ID[cid])[0]
    return _out[cid]


@pytest.mark.parametrize("a,b", P.twins("deconv") + P.twins("reg_head"))
def test_two_kernels_agree_bit_for_bit(gpu, a, b):
    """the same values through two views of one operator, in one process.  Different kernels: deconv C = 49 at cs 52 / 49
    (block / scalar), reg head at the aligned / unaligned dist_cs of k = 3, 5, 7 (k_reg_head_v<k> / k_reg_head)"""
    ca, cb = P.BY_ID[a], P.BY_ID[b]
    if ca["op"] == "reg_head" and ca["k"] in (3, 5, 7) or ca["C" if ca["op"] == "deconv" else "k"] == 49:
        assert ca["variant"] != cb["variant"], (a, b)
    ra, rb = _result(gpu, a), _result(gpu, b)
    assert torch.equal(ra, rb), "%s and %s differ: max |a - b| %.3g" % (a, b, float((ra - rb).abs().max()))


_CHILD = """
import importlib, sys
sys.path.insert(0, %(tests)r); sys.path.insert(0, %(root)r)
import __graft_entry__ as g
g.dfvo_amd()
import numpy as np
import op_cases as P
import test_op_cases_gpu as T
capi = importlib.import_module("df-vo_amd.capi")
capi.require_gpu()
out = {}
for case in P.CASES["corr"]:
    if case["variant"] >= 100:
        got, r = T.check_case(capi, case, expect_variant=case["variant_rt0"])
        out[case["id"]] = got.numpy()
np.savez(%(out)r, **out)
"""


def test_correlation_rt_and_generic_kernels_agree_bit_for_bit(gpu, tmp_path):
    """one child process under DFVO_CORR_RT=0 runs every k_correlation_rt case on k_correlation (its query must say so),
    with all checks of test_op_case; its outputs are the parent's rt outputs bit for bit"""
    tests = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "corr_rt0.npz")
    code = _CHILD % {"tests": tests, "root": os.path.dirname(tests), "out": out}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DFVO_CORR_RT="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    child = np.load(out)
    rt = [c for c in P.CASES["corr"] if c["variant"] >= 100]
    assert sorted(child.files) == sorted(c["id"] for c in rt) and len(rt) >= 50
    assert {c["variant"] // 100 for c in rt} == {1, 2, 3, 4, 6}
    for c in rt:
        mine = _result(gpu, c["id"]).numpy()
        assert np.array_equal(mine, child[c["id"]]), "%s: k_correlation_rt<%d> and k_correlation differ by %.3g" \
            % (c["id"], c["variant"] // 100, float(np.abs(mine - child[c["id"]]).max()))


def _refuse(gpu, R):
    """(return code, destination) of the refused call"""
    lib = gpu.lib()
    op = R["op"]
    x = lambda *s: torch.randn(*s).cuda()  # noqa: E731
    if op == "corr":
        a, b, dst = x(1, 3, 3, R["cs"]), x(1, 3, 3, R["cs"]), _Dst(1, 3, 3, 52)
        return lib.dfvo_correlation_view(C.c_void_p(a.data_ptr()), R["cs"], 0, C.c_void_p(b.data_ptr()), R["cs"], 0, 0, 1, 3, 3, R["C"],
                                         1, 0.1, dst.ptr, 52, None), dst
    h, w = R.get("h", 3), R.get("w", 3)
    if op == "warp":
        s, f, dst = x(1, h, w, R["scs"]), x(1, h, w, 2), _Dst(1, h, w, 8)
        return lib.dfvo_warp_view(C.c_void_p(s.data_ptr()), R["scs"], 0, 0, C.c_void_p(f.data_ptr()), 2, 0, 1.0, 1, h, w, 4,
                                  gpu.as_ptr(_lin(w)), gpu.as_ptr(_lin(h)), dst.ptr, 8, R["dco"], 0, 1, None), dst
    if op == "reg_prep":
        i, f, m, dst = x(1, h, w, 4), x(1, h, w, 2), x(1, 2), _Dst(1, h, w, 4)
        return lib.dfvo_reg_prep(C.c_void_p(i.data_ptr()), C.c_void_p(f.data_ptr()), 2, 0, 1.0, C.c_void_p(m.data_ptr()), 1, h, w,
                                 gpu.as_ptr(_lin(w)), gpu.as_ptr(_lin(h)), dst.ptr, None), dst
    if op == "mean":
        f, dst = x(1, 9, R["fcs"]), _Dst(1, 1, 1, 2)
        return lib.dfvo_flow_mean(C.c_void_p(f.data_ptr()), R["fcs"], 0, 1, 9, dst.ptr, None), dst
    if op == "resize":
        s, dst = x(1, 3, 3, R["C"]), _Dst(1, 2, 2, R["C"])
        return lib.dfvo_resize_bilinear(C.c_void_p(s.data_ptr()), 1, 3, 3, R["C"], dst.ptr, 2, 2, 0, None), dst
    raise ValueError(op)


@pytest.mark.parametrize("rid", [R["id"] for R in P.REFUSALS])
def test_refusals(gpu, rid):
    """DFVO_ERR_ARG with a message that names the function, nothing written, and the next valid call of the operator is
    correct"""
    R = next(R for R in P.REFUSALS if R["id"] == rid)
    lib = gpu.lib()
    rc, dst = _refuse(gpu, R)
    msg = lib.dfvo_last_error()
    assert rc == -2 and R["name"] in msg, (rid, rc, msg)
    torch.cuda.synchronize()
    _untouched(dst.read(rid), rid, "into the destination of a refused call")
    check_case(gpu, P.CASES[R["op"]][-1])


def test_report_of_the_variants_reached():
    """the per-variant report of this run (pytest -s): operator, variant code, cases, worst err / bound"""
    print("\n   operator variant cases worst err / bound")
    for (op, v) in sorted(_seen, key=str):
        print("   %-9s %-4s %3d  %.3f" % (op, v, _seen[(op, v)][1], _seen[(op, v)][0]))
