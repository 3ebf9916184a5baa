"""The convolution dispatcher's instantiations, one ragged layer for each: the table behind tests/test_conv_variants_gpu.py
(device) and tests/test_conv_variants_cpu.py (the table against the launcher sources).  Plain data and helpers; nothing here
touches the GPU.

A variant is named by the tag the per-launch profile records (the `variant` column of DFVO_CONV_PROFILE_CSV, see
conv_profile_end in df-vo_amd/csrc/conv_profile.hip): the launcher's family and its template arguments,
    igemm<WM,WN,TM,TN>   win3<WM,WN,TM,TN,KS>   head<KS,CO,py1|py2>   f16s<WC,WR,TC,TR>   f16s2<WC,WR,TC,TR>
    f16s2mix<WC,WR,TC,TRA,TRB>   f16g<WP,KSP,TC[,rag]>   taps<TH,TC>   f32g<WP,KSP,TC>   wino<WN>
followed in the profile by " np3" / " np1" (the f16 families, by packing) and " tickets" / " epilogue" (a launch whose K
slices over grid.z were finished in the kernel / by conv_splitk_epilogue).

VARIANTS      tag -> the packings (dfvo_set_conv_precision) in which dfvo_conv2d can reach it without an environment switch.
              The head kernels are exact fp32 in every packing.  conv_igemm_f32_kernel is listed under fp32 alone: in the f16
              packings only a kernel wider than 31 taps falls through to it.  wino<WN> needs dfvo_set_fp32_winograd (a call,
              not an environment switch): its two cases turn mode 2 on around the launch.
UNREACHABLE   what no case can run, each with its reason: the forms that only a switch read once per process selects.  (The
              three 256-row tiles of profile rows 2 / 4 / 6, which no tile rule chose, are no longer built.)
              The " epilogue" finish of a split-K launch is one of the latter (DFVO_SPLITK_FUSED=0): split-K needs fewer than
              600 tiles and the tickets cover 4096, so the in-kernel finish always applies; a child process of
              tests/test_nets_gpu.py compares the two finishes bit for bit.
CASES         per variant the smallest layer that reaches it, ragged in every dimension of the tile (see raggedness()), plus
              the view cases: sources, residual and destination as views of wider buffers, aligned and not.
"""
import re

PRECISIONS = ("fp32", "f16x3", "f16")
_ALL, _FP32, _F16, _F16X3 = PRECISIONS, ("fp32",), ("f16x3", "f16"), ("f16x3",)

VARIANTS = {}
for _t in ("2,2,4,4", "1,4,4,2", "1,4,2,2", "2,2,4,2", "2,2,2,2", "4,1,2,2", "2,2,2,1", "4,1,2,1", "4,1,1,1"):
    VARIANTS["igemm<%s>" % _t] = _FP32
for _t in ("2,2,4,4,3", "2,2,4,2,3", "1,4,4,2,3", "4,1,2,2,3", "4,1,2,1,5", "4,1,2,1,7"):
    VARIANTS["win3<%s>" % _t] = _FP32
for _k in (3, 5, 7):
    for _co in (1, 2):
        for _py in ("py1", "py2"):
            VARIANTS["head<%d,%d,%s>" % (_k, _co, _py)] = _ALL
VARIANTS["f16s<1,4,1,1>"] = _F16
for _t in ("2,2,2,3", "2,2,2,2", "1,4,2,3", "1,4,2,2", "1,4,1,3", "1,4,1,2"):
    VARIANTS["f16s2<%s>" % _t] = _F16
for _t in ("2,2,2,3,2", "1,4,2,3,2"):
    VARIANTS["f16s2mix<%s>" % _t] = _F16X3  # (the f16 packing keeps single heights: launch_f16s2's mix_ok)
for _t in ("4,1,2", "2,2,2", "1,4,2", "1,8,2", "4,1,1", "2,2,1", "1,4,1", "1,8,1", "1,16,1"):
    VARIANTS["f16g<%s>" % _t] = _F16
    VARIANTS["f32g<%s>" % _t] = _FP32
for _t in ("4,1,2,rag", "4,1,1,rag"):
    VARIANTS["f16g<%s>" % _t] = _F16
for _t in ("4,2", "4,1", "2,2", "2,1"):
    VARIANTS["taps<%s>" % _t] = _F16
for _t in ("1", "2"):
    VARIANTS["wino<%s>" % _t] = _FP32

UNREACHABLE = {
    # forms of reachable instantiations that only a test hook, read once per process, selects
    "DFVO_TAPS=0": "f16g<4,1,TC> on the tap-window kernel's layers: the child process of tests/test_nets_gpu.py compares the two",
    "DFVO_WIN_MIX=0": "single-height f16s2 launches where the mixed rule fires: child processes of "
                      "tests/test_ops_gpu.py::test_mixed_height_window_launches_are_bit_identical",
    "DFVO_WIN_FORCE_TR": "f16s2<.,.,.,2|3> whatever the grid: the same child processes",
    "DFVO_HEAD_PY1=0": "head<KS,CO,py2> on the small maps: the child process of tests/test_nets_gpu.py",
}
UNREACHABLE_TAGS = sorted(t for t in UNREACHABLE if "<" in t)

ACTS = {"none": 0, "leaky": 1, "relu": 2, "elu": 3, "sigmoid": 4}


def _case(cid, tag, n, h, w, c0, cout, k=(3, 3), stride=1, pad=None, c1=0, reflect=False, up0=False, act="none", res=False,
          zero_to=0, view=None, splitk="", only=None, wino=False, family=None, fills_block=False):
    """h, w: the map of source 0 as stored (the taps see 2h x 2w with up0).  tag: one tag, or {packing: tag} where the
    packings send the layer to different families.  view: overrides of cs0 co0 cs1 co1 dst_cs dst_co res_cs res_co
    (defaults: dense, offset 0).  only: the packings to run (default: those of the tag in VARIANTS).  fills_block: the case
    reaches its tag by a route that only a cout filling the block takes."""
    kh, kw = k
    tags = tag if isinstance(tag, dict) else {p: tag for p in (only or VARIANTS[tag])}
    v = dict(cs0=(c0 + 3) // 4 * 4, co0=0, cs1=(c1 + 3) // 4 * 4, co1=0, dst_cs=(max(cout, zero_to) + 3) // 4 * 4, dst_co=0,
             res_cs=(cout + 3) // 4 * 4, res_co=0)
    v.update(view or {})
    return dict(id=cid, tags=tags, N=n, h=h, w=w, c0=c0, c1=c1, cout=cout, kh=kh, kw=kw, stride=stride,
                pad=pad if pad is not None else (kh // 2, kw // 2), pad_mode=1 if reflect else 0, up0=1 if up0 else 0, act=ACTS[act],
                act_param=0.1 if act == "leaky" else 1.0, res=res, zero_to=zero_to, view=v, is_view=view is not None,
                splitk=splitk, wino=wino, family=family, fills_block=fills_block)


def _ring(tail):
    return {"fp32": "f32g<%s>" % tail, "f16x3": "f16g<%s>" % tail, "f16": "f16g<%s>" % tail}


CASES = [
    # ---- conv_igemm_f32_kernel (fp32): flat M tiles of BM = WM TM 16 pixels x BN = WN TN 16 couts.  Rows 9-11 need M >= 400000
    _case("igemm_128x128", "igemm<2,2,4,4>", 2, 501, 77, 4, 256, k=(1, 1), act="leaky"),
    _case("igemm_64x128_elu", "igemm<1,4,4,2>", 2, 7, 601, 4, 128, k=(1, 1), act="elu"),
    _case("igemm_32x128_1x33", "igemm<1,4,2,2>", 2, 5, 9, 4, 128, k=(1, 33)),
    _case("igemm_32x128_1x33_splitk", "igemm<1,4,2,2>", 2, 5, 9, 20, 128, k=(1, 33), splitk="tickets"),
    _case("igemm_64x64_zero_to", "igemm<2,2,2,2>", 2, 75, 57, 3, 49, k=(1, 1), zero_to=52),
    _case("igemm_64x64_s2_cat_splitk", "igemm<2,2,2,2>", 2, 150, 115, 20, 49, c1=20, stride=2, act="leaky", splitk="tickets"),
    _case("igemm_128x64_bigM", "igemm<2,2,4,2>", 2, 601, 333, 4, 49, k=(1, 1)),
    _case("igemm_64x32_res_n3", "igemm<2,2,2,1>", 3, 57, 51, 4, 17, k=(1, 1), res=True, act="relu"),
    _case("igemm_128x32_bigM_s2", "igemm<4,1,2,2>", 2, 1201, 667, 4, 17, stride=2, act="leaky"),
    _case("igemm_64x16_sigmoid", "igemm<4,1,1,1>", 2, 75, 57, 4, 5, k=(1, 1), act="sigmoid"),
    _case("igemm_64x16_refl_up", "igemm<4,1,1,1>", 2, 38, 57, 4, 5, reflect=True, up0=True, act="elu"),
    _case("igemm_128x16_bigM", "igemm<4,1,2,1>", 2, 601, 333, 4, 5, k=(1, 1)),
    _case("igemm_64x128_7x1_splitk", "igemm<1,4,4,2>", 2, 7, 601, 36, 128, k=(7, 1), act="leaky", splitk="tickets"),
    _case("igemm_64x32_s2_splitk", "igemm<2,2,2,1>", 2, 150, 115, 36, 17, stride=2, splitk="tickets"),
    _case("igemm_64x16_s2_splitk", "igemm<4,1,1,1>", 2, 150, 115, 36, 5, stride=2, act="leaky", splitk="tickets"),
    _case("igemm_view", "igemm<2,2,2,2>", 2, 75, 57, 4, 49, k=(1, 1), c1=4, res=True, act="leaky",
          view=dict(cs0=12, co0=4, cs1=16, co1=8, dst_cs=60, dst_co=4, res_cs=56, res_co=4)),
    _case("igemm_view_unaligned", "igemm<2,2,2,1>", 2, 75, 57, 4, 17, k=(1, 1), res=True,
          view=dict(cs0=8, co0=4, dst_cs=23, dst_co=3, res_cs=21, res_co=1)),
    # ---- conv_win_f32_kernel (fp32): TH = WM TM rows x 16 columns
    _case("win3_8x16x128", "win3<2,2,4,4,3>", 2, 131, 205, 4, 128, act="leaky"),
    _case("win3_8x16x64_zero_to", "win3<2,2,4,2,3>", 2, 37, 413, 4, 49, zero_to=52),
    # (the 128-cout route to the 64-wide tile, conv_window_cfg's tiles8 >= 1200: two column blocks per tile)
    _case("win3_8x16x64_two_column_blocks", "win3<2,2,4,2,3>", 2, 301, 253, 4, 128, act="leaky", fills_block=True),
    _case("win3_8x16x64_cat_splitk", "win3<2,2,4,2,3>", 2, 37, 413, 36, 49, c1=20, act="leaky", splitk="tickets"),
    _case("win3_4x16x128_refl_up_elu", "win3<1,4,4,2,3>", 2, 19, 207, 4, 128, reflect=True, up0=True, act="elu"),
    _case("win3_8x16x32_res", "win3<4,1,2,2,3>", 2, 37, 413, 3, 17, res=True, act="relu"),
    _case("win3_8x16x32_splitk", "win3<4,1,2,2,3>", 2, 37, 413, 52, 17, splitk="tickets"),
    _case("win5_n3", "win3<4,1,2,1,5>", 3, 27, 101, 20, 5, k=(5, 5)),
    _case("win5_splitk", "win3<4,1,2,1,5>", 2, 37, 109, 52, 5, k=(5, 5), splitk="tickets"),
    _case("win7_sigmoid", "win3<4,1,2,1,7>", 2, 37, 109, 20, 5, k=(7, 7), act="sigmoid"),
    _case("win3_view", "win3<4,1,2,2,3>", 2, 37, 413, 4, 17, c1=4, res=True, act="leaky",
          view=dict(cs0=8, co0=4, cs1=12, co1=4, dst_cs=28, dst_co=8, res_cs=24, res_co=4)),
    _case("win3_view_unaligned", "win3<4,1,2,2,3>", 2, 37, 413, 4, 17, view=dict(cs0=8, co0=4, dst_cs=22, dst_co=0)),
    # ---- conv_head_f32_kernel (every packing, exact fp32): 16 PY rows x 16 columns, 8-channel chunks
    _case("head3_1_py1_n3", "head<3,1,py1>", 3, 9, 57, 20, 1),
    _case("head3_1_py2_refl_sigmoid", "head<3,1,py2>", 2, 99, 509, 20, 1, reflect=True, act="sigmoid"),
    _case("head3_2_py1_cat", "head<3,2,py1>", 2, 9, 57, 20, 2, c1=3),
    _case("head3_2_py2", "head<3,2,py2>", 2, 99, 509, 4, 2, act="leaky"),
    _case("head5_1_py1_elu", "head<5,1,py1>", 2, 9, 57, 20, 1, k=(5, 5), act="elu"),
    _case("head5_1_py2", "head<5,1,py2>", 2, 99, 509, 4, 1, k=(5, 5)),
    _case("head5_2_py1", "head<5,2,py1>", 2, 9, 57, 20, 2, k=(5, 5)),
    _case("head5_2_py2_zero_to", "head<5,2,py2>", 2, 99, 509, 4, 2, k=(5, 5), zero_to=4),
    _case("head7_1_py1", "head<7,1,py1>", 2, 9, 57, 20, 1, k=(7, 7)),
    _case("head7_1_py2", "head<7,1,py2>", 2, 99, 509, 4, 1, k=(7, 7)),
    _case("head7_2_py1_refl_up", "head<7,2,py1>", 2, 9, 29, 20, 2, k=(7, 7), reflect=True, up0=True),
    _case("head7_2_py2_res", "head<7,2,py2>", 2, 99, 509, 4, 2, k=(7, 7), res=True),
    _case("head_view", "head<3,2,py1>", 2, 9, 57, 20, 2, c1=4, res=True,
          view=dict(cs0=28, co0=4, cs1=12, co1=8, dst_cs=8, dst_co=4, res_cs=8, res_co=4)),
    _case("head_view_unaligned", "head<5,2,py1>", 2, 9, 57, 20, 2, k=(5, 5), res=True,
          view=dict(cs0=24, co0=4, dst_cs=7, dst_co=3, res_cs=5, res_co=1)),
    # ---- the register-ring kernels, conv_gemm_f32g_kernel (fp32) and conv_gemm_f16s_kernel (f16x3 / f16): WP blocks of 32
    # pixels x 32 TC couts per workgroup, K sliced over KSP waves.  One layer reaches the same <WP,KSP,TC> in every packing
    _case("ring_4_1_2_res", _ring("4,1,2"), 2, 13, 21, 4, 49, k=(1, 1), res=True, act="leaky"),
    _case("ring_2_2_2", _ring("2,2,2"), 2, 13, 21, 18, 49, act="leaky"),
    _case("ring_1_4_2_cat", _ring("1,4,2"), 2, 13, 21, 20, 49, c1=20, act="relu"),
    _case("ring_1_8_2_zero_to", _ring("1,8,2"), 2, 13, 21, 68, 49, zero_to=52),
    _case("ring_4_1_1_elu", _ring("4,1,1"), 2, 13, 21, 4, 17, k=(1, 1), act="elu"),
    _case("ring_2_2_1_s2_sigmoid", _ring("2,2,1"), 2, 27, 41, 20, 17, stride=2, act="sigmoid"),
    _case("ring_1_4_1_refl_up", _ring("1,4,1"), 2, 7, 11, 36, 17, reflect=True, up0=True, act="elu"),
    _case("ring_1_8_1_n3", _ring("1,8,1"), 3, 13, 21, 68, 17, res=True),
    _case("ring_1_16_1", _ring("1,16,1"), 2, 13, 21, 116, 17, act="leaky"),
    _case("ring_rag_2", {"fp32": "f32g<4,1,2>", "f16x3": "f16g<4,1,2,rag>", "f16": "f16g<4,1,2,rag>"}, 2, 13, 21, 4, 49, k=(1, 1),
          act="leaky", zero_to=52),
    _case("ring_rag_1", {"fp32": "f32g<4,1,1>", "f16x3": "f16g<4,1,1,rag>", "f16": "f16g<4,1,1,rag>"}, 2, 13, 21, 4, 17, k=(1, 1),
          act="relu"),
    _case("ring_view", _ring("1,4,2"), 2, 13, 21, 20, 49, c1=20, res=True, act="leaky",
          view=dict(cs0=28, co0=4, cs1=32, co1=8, dst_cs=60, dst_co=4, res_cs=56, res_co=4)),
    # the destination of a RAG layer as an aligned view that is not the whole buffer; the same layer unaligned must leave RAG
    _case("ring_rag_view", {"fp32": "f32g<4,1,2>", "f16x3": "f16g<4,1,2,rag>", "f16": "f16g<4,1,2,rag>"}, 2, 13, 21, 4, 49, k=(1, 1),
          view=dict(cs0=12, co0=8, dst_cs=60, dst_co=8)),
    _case("ring_rag_view_unaligned", _ring("4,1,2"), 2, 13, 21, 4, 49, k=(1, 1), view=dict(cs0=12, co0=8, dst_cs=61, dst_co=7)),
    _case("ring_rag_1_view", {"fp32": "f32g<4,1,1>", "f16x3": "f16g<4,1,1,rag>", "f16": "f16g<4,1,1,rag>"}, 2, 13, 21, 4, 17, k=(1, 1),
          view=dict(cs0=8, co0=4, dst_cs=28, dst_co=4)),
    _case("ring_view_unaligned", _ring("1,4,1"), 2, 13, 21, 36, 17, res=True,
          view=dict(cs0=44, co0=4, dst_cs=21, dst_co=2, res_cs=19, res_co=1)),
    # ---- conv_win_f16s_kernel, the first window skeleton (f16x3 / f16): 4 rows x 32 columns x 32 couts
    _case("f16s_cat_res", "f16s<1,4,1,1>", 2, 203, 41, 4, 17, c1=4, res=True, act="leaky"),
    _case("f16s_refl_up_elu_n3", "f16s<1,4,1,1>", 3, 67, 21, 20, 17, reflect=True, up0=True, act="elu", zero_to=20),
    _case("f16s_view", "f16s<1,4,1,1>", 2, 203, 41, 4, 17, c1=4, res=True, act="leaky",
          view=dict(cs0=8, co0=4, cs1=12, co1=4, dst_cs=28, dst_co=8, res_cs=24, res_co=4)),
    _case("f16s_view_unaligned", "f16s<1,4,1,1>", 2, 203, 41, 4, 17, view=dict(cs0=8, co0=4, dst_cs=22, dst_co=1)),
    # ---- conv_win_f16s2_kernel, the second skeleton: WR TR rows x 32 columns x WC TC 32 couts
    _case("f16s2_4rows_128", "f16s2<2,2,2,2>", 2, 203, 41, 3, 100, act="leaky"),
    _case("f16s2_6rows_128_cat", "f16s2<2,2,2,3>", 2, 301, 41, 4, 100, c1=4, act="leaky"),
    _case("f16s2_8rows_64_zero_to", "f16s2<1,4,2,2>", 2, 401, 41, 4, 49, zero_to=52),
    _case("f16s2_12rows_64_res", "f16s2<1,4,2,3>", 2, 601, 41, 4, 49, res=True, act="relu"),
    _case("f16s2_8rows_32_n3", "f16s2<1,4,1,2>", 3, 269, 41, 4, 17, act="leaky"),
    _case("f16s2_12rows_32_refl_up_elu", "f16s2<1,4,1,3>", 2, 301, 21, 4, 17, reflect=True, up0=True, act="elu"),
    _case("f16s2_mixed_6_4_rows_128", "f16s2mix<2,2,2,3,2>", 2, 601, 41, 4, 100, act="leaky"),
    _case("f16s2_mixed_12_8_rows_64", "f16s2mix<1,4,2,3,2>", 2, 203, 301, 4, 49, res=True, act="leaky"),
    _case("f16s2_view", "f16s2<1,4,2,2>", 2, 401, 41, 4, 49, c1=4, res=True, act="leaky",
          view=dict(cs0=8, co0=4, cs1=12, co1=4, dst_cs=60, dst_co=8, res_cs=56, res_co=4)),
    _case("f16s2_view_unaligned", "f16s2<1,4,2,2>", 2, 401, 41, 4, 49, res=True, view=dict(cs0=8, co0=4, dst_cs=51, dst_co=1, res_cs=50)),
    # ---- conv_taps_f16s_kernel (f16x3 / f16): TH rows x 32 columns, one source, aligned destination, bias + none / leaky / relu
    _case("taps_4rows_32_zero_to", "taps<4,1>", 2, 13, 21, 3, 17, act="leaky", zero_to=20),
    _case("taps_4rows_64_7x1_n3", "taps<4,2>", 3, 13, 21, 4, 49, k=(7, 1), act="relu"),
    _case("taps_2rows_32_7x7", "taps<2,1>", 2, 401, 41, 36, 17, k=(7, 7), act="leaky"),
    _case("taps_2rows_64_7x7", "taps<2,2>", 2, 401, 41, 36, 49, k=(7, 7)),
    _case("taps_view", "taps<4,2>", 2, 13, 21, 4, 49, k=(1, 7), act="leaky", view=dict(cs0=12, co0=4, dst_cs=60, dst_co=8)),
    # the tap-window kernel and RAG decline an unaligned destination: the plain ring shape takes the layer
    _case("taps_view_unaligned", "f16g<4,1,2>", 2, 13, 21, 4, 49, k=(1, 7), act="leaky", view=dict(cs0=12, co0=4, dst_cs=51, dst_co=1),
          family="taps"),
    # ---- conv_wino_f32_kernel (fp32, dfvo_set_fp32_winograd(2) around the launch): tests/test_wino_gpu.py gates the kernel,
    # here its tag and its writes
    _case("wino_32", "wino<1>", 2, 13, 21, 4, 17, act="leaky", wino=True),
    _case("wino_64", "wino<2>", 2, 13, 21, 4, 49, act="leaky", wino=True),
]

FAMILIES = ("igemm", "win3", "head", "ring", "f16s", "f16s2", "f16s2mix", "taps", "wino")


def profile_tag(case, precision):
    """what the profile's variant column must say for `case` under `precision`"""
    tag = case["tags"][precision]
    fam = family_of(tag)
    np_ = {"f16x3": " np3", "f16": " np1"}[precision] if fam in ("f16s", "f16s2", "f16s2mix", "f16g", "taps") else ""
    return tag + np_ + (" " + case["splitk"] if case["splitk"] else "")


def family_of(tag):
    return re.match(r"\w+", tag).group(0)


for _c in CASES:  # the kernel family a case belongs to (the two register-ring kernels are one: they share their cases)
    if _c["family"] is None:
        _f = family_of(sorted(_c["tags"].values())[0])
        _c["family"] = "ring" if _f in ("f16g", "f32g") else _f


def tag_args(tag):
    return [int(a) if a.isdigit() else a for a in tag[tag.index("<") + 1:-1].split(",")]


def out_size(case):
    H, W = (2 * case["h"], 2 * case["w"]) if case["up0"] else (case["h"], case["w"])
    ho = (H + 2 * case["pad"][0] - case["kh"]) // case["stride"] + 1
    wo = (W + 2 * case["pad"][1] - case["kw"]) // case["stride"] + 1
    return H, W, ho, wo


def tile_of(tag):
    """(tile heights (empty: a flat run of pixels), pixels per flat tile or None, couts per block) of a tag"""
    fam, a = family_of(tag), tag_args(tag)
    if fam == "igemm":
        return (), a[0] * a[2] * 16, a[1] * a[3] * 16
    if fam == "win3":
        return (a[0] * a[2],), None, a[1] * a[3] * 16
    if fam == "head":
        return (16 if a[2] == "py1" else 32,), None, None
    if fam in ("f16s", "f16s2"):
        return (a[1] * a[3],), None, a[0] * a[2] * 32
    if fam == "f16s2mix":
        return (a[1] * a[3], a[1] * a[4]), None, a[0] * a[2] * 32
    if fam in ("f16g", "f32g"):
        return (), 32 * a[0], 32 * a[2]
    if fam == "taps":
        return (a[0],), None, 32 * a[1]
    if fam == "wino":
        return (16,), None, 32 * a[0]
    raise ValueError(tag)


# tags whose rule only admits couts that fill the block: conv_pick_bn returns 128 for the multiples of 128 alone
COUT_FILLS_BLOCK = {"igemm<2,2,4,4>", "igemm<1,4,4,2>", "igemm<1,4,2,2>", "win3<2,2,4,4,3>", "win3<1,4,4,2,3>"}


def raggedness(case):
    """the ragged-tile conditions a case violates (empty: none), from the tile sizes its tags name"""
    bad = []
    _, _, ho, wo = out_size(case)
    m = case["N"] * ho * wo
    if wo % 16 == 0:
        bad.append("Wo %d is a multiple of 16" % wo)
    if case["N"] < 2:
        bad.append("N < 2")
    if case["c0"] % 16 == 0 or ((case["c0"] + 3) // 4) % 4 != 1:
        bad.append("c0 %d: not a 4-channel tail behind whole 16-channel chunks" % case["c0"])
    for tag in set(case["tags"].values()):
        heights, flat, bn = tile_of(tag)
        for th in heights:
            if ho % th == 0:
                bad.append("%s: Ho %d is a multiple of the tile height %d" % (tag, ho, th))
        if flat and m % flat == 0:
            bad.append("%s: M %d is a multiple of the %d-pixel tile" % (tag, m, flat))
        if bn and case["cout"] % bn == 0 and tag not in COUT_FILLS_BLOCK and not case["fills_block"]:
            bad.append("%s: cout %d fills the %d-cout block" % (tag, case["cout"], bn))
    return bad
