"""tests/conv_variants.py against the launcher sources and against its own rules -- no GPU.

  table against source   the template-argument lists at the launch sites of the dispatcher sources, spelled as profile tags,
                         are exactly VARIANTS + the instantiations of UNREACHABLE: a launch site added to a launcher without a
                         case fails here, before any GPU run
  coverage               every VARIANTS entry has a case in each of its packings; every kernel family has its view cases, aligned
                         and not, and the operand forms it supports
  raggedness             every case is ragged in every dimension of the tile its tag names (conv_variants.raggedness)"""
import os
import re

import conv_variants as V

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "df-vo_amd", "csrc")

# launcher template -> how its launch sites' arguments spell the tag
LAUNCHERS = {
    "conv_igemm_f32.hip": {"launch_cfg": "igemm", "launch_win3": "win3", "launch_head": "head"},
    "conv_f16.hip": {"launch_f16g_cfg": "f16g"},
    "conv_gemm_f32g.hip": {"launch_f32g_cfg": "f32g"},
    "conv_win_f16s.h": {"launch_f16s_cfg": "f16s"},
    "conv_win_f16s2.h": {"launch_f16s2_cfg": "f16s2", "launch_f16s2_mix": "f16s2mix"},
    "conv_taps_f16s.hip": {"taps_launch": "taps"},
    "conv_wino_f32.hip": {"launch_wino_cfg": "wino"},
}


def _source_tags():
    tags, sites = set(), 0
    for fname, launchers in LAUNCHERS.items():
        src = open(os.path.join(CSRC, fname)).read()
        for m in re.finditer(r"\b(%s)<([^<>()]*)>\(" % "|".join(launchers), src):
            args = [a.strip() for a in m.group(2).split(",")]
            if not all(re.fullmatch(r"\d+|true|false", a) for a in args):
                continue  # (a template's own forwarding call, spelled with its parameters)
            fam = launchers[m.group(1)]
            sites += 1
            if fam == "win3" and len(args) == 4:
                args.append("3")  # launch_win3's default KS
            if fam == "f16g":  # <WP, KSP, TC[, PF, RAG]>
                assert len(args) in (3, 5) and (len(args) == 3 or args[3] == "3"), m.group(0)
                args = args[:3] + (["rag"] if len(args) == 5 and args[4] == "true" else [])
            if fam == "head":  # launch_head<KS, CO> launches PY = 1 and PY = 2 of the kernel
                assert "conv_head_f32_kernel<KS, CO, 1>" in src and "conv_head_f32_kernel<KS, CO, 2>" in src
                tags.update("head<%s,py%d>" % (",".join(args), py) for py in (1, 2))
                continue
            tags.add("%s<%s>" % (fam, ",".join(args)))
    return tags, sites


def test_the_table_lists_exactly_the_instantiations_of_the_launchers():
    tags, sites = _source_tags()
    # (62 sites today: 65 before the three 256-row igemm tiles went)
    assert sites >= 60, "the launch sites were not found (%d): did a launcher's name change?" % sites
    table = set(V.VARIANTS) | set(V.UNREACHABLE_TAGS)
    assert tags == table, "in the sources only: %s; in the table only: %s" % (sorted(tags - table), sorted(table - tags))
    assert not set(V.VARIANTS) & set(V.UNREACHABLE)


def test_unreachable_holds_only_the_known_entries_each_with_a_reason():
    assert set(V.UNREACHABLE) == {"DFVO_TAPS=0", "DFVO_WIN_MIX=0", "DFVO_WIN_FORCE_TR", "DFVO_HEAD_PY1=0"}
    assert all(isinstance(r, str) and len(r) > 20 for r in V.UNREACHABLE.values())
    # rows 2 / 4 / 6 stay empty: conv_pick_bm has no path to 256, and no 256-row tile is launched
    src = open(os.path.join(CSRC, "conv_dispatch.hip")).read()
    body = src[src.index("static int conv_pick_bm("):src.index("// exact-fp32 mode: which layers leave")]
    assert "256" not in body
    assert not re.search(r"launch_cfg<\s*4,\s*1,\s*4,", open(os.path.join(CSRC, "conv_igemm_f32.hip")).read())
    # the switches are what the sources read
    srcs = "".join(open(os.path.join(CSRC, f)).read() for f in LAUNCHERS)
    for name in ("DFVO_TAPS", "DFVO_WIN_MIX", "DFVO_WIN_FORCE_TR", "DFVO_HEAD_PY1"):
        assert '"%s"' % name in srcs, name


def test_every_variant_has_a_case_in_each_of_its_packings():
    ids = [c["id"] for c in V.CASES]
    assert len(ids) == len(set(ids))
    covered = {(t, p) for c in V.CASES for p, t in c["tags"].items()}
    missing = [(t, p) for t, ps in V.VARIANTS.items() for p in ps if (t, p) not in covered]
    assert not missing, missing
    for c in V.CASES:
        for p, t in c["tags"].items():
            assert t in V.VARIANTS and p in V.VARIANTS[t], (c["id"], p, t)
    # the split-K finish: every contracting fp32 kernel has a case finished by tickets.  (" epilogue" cannot be reached
    # without DFVO_SPLITK_FUSED=0: split-K needs fewer than 600 tiles, the tickets cover 4096 -- tests/test_nets_gpu.py's
    # child process compares the two finishes bit for bit.)
    split = {V.family_of(t) for c in V.CASES if c["splitk"] for t in c["tags"].values()}
    assert all(c["splitk"] in ("", "tickets") for c in V.CASES) and split == {"igemm", "win3"}


def test_every_case_is_ragged_in_every_dimension_of_its_tile():
    bad = {c["id"]: V.raggedness(c) for c in V.CASES if V.raggedness(c)}
    assert not bad, bad
    for c in V.CASES:  # the views hold together
        v, c0p, c1p = c["view"], (c["c0"] + 3) // 4 * 4, (c["c1"] + 3) // 4 * 4
        assert v["co0"] % 4 == 0 and v["cs0"] % 4 == 0 and v["co0"] + c0p <= v["cs0"], c["id"]
        assert not c["c1"] or (v["co1"] % 4 == 0 and v["cs1"] % 4 == 0 and v["co1"] + c1p <= v["cs1"]), c["id"]
        assert v["dst_co"] + max(c["cout"], c["zero_to"]) <= v["dst_cs"], c["id"]
        assert not c["res"] or v["res_co"] + c["cout"] <= v["res_cs"], c["id"]
        assert c["zero_to"] == 0 or c["zero_to"] > c["cout"], c["id"]


# what a family's kernels compute at all (launch_conv sends anything else elsewhere)
_ALL_FORMS = {"n3", "two_sources", "residual", "reflect_up", "elu", "zero_to"}
FORMS = {"igemm": _ALL_FORMS | {"sigmoid"}, "win3": _ALL_FORMS | {"sigmoid"}, "head": _ALL_FORMS | {"sigmoid"},
         "ring": _ALL_FORMS | {"sigmoid"}, "f16s": _ALL_FORMS, "f16s2": _ALL_FORMS, "taps": {"n3", "zero_to"}}
VIEW_FAMILIES = ("igemm", "win3", "head", "f16s", "f16s2", "ring", "taps")


def _forms(c):
    f = set()
    if c["N"] == 3: f.add("n3")
    if c["c1"]: f.add("two_sources")
    if c["res"]: f.add("residual")
    if c["pad_mode"] == 1 and c["up0"]: f.add("reflect_up")
    if c["act"] == V.ACTS["elu"]: f.add("elu")
    if c["act"] == V.ACTS["sigmoid"]: f.add("sigmoid")
    if c["zero_to"] > c["cout"]: f.add("zero_to")
    return f


def test_every_family_has_its_operand_forms_and_view_cases():
    for fam, want in FORMS.items():
        cases = [c for c in V.CASES if c["family"] == fam]
        have = set().union(*[_forms(c) for c in cases])
        assert want <= have, "%s lacks %s" % (fam, sorted(want - have))
    for fam in VIEW_FAMILIES:
        views = [c for c in V.CASES if c["family"] == fam and c["is_view"]]
        def unaligned(c):
            return c["view"]["dst_co"] % 2 == 1 or c["view"]["dst_cs"] % 4 != 0
        aligned = [c for c in views if not unaligned(c)]
        assert any(c["view"]["cs0"] > c["c0"] and c["view"]["co0"] in (4, 8) and c["view"]["dst_cs"] > c["cout"] and c["view"]["dst_co"] != 0
                   and (fam == "taps" or (c["c1"] and c["view"]["co1"] != 0 and c["res"] and c["view"]["res_co"] != 0))
                   for c in aligned), "%s: no aligned view case" % fam
        assert any(unaligned(c) for c in views), "%s: no unaligned destination" % fam
    # the aligned-only paths decline the unaligned destinations: the tags say so
    by_id = {c["id"]: c for c in V.CASES}
    assert set(by_id["taps_view_unaligned"]["tags"].values()) == {"f16g<4,1,2>"}
    assert set(by_id["taps_view"]["tags"].values()) == {"taps<4,2>"}
    assert by_id["ring_rag_view"]["tags"]["f16x3"] == "f16g<4,1,2,rag>" and by_id["ring_rag_view_unaligned"]["tags"]["f16x3"] == "f16g<4,1,2>"
    for a, b in (("taps_view", "taps_view_unaligned"), ("ring_rag_view", "ring_rag_view_unaligned")):  # the same layer, but for the view
        same = ("N", "h", "w", "c0", "c1", "cout", "kh", "kw", "stride", "pad", "pad_mode", "up0", "act", "res")
        assert all(by_id[a][k] == by_id[b][k] for k in same), (a, b)
