"""GPU: the pose net's own convolution shapes through dfvo_conv2d against float64, with the method and the per-packing bounds
of tests/test_conv_variants_gpu.py (banded operands, sentinel destination, tests/layer_bounds.py): the 7x7 / stride-2 stem over
SIX input channels -- two 4-channel groups, the second with two zero pad channels -- at 37 x 53 and 64 x 96, and PoseDecoder's
1x1 512 -> 256, 3x3 256 -> 256 and 1x1 256 -> 12 layers on the 2 x 3 and 3 x 5 maps of the 64 x 96 and 96 x 160 feeds."""
import pytest
import torch

import conv_variants as V
import test_conv_variants_gpu as TV

pytestmark = pytest.mark.gpu

_ANY = {p: "posenet<0>" for p in V.PRECISIONS}  # (no variant tag is asserted here: the dispatcher's choice is not this test's)
CASES = [
    V._case("pose_stem_37x53", _ANY, 1, 37, 53, 6, 64, k=(7, 7), stride=2, pad=(3, 3), act="relu"),
    V._case("pose_stem_64x96", _ANY, 1, 64, 96, 6, 64, k=(7, 7), stride=2, pad=(3, 3), act="relu"),
    V._case("pose_squeeze_2x3", _ANY, 1, 2, 3, 512, 256, k=(1, 1), act="relu"),
    V._case("pose_squeeze_3x5", _ANY, 1, 3, 5, 512, 256, k=(1, 1), act="relu"),
    V._case("pose_3x3_2x3", _ANY, 1, 2, 3, 256, 256, act="relu"),
    V._case("pose_3x3_3x5", _ANY, 1, 3, 5, 256, 256, act="relu"),
    V._case("pose_out_2x3", _ANY, 1, 2, 3, 256, 12, k=(1, 1)),
    V._case("pose_out_3x5", _ANY, 1, 3, 5, 256, 12, k=(1, 1)),
]


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_pose_net_layer(gpu, conv_precision, monkeypatch, tmp_path, cid):
    case = next(c for c in CASES if c["id"] == cid)
    csv = tmp_path / "conv_profile.csv"
    monkeypatch.setenv("DFVO_CONV_PROFILE_CSV", str(csv))
    tags, n_ovf, front, back, out = TV._run(gpu, case, conv_precision, csv)
    assert len(tags) == 1 and n_ovf == 0, (tags, n_ovf)
    cout = case["cout"]
    assert bool((front == TV.SENTINEL).all()) and bool((back == TV.SENTINEL).all()), "wrote outside the destination buffer"
    assert bool((out[..., cout:] == TV.SENTINEL).all()), "wrote outside the layer's channels"
    got = out[..., :cout].permute(0, 3, 1, 2)
    assert bool(torch.isfinite(got).all()) and not bool((got == TV.SENTINEL).any())
    ref, bound = TV._reference(case, conv_precision)
    err = (got.double() - ref).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    print("   %-18s %-5s %-28s max|ref| %.2e  max err %.2e  worst err / bound %.3f"
          % (cid, conv_precision, tags[0], float(ref.abs().max()), float(err.max()), ratio))
    assert bool((err <= bound).all()), "%s %s %s: worst err / bound %.3f" % (cid, conv_precision, tags[0], ratio)
