"""CPU: the case lists of tests/resample_cases.py are sharp.  Every deliberately wrong variant of a resampler (a "mutant":
another index formula, swapped sizes, a dropped factor ...) changes the result on at least one case -- bit-wise for the
depth post-processing and the frame tail, beyond the tests/flow_bounds.py bound in at least one output element for the
flow operators -- so that a kernel computing the mutant fails tests/test_resamplers_gpu.py.  The unmutated restatements
equal the oracle's references, which are what the device is compared with."""
import numpy as np
import pytest
import torch

import resample_cases as RC
from oracle import nets_torch as O


def _depth_differs(a, b):
    (raw_a, proc_a), (raw_b, proc_b) = a, b
    return not (np.array_equal(raw_a.view(np.uint32), raw_b.view(np.uint32)) and np.array_equal(proc_a, proc_b))


def test_depth_restatement_equals_the_oracle():
    """depth_post_variant without a mutant is cv2_shim.resize(INTER_NEAREST) + preprocess_depth on every case"""
    n = 0
    for tag, d, H, W, crop, rng in list(RC.depth_cases()) + list(RC.range_cases()):
        want, got = RC.depth_post_ref(d, H, W, crop, rng), RC.depth_post_variant(d, H, W, crop, rng)
        assert got[0].dtype == want[0].dtype == np.float32 and got[1].dtype == want[1].dtype == np.float64, tag
        assert not _depth_differs(got, want), tag
        n += 1
    assert n == len(RC.DEPTH_SIZES) * len(RC.CROPS) + len(RC.RANGES)


def test_depth_cases_cover_what_they_claim():
    for (h, w), (H, W) in RC.DEPTH_SIZES:
        boxes = {name: RC.crop_box(RC.crop_fractions(name, H, W), H, W) for name in RC.CROPS}
        assert boxes["full"] == (0, H, 0, W)
        y0, y1, x0, x1 = boxes["empty"]
        assert y0 == y1 and x1 > x0
        y0, y1, x0, x1 = boxes["one_pixel"]
        assert (y1 - y0, x1 - x0) == (1, 1) and y1 <= H and x1 <= W
    assert sum(1 for (_, _), (H, W) in RC.DEPTH_SIZES if (H * W) % 256) >= 8  # the last block is a partial one
    # the range input holds both ends of the range, as the float the C entry receives, and their neighbours
    d = RC.range_input((0.1, 50.0))
    lo = np.float32(0.1)
    assert float(lo) > 0.1 and lo in d and np.nextafter(lo, np.float32(1)) in d and np.nextafter(lo, np.float32(0)) in d
    assert np.float32(50) in d and np.signbit(d[d == 0]).tolist() == [False, True]
    # what the reference does with non-finite depth (the device deliberately answers 0.0: tests/test_resamplers_gpu.py)
    (_, _), (H, W) = RC.RANGE_SIZE
    raw, proc = RC.depth_post_ref(RC.nonfinite_input(), H, W, RC.crop_fractions("full", H, W), RC.DEPTH_RANGE)
    assert np.isnan(proc[~np.isfinite(raw)]).all() and (~np.isfinite(raw)).sum() >= 2


@pytest.mark.parametrize("mutant", RC.DEPTH_MUTANTS)
def test_depth_mutants_are_caught(mutant):
    cases = list(RC.depth_cases()) + list(RC.range_cases())
    caught = [tag for tag, d, H, W, crop, rng in cases
              if _depth_differs(RC.depth_post_variant(d, H, W, crop, rng, mutant), RC.depth_post_ref(d, H, W, crop, rng))]
    sizes = sorted({t.split(" ")[0] for t in caught if not t.startswith("range")})
    print("   %-28s caught by %d of %d cases, %d of %d sizes: %s" % (mutant, len(caught), len(cases), len(sizes),
                                                                    len(RC.DEPTH_SIZES), " ".join(sizes)))
    assert caught, mutant
    if mutant in RC.DEPTH_INDEX_MUTANTS:
        assert len(sizes) >= 3, (mutant, sizes)


def test_tail_cases_cover_what_they_claim():
    tags = [c[0] for c in RC.TAIL_CASES]
    assert len(set(tags)) == len(tags)
    for tag, img, (y0, y1, x0, x1), oh, ow, bgr in RC.tail_cases():
        ih, iw = img.shape[:2]
        assert 0 <= y0 < y1 <= ih and 0 <= x0 < x1 <= iw, tag
        want = RC.tail_ref(img, (y0, y1, x0, x1), oh, ow, bgr)
        assert want.shape == (oh, ow, 3) and want.max() < 64, tag  # nothing outside the window took part
        if "2x2 area" in tag:
            assert (y1 - y0, x1 - x0) == (2 * oh, 2 * ow) and iw > x1 - x0, tag
    (ih, iw), crop, _, _ = RC.TAIL_FRACTION_CASE
    assert RC.crop_box(crop, ih, iw) == (11, 37, 21, 53)


@pytest.mark.parametrize("mutant", RC.TAIL_MUTANTS)
def test_tail_mutants_are_caught(mutant):
    caught = [tag for tag, img, box, oh, ow, bgr in RC.tail_cases()
              if not np.array_equal(RC.tail_ref(img, box, oh, ow, bgr, mutant), RC.tail_ref(img, box, oh, ow, bgr))]
    print("   %-28s caught by: %s" % (mutant, "; ".join(caught)))
    assert caught, mutant


def test_flow_cases_are_the_net_sizes_and_down_sample():
    for (h, w), (th, tw) in RC.FLOW_INPUT_CASES:
        assert O.get_target_size(h, w) == (th, tw) and th < h and tw < w
    for (h, w), (H, W), _ in RC.FLOW_POST_CASES:
        assert float(H / h) != float(W / w) and (H * W) % 256
    assert RC.FLOW_POST_SCALE == 10.0


def _exceeds(got, ref, bound):
    return bool(((got - ref).abs() > bound).any())


@pytest.mark.parametrize("mutant", RC.FLOW_MUTANTS)
def test_flow_mutants_are_caught(mutant):
    caught = []
    if mutant == "align_corners=False":
        for tag, u8, th, tw in RC.flow_input_cases():
            ref, bound = RC.flow_input_ref(u8, th, tw)
            if _exceeds(RC.flow_input_ref(u8, th, tw, mutant)[0], ref, bound):
                caught.append("input " + tag)
    for tag, flow, H, W in RC.flow_post_cases():
        (rf, rb), (bf, bb) = RC.flow_post_resize_ref(flow, H, W)
        if mutant == "bwd not negated":
            rc, bc = RC.flow_consistency_ref(rf.float(), rb.float())
            if _exceeds(RC.flow_consistency_ref(rf.float(), rb.float(), mutant)[0], rc, bc):
                caught.append("consistency " + tag)
        else:
            (mf, mb), _ = RC.flow_post_resize_ref(flow, H, W, mutant)
            if _exceeds(mf, rf, bf) or _exceeds(mb, rb, bb):
                caught.append("post " + tag)
    print("   %-22s caught by: %s" % (mutant, "; ".join(caught)))
    assert caught, mutant
    if mutant == "align_corners=False":
        assert any(c.startswith("input") for c in caught) and any(c.startswith("post") for c in caught)


def test_flow_references_pass_their_own_bounds_in_float32():
    """the bounds admit a plain fp32 evaluation of the same operators (they are not so tight that only float64 passes)"""
    for tag, u8, th, tw in RC.flow_input_cases():
        ref, bound = RC.flow_input_ref(u8, th, tw)
        x = torch.from_numpy(np.transpose(u8 / 255, (2, 0, 1))).unsqueeze(0).float()
        got = torch.nn.functional.interpolate(x, (th, tw), mode="bilinear", align_corners=True)
        assert not _exceeds(got.double(), ref, bound), tag
