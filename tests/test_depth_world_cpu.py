"""The calibrated depth world (tests/depth_world.py) and the power of the depth net's float64-anchor gate, on the CPU.

test_nets_gpu.py::test_depthnet_distance_to_the_exact_function gates the device's per-pixel relative depth error against
the net evaluated in float64.  Here the same gate is applied to the torch-CPU oracle with one plausible device bug
injected at a time: every such bug must land at least 10x outside the gate, and the unmutated oracle must pass it."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import depth_world as W
from oracle import nets_torch as O
from synth import image_pair

H, W_ = 192, 640
SIZES = [(64, 96), (192, 640), (320, 1024)]


def _frame(h, w):
    return image_pair(h, w, seed=55)[0]


@pytest.fixture(scope="module")
def world():
    sd = W.calibrated_monodepth2_state_dict(4869, H, W_)
    img = _frame(H, W_)
    d64 = O.depth_inference(sd, img, dtype=torch.float64)
    o32 = W.rel_err_stats(O.depth_inference(sd, img), d64)
    return sd, img, d64, o32


def test_calibrated_world_is_deterministic():
    a = W._calibrated.__wrapped__(4869, 64, 96)
    b = W.calibrated_monodepth2_state_dict(4869, 64, 96)
    assert set(a) == set(b) == set(O.monodepth2_state_dict(4869))
    for k in a:
        assert a[k].dtype == torch.float32 and torch.equal(a[k], b[k]), k


def test_layer_walk_equals_the_oracle(world):
    """depth_world.activations (the inventory's layer list) computes the oracle's scale-0 disparity"""
    sd, img, d64, _ = world
    disp = W.activations(sd, img)["disp"][0, 0].numpy()
    np.testing.assert_allclose(disp, W.disparity(d64), rtol=0, atol=1e-12)


def test_folded_scales_span_three_decades_with_the_edge_channels(world):
    sd = world[0]
    scales = {L["bn"]: W.fold(sd, L["bn"])[0] for L in W.DEPTH_LAYERS if L["bn"]}
    s = np.abs(np.concatenate(list(scales.values())))
    print("folded scales: %.2e .. %.2e" % (s.min(), s.max()))
    assert s.max() / s.min() >= 1e3
    conv, bn, ch = W.DEAD
    assert float(sd[conv + ".weight"][ch].abs().max()) == 0
    assert float(sd[bn + ".running_var"][ch]) == 0 and float(sd[bn + ".running_mean"][ch]) == 0
    assert np.isclose(scales[bn][ch], float(sd[bn + ".weight"][ch]) / np.sqrt(1e-5), rtol=1e-6, atol=0)
    bn, ch, gamma = W.NEAR_DEAD
    L = next(L for L in W.DEPTH_LAYERS if L["bn"] == bn)
    wf = W.folded_params(sd, L)[0][ch].abs()
    assert float(sd[bn + ".weight"][ch]) == np.float32(gamma)
    assert 0 < float(wf.max()) < 2.0 ** -14, "near-dead channel's folded weights are not f16-subnormal: %.3e" % float(wf.max())


@pytest.mark.parametrize("h,w", SIZES)
def test_calibrated_world_is_unsaturated(h, w):
    sd = W.calibrated_monodepth2_state_dict(4869, h, w)
    d64 = O.depth_inference(sd, _frame(h, w), dtype=torch.float64)
    frac = W.unsaturated_fraction(W.disparity(d64))
    print("%dx%d: %.4f of the disparities in [0.02, 0.98]" % (h, w, frac))
    assert frac >= 0.9


# ---- mutations: what a device bug would do to the depth -----------------------------------------------------------------
def _bn_param(sd, bn, key, fn):
    sd = dict(sd)
    sd[bn + key] = fn(sd[bn + key].clone())
    return sd


def _drop_mean(sd):
    return _bn_param(sd, "encoder.layer2.0.bn1", ".running_mean", torch.zeros_like)


def _eps_1e3(sd):
    """bn_fold with eps 1e-3: every running_var seen 1e-3 - 1e-5 larger"""
    sd = dict(sd)
    for L in W.DEPTH_LAYERS:
        if L["bn"]:
            sd[L["bn"] + ".running_var"] = sd[L["bn"] + ".running_var"] + (1e-3 - 1e-5)
    return sd


def _scale_one_channel(sd, bn="encoder.layer3.1.bn2", ch=3):
    """the packer multiplies one channel's weights by 1.01 x its fold scale (the shift stays right)"""
    scale, _ = W.fold(sd, bn)
    sd = _bn_param(sd, bn, ".weight", lambda g: torch.cat([g[:ch], g[ch:ch + 1] * 1.01, g[ch + 1:]]))
    return _bn_param(sd, bn, ".bias", lambda b: b + torch.eye(len(b))[ch] * 0.01 * float(scale[ch]) *
                     float(sd[bn + ".running_mean"][ch]))


def _drop_shift(sd, bn="encoder.layer1.1.bn1"):
    """the layer's epilogue adds no shift: beta' = mean x scale makes the batch norm a pure scale"""
    scale, _ = W.fold(sd, bn)
    return _bn_param(sd, bn, ".bias", lambda b: sd[bn + ".running_mean"] * torch.from_numpy(scale))


def _f16_weights(sd, name="decoder.9.conv.conv"):
    """one f16x3 decoder layer that lost its lo plane"""
    sd = dict(sd)
    sd[name + ".weight"] = sd[name + ".weight"].half().float()
    return sd


@contextlib.contextmanager
def _head_zero_padded():
    orig = O._conv3x3_refl

    def conv(sd, name, x):
        if name == "decoder.10.conv":
            return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=1)
        return orig(sd, name, x)

    O._conv3x3_refl = conv
    try:
        yield
    finally:
        O._conv3x3_refl = orig


MUTATIONS = {"running_mean_ignored_in_one_bn": _drop_mean, "bn_eps_1e-3": _eps_1e3,
             "one_channel_fold_scale_x1.01": _scale_one_channel, "shift_dropped_in_one_layer": _drop_shift,
             "decoder.9_f16_rounded_weights": _f16_weights, "head_zero_padded": None}


def test_unmutated_oracle_passes_the_anchor_gate(world):
    sd, img, d64, o32 = world
    again = W.rel_err_stats(O.depth_inference(sd, img), d64)
    gate = W.anchor_gate(o32)
    print("oracle fp32 vs float64: max %.2e p99 %.2e median %.2e | gate %.2e %.2e %.2e" % (o32 + gate))
    assert all(a <= g for a, g in zip(again, gate))


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_anchor_gate_catches_the_mutation(world, mutation):
    sd, img, d64, o32 = world
    if MUTATIONS[mutation] is None:
        with _head_zero_padded():
            got = O.depth_inference(sd, img)
    else:
        got = O.depth_inference(MUTATIONS[mutation](sd), img)
    gate = W.anchor_gate(o32)
    m = W.rel_err_stats(got, d64)
    ratios = tuple(a / g for a, g in zip(m, gate))
    print("MUTATION %-32s rel err max %.2e p99 %.2e median %.2e | / gate: %.0fx %.0fx %.0fx" % ((mutation,) + m + ratios))
    assert max(ratios) >= 10, (mutation, m, gate)
