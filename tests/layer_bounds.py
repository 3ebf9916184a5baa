"""Per-output error bounds of one convolution against float64, shared by the per-layer tests of both nets
(tests/test_depth_layers_gpu.py, tests/test_flow_layers_gpu.py).

With sabs = sum |w x| + |bias| + |residual| per output (the float64 convolution of the magnitudes):
    fp32    2^-20 sabs
    f16x3   (2^-22 + 2^-20) sabs + 2^-36 (sum|w| [some |x| < 2^-14] + sum|x| [some |w| < 2^-14])
    f16     2^-20 sabs against the f16-ROUNDED operands
A layer that the device runs in exact fp32 under every packing (the one- and two-channel head kernel) takes the fp32 bound
in every mode.  ReLU, leaky ReLU, ELU and the sigmoid are 1-Lipschitz, so the bound carries through the epilogue."""
import torch


def conv_bound(conv, xin, w64, b64, res64, precision, exact_fp32=False):
    """(reference operands x, w, the float64 pre-activation y, per-output bound): `conv(x, w, b)` is the layer's float64
    convolution; xin / w64 / b64 / res64 are the fp32 operands widened (res64 None or a tensor)"""
    if precision == "f16" and not exact_fp32:
        xin, w64 = xin.half().double(), w64.half().double()
    r64 = res64 if res64 is not None else 0.0
    y = conv(xin, w64, b64) + r64
    sabs = conv(xin.abs(), w64.abs(), None) + b64.abs().view(1, -1, 1, 1) + (res64.abs() if res64 is not None else 0.0)
    bound = 2.0 ** -20 * sabs
    if precision == "f16x3" and not exact_fp32:
        bound = bound + 2.0 ** -22 * sabs
        if float(xin.abs().min()) < 2.0 ** -14:
            bound = bound + 2.0 ** -36 * conv(torch.ones_like(xin), w64.abs(), None)
        if float(w64.abs().min()) < 2.0 ** -14:
            bound = bound + 2.0 ** -36 * conv(xin.abs(), torch.ones_like(w64), None)
    return xin, w64, y, bound
