"""Winograd F(2x2,3x3) in fp32 on the CPU, and its per-output error bound against float64 -- shared by tests/test_wino_cpu.py
and tests/test_wino_gpu.py (the device kernel: df-vo_amd/csrc/conv_wino_f32.hip).

The bound is the Winograd analogue of layer_bounds.conv_bound's fp32 row, the same constant on the magnitudes of the products
the algorithm really forms:
    bound = 2^-20 (wabs + |bias| + |residual|),   wabs = |A^T| [ sum_c (|G| |g| |G^T|) o (|B^T| |d| |B|) ] |A|   (float64)
Where the constant's room comes from: U is rounded once (2^-24), V carries at most 3 roundings of sums of 4 inputs, the
channel sum is an fp32 fmaf chain (the fp32 row's own term), Y adds 9 products with at most 8 roundings -- each relative
to partial sums that |.|-arithmetic dominates; emulated in fp32 on four shapes (cin 32 .. 386) the error stayed below
0.25 * 2^-24 wabs, so the gate has 64x room while a wrong coefficient or tile is O(1) wabs.
ReLU, leaky ReLU and ELU (a <= 1) are 1-Lipschitz, so the bound carries through the epilogue."""
import numpy as np
import torch
import torch.nn.functional as F

G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
BT = torch.tensor([[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 1.0, 0.0], [0.0, -1.0, 1.0, 0.0], [0.0, 1.0, 0.0, -1.0]], dtype=torch.float64)
AT = torch.tensor([[1.0, 1.0, 1.0, 0.0], [0.0, 1.0, -1.0, -1.0]], dtype=torch.float64)


def filter_transform(w64, g=G):
    """U = G g G^T per filter, in the operation order of conv_pack_wino_f32.h: [cout, cin, 4, 4] float64"""
    assert w64.dtype == torch.float64 and w64.shape[-2:] == (3, 3)
    if g is not G:  # magnitudes: a plain product
        return g @ w64 @ g.T
    def rows(a, b, c):
        return torch.stack([a, 0.5 * ((a + b) + c), 0.5 * ((a - b) + c), c], dim=-1)
    t = rows(w64[..., 0, :], w64[..., 1, :], w64[..., 2, :])            # [.., 3 (j), 4 (i)]
    u = rows(t[..., 0, :], t[..., 1, :], t[..., 2, :])                  # [.., 4 (i), 4 (j)]
    return u


def _windows(x):
    """NCHW -> the 4x4 input windows of the 2x2 output tiles, zero outside the map: [N, C, Th, Tw, 4, 4]"""
    n, c, h, w = x.shape
    th, tw = (h + 1) // 2, (w + 1) // 2
    xp = F.pad(x, (1, 2 * tw - w + 1, 1, 2 * th - h + 1))
    return xp.unfold(2, 4, 2).unfold(3, 4, 2)


def _winograd(x, u, bt, at):
    """sum_c U o (bt d bt^T), then at M at^T, in the dtype of x: [N, cout, H, W]"""
    n, c, h, w = x.shape
    d = _windows(x)
    th, tw = d.shape[2], d.shape[3]
    bt, at = bt.to(x.dtype), at.to(x.dtype)
    v = bt @ d @ bt.T                                                   # entries 0 / +-1: sums of two inputs, one rounding each
    v16 = v.permute(4, 5, 1, 0, 2, 3).reshape(16, c, n * th * tw)
    u16 = u.to(x.dtype).permute(2, 3, 0, 1).reshape(16, u.shape[0], c)
    m = torch.bmm(u16, v16).reshape(4, 4, u.shape[0], n, th, tw).permute(3, 2, 4, 5, 0, 1)
    y = at @ m @ at.T                                                   # [N, cout, Th, Tw, 2, 2]
    y = y.permute(0, 1, 2, 4, 3, 5).reshape(n, u.shape[0], 2 * th, 2 * tw)
    return y[:, :, :h, :w]


def wino_conv_f32(x, w, b=None):
    """the algorithm as the device runs it, in torch fp32: U from float64 rounded once, V, the channel sum and Y in fp32"""
    assert x.dtype == torch.float32 and w.dtype == torch.float32
    u = filter_transform(w.double()).float()
    y = _winograd(x, u, BT, AT)
    return y if b is None else y + b.view(1, -1, 1, 1)


def wino_bound(x, w, b=None, res=None):
    """(float64 pre-activation of the 3x3 / pad 1 convolution of the fp32 operands, per-output bound)"""
    x64, w64 = x.double(), w.double()
    y = F.conv2d(x64, w64, None, padding=1)
    wabs = _winograd(x64.abs(), filter_transform(w64.abs(), G.abs()), BT.abs(), AT.abs())
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1)
        wabs = wabs + b.double().abs().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
        wabs = wabs + res.double().abs()
    return y, 2.0 ** -20 * wabs


def act64(y, act, a):
    return {0: lambda t: t, 1: lambda t: F.leaky_relu(t, a), 2: F.relu, 3: lambda t: F.elu(t, a)}[act](y)


# The operator cases of the issue: name, N, H, W, c0, c1, cout, act, act_param, scale of the inputs, views.
# views: cs0, co0, cs1, dst_cs, dst_co, dst_zero_to, res (None | (res_cs, res_co))
CASES = [
    dict(name="a_leaky_2x13x37", N=2, H=13, W=37, c0=32, c1=0, cout=32, act=1, a=0.1),
    dict(name="b_views_1x16x64", N=1, H=16, W=64, c0=128, c1=2, cout=128, act=0, a=0.0, cs0=132, co0=4, cs1=4, dst_cs=136, dst_co=8),
    dict(name="c_res_view_2x6x10", N=2, H=6, W=10, c0=386, c1=0, cout=128, act=0, a=0.0, res=(132, 4)),
    dict(name="d_elu_1x9x9", N=1, H=9, W=9, c0=20, c1=0, cout=48, act=3, a=1.0),
    dict(name="e_zero_to_1x8x12", N=1, H=8, W=12, c0=12, c1=0, cout=9, act=0, a=0.0, dst_cs=12, dst_zero_to=12),
    dict(name="f_1x1x5", N=1, H=1, W=5, c0=16, c1=0, cout=16, act=1, a=0.1),
    dict(name="f_1x2x2", N=1, H=2, W=2, c0=16, c1=0, cout=16, act=1, a=0.1),
    dict(name="g_scaled_1e5", N=2, H=13, W=37, c0=32, c1=0, cout=32, act=1, a=0.1, scale=1e5),
]


def case_tensors(c):
    """seeded operands of a case: x (both sources concatenated), w, b, res (or None)"""
    g = torch.Generator().manual_seed(sum(map(ord, c["name"])))
    cin = c["c0"] + c["c1"]
    x = torch.randn(c["N"], cin, c["H"], c["W"], generator=g) * c.get("scale", 1.0)
    w = torch.randn(c["cout"], cin, 3, 3, generator=g) / np.sqrt(cin * 9)
    b = torch.randn(c["cout"], generator=g) * 0.1
    res = torch.randn(c["N"], c["cout"], c["H"], c["W"], generator=g) if c.get("res") else None
    return x, w, b, res
