"""Per-output error bounds of the flow net's non-conv operators against float64, derived from each kernel's fp32 arithmetic
(df-vo_amd/csrc/ops.hip), not fitted to measurements.  u = 2^-24 (fp32 unit roundoff).  Every operand is the same fp32
value on both sides; the reference is the operator evaluated in float64 (tests/flow_world.py).

bilinear sample (warp, reg prep, consistency, resize, input)
    16 u M + dx Lx + dy Ly.  M = max |v| over the four corners: the corner weights come out of at most three roundings
    each (<= 3u, four of them: 12u M) and the weighted sum out of four (4u M).  dx, dy bound the error of the fp32 sample
    coordinate in pixels; Lx, Ly are the largest horizontal / vertical differences of neighbouring values in the 4 x 4
    neighbourhood of the cell (zero padding included), so that a coordinate error that crosses into the next cell is
    covered too.
warp coordinate
    ix = (lin_x[x] + f mult / s + 1) s, s = (W - 1) / 2: five roundings (product, quotient, two sums, product) of
    intermediates whose size in pixels is at most 2s + |f mult|: dx = 6u (s + |f mult|) (5u, rounded up for the
    second-order terms).
resize / input coordinate
    real = scale * o (align_corners) or 2 o + 0.5 (x2 down): dx = 2u (|real| + 1).  The general src_index (any size, either
    align_corners setting: resize_bound) has the same two roundings -- the fp32 scale and the product, or the fp32 scale and
    the rounding of the double scale (o + 0.5) - 0.5 to float -- so the same dx holds; past the last pixel the kernel
    clamps where bilinear_bound pads with zeros, which only enlarges M, Lx and Ly there.
consistency coordinate
    px = ((x + fx) / (W - 1) - 0.5) * 2, then (px + 1) (W - 1) / 2: five roundings of intermediates of at most
    |x + fx| + W pixels: dx = 6u (|x + fx| + W).
correlation
    c u sum|a b| / C with c = C/32 + 34: a term passes through at most C/32 fmaf roundings in its partial sum, 31 in the
    sum of the 32 partials, one in the division and one in the leaky ReLU (1-Lipschitz).
deconv (depthwise 4x4, stride 2)
    5 u sum|w x|: at most four taps per output, four roundings each, rounded up.
flow mean
    a sum of floats in double, rounded once: within one ulp of float32(mean64).
reg prep
    channel 0 = sqrt(s + 1e-6f), s = sum_c d_c^2, d_c = a_c - warp_c.  With e_c = bilinear bound + u (|d_c| + bilinear bound):
    ds = sum_c (2 |d_c| e_c + e_c^2) + 4u s + u 1e-6 + |1e-6f - 1e-6|, and |sqrt(s + ds) - sqrt(s)| <= ds / sqrt(s + 1e-6),
    i.e. up to 500 ds; plus 2u out (sqrtf within one ulp).  Channels 1, 2: one rounding of f - mean, u |f - mean|.
reg head
    v_c = -(d_c^2) and v_c - m are rounded in fp32 before expf, so each weight e_c = exp(v_c - m) carries a relative error
    rho_c = 1.01 u (|v_c| + |v_c - m|) + 4u (expf within two ulp); the error of m is a common factor that cancels.  The
    weighted mean y = (sum w_c e_c f_c + b) / sum e_c, accumulated in double, then moves by at most
    sum_c p_c rho_c |w_c f_c - y| (p_c = e_c / sum e), plus u |y| for the final rounding.
    k_reg_head (any k, any view) runs the operations of k_reg_head_v<k> in the same order -- fp32 -(d d), fmaxf, expf of the
    fp32 difference, the three sums in double, one rounding of the quotient -- so the same bound holds for it.
flow post
    resize: rw (17u M + dx Lx + dy Ly) + 2u |out| on the x10 flow (the x10 is one more rounding per corner, rw = float(W / w)
    and the product one each); consistency: sqrt(sum_c (e_c + u |d_c|)^2) + 3u diff, e_c the bilinear bound of -bwd."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def _gather(m, yi, xi):
    """m [N,C,Hm,Wm], yi / xi [N,Ho,Wo] long -> [N,C,Ho,Wo]"""
    n, c, hm, wm = m.shape
    idx = (yi * wm + xi).view(n, 1, -1).expand(n, c, -1)
    return torch.gather(m.reshape(n, c, -1), 2, idx).view(n, c, *yi.shape[1:])


def bilinear_bound(src, ix, iy, dx, dy, c_round=16.0):
    """per-output bound of a zero-padded bilinear sample of src [N,C,H,W] (float64) at pixel coordinates ix, iy [N,Ho,Wo]
    with coordinate errors dx, dy: c_round u M + dx Lx + dy Ly (module docstring)"""
    n, c, h, w = src.shape
    sp = F.pad(src, (3, 3, 3, 3))
    ddx = (sp[..., 1:] - sp[..., :-1]).abs()
    ddy = (sp[..., 1:, :] - sp[..., :-1, :]).abs()
    mx = F.max_pool2d(ddx, (4, 3), 1)
    my = F.max_pool2d(ddy, (3, 4), 1)
    m4 = F.max_pool2d(sp.abs(), 2, 1)
    x0 = torch.floor(ix).clamp(-2, w).long()
    y0 = torch.floor(iy).clamp(-2, h).long()
    lx, ly = _gather(mx, y0 + 2, x0 + 2), _gather(my, y0 + 2, x0 + 2)
    mm = _gather(m4, y0 + 3, x0 + 3)
    return c_round * U * mm + dx.unsqueeze(1) * lx + dy.unsqueeze(1) * ly


def lin(n):
    """the fp32 torch.linspace(-1, 1, n) grid the net uploads, widened"""
    return torch.linspace(-1.0, 1.0, n).double()


def warp_coords(flow, mult):
    """(ix, iy, dx, dy) of launch_warp / reg prep: flow [N,2,H,W] float64 (fp32 values)"""
    n, _, h, w = flow.shape
    sx, sy = (w - 1) / 2.0, (h - 1) / 2.0
    fx, fy = flow[:, 0] * mult, flow[:, 1] * mult
    ix = (lin(w).view(1, 1, w) + fx / sx + 1.0) * sx
    iy = (lin(h).view(1, h, 1) + fy / sy + 1.0) * sy
    return ix, iy, 6 * U * (sx + fx.abs()), 6 * U * (sy + fy.abs())


def warp_bound(src, flow, mult, swap):
    s = src.flip(0) if swap else src
    ix, iy, dx, dy = warp_coords(flow, mult)
    return 1.01 * bilinear_bound(s, ix, iy, dx, dy)


def resize_half_bound(src):
    """launch_resize_bilinear x2 down (align_corners=False): real = 2 o + 0.5"""
    n, c, h, w = src.shape
    ho, wo = h // 2, w // 2
    ix = (2.0 * torch.arange(wo, dtype=torch.float64) + 0.5).view(1, 1, wo).expand(n, ho, wo)
    iy = (2.0 * torch.arange(ho, dtype=torch.float64) + 0.5).view(1, ho, 1).expand(n, ho, wo)
    return 1.01 * bilinear_bound(src, ix, iy, 2 * U * (ix + 1), 2 * U * (iy + 1))


def resize_bound(src, ho, wo, align_corners):
    """launch_resize_bilinear of src [N,C,H,W] to ho x wo with the general src_index: dx = 2u (|real| + 1)"""
    n, c, h, w = src.shape

    def real(n_out, n_in):
        o = torch.arange(n_out, dtype=torch.float64)
        if align_corners:
            return o * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        return ((n_in / n_out) * (o + 0.5) - 0.5).clamp(min=0.0)
    ix = real(wo, w).view(1, 1, wo).expand(n, ho, wo)
    iy = real(ho, h).view(1, ho, 1).expand(n, ho, wo)
    return 1.01 * bilinear_bound(src, ix, iy, 2 * U * (ix + 1), 2 * U * (iy + 1))


def aligned_coords(n, h, w, H, W):
    """sample coordinates of an align_corners=True resize of an h x w map to H x W, and their errors"""
    ix = (torch.arange(W, dtype=torch.float64) * ((w - 1) / (W - 1))).view(1, 1, W).expand(n, H, W)
    iy = (torch.arange(H, dtype=torch.float64) * ((h - 1) / (H - 1))).view(1, H, 1).expand(n, H, W)
    return ix, iy, 2 * U * (ix + 1), 2 * U * (iy + 1)


def input_bound(img):
    """launch_img_u8_to_flow_input: img [1,3,h,w] = float32(u8 / 255) widened, to the net size (th, tw)"""
    return lambda th, tw: 1.01 * bilinear_bound(img, *aligned_coords(1, img.shape[2], img.shape[3], th, tw))


def corr_bound(f1, f2, stride, swap2, corr_fn):
    c = f1.shape[1]
    return (c / 32 + 34) * U * corr_fn(f1.abs(), (f2.flip(0) if swap2 else f2).abs(), stride)


def deconv_bound(x, w):
    return 5 * U * F.conv_transpose2d(x.abs(), w.abs(), None, stride=2, padding=1, groups=x.shape[1])


def mean_ulp(mean64):
    m32 = mean64.float()
    return (torch.nextafter(m32.abs(), torch.tensor(np.inf, dtype=torch.float32)) - m32.abs()).double()


def reg_prep_bound(img, flow, mean, mult, ref):
    """img [N,3,H,W], flow [N,2,H,W], mean [N,2,1,1]; ref = reg_prep_ref's float64 output [N,3,H,W]"""
    wb = warp_bound(img, flow, mult, swap=1)
    from oracle import nets_torch as O
    d = img - O.backward_warp(img.flip(0), flow * mult)
    e = wb + U * (d.abs() + wb)
    s = d.pow(2).sum(1, True)
    ds = (2 * d.abs() * e + e * e).sum(1, True) + 4 * U * s + U * 1e-6 + abs(float(np.float32(1e-6)) - 1e-6)
    b0 = 1.01 * ds / (s + 1e-6).sqrt() + 2 * U * ref[:, 0:1]
    b12 = 1.01 * U * (flow - mean).abs()
    return torch.cat([b0, b12], 1)


def reg_head_bound(dist, flow, wx, bx, wy, by, k, ref):
    """dist [N,k*k,H,W], flow [N,2,H,W], wx / wy [1,k*k,1,1] weights, ref = reg_head_ref's output [N,2,H,W]"""
    r = (k - 1) // 2
    v = -dist.pow(2)
    m = v.max(1, True)[0]
    p = (v - m).exp()
    p = p / p.sum(1, True)
    rho = 1.01 * U * (v.abs() + (v - m).abs()) + 4 * U
    out = []
    for ch, (w, b) in enumerate(((wx, bx), (wy, by))):
        uf = F.unfold(flow[:, ch:ch + 1], k, stride=1, padding=r).view_as(dist)
        wu = w.view(1, -1, 1, 1) * uf
        y = ref[:, ch:ch + 1]
        out.append(1.01 * (p * rho * (wu - y).abs()).sum(1, True) + U * y.abs()
                   + 2.0 ** -40 * ((p * wu.abs()).sum(1, True) + abs(float(b))))
    return torch.cat(out, 1)


def post_resize_bound(flow, scale, H, W):
    """launch_flow_post's k_flow_resize on flow [2,2,h,w]: (fwd bound, bwd bound) [1,2,H,W] each"""
    n, _, h, w = flow.shape
    rh, rw = H / h, W / w
    ix, iy, dx, dy = aligned_coords(n, h, w, H, W)
    b = bilinear_bound(flow * scale, ix, iy, dx, dy, c_round=17.0)
    from oracle import nets_torch as O
    out = O.resize_dense_flow(flow * scale, H, W)
    b = 1.01 * b * torch.tensor([rw, rh], dtype=torch.float64).view(1, 2, 1, 1) + 2 * U * out.abs()
    return b[0:1], b[1:2]


def consistency_bound(fwd, bwd, ref):
    """k_flow_consistency on the fp32 fwd / bwd [1,2,H,W]; ref its float64 value [1,H,W,1]"""
    _, _, H, W = fwd.shape
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    px, py = x + fwd[:, 0], y + fwd[:, 1]
    e = bilinear_bound(-bwd, px, py, 6 * U * (px.abs() + W), 6 * U * (py.abs() + H))
    from oracle import nets_torch as O
    warped = F.grid_sample(-bwd, O.flow_to_pix(fwd), mode="bilinear", padding_mode="zeros", align_corners=True)
    d = (fwd - warped).abs()
    diff = ref.permute(0, 3, 1, 2)
    return 1.01 * (e + U * d).pow(2).sum(1, True).sqrt() + 3 * U * diff
