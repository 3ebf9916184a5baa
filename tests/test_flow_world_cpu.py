"""The flow net's float64 walk (tests/flow_world.py) and the power of the non-conv bounds (tests/flow_bounds.py), on the CPU.

The walk must compute the oracle's float64 flow; the random world must keep the conditioning the per-operator bounds were
judged in; and each bound, applied to a float32 CPU restatement of its operator on the operator's real input, must pass
the unmutated restatement and put a plausible device bug at least 10x outside at its worst output."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_bounds as B
import flow_world as FW
from oracle import nets_torch as O


@pytest.fixture(scope="module")
def random_world():
    sd, ref, cur = FW.world("random")
    return sd, FW.walk64("random")


@pytest.mark.parametrize("world", FW.WORLDS)
def test_float64_walk_equals_the_oracle(world):
    """random world: bit for bit.  Tunnel world: torch's float64 feature convolutions at batch 1 (the net's per-frame
    launches) and at batch 2 (the oracle) add in different orders at 256x640, so the level flows agree to 1e-12 relative
    there; fwd / bwd / diff still agree bit for bit"""
    sd, ref, cur = FW.world(world)
    acts = FW.walk64(world)
    O._grid_cache.clear()
    fwd, bwd, diff, raw = O.flow_inference(sd, ref, cur, return_levels=True, dtype=torch.float64)
    O._grid_cache.clear()
    for l in range(2, 7):
        got, want = acts["L%d.flow" % l], raw[l]
        if world == "random":
            assert torch.equal(got, want), l
        else:
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), l
    assert np.array_equal(acts["fwd"][0].numpy(), fwd)
    assert np.array_equal(acts["bwd"][0].numpy(), bwd)
    assert np.array_equal(acts["diff"][0].numpy(), diff)


def test_inventory_lists_every_launch():
    ops = [L["op"] for L in FW.FLOW_LAYERS]
    assert ops.count("conv") == 2 * 10 + sum(4 + 4 + 6 + (2 if l < 5 else 1) + (1 if l < 5 else 0) + (2 if l == 2 else 0)
                                             for l in range(2, 7))
    assert ops.count("warp") == 9 and ops.count("corr") == 5 and ops.count("deconv") == 6
    assert ops.count("mean") == ops.count("reg_prep") == ops.count("reg_head") == 5
    assert ops.count("resize") == 10 and ops.count("input") == 2 and ops.count("post") == 1


def test_random_world_conditioning(random_world):
    """per level: the flow entering regularisation (measured max 6.2-14.6, median 3.0-9.5 px), the softmax max-probability
    (median <= 0.6, at most 1 % above 0.99) and |dist| (not saturated)"""
    sd, acts = random_world
    for l in range(2, 7):
        L = next(L for L in FW.FLOW_LAYERS if L["op"] == "reg_head" and L["level"] == l)
        fl = acts["L%d.flowS" % l]
        mag = fl.pow(2).sum(1).sqrt()
        v = -acts[L["dist"]].pow(2)
        p = (v - v.max(1, True)[0]).exp()
        pmax = (p / p.sum(1, True)).max(1)[0]
        d = acts[L["dist"]].abs()
        print("level %d: flow max %.2f median %.2f px | p_max median %.3f, > 0.99: %.4f | |dist| median %.2f max %.2f"
              % (l, float(mag.max()), float(mag.median()), float(pmax.median()), float((pmax > 0.99).double().mean()),
                 float(d.median()), float(d.max())))
        assert 0.5 <= float(mag.max()) <= 25 and 1.0 <= float(mag.median()) <= 12
        assert float(pmax.median()) <= 0.6 and float((pmax > 0.99).double().mean()) <= 0.01
        assert 0.5 <= float(d.median()) and float(d.max()) <= 40


# ---- the bounds against float32 restatements, with and without one injected bug ---------------------------------------
def _entry(op, level, **kw):
    return next(L for L in FW.FLOW_LAYERS if L["op"] == op and L["level"] == level
                and all(L.get(k) == v for k, v in kw.items()))


def _ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def _case(name, acts, sd, bug, level):
    """(float32 restatement with `bug` or without (None), float64 reference, bound) of one operator on its real input"""
    a32 = {k: v.float() for k, v in acts.items()}
    a64 = {k: v.double() for k, v in a32.items()}
    if name == "warp":
        L = _entry("warp", level, append_flow=1)
        s, f = a32[L["src"]], a32[L["flow"]]
        mult, swap = L["mult"], L["swap"]
        if bug == "wrong_kdbl":
            mult = FW.KDBL[level + 1] if level < 6 else FW.KDBL[5]
        if bug == "swap_ignored":
            swap = 0
        if bug == "align_corners_false":
            g = torch.cat([f[:, 0:1] * mult / ((f.shape[3] - 1) / 2), f[:, 1:2] * mult / ((f.shape[2] - 1) / 2)], 1)
            grid = torch.stack(torch.meshgrid(B.lin(f.shape[2]).float(), B.lin(f.shape[3]).float(), indexing="ij")[::-1], 0)
            got = F.grid_sample(s.flip(0), (grid.unsqueeze(0) + g).permute(0, 2, 3, 1), align_corners=False)
        else:
            got = FW.warp_ref(s, f, mult, swap)
        return got, FW.warp_ref(a64[L["src"]], a64[L["flow"]], L["mult"], L["swap"]), \
            B.warp_bound(a64[L["src"]], a64[L["flow"]], L["mult"], L["swap"])
    if name == "reg_prep":
        L = _entry("reg_prep", level)
        img, fl, mean = a32[L["img"]], a32[L["flow"]], a32[L["mean"]]
        ref = FW.reg_prep_ref(a64[L["img"]], a64[L["flow"]], a64[L["mean"]], L["mult"])
        bound = B.reg_prep_bound(a64[L["img"]], a64[L["flow"]], a64[L["mean"]], L["mult"], ref)
        if bug == "mean_not_subtracted":
            mean = torch.zeros_like(mean)
        if bug == "mean_of_the_other_sample":
            mean = mean.flip(0)
        got = FW.reg_prep_ref(img, fl, mean, L["mult"])
        if bug == "eps_dropped":
            d = img - O.backward_warp(img.flip(0), fl * L["mult"])
            got = torch.cat([d.pow(2).sum(1, True).sqrt(), got[:, 1:]], 1)
        return got, ref, bound
    if name == "reg_head":
        L = _entry("reg_head", level)
        rm = L["wx"]
        args = [sd[L["wx"] + ".weight"], sd[L["wx"] + ".bias"], sd[L["wy"] + ".weight"], sd[L["wy"] + ".bias"]]
        ref = FW.reg_head_ref(a64[L["dist"]], a64[L["flow"]], *[a.double() for a in args], L["k"])
        bound = B.reg_head_bound(a64[L["dist"]], a64[L["flow"]], args[0].double(), float(args[1]), args[2].double(),
                                 float(args[3]), L["k"], ref)
        if bug == "unfold_clamped":
            r = (L["k"] - 1) // 2
            fl = F.pad(a32[L["flow"]], (r, r, r, r), mode="replicate")
            v = -a32[L["dist"]].pow(2)
            e = (v - v.max(1, True)[0]).exp()
            outs = []
            for ch, (w, b) in enumerate(((args[0], args[1]), (args[2], args[3]))):
                uf = F.unfold(fl[:, ch:ch + 1], L["k"]).view_as(e)
                outs.append(F.conv2d(e * uf, w, b) / e.sum(1, True))
            return torch.cat(outs, 1), ref, bound
        assert rm
        r = (L["k"] - 1) // 2
        v = -a32[L["dist"]].pow(2)
        e = (v - v.max(1, True)[0]).exp().double()
        outs = []
        for ch, (w, b) in enumerate(((args[0], args[1]), (args[2], args[3]))):
            uf = F.unfold(a64[L["flow"]][:, ch:ch + 1], L["k"], padding=r).view_as(e)
            outs.append((F.conv2d(e * uf, w.double(), b.double()) / e.sum(1, True)).float())
        return torch.cat(outs, 1), ref, bound
    if name == "corr":
        L = _entry("corr", level)
        f1, f2 = a32[L["src1"]], a32[L["src2"]]
        got = FW.corr_ref(f1, f2, L["stride"], L["swap2"])
        if bug == "one_displacement_shifted":
            got = got.clone()
            got[:, 24] = got[:, 25]
        return got, FW.corr_ref(a64[L["src1"]], a64[L["src2"]], L["stride"], L["swap2"]), \
            B.corr_bound(a64[L["src1"]], a64[L["src2"]], L["stride"], L["swap2"], O.correlation)
    if name == "deconv":
        L = _entry("deconv", level, C=2)
        w = sd[L["w"]].float()
        got = FW.deconv_ref(a32[L["src"]], w.flip(-1, -2) if bug == "kernel_not_flipped" else w)
        return got, FW.deconv_ref(a64[L["src"]], w.double()), B.deconv_bound(a64[L["src"]], w.double())
    if name == "post_resize":
        f = a32["L2.flow"]
        H, W = acts["fwd"].shape[2:]
        fwd, _ = FW.post_resize_ref(f, 10.0, H, W)
        if bug == "rw_rh_swapped":
            fwd = torch.cat([fwd[:, 0:1] * (H / f.shape[2]) / (W / f.shape[3]), fwd[:, 1:2] * (W / f.shape[3]) / (H / f.shape[2])], 1)
        rf, _ = FW.post_resize_ref(a64["L2.flow"], 10.0, H, W)
        return fwd, rf, B.post_resize_bound(a64["L2.flow"], 10.0, H, W)[0]
    if name == "consistency":
        fwd, bwd = a32["fwd"], a32["bwd"]
        got = FW.consistency_ref(fwd, -bwd if bug == "plus_bwd" else bwd).permute(0, 3, 1, 2)
        fd, bd = fwd.double(), bwd.double()
        rc = FW.consistency_ref(fd, bd)
        return got, rc.permute(0, 3, 1, 2), B.consistency_bound(fd, bd, rc)
    if name == "mean":
        fl = a32["L%d.flowS" % level]
        m64 = FW.mean_ref(fl.double())
        got = (fl.double().view(2, 2, -1).sum(2) / fl[0, 0].numel()).float().view(2, 2, 1, 1)
        if bug == "float32_running_sum":
            tot = np.add.accumulate(fl.reshape(2, 2, -1).numpy(), axis=2, dtype=np.float32)[..., -1]
            got = torch.from_numpy(tot / np.float32(fl[0, 0].numel())).view(2, 2, 1, 1)
        return got, m64, B.mean_ulp(m64)
    raise ValueError(name)


MUTATIONS = {
    "warp": ["wrong_kdbl", "align_corners_false", "swap_ignored"],
    "reg_prep": ["mean_not_subtracted", "mean_of_the_other_sample", "eps_dropped"],
    "reg_head": ["unfold_clamped"],
    "corr": ["one_displacement_shifted"],
    "deconv": ["kernel_not_flipped"],
    "post_resize": ["rw_rh_swapped"],
    "consistency": ["plus_bwd"],
    "mean": ["float32_running_sum"],
}


LEVELS = {"deconv": (2, 3, 4, 5), "post_resize": (2,), "consistency": (2,)}


def _worst(op, acts, sd, bug):
    return max(_ratio(*_case(op, acts, sd, bug, l)) for l in LEVELS.get(op, (2, 3, 4, 5, 6)))


@pytest.mark.parametrize("op", list(MUTATIONS))
def test_float32_restatement_passes_the_bound(random_world, op):
    sd, acts = random_world
    ratio = _worst(op, acts, sd, None)
    print("%-12s float32 restatement: worst err / bound %.3f" % (op, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("op,bug", [(op, b) for op, bugs in MUTATIONS.items() for b in bugs])
def test_bound_catches_the_mutation(random_world, op, bug):
    """the worst output over the levels the operator runs at.  The dropped 1e-6 shows where the brightness error is near
    zero: in the coded tunnel world's uniform regions (the random world's smallest errors put it 2.5x outside)"""
    sd, acts = random_world
    if bug == "eps_dropped":
        sd, acts = FW.world("tunnel")[0], FW.walk64("tunnel")
    ratio = _worst(op, acts, sd, bug)
    print("MUTATION %-12s %-26s worst err / bound %.3g" % (op, bug, ratio))
    assert ratio >= 10
