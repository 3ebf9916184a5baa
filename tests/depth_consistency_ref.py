"""Restatements and inputs for the depth-consistency tests: DepthConsistency.warp_and_reproj_depth + compute_depth_diff
(libs/matching/depth_consistency.py:69-151 over libs/geometry/{backprojection, transformation3d, projection}.py) in torch, and
kp_selection.local_bestN with the depth mask (kp_selection.py:74-200) over oracle.tracker_np.  Both are pinned to fixtures the
reference's own classes wrote (tests/golden/make_golden_posenet.py, tests/test_posenet_surface_cpu.py)."""
import importlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tracker_np as T


def depth_consistency_torch(cur_depth, ref_depth, K, inv_K, pose, dtype=torch.float32):
    """cur_depth, ref_depth [H, W] float32; K, inv_K [3, 3] and pose [4, 4] float32 (what .float() leaves of the reference's
    float64 matrices) -> depth_diff [H, W].  dtype=torch.float64 evaluates the same float32 inputs in double: the anchor."""
    h, w = cur_depth.shape
    d = torch.from_numpy(np.ascontiguousarray(cur_depth)).to(dtype).view(1, 1, -1)
    ref = torch.from_numpy(np.ascontiguousarray(ref_depth)).to(dtype).view(1, 1, h, w)
    K, inv_K, pose = (torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(dtype)[None] for m in (K, inv_K, pose))
    mesh = np.meshgrid(range(w), range(h), indexing='xy')
    xy = torch.from_numpy(np.stack(mesh, axis=0).astype(np.float32)).to(dtype).view(1, 2, -1)
    xy1 = torch.cat([xy, torch.ones(1, 1, h * w, dtype=dtype)], 1)
    points = torch.cat([d * torch.matmul(inv_K, xy1), torch.ones(1, 1, h * w, dtype=dtype)], 1)      # backprojection.py:61-63
    moved = torch.matmul(pose, points)                                                                # transformation3d.py:31
    K4 = torch.zeros(1, 3, 4, dtype=dtype)
    K4[:, :, :3] = K
    p2 = torch.matmul(K4, moved)                                                                      # projection.py:46-57
    pix = (p2[:, :2] / (p2[:, 2:3] + 1e-7)).view(1, 2, h, w).permute(0, 2, 3, 1).clone()
    pix[..., 0] /= w - 1
    pix[..., 1] /= h - 1
    pix = (pix - 0.5) * 2
    warp = F.grid_sample(ref, pix, mode='bilinear', padding_mode='border', align_corners=True)      # torch 1.1's corners
    reproj = torch.matmul(pose[:, :3, :], points).view(1, 3, h, w)[:, 2:]
    return ((warp - reproj).abs() / reproj).clamp(0, 1)[0, 0].numpy(), reproj[0, 0].numpy()


def tunnel_scene(h, w, k, step=0.3):
    """two views of synthetic.py's tunnel world: the raw depths of frame k + 1 (current) and frame k (reference), clipped to
    [2, 40] m, K, K^-1 and the pose current -> reference (|t| <= 0.5 m), all float32 as the reference hands them to torch"""
    syn = importlib.import_module("df-vo_amd.synthetic")
    K = syn.kitti_K(h, w)
    poses = syn.tunnel_poses(k + 2, step=step, seed=7)
    py, px = np.mgrid[0:h, 0:w].astype(np.float64)
    depth = [np.clip(syn.tunnel_cast(K, poses[i], py, px)[1], 2.0, 40.0).astype(np.float32) for i in (k + 1, k)]
    pose = np.linalg.inv(poses[k]) @ poses[k + 1]
    assert np.linalg.norm(pose[:3, 3]) <= 0.5
    return depth[0], depth[1], K.astype(np.float32), np.linalg.inv(K).astype(np.float32), pose.astype(np.float32)


def masked_kp_case(h, w, seed, frac, nan_frac=0.0):
    """seeded flow, flow_diff (make_golden.kp_case's recipe) and depth_diff maps of the masked local_bestN fixtures"""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    diff = rng.random((int(h), int(w), 1), dtype=np.float32) * np.float32(0.1 / frac)
    diff[rng.random((int(h), int(w), 1)) < 0.01] = np.float32(0.05)  # ties
    flow = (rng.standard_normal((2, int(h), int(w))) * 3).astype(np.float32)
    ddiff = (rng.random((int(h), int(w)), dtype=np.float32) ** 2 * np.float32(0.2)).astype(np.float32)
    ddiff[: int(h) // 3, : int(w) // 4] = np.float32(1.0)  # a region the depth mask empties
    if nan_frac:
        ddiff[rng.random((int(h), int(w))) < nan_frac] = np.float32("nan")
    return diff, flow, ddiff


def local_bestN_masked(flow, flow_diff, depth_diff, num_bestN=2000, num_row=10, num_col=10, thre=0.1, depth_thre=0.05,
                       score_method="flow"):
    """kp_selection.py:74-200 with kp_selection.depth_consistency.enable: a cell's candidates are score < thre AND
    depth_diff < depth_thre, ranked by the score alone in numpy's scalar introselect order; the "enough good pixels" rule
    stays on flow_diff.  flow [2,H,W], flow_diff [H,W,1], depth_diff [H,W] -> dict(good_kp_found, kp1_best, kp2_best [1,N,2])"""
    h, w, _ = flow_diff.shape
    kp1 = np.expand_dims(T.image_grid(h, w), 0)
    kp2 = kp1 + np.transpose(np.expand_dims(flow, 0), (0, 2, 3, 1))
    n_best = math.floor(num_bestN / (num_col * num_row))
    diff = np.expand_dims(flow_diff, 0)
    ddiff = depth_diff.reshape(1, h, w, 1)
    out = {"good_kp_found": True}
    if (diff[0, :, :, 0] < thre).sum() < num_bestN * 0.1:
        out["good_kp_found"] = False
        return out
    sel, good_region_cnt = [], 0
    for row in range(num_row):
        for col in range(num_col):
            x0 = [int(h / num_row * row), int(w / num_col * col)]
            x1 = [int(h / num_row * (row + 1)) - 1, int(w / num_col * (col + 1)) - 1]
            tile = diff[:, x0[0]:x1[0], x0[1]:x1[1]].copy()
            if score_method == "flow_ratio":
                tmp_flow = np.transpose(np.expand_dims(flow[:, x0[0]:x1[0], x0[1]:x1[1]], 0), (0, 2, 3, 1))
                with np.errstate(divide="ignore", invalid="ignore"):
                    tile = tile / np.linalg.norm(tmp_flow, axis=3, keepdims=True)
            with np.errstate(invalid="ignore"):
                where = np.where((tile < thre) & (ddiff[:, x0[0]:x1[0], x0[1]:x1[1]] < depth_thre))
            num_to_pick = min(n_best, len(where[0]))
            if num_to_pick != 0:
                good_region_cnt += 1
            order = T.argpartition_c(tile[where], num_to_pick - 1)[:num_to_pick]
            for i in order:
                sel.append((where[1][i] + x0[0], where[2][i] + x0[1]))
    if good_region_cnt < (num_row * num_col) * 0.1:
        out["good_kp_found"] = False
        return out
    ys = np.asarray([s[0] for s in sel], np.int64)
    xs = np.asarray([s[1] for s in sel], np.int64)
    out["kp1_best"] = kp1[:, ys, xs]
    out["kp2_best"] = kp2[:, ys, xs]
    return out
