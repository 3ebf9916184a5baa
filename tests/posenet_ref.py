"""Torch restatement of the monodepth2 pose net (pose/monodepth2/monodepth2.py:86-99, pose_decoder.py:35-54,
layers.py:28-104) for the pose-net tests, over oracle.nets_torch.resnet18_encoder.  dtype=torch.float64 evaluates the same
fp32 weights and inputs in double: the anchor of the accuracy tests (oracle/nets_torch.py: flow_inference)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets_torch as O

# parameter vectors (axis-angle, translation) of tests/test_pose_math_cpu.py: the net's scale (1e-4 .. 1e-1), the zero
# vector (angle 0: axis = 0 / 1e-7) and one large angle (3 rad)
MATH_CASES = [
    [1.0e-4, -2.0e-4, 3.0e-4, 1.0e-3, -2.0e-3, 5.0e-2],
    [3.1e-3, 1.2e-3, -4.7e-3, -2.3e-2, 4.1e-3, 9.7e-2],
    [-1.7e-2, 5.3e-2, 2.9e-2, 6.1e-2, -8.3e-2, 1.0e-1],
    [1.0e-1, -1.0e-1, 1.0e-1, 1.0e-4, 1.0e-4, -1.0e-4],
    [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
    [0.0, 0.0, 0.0, 1.0e-2, -2.0e-2, 3.0e-2],
    [1.2, -2.0, 1.8708287, 0.05, -0.02, 0.1],
]


def record_parity(section, values):
    """the measured distances of the GPU tests: merged into the JSON file DFVO_POSENET_PARITY_JSON names, when it is set
    (profiles/posenet_parity.json is a copy of one such run)"""
    import json
    import os
    path = os.environ.get("DFVO_POSENET_PARITY_JSON")
    if not path:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data.setdefault(section, {}).update(values)
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def pose_decoder(sd, feat):
    """pose_decoder.py:35-54 with one input feature and two predicted frames -> [N, 12]"""
    x = F.relu(F.conv2d(feat, sd['net.0.weight'], sd['net.0.bias']))
    x = F.relu(F.conv2d(x, sd['net.1.weight'], sd['net.1.bias'], padding=1))
    x = F.relu(F.conv2d(x, sd['net.2.weight'], sd['net.2.bias'], padding=1))
    x = F.conv2d(x, sd['net.3.weight'], sd['net.3.bias'])
    return 0.01 * x.mean(3).mean(2)


def rotation(axisangle):
    """layers.py:64-103 for one [3] vector -> [3, 3]"""
    angle = torch.norm(axisangle)
    x, y, z = axisangle / (angle + 1e-7)
    ca, sa = torch.cos(angle), torch.sin(angle)
    C = 1 - ca
    xC, yC, zC = x * C, y * C, z * C
    return torch.stack([torch.stack([x * xC + ca, x * yC - z * sa, z * xC + y * sa]),
                        torch.stack([x * yC + z * sa, y * yC + ca, y * zC - x * sa]),
                        torch.stack([z * xC - y * sa, y * zC + x * sa, z * zC + ca])])


def transformation_inverted(params6):
    """transformation_from_parameters(axisangle, translation, invert=True): M = R^T . T(-t), in params6's dtype"""
    p = torch.as_tensor(params6)
    M = torch.zeros(4, 4, dtype=p.dtype)
    M[:3, :3] = rotation(p[:3]).t()
    T = torch.eye(4, dtype=p.dtype)
    T[:3, 3] = -p[3:]
    M[3, 3] = 1
    return M @ T


@torch.no_grad()
def posenet_parameters(sd, img6, dtype=torch.float32):
    """img6: [1, 6, H, W] float32 of k/255 values -> (the six raw parameters of frame 0 as a numpy vector, feats[4])"""
    x = img6.to(dtype)
    if dtype != torch.float32:
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    feats = O.resnet18_encoder(sd, x)
    out = pose_decoder(sd, feats[4])
    return out[0, :6].numpy(), feats[4].numpy()


def pair_tensor(img0_u8, img1_u8):
    """DeepModel.forward_pose's input (deep_models.py:217-225) of two feed-size uint8 frames: [1, 6, H, W] float32"""
    t = [torch.from_numpy(np.ascontiguousarray(i)).permute(2, 0, 1).contiguous().float().div(255).unsqueeze(0) for i in (img0_u8, img1_u8)]
    return torch.cat(t, 1)
