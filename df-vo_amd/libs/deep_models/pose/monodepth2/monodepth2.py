"""Monodepth2PoseNet with the reference's surface
(/root/reference/libs/deep_models/pose/monodepth2/monodepth2.py:24-119) over the dfvo_posenet_* C ABI."""
import ctypes as C
import os

import numpy as np
import torch

from ..... import capi
from ..deep_pose import DeepPose


class Monodepth2PoseNet(DeepPose):
    def __init__(self, *args, **kwargs):
        super(Monodepth2PoseNet, self).__init__(*args, **kwargs)
        self.enable_finetune = False
        self.model = None
        # monodepth2.py:73-74; DeepModel.forward_pose feeds the DEPTH net's feed size (deep_models.py:221): the device net is
        # built for whatever size the first call brings (_net)
        self.feed_height = 192
        self.feed_width = 640
        self._params = None
        self._net_size = None
        self._precision = None  # the conv precision in force when the first net was packed (_net)

    def initialize_network_model(self, weight_path, dataset, finetune):
        """monodepth2.py:31-84: directory with pose_encoder.pth + pose.pth, or a dict
        {'encoder': state_dict, 'decoder': state_dict}.  Packs the net at the 192 x 640 feed size."""
        if finetune:
            raise NotImplementedError("online finetuning is training; out of scope of the inference hot path")
        if isinstance(weight_path, dict):
            enc, dec = weight_path['encoder'], weight_path['decoder']
        else:
            enc = torch.load(os.path.join(weight_path, 'pose_encoder.pth'), map_location="cpu")
            dec = torch.load(os.path.join(weight_path, 'pose.pth'), map_location="cpu")
        if 'kitti' in dataset:
            self.stereo_baseline_multiplier = 5.4
        elif 'tum' in dataset:
            self.stereo_baseline_multiplier = 1.
        elif 'robotcar' in dataset:
            self.stereo_baseline_multiplier = 5.4
        else:
            self.stereo_baseline_multiplier = 1.
        params = {}
        for k, v in enc.items():
            if hasattr(v, "detach") and v.dim() > 0 and "num_batches_tracked" not in k and not k.startswith("encoder.fc"):
                params[k] = v.detach().cpu().float().numpy()
        for k, v in dec.items():
            params[k] = v.detach().cpu().float().numpy()
        self._params = params
        self._net(self.feed_height, self.feed_width)

    def _net(self, h, w):
        """the device net for an h x w feed (the weights do not depend on it; the activations and the packing hints do).
        A later size is packed in the conv precision that was in force when the first one was."""
        if self._net_size == (h, w):
            return self.model
        lib = capi.lib()
        capi.require_gpu()
        before = lib.dfvo_get_conv_precision()
        if self._net_size is None:
            self._precision = before
        net = C.c_void_p()
        capi.check(lib.dfvo_posenet_create(int(h), int(w), float(self.stereo_baseline_multiplier), None, C.byref(net)))
        try:
            capi.check(lib.dfvo_set_conv_precision(self._precision))
            capi.set_params(lib.dfvo_posenet_set_param, net, self._params)
            capi.check(lib.dfvo_posenet_finalize(net))
        except Exception:
            lib.dfvo_posenet_destroy(net)
            raise
        finally:
            capi.check(lib.dfvo_set_conv_precision(before))
        if self.model is not None:
            lib.dfvo_posenet_destroy(self.model)
        self.model, self._net_size = net, (h, w)
        return net

    def inference_pose_images_u8(self, img0_u8, img1_u8, feed_height, feed_width):
        """two uint8 [H, W, 3] frames of one size -> float32 [4, 4]: the Pillow-exact LANCZOS resize of each to the feed size
        (deep_models.py:217-225) runs on the device in front of the net; the translation carries the baseline multiplier"""
        assert img0_u8.shape == img1_u8.shape and img0_u8.ndim == 3 and img0_u8.shape[2] == 3
        assert img0_u8.dtype == np.uint8 and img1_u8.dtype == np.uint8
        pose = np.zeros((4, 4), np.float32)
        capi.check(capi.lib().dfvo_posenet_forward_images_host(
            self._net(feed_height, feed_width), capi.as_ptr(np.ascontiguousarray(img0_u8)), capi.as_ptr(np.ascontiguousarray(img1_u8)),
            int(img0_u8.shape[0]), int(img0_u8.shape[1]), capi.as_ptr(pose)))
        return pose

    def inference(self, imgs):
        """monodepth2.py:86-99: [1, 6, h, w] float tensor of k/255 values (ToTensor of two uint8 images, concatenated on
        dim 1) -> [1, 4, 4], the relative pose from image 2 to image 1 WITHOUT the baseline multiplier"""
        self.inference_pose(imgs)
        return self.pred_pose

    def inference_no_grad(self, imgs):
        return self.inference(imgs)

    def inference_pose(self, img):
        """monodepth2.py:101-119: -> [1, 4, 4] with the translation x stereo_baseline_multiplier.  The device net applies the
        multiplier; pred_pose (the unmultiplied prediction) divides it out again on the host."""
        a = img.detach().cpu().numpy()
        assert a.ndim == 4 and a.shape[0] == 1 and a.shape[1] == 6, "expected a [1, 6, H, W] image pair"
        a = a[0].transpose(1, 2, 0).astype(np.float64) * 255.0
        u = np.rint(a)
        if np.abs(a - u).max() > 1e-3:
            raise capi.DfvoError("Monodepth2PoseNet.inference_pose expects images quantised to k/255")
        u = u.astype(np.uint8)
        h, w = u.shape[:2]
        pose = self.inference_pose_images_u8(np.ascontiguousarray(u[..., :3]), np.ascontiguousarray(u[..., 3:]), h, w)
        out = torch.from_numpy(pose)[None]
        self.pred_pose = out.clone()
        self.pred_pose[:, :3, 3] /= self.stereo_baseline_multiplier
        return out
