"""DeepPose with the reference's surface (/root/reference/libs/deep_models/pose/deep_pose.py:14-79): the base class of the
two-view pose net interface."""
import torch


class DeepPose:
    def __init__(self):
        self.device = torch.device('cuda')
        self.enable_finetune = False

    def initialize_network_model(self, weight_path):
        raise NotImplementedError

    def inference(self, imgs):
        raise NotImplementedError

    def inference_pose(self, img):
        raise NotImplementedError

    def inference_no_grad(self, imgs):
        """deep_pose.py:57-67"""
        return self.inference(imgs)

    def setup_train(self, deep_model, cfg):
        raise NotImplementedError("online finetuning is out of scope of the inference hot path")
