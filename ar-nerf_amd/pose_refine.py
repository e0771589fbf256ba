"""Camera pose refinement of the reference (--optimize_ext, opt.py:54): every
training image gets an axis-angle correction dR and a translation dT
(train.py:132-137), applied to its pose before the rays are formed
(train.py:92-95) and stepped by their own FusedAdam at a hard-coded 1e-6
(train.py:148-149).  The gradient reaches them from the loss through
render() -> RayMarcher.backward (ngp_ray_segment_sum) <- the field's input
gradients (ngp_field_input_grad).

dR and dT are views of ONE flat parameter `ext` = [dR (N,3) | dT (N,3) | pad]
padded to a multiple of 4 floats: optimizers.FusedAdam (the native Adam
launch) takes no other size, and one launch then steps both."""
import torch
from torch import nn

from datasets.ray_utils import axisangle_to_R, get_rays
from optimizers import FusedAdam


class PoseRefiner(nn.Module):
    def __init__(self, n_images, device="cuda"):
        super().__init__()
        self.n_images = int(n_images)
        n = 6 * self.n_images
        self.ext = nn.Parameter(torch.zeros((n + 3) // 4 * 4, device=device))  # zero: the poses as loaded

    @property
    def dR(self):
        """(N_img,3) axis-angle corrections (a view of `ext`)"""
        return self.ext[:3 * self.n_images].view(self.n_images, 3)

    @property
    def dT(self):
        """(N_img,3) translation corrections (a view of `ext`)"""
        return self.ext[3 * self.n_images:6 * self.n_images].view(self.n_images, 3)

    def poses_of(self, img_idxs, poses):
        """train.py:92-95 on the gathered poses (n,3,4): [dR @ R | t + dT]; `poses` is not modified."""
        p = poses[img_idxs]
        R = axisangle_to_R(self.dR[img_idxs]) @ p[..., :3]
        t = p[..., 3] + self.dT[img_idxs]
        return torch.cat([R, t[..., None]], -1)

    def rays(self, img_idxs, pix_idxs, directions, poses):
        """train.py:85-97 -> rays_o, rays_d (n,3) of the batch, differentiable w.r.t. dR / dT."""
        return get_rays(directions[pix_idxs], self.poses_of(img_idxs, poses))

    def optimizer(self, lr=1e-6):
        """The reference's FusedAdam([dR, dT], 1e-6) (the learning rate is hard-coded there)."""
        return FusedAdam([self.ext], lr)

    @torch.no_grad()
    def refined_poses(self, poses):
        """(N_img,3,4): every image's pose with its correction applied"""
        return self.poses_of(torch.arange(self.n_images, device=poses.device), poses)

    def state_dict_reference(self):
        """{'dR', 'dT'}: the reference checkpoint's keys for the two parameters"""
        return {"dR": self.dR.detach().clone(), "dT": self.dT.detach().clone()}

    @torch.no_grad()
    def load_reference(self, state):
        self.dR.copy_(state["dR"].to(self.ext))
        self.dT.copy_(state["dT"].to(self.ext))
