"""`metrics` for MI355X: the reference's root module metrics.py (`mse`, `psnr`)
and the measurement of its validation step (train.py:68-70, 208-249:
torchmetrics' PeakSignalNoiseRatio and StructuralSimilarityIndexMeasure at
data_range 1, one value per test image, averaged over the images).

`mse` and `psnr` keep the reference's signature and semantics and are torch
expressions on any device.  `ssim` and `ImageMetrics` run ngp_image_metrics
(csrc/metrics.hip): the frame's MSE and SSIM in one launch pair, fp64 inside,
bit-identical from call to call.  There is no CPU fallback for them.
"""
from __future__ import annotations

import math

import torch

import vren


def mse(image_pred, image_gt, valid_mask=None, reduction='mean'):
    """metrics.py:4-10"""
    value = (image_pred - image_gt) ** 2
    if valid_mask is not None:
        value = value[valid_mask]
    if reduction == 'mean':
        return torch.mean(value)
    return value


@torch.no_grad()
def psnr(image_pred, image_gt, valid_mask=None, reduction='mean'):
    """metrics.py:13-15"""
    return -10 * torch.log10(mse(image_pred, image_gt, valid_mask, reduction))


def _frame(name, x, w, h):
    vren._check(name, x, torch.float32)
    if tuple(x.shape) not in ((h * w, 3), (h, w, 3)):
        raise RuntimeError(f"{name} must be (h*w, 3) or (h, w, 3) for img_wh {(w, h)}, got {tuple(x.shape)}")


def _wh(img_wh):
    w, h = (int(v) for v in img_wh)
    if w < 11 or h < 11:
        raise ValueError(f"img_wh {(w, h)}: the SSIM window needs at least 11 x 11 pixels")
    return w, h


def _workspace(w, h, device):
    return torch.empty(max(1, vren.lib().ngp_image_metrics_ws_bytes(h, w) // 8), dtype=torch.float64, device=device)


def ssim(image_pred, image_gt, img_wh, clamp=False, return_map=False):
    """SSIM of one frame (0-dim CUDA tensor): image_pred, image_gt CUDA fp32
    (h*w, 3) or (h, w, 3), img_wh = (w, h) as the datasets give it.  clamp:
    image_pred is clamped to [0, 1] first (image_gt never).  return_map: also
    the (3, h-10, w-10) index of every whole 11x11 window, whose mean it is.
    Does not synchronise."""
    w, h = _wh(img_wh)
    _frame("image_pred", image_pred, w, h)
    _frame("image_gt", image_gt, w, h)
    dev = image_pred.device
    out = torch.empty(2, dtype=torch.float32, device=dev)
    smap = torch.empty(3, h - 10, w - 10, dtype=torch.float32, device=dev) if return_map else None
    with torch.cuda.device(dev):
        vren.kernels().ngp_image_metrics(image_pred, image_gt, h, w, int(bool(clamp)), _workspace(w, h, dev), out,
                                         smap, vren._stream())
    return (out[1], smap) if return_map else out[1]


class ImageMetrics:
    """Per-image PSNR and SSIM of up to max_frames test frames of img_wh =
    (w, h), kept on the device: update() launches into the next frame's slot of
    a (max_frames, 2) buffer of (MSE, SSIM) and does not synchronise; compute()
    synchronises once."""

    def __init__(self, img_wh, max_frames, device):
        self.w, self.h = _wh(img_wh)
        self.max_frames = int(max_frames)
        if self.max_frames < 1:
            raise ValueError("ImageMetrics needs max_frames >= 1")
        self.device = torch.device(device)
        self.values = torch.zeros(self.max_frames, 2, dtype=torch.float32, device=self.device)
        self._ws = _workspace(self.w, self.h, self.device)
        self.n = 0

    def reset(self):
        self.n = 0

    def update(self, pred, gt, clamp=True):
        """pred, gt: CUDA fp32 (h*w, 3) or (h, w, 3); clamp: pred to [0, 1]
        first (sigmoid models; not raw-HDR radiance)."""
        if self.n >= self.max_frames:
            raise RuntimeError(f"ImageMetrics holds {self.max_frames} frames; update() called for one more")
        _frame("pred", pred, self.w, self.h)
        _frame("gt", gt, self.w, self.h)
        with torch.cuda.device(self.device):
            vren.kernels().ngp_image_metrics(pred, gt, self.h, self.w, int(bool(clamp)), self._ws,
                                             self.values[self.n], None, vren._stream())
        self.n += 1

    def compute(self):
        """{'psnr': [per frame], 'ssim': [per frame], 'mean_psnr', 'mean_ssim',
        'mse': [per frame]} of the frames so far; psnr = -10 log10(max(mse,
        1e-12)), the means over images as validation_epoch_end takes them
        (train.py:240-249).  One device-to-host copy."""
        vals = self.values[:self.n].cpu().double().tolist()
        psnrs = [-10 * math.log10(max(m, 1e-12)) for m, _ in vals]
        ssims = [s for _, s in vals]
        k = max(1, len(vals))
        return {"psnr": psnrs, "ssim": ssims, "mse": [m for m, _ in vals], "mean_psnr": sum(psnrs) / k,
                "mean_ssim": sum(ssims) / k}
