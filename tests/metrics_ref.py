"""fp64 reference of ngp_image_metrics (include/ngp_amd.h): the frame's MSE
and the SSIM of Wang et al. as torchmetrics' StructuralSimilarityIndexMeasure
evaluates it at data_range 1 -- 11x11 Gaussian window (sigma 1.5, sum 1),
C1 = 1e-4, C2 = 9e-4, whole windows only (torchmetrics pads by reflection and
crops the padded border away again, so its mean is the mean over these).

Written independently of the kernel's structure: every window is the DIRECT
two-dimensional 11x11 weighted sum over its 121 pixels (one vectorised term
per tap), not two separable passes; all arithmetic is numpy float64.
"""
import numpy as np

K = 11
SIGMA = 1.5
C1 = 0.01 ** 2
C2 = 0.03 ** 2


def window1d():
    d = np.arange(K, dtype=np.float64) - (K - 1) / 2
    g = np.exp(-0.5 * (d / SIGMA) ** 2)
    return g / g.sum()


def window2d():
    g = window1d()
    return np.outer(g, g)


def _image(x, h, w):
    """(h*w,3) or (h,w,3) fp32 tensor / array -> (h,w,3) fp32 array"""
    x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    assert x.dtype == np.float32 and x.size == 3 * h * w
    return x.reshape(h, w, 3)


def moments(x, y):
    """x, y (h,w) float64 -> the five window sums E[x], E[y], E[x^2], E[y^2],
    E[xy], each (h-10, w-10)"""
    h, w = x.shape
    oh, ow = h - (K - 1), w - (K - 1)
    W = window2d()
    planes = (x, y, x * x, y * y, x * y)
    out = [np.zeros((oh, ow)) for _ in planes]
    for i in range(K):
        for j in range(K):
            for o, p in zip(out, planes):
                o += W[i, j] * p[i:i + oh, j:j + ow]
    return out


def index(mx, my, exx, eyy, exy):
    vx, vy, cxy = exx - mx * mx, eyy - my * my, exy - mx * my
    return ((2 * (mx * my) + C1) * (2 * cxy + C2)) / (((mx * mx + my * my) + C1) * ((vx + vy) + C2))


def image_metrics(pred, gt, h, w, clamp=False):
    """-> (ssim_map (3,h-10,w-10) float64, ssim, mse), pred clamped to [0,1]
    first with clamp (gt never)"""
    p, g = _image(pred, h, w), _image(gt, h, w)
    if clamp:
        p = np.clip(p, np.float32(0), np.float32(1))
    p, g = p.astype(np.float64), g.astype(np.float64)
    smap = np.stack([index(*moments(p[..., c], g[..., c])) for c in range(3)])
    return smap, float(smap.mean()), float(((p - g) ** 2).mean())


def ssim_torch_fp32(pred, gt, h, w):
    """The same index the way torchmetrics evaluates it, in fp32 torch ops on
    the tensors' device: one grouped conv2d of the 2-D window over (x, y, xx,
    yy, xy), whole windows only.  For scale and for timing only -- its
    E[x^2] - mu^2 cancels in fp32, so it is no reference for the kernel."""
    import torch
    import torch.nn.functional as F
    x = pred.reshape(h, w, 3).permute(2, 0, 1).unsqueeze(0)
    y = gt.reshape(h, w, 3).permute(2, 0, 1).unsqueeze(0)
    g = torch.tensor(window1d(), dtype=torch.float32, device=x.device)
    kernel = (g[:, None] * g[None, :]).expand(3, 1, K, K).contiguous()
    mx, my, exx, eyy, exy = F.conv2d(torch.cat([x, y, x * x, y * y, x * y]), kernel, groups=3)
    vx, vy, cxy = exx - mx * mx, eyy - my * my, exy - mx * my
    smap = ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return smap, smap.mean()
