"""Object shading for insertion frames: the SG branch of the reference app's
Insertor.render_object (insert/main.py:521-594) and its SG_render_core
(insert/render_utils.py:265-375) -- a physically based shade of every pixel
the virtual object covers under L spherical-Gaussian lights -- as one HIP
launch (csrc/shade.hip).

sg_shade        the kernel: whole-frame obj_rgb, no temporaries, no host wait
sg_shade_torch  the same result from torch ops over (pixels, L) temporaries,
                as the reference formulates it: the path for CPU tensors and
                the baseline scripts/bench_shade.py times the kernel against

A pixel is covered when it lies in the model's box `bbox` = (hs, ws, hl, wl)
and obj_depth > 1e-6 (an fp32 compare); every other pixel of the frame is 0.
A covered pixel with a zero normal is out of contract (0/0, as in the
reference).  The self-shadow `decay` and the SSDF cast shadow of an SG-lit frame
are sg_shadow.py's.  Not here: the SH / neural-BRDF shade, the
SH path's shadow_field and the raster shadow_cast, tone mapping.
"""
from __future__ import annotations

import math

import torch

import vren

EPS = 1e-6
COS_LAMBDA, COS_AMP, COS_OFF = 0.0315, 32.7080, 31.7003  # the clamped cosine as an SG, and its offset


def _arg(name, x, dtype, numel=None, shape_text=None):
    """vren._check, with every failure (dtype and size alike) a ValueError"""
    try:
        vren._check(name, x, dtype)
    except RuntimeError as e:
        raise ValueError(str(e)) from None
    if numel is not None and x.numel() != numel:
        raise ValueError(f"{name} must be {shape_text}, got {tuple(x.shape)}")
    return x


def _bbox_ints(bbox, H, W):
    hs, ws, hl, wl = (int(v) for v in bbox)
    if not (0 <= hs <= hl <= H and 0 <= ws <= wl <= W):
        raise ValueError(f"bbox (hs, ws, hl, wl) = {(hs, ws, hl, wl)} does not lie in the {H} x {W} frame")
    return hs, ws, hl, wl


def _bbox_tensor(bbox, H, W, device):
    if isinstance(bbox, torch.Tensor):
        if bbox.dtype != torch.int32 or bbox.numel() != 4 or not bbox.is_cuda or not bbox.is_contiguous():
            raise ValueError("bbox must be four ints or a device int32[4] tensor (hs, ws, hl, wl)")
        return bbox
    return torch.tensor(_bbox_ints(bbox, H, W), dtype=torch.int32, device=device)


def _launch(H, W, directions, c2w, bbox, normals, obj_depth, lSGs, metal, rough, albedo, decay, clamp01, out):
    """Checks and the launch; bbox a device int32[4], c2w a device (3,4) fp32, out (H*W*3) fp32."""
    n = H * W
    f32 = torch.float32
    _arg("directions", directions, f32, 3 * n, f"(H*W,3) = ({n},3)")
    _arg("c2w", c2w, f32, 12, "(3,4)")
    _arg("normals", normals, f32, 3 * n, f"(H*W,3) = ({n},3)")
    _arg("obj_depth", obj_depth, f32, n, f"(H*W) = ({n})")
    _arg("lSGs", lSGs, f32)
    if lSGs.dim() != 2 or lSGs.shape[1] != 7 or lSGs.shape[0] < 1:
        raise ValueError(f"lSGs must be (L,7) with L >= 1, got {tuple(lSGs.shape)}")
    L = lSGs.shape[0]
    if decay is not None:
        _arg("decay", decay, f32)
        if decay.dim() < 2 or decay.shape[-1] != L or decay.numel() != n * L:
            raise ValueError(f"decay must be (H*W, L) = ({n},{L}), got {tuple(decay.shape)}")
    albedo_rows = 0
    if albedo is not None:
        _arg("albedo", albedo, f32)
        if albedo.numel() not in (3, 3 * n):
            raise ValueError(f"albedo must be (1,3) or (H*W,3) = ({n},3), got {tuple(albedo.shape)}")
        albedo_rows = albedo.numel() // 3
    metal_map = rough_map = None
    if isinstance(metal, torch.Tensor):
        metal_map, metal = _arg("metal", metal, f32, n, f"a number or an (H*W) = ({n}) map"), 0.0
    if isinstance(rough, torch.Tensor):
        rough_map, rough = _arg("rough", rough, f32, n, f"a number or an (H*W) = ({n}) map"), 0.0
    _arg("out", out, f32, 3 * n, f"(H,W,3) = ({H},{W},3)")
    vren.kernels().ngp_sg_shade(bbox, H, W, directions, c2w, normals, obj_depth, lSGs, L, decay, albedo, albedo_rows,
                                metal_map, float(metal), rough_map, float(rough), int(bool(clamp01)), out,
                                vren._stream())


@torch.no_grad()
def sg_shade(H, W, directions, c2w, bbox, normals, obj_depth, lSGs, metal=0.9, rough=0.2, albedo=None, decay=None,
             clamp01=True, out=None):
    """The shaded object over the whole frame -> obj_rgb (H,W,3) fp32.

    directions (H*W,3): the camera's per-pixel directions; c2w (3,4): the pose.
    bbox: the model's box (hs, ws, hl, wl) as four ints (checked against the
    frame) or a device int32[4] tensor (clamped to the frame by the kernel).
    normals (H,W,3), any length but zero; obj_depth (H,W).
    lSGs (L,7): axis, sharpness, rgb amplitude of each light.
    metal: a number or an (H*W) map.  rough: a number, used as given, or an
    (H*W) map, clipped to [0.2, 1].  albedo: None (ones), (1,3) or (H*W,3).
    decay: None or (H*W, L), the self-shadow factor on each light's amplitude.
    clamp01: clamp the radiance to [0,1] (LDR), else relu (HDR).
    out: an (H,W,3) fp32 tensor to write (e.g. a renderer's obj_rgb buffer).

    CPU tensors go through sg_shade_torch."""
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"bad frame size {H} x {W}")
    if isinstance(normals, torch.Tensor) and not normals.is_cuda:
        if not isinstance(bbox, torch.Tensor):
            bbox = _bbox_ints(bbox, H, W)
        res = sg_shade_torch(H, W, directions, c2w, bbox, normals, obj_depth, lSGs, metal, rough, albedo, decay,
                             clamp01)
        if out is not None:
            out.copy_(res.reshape(out.shape))
            return out.view(H, W, 3)
        return res
    _arg("normals", normals, torch.float32)
    dev = normals.device
    if out is None:
        out = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    _arg("c2w", c2w, torch.float32)
    _launch(H, W, directions, c2w, _bbox_tensor(bbox, H, W, dev), normals, obj_depth, lSGs, metal, rough, albedo,
            decay, clamp01, out)
    return out.view(H, W, 3)


# ------------------------------------------------------------ torch formulation
def _dot(a, b):
    return (a * b).sum(-1, keepdim=True)


def _sg_product(ax1, lam1, amp1, ax2, lam2, amp2):
    """The product of two SGs (axis (...,3), sharpness (...,1), amplitude (...,3)) is an SG"""
    lm = lam1 + lam2
    um = (lam1 * ax1 + lam2 * ax2) / lm
    ln = torch.linalg.vector_norm(um, dim=-1, keepdim=True)
    return um * (1.0 / ln), lm * ln, amp1 * amp2 * torch.exp(lm * (ln - 1.0))


def _sg_hemisphere(ax, lam, amp, n):
    """The integral of an SG over the hemisphere about n (a fitted sigmoid between the two closed-form ends)"""
    cos_beta = _dot(ax, n)
    lv = lam.clamp(min=EPS)
    il = 1.0 / lv
    t = torch.sqrt(lv) * (1.6988 + 10.8438 * il) / (1.0 + 6.2201 * il + 10.2415 * il * il)
    inv_a = torch.exp(-t)
    up = (cos_beta >= 0).to(lam.dtype)
    inv_b = torch.exp(-t * cos_beta.clamp(min=0.0))
    s1 = (1.0 - inv_a * inv_b) / (1.0 - inv_a + inv_b - inv_a * inv_b)
    b = torch.exp(t * cos_beta.clamp(max=0.0))
    s2 = (b - inv_a) / ((1.0 - inv_a) * (b + 1.0))
    s = up * s1 + (1.0 - up) * s2
    Ab = 2.0 * math.pi / lv * (torch.exp(-lv) - torch.exp(-2.0 * lv))
    Au = 2.0 * math.pi / lv * (1.0 - torch.exp(-lv))
    return (Ab * (1.0 - s) + Au * s) * amp


def _sg_irradiance(ax, lam, amp, n):
    """sum over the lights (dim 1) of each lobe against the clamped cosine about n (P,1,3); rectified after the sum"""
    cos_lam = torch.full_like(lam, COS_LAMBDA)
    cos_amp = torch.full_like(amp, COS_AMP)
    cax, clam, camp = _sg_product(ax, lam, amp, n.expand_as(ax), cos_lam, cos_amp)
    irr = _sg_hemisphere(cax, clam, camp, n) - COS_OFF * _sg_hemisphere(ax, lam, amp, n)
    return torch.relu(irr.sum(1))


@torch.no_grad()
def sg_shade_torch(H, W, directions, c2w, bbox, normals, obj_depth, lSGs, metal=0.9, rough=0.2, albedo=None,
                   decay=None, clamp01=True):
    """sg_shade from torch ops in the reference's formulation: a boolean-mask
    gather of the covered pixels, (pixels, L, .) temporaries for every step of
    the light sum, a masked scatter into the frame.  Any device, any float
    dtype (the dtype of `normals`); bbox as ints or a tensor (clamped)."""
    H, W = int(H), int(W)
    dt, dev = normals.dtype, normals.device
    hs, ws, hl, wl = (int(v) for v in (bbox.tolist() if isinstance(bbox, torch.Tensor) else bbox))
    hs, hl = min(max(hs, 0), H), min(max(hl, 0), H)
    ws, wl = min(max(ws, 0), W), min(max(wl, 0), W)
    inbox = torch.zeros(H, W, dtype=torch.bool, device=dev)
    if hl > hs and wl > ws:
        inbox[hs:hl, ws:wl] = True
    mask = inbox.reshape(-1) & (obj_depth.reshape(-1) > EPS)
    out = torch.zeros(H * W, 3, dtype=dt, device=dev)
    P = int(mask.sum())
    if P == 0:
        return out.view(H, W, 3)
    n = normals.reshape(-1, 3)[mask]
    n = n / torch.linalg.vector_norm(n, dim=-1, keepdim=True)
    d = directions.reshape(-1, 3)[mask].to(dt) @ c2w.to(dt)[:, :3].T
    v = -(d / torch.linalg.vector_norm(d, dim=-1, keepdim=True))
    if albedo is None:
        alb = torch.ones(P, 3, dtype=dt, device=dev)
    else:
        alb = albedo.reshape(-1, 3)
        alb = alb.expand(P, 3) if alb.shape[0] == 1 else alb[mask]
    if isinstance(metal, torch.Tensor):
        met = metal.reshape(-1, 1)[mask]
    else:
        met = torch.full((P, 1), float(metal), dtype=dt, device=dev)
    if isinstance(rough, torch.Tensor):
        rgh = rough.reshape(-1, 1)[mask].clamp(0.2, 1.0)
    else:
        rgh = torch.full((P, 1), float(rough), dtype=dt, device=dev)
    L = lSGs.shape[0]
    lax = lSGs[None, :, :3].expand(P, L, 3)
    llam = lSGs[None, :, 3:4].expand(P, L, 1)
    lamp = lSGs[None, :, 4:].expand(P, L, 3)
    if decay is not None:
        lamp = lamp * decay.reshape(H * W, L)[mask][:, :, None]

    ndv = _dot(n, v)
    m2 = rgh * rgh
    dax = (ndv * n * 2.0 - v)[:, None, :].expand(P, L, 3)
    dlam = (2.0 / m2 / (4.0 * ndv.clamp(min=EPS)))[:, None, :].expand(P, L, 1)
    damp = (1.0 / (math.pi * m2))[:, None, :].expand(P, L, 3)
    n_l = n[:, None, :]
    pax, plam, pamp = _sg_product(dax, dlam, damp, lax, llam, lamp)
    spec_irr = _sg_irradiance(pax, plam, pamp, n_l)
    diff_irr = _sg_irradiance(lax, llam, lamp, n_l)

    ndv_pos = torch.relu(ndv)
    om5 = torch.pow(1.0 - ndv_pos, 5)
    F0 = 0.04 * (1.0 - met) + alb * met
    F = F0 + (1.0 - F0) * om5
    tan2 = m2 * (1.0 / ndv_pos ** 2 - 1.0).clamp(min=0.0)
    G = 1.0 / (0.5 * (torch.sqrt(1.0 + tan2) - 1.0) * 2.0 + 1.0)
    Moi = F * G / (4.0 * ndv_pos * ndv_pos + EPS)
    kS = F0 + (torch.maximum((1.0 - rgh).expand_as(F0), F0) - F0) * om5
    kD = (1.0 - kS) * (1.0 - met)
    rad = kD * (alb / math.pi * diff_irr) + Moi * spec_irr
    out[mask] = rad.clamp(0.0, 1.0) if clamp01 else torch.relu(rad)
    return out.view(H, W, 3)
