"""SSDF soft shadows for insertion frames under SG lights: what the reference
app's insert/sg_shadow.py computes for every frame -- the self-shadow decay of
each light per object pixel (calc_self_shadow_light_dacay, main.py:558-567) and
the cast-shadow factor over the screen's surface points (calc_shadow_factor,
main.py:492-519) with its 3 x 3 blur and multiply -- as HIP launches
(csrc/shadow.hip).

SGShadow         holds the asset tensors and a light workspace per L:
                 calc_shadow_factor, self_shadow_decay,
                 calc_self_shadow_light_dacay (the reference's spelling and
                 (P,L,7) result), frame_decay (the decay of a frame's covered
                 pixels, for InsertRenderer.self_shadow_decay)
shadow_apply     rgb * blur3x3(factor) into a new tensor
sg_shadow_torch  factor and decay from torch ops over (points, C) and
                 (points, L) temporaries, as the reference formulates them: the
                 path for CPU tensors and the baseline scripts/bench_shadow.py
                 times the kernels against

The assets are the app's, handed over as tensors (nothing is loaded here):
coeff (G,G,G,C), the PCA coefficient volume as stored (before the reference's
permute: a point's x indexes the first axis); components (C,envH,envW); mean
(envH,envW); fh_tab (n_lambda,n_theta), the hemisphere-integral table.
The two calls treat rot_inv differently, as the reference's do:
calc_shadow_factor expects light axes that are already rotated, the decay
rotates them itself.  Out of contract: an axis component outside [-1,1], a
sharpness of 0, a colour channel whose summed hemisphere integral is 0.
Not here: the SH path's shadow_field, the raster shadow_cast, loading assets.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import vren
from capi import C as _C
from shading import _arg, _bbox_tensor

MAX_COMPONENTS = _C["NGP_SSDF_MAX_COMPONENTS"]
LIGHT_TILE = _C["NGP_SSDF_LIGHT_TILE"]
LIGHT_WORDS = _C["NGP_SSDF_LIGHT_WORDS"]
LUMA = (0.2989, 0.5870, 0.1140)
BLUR_SIGMA = 0.8  # torchvision's default for a kernel of 3: 0.3 * ((3 - 1) * 0.5 - 1) + 0.8


def _lights_arg(lSGs):
    if not isinstance(lSGs, torch.Tensor) or lSGs.dim() != 2 or lSGs.shape[1] != 7 or lSGs.shape[0] < 1:
        raise ValueError(f"lSGs must be (L,7) with L >= 1, got {tuple(getattr(lSGs, 'shape', ()))}")
    return lSGs.shape[0]


# ------------------------------------------------------------ torch formulation
def _sample2d(img, x, y):
    """img (K,h,w) at the n coordinates (x, y): bilinear, pixel centres, border padding -> (K,n)"""
    grid = torch.stack([x, y], -1).reshape(1, 1, -1, 2)
    return F.grid_sample(img.unsqueeze(0), grid, mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0]


@torch.no_grad()
def sg_shadow_torch(coeff, components, mean, fh_tab, vol_range, scale, pts, model_pos, lSGs, rot_inv=None,
                    rotate_lights=False, angle_decay_fac=0.4, shadow_pow_fac=2, self_shadow_pow_fac=0.1,
                    want=("factor", "decay")):
    """(factor (P) or None, decay (P,L) or None) from torch ops, in the dtype and
    on the device of `pts`.  rotate_lights: apply rot_inv to the light axes too
    (the decay call of the reference does, its factor call does not)."""
    dt, dev = pts.dtype, pts.device
    c = lambda t: t.to(device=dev, dtype=dt)  # noqa: E731
    coeff, components, mean, fh_tab, lSGs, model_pos = (c(t) for t in (coeff, components, mean, fh_tab, lSGs, model_pos))
    G, C = coeff.shape[0], coeff.shape[-1]
    L = _lights_arg(lSGs)
    half_pi = math.pi / 2

    # per light: the components and the mean at the light's direction, the table row, fh_n
    axes = lSGs[:, :3]
    if rotate_lights and rot_inv is not None:
        axes = (c(rot_inv) @ axes.T).T
    phi = torch.arccos(axes[:, 1])
    theta = torch.arctan2(axes[:, 2], axes[:, 0])
    lx, ly = theta / math.pi, phi / math.pi * 2 - 1
    comp_s = _sample2d(components.reshape(C, *components.shape[-2:]), lx, ly)      # C,L
    mean_s = _sample2d(mean.reshape(1, *mean.shape[-2:]), lx, ly)                  # 1,L
    lam, amp = lSGs[:, 3], lSGs[:, 4:]
    row = (torch.log10(torch.abs(lam + 1e-6)) - 1.5) / 2.5
    exp_term = 1.0 - torch.exp(-1.0 * lam)
    fh_n = 2 * math.pi / lam * exp_term                                            # L

    # per point: the normalised position, the angle correction, the PCA vector
    m = pts.reshape(-1, 3) - model_pos.reshape(1, 3)
    if rot_inv is not None:
        m = (c(rot_inv) @ m.T).T
    q = m / scale / vol_range
    dis = torch.linalg.vector_norm(q, dim=-1, keepdim=True).clip(min=1)
    q = q / dis
    raw = torch.asin(torch.tensor([1.0 / vol_range], dtype=dt, device=dev))
    delta = (raw - torch.asin(1.0 / (dis * vol_range))) * angle_decay_fac          # P,1
    vol = coeff.permute(3, 2, 1, 0).unsqueeze(0)                                   # 1,C,D,H,W: x -> the first stored axis
    pca = F.grid_sample(vol, q.reshape(1, 1, 1, -1, 3), mode="bilinear", padding_mode="border", align_corners=True)
    pca = pca.reshape(C, -1).T                                                     # P,C

    # per pair
    ssdf = torch.clip(pca @ comp_s + mean_s + delta, -half_pi, half_pi)            # P,L
    grid = torch.stack([ssdf / half_pi, row.unsqueeze(0).expand_as(ssdf)], -1).unsqueeze(0)
    fh = F.grid_sample(fh_tab.reshape(1, 1, *fh_tab.shape[-2:]), grid, mode="bilinear", padding_mode="border",
                       align_corners=False)[0, 0]                                  # P,L
    factor = decay = None
    if "decay" in want:
        decay = torch.pow(torch.abs(fh / fh_n.unsqueeze(0)).clip(0, 1), self_shadow_pow_fac)
    if "factor" in want:
        inte_l = (2 * math.pi * (amp / lam.unsqueeze(1)) * exp_term.unsqueeze(1)).sum(0, keepdim=True)  # 1,3
        f = torch.abs((fh @ amp) / inte_l).clip(0, 1)
        factor = torch.pow(LUMA[0] * f[:, 0] + LUMA[1] * f[:, 1] + LUMA[2] * f[:, 2], shadow_pow_fac)
    return factor, decay


def blur_weights(dtype=torch.float64):
    """The 1-D weights of torchvision's gaussian_blur(kernel 3): exp(-0.5 (x/0.8)^2), x = -1, 0, 1, normalised"""
    w = torch.exp(-0.5 * (torch.tensor([-1.0, 0.0, 1.0], dtype=dtype) / BLUR_SIGMA) ** 2)
    return w / w.sum()


@torch.no_grad()
def shadow_apply_torch(frame_rgb, factor, H, W):
    """rgb * blur3x3(factor) from torch ops (reflect padding, the outer product of the 1-D weights)"""
    dt = frame_rgb.dtype
    w = blur_weights(dt).to(frame_rgb.device)
    k = (w[:, None] * w[None, :]).reshape(1, 1, 3, 3)
    f = F.pad(factor.reshape(1, 1, H, W).to(dt), (1, 1, 1, 1), mode="reflect")
    return frame_rgb.reshape(H, W, 3) * F.conv2d(f, k).reshape(H, W, 1)


@torch.no_grad()
def shadow_apply(frame_rgb, factor, H, W, out=None):
    """ssdf_shadow's last step (main.py:503-519): frame_rgb (H,W,3) times the 3 x 3
    Gaussian blur of factor (H,W) -> a new (H,W,3) tensor (or `out`); frame_rgb
    is left as it is.  H, W >= 2 (reflect padding)."""
    H, W = int(H), int(W)
    if H < 2 or W < 2 or H * W >= 2 ** 31:
        raise ValueError(f"the blur's reflect padding needs a frame of at least 2 x 2, got {H} x {W}")
    n = H * W
    if isinstance(frame_rgb, torch.Tensor) and not frame_rgb.is_cuda:
        for name, t, m in (("frame_rgb", frame_rgb, 3 * n), ("factor", factor, n), ("out", out, 3 * n)):
            if t is None and name == "out":
                continue
            if not isinstance(t, torch.Tensor) or t.is_cuda or not t.is_floating_point() or t.numel() != m:
                raise ValueError(f"{name} must be a floating-point CPU tensor of {m} values for a {H} x {W} frame, "
                                 f"got {tuple(getattr(t, 'shape', ()))}")
        res = shadow_apply_torch(frame_rgb, factor, H, W)
        if out is not None:
            out.copy_(res.reshape(out.shape))
            return out.view(H, W, 3)
        return res
    _arg("frame_rgb", frame_rgb, torch.float32, 3 * n, f"(H,W,3) = ({H},{W},3)")
    _arg("factor", factor, torch.float32, n, f"(H,W) = ({H},{W})")
    if out is None:
        out = torch.empty(n, 3, dtype=torch.float32, device=frame_rgb.device)
    _arg("out", out, torch.float32, 3 * n, f"(H,W,3) = ({H},{W},3)")
    if out.data_ptr() == frame_rgb.data_ptr():
        raise ValueError("out must not be frame_rgb: the unshadowed frame is kept")
    vren.kernels().ngp_shadow_apply(frame_rgb, factor, H, W, out, vren._stream())
    return out.view(H, W, 3)


class SGShadow:
    """The app's SGShadow over tensors it has loaded: coeff (G,G,G,C),
    components (C,envH,envW), mean (envH,envW) or (1,envH,envW), fh_tab
    (n_lambda,n_theta).  Device tensors (contiguous fp32) run the kernels; CPU
    tensors take sg_shadow_torch.  delta_angle_decay_fac, delta_shadow_fac and
    delta_self_shadow_fac are the reference's mutable factors (the app's sliders
    write them, main.py:1106-1110): every call reads them anew."""

    def __init__(self, coeff, components, mean, fh_tab, vol_range, angle_decay_fac=0.4, shadow_pow_fac=2,
                 self_shadow_pow_fac=0.1):
        for name, t in (("coeff", coeff), ("components", components), ("mean", mean), ("fh_tab", fh_tab)):
            if not isinstance(t, torch.Tensor) or not t.is_floating_point():
                raise ValueError(f"{name} must be a floating-point tensor")
        if coeff.dim() != 4 or not (coeff.shape[0] == coeff.shape[1] == coeff.shape[2]) or coeff.shape[0] < 2:
            raise ValueError(f"coeff must be (G,G,G,C) with G >= 2, got {tuple(coeff.shape)}")
        G, C = coeff.shape[0], coeff.shape[3]
        if not 1 <= C <= MAX_COMPONENTS:
            raise ValueError(f"coeff holds {C} components per cell: 1 .. {MAX_COMPONENTS} are supported")
        if components.dim() != 3 or components.shape[0] != C:
            raise ValueError(f"components must be (C,envH,envW) with C = {C}, got {tuple(components.shape)}")
        envH, envW = components.shape[1:]
        if mean.numel() != envH * envW or tuple(mean.shape[-2:]) != (envH, envW):
            raise ValueError(f"mean must be (envH,envW) = ({envH},{envW}), got {tuple(mean.shape)}")
        if fh_tab.dim() != 2 or fh_tab.numel() < 1:
            raise ValueError(f"fh_tab must be (n_lambda,n_theta), got {tuple(fh_tab.shape)}")
        if not float(vol_range) > 0:
            raise ValueError(f"vol_range must be positive, got {vol_range}")
        self.is_cuda = coeff.is_cuda
        if self.is_cuda:
            for name, t in (("coeff", coeff), ("components", components), ("mean", mean), ("fh_tab", fh_tab)):
                _arg(name, t, torch.float32)
        self.coeff, self.components, self.mean, self.fh_tab = coeff, components, mean, fh_tab
        self.grid_size, self.ncomponents, self.envH, self.envW = G, C, envH, envW
        self.vol_range = float(vol_range)
        self.delta_angle_decay_fac = angle_decay_fac
        self.delta_shadow_fac = shadow_pow_fac
        self.delta_self_shadow_fac = self_shadow_pow_fac
        self._ws = {}  # L -> the light workspace (L * LIGHT_WORDS + 4 floats)

    # ------------------------------------------------------------ pieces
    def _lights(self, lSGs, rot_inv):
        """The per-light pre-pass into the workspace of this L (rot_inv: rotate the axes first, or None)"""
        L = _lights_arg(lSGs)
        _arg("lSGs", lSGs, torch.float32)
        ws = self._ws.get(L)
        if ws is None:
            if len(self._ws) >= 8:
                self._ws.clear()
            ws = self._ws[L] = torch.zeros(L * LIGHT_WORDS + 4, dtype=torch.float32, device=self.coeff.device)
        vren.kernels().ngp_sg_shadow_lights(lSGs, L, rot_inv, self.components, self.mean, self.ncomponents, self.envH,
                                            self.envW, ws, vren._stream())
        return ws, L

    def _tensor(self, name, x, numel=None, shape_text=None):
        """One tensor argument: on the device a contiguous fp32 CUDA tensor (shading._arg), on the CPU path a
        floating-point CPU tensor; every failure a ValueError"""
        if self.is_cuda:
            return _arg(name, x, torch.float32, numel, shape_text)
        if not isinstance(x, torch.Tensor) or x.is_cuda or not x.is_floating_point():
            raise ValueError(f"{name} must be a floating-point CPU tensor (this SGShadow holds CPU tensors)")
        if numel is not None and x.numel() != numel:
            raise ValueError(f"{name} must be {shape_text}, got {tuple(x.shape)}")
        return x

    def _common(self, scale, model_pos, rot_inv):
        self._tensor("model_pos", model_pos, 3, "(3)")
        if rot_inv is not None:
            self._tensor("rot_inv", rot_inv, 9, "(3,3)")
        if not float(scale) > 0:
            raise ValueError(f"scale must be positive, got {scale}")

    def _point_args(self, scale, pts, model_pos, lSGs, rot_inv):
        """Every check of a point-list call, before anything is allocated or launched -> (P, L)"""
        self._tensor("pts", pts)
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"pts must be (P,3), got {tuple(pts.shape)}")
        self._common(scale, model_pos, rot_inv)
        L = _lights_arg(lSGs)
        self._tensor("lSGs", lSGs)
        return pts.shape[0], L

    def _out(self, name, out, shape, text):
        """`out` checked against `shape`, or a new tensor of it"""
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.coeff.device)
        n = 1
        for v in shape:
            n *= v
        return self._tensor(name, out, n, text)

    def _volume_args(self, ws, L):
        return (self.coeff, self.grid_size, self.ncomponents, self.vol_range, float(self.delta_angle_decay_fac), ws, L,
                self.fh_tab, self.fh_tab.shape[0], self.fh_tab.shape[1])

    def _points(self, scale, pts, model_pos, lSGs, rot_inv, rotate_lights, factor, decay):
        """The launches of a checked call (factor / decay: checked outputs or None)"""
        ws, L = self._lights(lSGs, rot_inv if rotate_lights else None)
        P = pts.shape[0]
        if P == 0:  # (an empty tensor has no address to hand over)
            return
        vren.kernels().ngp_sg_shadow_points(pts, P, model_pos, rot_inv, float(scale), *self._volume_args(ws, L),
                                            float(self.delta_shadow_fac), float(self.delta_self_shadow_fac), factor,
                                            decay, vren._stream())

    def _torch(self, scale, pts, model_pos, lSGs, rot_inv, rotate_lights, want):
        return sg_shadow_torch(self.coeff, self.components, self.mean, self.fh_tab, self.vol_range, float(scale), pts,
                               model_pos, lSGs, rot_inv, rotate_lights, self.delta_angle_decay_fac,
                               self.delta_shadow_fac, self.delta_self_shadow_fac, want)

    # --------------------------------------------------------------- API
    @torch.no_grad()
    def calc_shadow_factor(self, scale, pts, model_pos, lSGs, rot_inv=None, out=None):
        """The cast-shadow factor of every point -> (P).  scale: the model's radius; pts (P,3); model_pos (3);
        lSGs (L,7) with axes ALREADY rotated by rot_inv where one is given (main.py:496-499); rot_inv (3,3)
        rotates the points only."""
        P, L = self._point_args(scale, pts, model_pos, lSGs, rot_inv)
        if not self.is_cuda:
            res = self._torch(scale, pts, model_pos, lSGs, rot_inv, False, ("factor",))[0]
            return res if out is None else self._out("out", out, (P,), f"(P) = ({P})").copy_(res.reshape(out.shape))
        out = self._out("out", out, (P,), f"(P) = ({P})")
        self._points(scale, pts, model_pos, lSGs, rot_inv, False, out, None)
        return out

    @torch.no_grad()
    def self_shadow_decay(self, scale, pts, model_pos, lSGs, rot_inv=None, out=None):
        """The factor on every light's amplitude at every point -> (P,L), what shading.sg_shade takes as
        `decay`.  rot_inv rotates the points and the light axes (the lights are given unrotated)."""
        P, L = self._point_args(scale, pts, model_pos, lSGs, rot_inv)
        if not self.is_cuda:
            res = self._torch(scale, pts, model_pos, lSGs, rot_inv, True, ("decay",))[1]
            return res if out is None else self._out("out", out, (P, L), f"(P,L) = ({P},{L})").copy_(
                res.reshape(out.shape))
        out = self._out("out", out, (P, L), f"(P,L) = ({P},{L})")
        self._points(scale, pts, model_pos, lSGs, rot_inv, True, None, out)
        return out

    @torch.no_grad()
    def factor_and_decay(self, scale, pts, model_pos, lSGs, rot_inv=None, rotate_lights=False):
        """Both results of one launch over the same lights -> ((P), (P,L)); rotate_lights as sg_shadow_torch's"""
        P, L = self._point_args(scale, pts, model_pos, lSGs, rot_inv)
        if not self.is_cuda:
            return self._torch(scale, pts, model_pos, lSGs, rot_inv, rotate_lights, ("factor", "decay"))
        factor, decay = self._out("factor", None, (P,), ""), self._out("decay", None, (P, L), "")
        self._points(scale, pts, model_pos, lSGs, rot_inv, rotate_lights, factor, decay)
        return factor, decay

    @torch.no_grad()
    def calc_self_shadow_light_dacay(self, scale, pts, model_pos, lSGs, rot_inv=None):
        """The reference's call (its spelling): the lights repeated per point with their amplitudes decayed ->
        (P,L,7).  A (P,L,7) temporary: sg_shade takes the (P,L) decay of self_shadow_decay directly."""
        decay = self.self_shadow_decay(scale, pts, model_pos, lSGs, rot_inv)
        P, L = decay.shape
        lights = lSGs.to(decay.dtype)
        return torch.cat([lights[None, :, :4].expand(P, L, 4), lights[None, :, 4:] * decay[:, :, None]], -1)

    @torch.no_grad()
    def frame_decay(self, H, W, directions, c2w, bbox, obj_depth, scale, model_pos, lSGs, out, rot_inv=None):
        """The decay rows of a frame's covered pixels (inside bbox, obj_depth > 1e-6), at the points
        c2w[:,3] + obj_depth * normalize(ray direction) (main.py:551-561), into out (H*W,L); other rows keep
        their values.  Device tensors only."""
        if not self.is_cuda:
            raise ValueError("frame_decay runs on the device: build SGShadow from CUDA tensors")
        H, W = int(H), int(W)
        if H < 1 or W < 1 or H * W >= 2 ** 31:
            raise ValueError(f"bad frame size {H} x {W}")
        n = H * W
        _arg("directions", directions, torch.float32, 3 * n, f"(H*W,3) = ({n},3)")
        _arg("c2w", c2w, torch.float32, 12, "(3,4)")
        _arg("obj_depth", obj_depth, torch.float32, n, f"(H,W) = ({H},{W})")
        self._common(scale, model_pos, rot_inv)
        bbox = _bbox_tensor(bbox, H, W, self.coeff.device)
        ws, L = self._lights(lSGs, rot_inv)
        _arg("out", out, torch.float32, n * L, f"(H*W,L) = ({n},{L})")
        vren.kernels().ngp_sg_shadow_frame_decay(bbox, H, W, directions, c2w, obj_depth, model_pos, rot_inv,
                                                 float(scale), *self._volume_args(ws, L),
                                                 float(self.delta_self_shadow_fac), out, vren._stream())
        return out
