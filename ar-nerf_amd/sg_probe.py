"""SG light probes: from the cube map rendered at a scene point to the
(axis, sharpness, rgb) lights that shading.sg_shade and sg_shadow.SGShadow
consume -- what the reference app's NGP_Insertor.generate_probe(pt,
SH_probe=False) (insert/main.py:306-352) does after its render:
cubemap2env_map (insert/render_utils.py:117-189), EnvOptim.eval
(insert/envfit.py:275-297) and trans_raw_sg -- as HIP launches
(csrc/sgfit.hip).

env_dirs         the equirectangular directions of SG2Envmap / cubemap2env_map
cubemap_sample   the cube-map lookup along any directions (no blur, no roughness)
cubemap2env_map  the (H,W,3) env map of a cube map
SG2Envmap        the (H,W,3) env map of a set of raw lights
parse_raw_sg, trans_raw_sg   the raw rows normalised (a copy / in place)
EnvOptim         the warm-started Adam fit: lgtSGs, N_iter, eval(im)
sg_fit_torch     the same optimisation from torch autograd and
                 torch.optim.Adam over the (pixels, L, 3) tensors, as the
                 reference formulates it: the path for CPU tensors and other
                 dtypes, and the baseline scripts/bench_sg_probe.py times the
                 kernels against
probes.sg_probe renders the cube map and runs the chain.

Not here: SGFittingNet / EnvTrainer, upper_hemi, the blurred cube-map stack of
spec_shade (rough / blur_cm), gen_probe_HDR_mapping, visualisation.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import vren
from capi import C as _C
from shading import _arg

TINY_NUMBER = 1e-8
MAX_LIGHTS = _C["NGP_SG_FIT_MAX_LIGHTS"]
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
SEL_MAP = (2, 4, 0)          # axis of the largest |component| -> the face of its positive side
SEL_MASK = ((1, 2), (0, 2), (0, 1))

_DIRS = {}


def env_dirs(H, W, device=None):
    """The (H*W,3) fp32 directions of the reference's equirectangular map (envfit.py:30-42,
    render_utils.py:172-185): phi = linspace(0, pi, H) down the rows, theta = linspace(-pi/2, 3pi/2, W) along
    them, (cos theta sin phi, cos phi, sin theta sin phi).  Built with torch ops on the CPU (the reference's
    values bit for bit), cached per shape and device."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"bad env map size {H} x {W}")
    dev = torch.device("cpu" if device is None else device)
    key = (H, W, str(dev))
    d = _DIRS.get(key)
    if d is None:
        phi, theta = torch.meshgrid([torch.linspace(0., math.pi, H, dtype=torch.float32),
                                     torch.linspace(-0.5 * math.pi, 1.5 * math.pi, W, dtype=torch.float32)],
                                    indexing="ij")
        d = torch.stack([torch.cos(theta) * torch.sin(phi), torch.cos(phi), torch.sin(theta) * torch.sin(phi)], -1)
        if len(_DIRS) >= 16:
            _DIRS.clear()
        d = _DIRS[key] = d.reshape(-1, 3).contiguous().to(dev)
    return d


def _on_device(*tensors):
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _float_tensor(name, x, last=None):
    if not isinstance(x, torch.Tensor) or not x.is_floating_point():
        raise ValueError(f"{name} must be a floating-point tensor")
    if last is not None and (x.dim() < 1 or x.shape[-1] != last):
        raise ValueError(f"{name} must end in a dimension of {last}, got {tuple(x.shape)}")
    return x


def _lights_arg(lgtSGs):
    _float_tensor("lgtSGs", lgtSGs)
    if lgtSGs.dim() != 2 or lgtSGs.shape[1] != 7 or not 1 <= lgtSGs.shape[0] <= MAX_LIGHTS:
        raise ValueError(f"lgtSGs must be (L,7) with 1 <= L <= {MAX_LIGHTS}, got {tuple(lgtSGs.shape)}")
    return lgtSGs.shape[0]


# ------------------------------------------------------------------ raw rows
def parse_raw_sg(sg):
    """envfit.py:17-21 -> (lobes (...,3), lambdas (...,1), mus (...,3))"""
    lobes = sg[..., :3] / (torch.norm(sg[..., :3], dim=-1, keepdim=True) + TINY_NUMBER)
    return lobes, torch.abs(sg[..., 3:4]), torch.abs(sg[..., -3:])


def trans_raw_sg(sg):
    """envfit.py:23-27: the rows normalised IN PLACE (unit axis, |sharpness|, |amplitude|); returns sg"""
    sg[..., :3] = sg[..., :3] / (torch.norm(sg[..., :3], dim=-1, keepdim=True) + TINY_NUMBER)
    sg[..., 3:4] = torch.abs(sg[..., 3:4])
    sg[..., -3:] = torch.abs(sg[..., -3:])
    return sg


# ------------------------------------------------------------ torch formulation
def cubemap_sample_torch(cubemap, dirs, res):
    """The lookup from torch ops (grid_sample), in the dtype and on the device of `dirs`"""
    dirs = dirs.reshape(-1, 3)
    cm = cubemap.to(device=dirs.device, dtype=dirs.dtype).reshape(6, res, res, 3)
    rgbs = torch.ones_like(dirs)
    max_ax, max_id = torch.max(torch.abs(dirs), -1)
    q = dirs / max_ax.unsqueeze(-1)
    for axis in range(3):
        sel = q[:, axis]
        for face, m in ((SEL_MAP[axis], (max_id == axis) & (sel > 0)), (SEL_MAP[axis] + 1, (max_id == axis) & (sel < 0))):
            if not bool(m.any()):
                continue
            u, v = q[m, SEL_MASK[axis][0]], q[m, SEL_MASK[axis][1]]
            grid = torch.stack([v, u], -1).reshape(1, 1, -1, 2)      # x walks the second index, y the first
            img = cm[face].permute(2, 0, 1).unsqueeze(0)
            rgbs[m] = F.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0].T
    return rgbs


def sg_envmap_torch(lgtSGs, dirs):
    """sum_l mu_l exp(lam_l (v . a_l - 1)) over the (P,L,3) tensor -> (P,3) (envfit.py:43-55)"""
    lobes, lambdas, mus = parse_raw_sg(lgtSGs.unsqueeze(0))
    dots = torch.sum(dirs.unsqueeze(-2) * lobes, dim=-1, keepdim=True)
    return torch.sum(mus * torch.exp(lambdas * (dots - 1.)), dim=-2)


def sg_fit_torch(lgtSGs, target, dirs, n_iter, lr=1e-1, optimizer=None, losses=None):
    """n_iter steps of torch.optim.Adam on mse(SG2Envmap(lgtSGs), target), as EnvOptim.eval writes them
    (envfit.py:284-297).  lgtSGs: a leaf tensor (L,7) that requires grad, updated in place; target (P,3) or
    (H,W,3); dirs (P,3); any device and dtype.  optimizer: the Adam object to go on with (warm state), or None
    for a fresh one.  losses: a list that receives each iteration's loss (detached tensors).
    Returns (lgtSGs.detach(), optimizer)."""
    if optimizer is None:
        optimizer = torch.optim.Adam([lgtSGs], lr=lr, betas=BETAS, eps=ADAM_EPS)
    target = target.reshape(-1, 3)
    for _ in range(int(n_iter)):
        optimizer.zero_grad()
        loss = F.mse_loss(sg_envmap_torch(lgtSGs, dirs), target)
        loss.backward()
        optimizer.step()
        if losses is not None:
            losses.append(loss.detach())
    return lgtSGs.detach(), optimizer


# --------------------------------------------------------------------- API
@torch.no_grad()
def cubemap_sample(cubemap, dirs, res, rough=None, blur_cm=False):
    """render_utils.py:117-167 without blur: cubemap (6*res*res,3) (faces +z, -z, +x, -x, +y, -y), dirs
    (...,3) -> (n,3).  Device fp32 tensors run the kernel, anything else grid_sample."""
    if rough is not None or blur_cm:
        raise ValueError("the roughness-blurred cube-map stack (rough / blur_cm) belongs to the SH path: not supported")
    res = int(res)
    _float_tensor("cubemap", cubemap)
    _float_tensor("dirs", dirs, 3)
    if res < 1 or cubemap.numel() != 18 * res * res:
        raise ValueError(f"cubemap must hold 6 x {res} x {res} x 3 values, got {tuple(cubemap.shape)}")
    if not _on_device(cubemap, dirs):
        if cubemap.device != dirs.device or cubemap.dtype != dirs.dtype:
            raise ValueError("cubemap and dirs must share a device and a dtype")
        return cubemap_sample_torch(cubemap, dirs, res)
    _arg("cubemap", cubemap, torch.float32)
    _arg("dirs", dirs, torch.float32)
    n = dirs.numel() // 3
    out = torch.empty(n, 3, dtype=torch.float32, device=dirs.device)
    if n:
        vren.kernels().ngp_cubemap_sample(cubemap, res, dirs, n, out, vren._stream())
    return out


@torch.no_grad()
def cubemap2env_map(cubemap, cm_resol, H, W):
    """render_utils.py:172-189: the (H,W,3) equirectangular map of a cube map"""
    _float_tensor("cubemap", cubemap)
    return cubemap_sample(cubemap, env_dirs(H, W, cubemap.device).to(cubemap.dtype), cm_resol).reshape(int(H), int(W), 3)


@torch.no_grad()
def SG2Envmap(lgtSGs, H, W, upper_hemi=False):
    """envfit.py:30-56: the (H,W,3) env map of raw lights (L,7)"""
    if upper_hemi:
        raise ValueError("upper_hemi is not supported")
    L = _lights_arg(lgtSGs)
    H, W = int(H), int(W)
    dirs = env_dirs(H, W, lgtSGs.device)
    if not _on_device(lgtSGs):
        return sg_envmap_torch(lgtSGs, dirs.to(lgtSGs.dtype)).reshape(H, W, 3)
    _arg("lgtSGs", lgtSGs, torch.float32)
    out = torch.empty(H * W, 3, dtype=torch.float32, device=lgtSGs.device)
    vren.kernels().ngp_sg_envmap(lgtSGs, L, dirs, H * W, out, vren._stream())
    return out.view(H, W, 3)


class EnvOptim:
    """envfit.py:275-297 over device tensors: lgtSGs (L,7), the raw lights (lobe, sharpness, amplitude), drawn
    as randn with the sharpness column times 100 (on the CPU under `generator`); eval(im) runs N_iter Adam
    steps at `lr` on mse(SG2Envmap(lgtSGs), im) and returns lgtSGs (the live tensor, detached, as the
    reference does).  The Adam moments and the step count persist across eval calls (a warm start) until
    reset().  Also: last_grad (L,7), the gradient of the last iteration; losses (N_iter), the loss before
    each step of the last eval -- device tensors, no synchronisation.

    On a CUDA device with fp32 images the iterations are kernel launches (two each); a CPU object (device
    None / 'cpu'), or an image of another dtype, runs sg_fit_torch on a parameter of the image's dtype that
    is kept between calls; an object that has taken that path stays on it until reset()."""

    def __init__(self, numLgtSGs=32, N_iter=25, lr=1e-1, generator=None, device=None):
        L = int(numLgtSGs)
        if not 1 <= L <= MAX_LIGHTS:
            raise ValueError(f"numLgtSGs must be 1 .. {MAX_LIGHTS}, got {numLgtSGs}")
        self.device = torch.device("cpu" if device is None else device)
        self.N_iter, self.lr = N_iter, float(lr)
        init = torch.randn(L, 7, generator=generator)
        init[..., 3:4] *= 100.
        self.reset(init)

    def reset(self, lgtSGs=None):
        """Forget the Adam state (moments and step count); lgtSGs: new raw lights (L,7), or None to keep them"""
        if lgtSGs is not None:
            L = _lights_arg(lgtSGs)
            self.lgtSGs = lgtSGs.detach().to(device=self.device, dtype=torch.float32).contiguous().clone()
        L = self.lgtSGs.shape[0]
        dev = self.device
        self.exp_avg = torch.zeros(L, 7, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(L, 7, dtype=torch.float32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.last_grad = torch.zeros(L, 7, dtype=torch.float32, device=dev)
        self.losses = torch.zeros(0, dtype=torch.float32, device=dev)
        self._ws = None
        self._torch = None       # (parameter, optimizer) of the torch path

    @property
    def numLgtSGs(self):
        return self.lgtSGs.shape[0]

    def _eval_torch(self, im, n_iter, H, W):
        if self._torch is None or self._torch[0].dtype != im.dtype or self._torch[0].device != im.device:
            p = self.lgtSGs.detach().to(device=im.device, dtype=im.dtype).clone().requires_grad_(True)
            self._torch = (p, torch.optim.Adam([p], lr=self.lr, betas=BETAS, eps=ADAM_EPS))
        p, opt = self._torch
        for g in opt.param_groups:
            g["lr"] = self.lr
        losses = []
        with torch.enable_grad():
            sg_fit_torch(p, im, env_dirs(H, W, im.device).to(im.dtype), n_iter, self.lr, opt, losses)
        if n_iter:
            self.last_grad = p.grad.detach().clone()
        self.losses = torch.stack(losses) if losses else torch.zeros(0, dtype=im.dtype, device=im.device)
        self.lgtSGs = p.detach()
        return self.lgtSGs

    @torch.no_grad()
    def eval(self, im):
        """im (H,W,3), non-negative radiance -> lgtSGs (L,7) after N_iter more Adam steps"""
        _float_tensor("im", im, 3)
        if im.dim() != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError(f"im must be (H,W,3), got {tuple(im.shape)}")
        n_iter = int(self.N_iter)
        if n_iter < 0:
            raise ValueError(f"N_iter must not be negative, got {self.N_iter}")
        H, W = im.shape[:2]
        if not (self.device.type == "cuda" and _on_device(im)) or self._torch is not None:
            return self._eval_torch(im, n_iter, H, W)
        _arg("im", im, torch.float32)
        P, L = H * W, self.lgtSGs.shape[0]
        K = vren.kernels()
        nbytes = K.ngp_sg_fit_workspace_bytes(P, L)
        if nbytes <= 0:
            raise ValueError(f"an env map of {H} x {W} pixels is out of range")
        if self._ws is None or self._ws.numel() * 8 < nbytes:
            self._ws = torch.empty(nbytes // 8, dtype=torch.float64, device=im.device)
        self.losses = torch.zeros(n_iter, dtype=torch.float32, device=im.device)
        if n_iter:
            K.ngp_sg_fit(self.lgtSGs, L, env_dirs(H, W, im.device), im, P, n_iter, self.lr, self.exp_avg,
                         self.exp_avg_sq, self.step, self._ws, self.last_grad, self.losses, vren._stream())
        return self.lgtSGs
