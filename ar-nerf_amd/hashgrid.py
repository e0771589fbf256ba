"""Hash-grid + fused-MLP field on MI355X (replaces tinycudann as used by
models/networks.py:37-78 of the reference).

Parameters follow tcnn's flat-params model, but as ONE fp32 master buffer
    params = [W1 64x32 | W2 16x64 | W3 64x32 | W4 64x64 | W5 16x64 | table (entries x 2)]
(W* row-major [out][in]; W1,W2 = xyz_encoder's MLP, W3..W5 = rgb_net, W5
rows 3..15 padding) and an fp16 shadow of the same layout that the kernels
read (tcnn keeps the same fp32-master / fp16-compute split).  The shadow is
refreshed lazily whenever the master's version counter changes.

All compute goes through libngp_amd.so; nothing here runs on the CPU.
"""
from __future__ import annotations

import ctypes  # noqa: F401  (ctypes, c_float, _ptr: names tests and diagnostics reach through this module)
import math
from ctypes import c_float, c_void_p  # noqa: F401

import numpy as np
import torch

import vren
from capi import C, ngp_hashgrid_t

N_LEVELS = C["NGP_MAX_LEVELS"]
# colour-output modes of the field kernels
RGB_SIGMOID, RGB_NONE, RGB_LEAKY_RELU, RGB_RELU = (C["NGP_RGB_" + m] for m in ("SIGMOID", "NONE", "LEAKY_RELU", "RELU"))
MLP_PARAMS = C["NGP_MLP_PARAMS"]
OW = {"W1": (0, 64, 32), "W2": (2048, 16, 64), "W3": (3072, 64, 32), "W4": (5120, 64, 64), "W5": (9216, 16, 64)}

_lib = vren.lib  # the one loader, under the name this module's callers use (the raw view)
_K = vren.kernels  # the checked view this module calls through


def _ptr(t):  # (raw-view callers; product code passes tensors)
    return c_void_p(t.data_ptr()) if t is not None else None


class HashGrid:
    """Level table for the reference's encoding config (models/networks.py:33-49)."""

    def __init__(self, scale: float, n_levels=16, log2_T=19, base_resolution=16, per_level_scale=None):
        if per_level_scale is None:
            per_level_scale = float(np.exp(np.log(2048 * scale / base_resolution) / (n_levels - 1)))
        self.scale, self.n_levels, self.log2_T = scale, n_levels, log2_T
        self.base_resolution, self.per_level_scale = base_resolution, per_level_scale
        d = ngp_hashgrid_t()
        d.n_levels = n_levels
        self.n_entries = int(_K().ngp_hashgrid_levels(n_levels, log2_T, base_resolution, per_level_scale, d.scales,
                                                      d.res, d.offsets, d.sizes))
        for i in range(3):
            d.xyz_min[i] = -scale
            d.xyz_max[i] = scale
        self.desc = d

    @property
    def resolutions(self):
        return list(self.desc.res)[: self.n_levels]

    @property
    def offsets(self):
        return list(self.desc.offsets)[: self.n_levels + 1]

    @property
    def n_params(self):
        return MLP_PARAMS + 2 * self.n_entries


def init_params(grid: HashGrid, seed=4, table_init=1e-4, device="cuda"):
    """tcnn init: hash table U(-1e-4, 1e-4); MLPs Xavier-uniform per matrix."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for name in ("W1", "W2", "W3", "W4", "W5"):
        _, out_d, in_d = OW[name]
        a = math.sqrt(6.0 / (in_d + out_d))
        parts.append((torch.rand(out_d * in_d, generator=g) * 2 - 1) * a)
    parts.append((torch.rand(2 * grid.n_entries, generator=g) * 2 - 1) * table_init)
    return torch.cat(parts).to(device)


def _check(x, name, dtype, numel=None):
    vren._check(name, x, dtype)
    if numel is not None and x.numel() != numel:
        raise RuntimeError(f"{name} must have {numel} elements, got {x.numel()}")


def field_forward(xyzs, dirs, grid: HashGrid, params16, save_enc=True, n_dev=None, want_h=False, rgb_act=0):
    """Fused NGP.forward (models/networks.py:133-146) -> sigmas (n), rgbs (n,3), enc (n,32) fp16 | None, h | None
    rgb_act: the colour-output mode RGB_* (networks.py:152-157)."""
    n = xyzs.shape[0]
    dev = xyzs.device
    _check(xyzs, "xyzs", torch.float32); _check(dirs, "dirs", torch.float32)
    _check(params16, "params16", torch.float16, grid.n_params)
    sig = torch.empty(n, device=dev)
    rgb = torch.empty(n, 3, device=dev)
    enc = torch.empty(n, 32, dtype=torch.float16, device=dev) if save_enc else None
    h = torch.empty(n, 16, dtype=torch.float16, device=dev) if want_h else None
    _K().ngp_field_forward_act(xyzs, dirs, n, n_dev, grid.desc, params16[MLP_PARAMS:], params16, sig, rgb, enc, h,
                               int(rgb_act), vren._stream())
    return sig, rgb, enc, h


def density_forward(xyzs, grid: HashGrid, params16, want_h=False, n_dev=None):
    """NGP.density (models/networks.py:95-108) -> sigmas (n), h (n,16) fp16 | None"""
    n = xyzs.shape[0]
    _check(xyzs, "xyzs", torch.float32)
    _check(params16, "params16", torch.float16, grid.n_params)
    sig = torch.empty(n, device=xyzs.device)
    h = torch.empty(n, 16, dtype=torch.float16, device=xyzs.device) if want_h else None
    _K().ngp_density_forward(xyzs, n, n_dev, grid.desc, params16[MLP_PARAMS:], params16, sig, h, vren._stream())
    return sig, h


def density_input_grad(xyzs, grid: HashGrid, params16, dL_dsigma=None):
    """dL/dx (n,3) of NGP.density through hash grid + density MLP + TruncExp
    (dL_dsigma None = ones: d sigma / d x, render_surface_normal)."""
    n = xyzs.shape[0]
    _check(xyzs, "xyzs", torch.float32)
    _check(params16, "params16", torch.float16, grid.n_params)
    if dL_dsigma is not None:
        _check(dL_dsigma, "dL_dsigma", torch.float32)
    out = torch.empty(n, 3, device=xyzs.device)
    _K().ngp_density_input_grad(xyzs, n, grid.desc, params16[MLP_PARAMS:], params16, dL_dsigma, out, vren._stream())
    return out


def field_input_grad(xyzs, dirs, grid: HashGrid, params16, enc, dL_drgb, denc, rgb_act=0, n_dev=None,
                     sample_idx=None, want_dirs=True):
    """Input gradients of field_forward over the listed rows (sample_idx (n) i32 with the count in n_dev,
    the list of ngp_gradient_rows; None: all rows) -> dL/dxyzs (n,3), dL/ddirs (n,3) | None, zero on the
    unlisted rows.  denc (n,32) f32: dL/d(encoding) as the MLP backward (ngp_field_backward_mlp_act)
    wrote it for the same list -- it carries dL/dsigma and the colour path through h.  want_dirs=False:
    the position part alone (dirs, enc, dL_drgb may be None)."""
    n = xyzs.shape[0]
    _check(xyzs, "xyzs", torch.float32)
    _check(params16, "params16", torch.float16, grid.n_params)
    _check(denc, "denc", torch.float32)
    if denc.numel() < 32 * (n if sample_idx is None else sample_idx.numel()):
        raise RuntimeError("denc must hold 32 floats per listed row")
    if sample_idx is not None:
        _check(sample_idx, "sample_idx", torch.int32)
        if n_dev is None:
            raise RuntimeError("sample_idx needs its count in n_dev")
    if want_dirs:
        _check(dirs, "dirs", torch.float32); _check(enc, "enc", torch.float16); _check(dL_drgb, "dL_drgbs", torch.float32)
        if dirs.numel() != 3 * n or enc.numel() != 32 * n or dL_drgb.numel() != 3 * n:
            raise RuntimeError("dirs (n,3), enc (n,32) and dL_drgbs (n,3) must match xyzs (n,3)")
    dx = torch.zeros(n, 3, device=xyzs.device)
    dd = torch.zeros(n, 3, device=xyzs.device) if want_dirs else None
    rows = n if sample_idx is None else sample_idx.numel()
    if not want_dirs:
        dirs = enc = dL_drgb = None
    _K().ngp_field_input_grad(xyzs, dirs, rows, n_dev, sample_idx, grid.desc, params16[MLP_PARAMS:], params16, enc,
                              dL_drgb, denc, int(rgb_act), dx, dd, vren._stream())
    return dx, dd


def field_backward(xyzs, dirs, grid: HashGrid, params16, enc, dL_dsig, dL_drgb, grad, n_dev=None, denc_ws=None,
                   rgb_act=0):
    """Accumulates dL/dparams (fp32, params layout) into `grad` (rgb_act: the forward's colour mode)."""
    n = xyzs.shape[0]
    _check(grad, "grad", torch.float32, grid.n_params)
    _check(enc, "enc", torch.float16)
    _check(dL_dsig, "dL_dsigmas", torch.float32); _check(dL_drgb, "dL_drgbs", torch.float32)
    if denc_ws is None:
        denc_ws = torch.empty(n, 32, device=xyzs.device)
    _K().ngp_field_backward_act(xyzs, dirs, n, n_dev, grid.desc, enc, params16, dL_dsig, dL_drgb, denc_ws, grad,
                                grad[MLP_PARAMS:], int(rgb_act), vren._stream())


BIN_LEVEL_LO, BIN_MERGE_HI = 8, 11  # the trainer's hybrid split on object scenes (trainer.NGPTrainer)
BIN_WS_SAMPLES = 1 << 20  # binned workspace: gradient-carrying samples it holds (the rest: atomic path, exact)
COARSE_REP, COARSE_REP_LEVELS = 8, 4  # the trainer's gradient replicas of the coarsest atomic levels
_bin_ws = {}
_rep_bufs = {}


def _binned_workspace(device):
    """The binned hash backward's workspace (ngp_hash_backward_binned_workspace(BIN_WS_SAMPLES) bytes),
    one per device, allocated on first use and reused by every drop-in backward."""
    ws = _bin_ws.get(device)
    if ws is None:
        nbytes = _K().ngp_hash_backward_binned_workspace(BIN_WS_SAMPLES)
        ws = _bin_ws[device] = torch.empty((nbytes + 255) // 256, 64, dtype=torch.int32, device=device)
    return ws


def _rep_buffer(grid, device):
    """Replicas of the coarse levels' gradient (ngp_hash_backward_levels_rep; zero between calls)."""
    key = (device, tuple(grid.offsets))
    rep = _rep_bufs.get(key)
    if rep is None:
        nrep = _K().ngp_hash_backward_rep_floats(grid.desc, COARSE_REP_LEVELS, COARSE_REP)
        rep = _rep_bufs[key] = torch.zeros(nrep, device=device)
    return rep


def field_backward_sparse(xyzs, dirs, grid: HashGrid, params16, enc, dL_dsig, dL_drgb, grad, rgb_act=0,
                          want_xyzs=False, want_dirs=False):
    """field_backward over the samples that carry gradient only, with the
    training step's hybrid hash backward: the rows with a nonzero dL/dsigma or
    dL/drgb are listed on the device (ngp_gradient_rows: no host sync) -- the
    compositing backward leaves every sample past its ray's termination at
    exact zero, and a zero row adds exactly nothing -- then the MLP backward,
    the atomic coarse levels [0, 8) (levels 0-3 into 8 gradient replicas, folded
    after) and the binned levels [8, 16) over that list
    (the same gradient as field_backward up to fp32 summation order).
    want_xyzs / want_dirs: also -> (dL/dxyzs | None, dL/ddirs | None) over the same list
    (field_input_grad, after the MLP backward has written dL/denc).  grad None: frozen
    parameters -- the MLP backward still runs for dL/denc, its dW goes to a throwaway
    buffer, and the hash backward is skipped."""
    n = xyzs.shape[0]
    want_in = want_xyzs or want_dirs
    if grad is None:
        if not want_in:
            return None, None
        mlp_grad = torch.zeros(MLP_PARAMS, device=xyzs.device)
    else:
        _check(grad, "grad", torch.float32, grid.n_params)
        mlp_grad = grad
    _check(enc, "enc", torch.float16)
    _check(dL_dsig, "dL_dsigmas", torch.float32); _check(dL_drgb, "dL_drgbs", torch.float32)
    if n == 0:
        z = torch.zeros(0, 3, device=xyzs.device)
        return (z if want_in else None), (z.clone() if want_dirs else None)
    dev = xyzs.device
    K, s = _K(), vren._stream()
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    K.ngp_gradient_rows(dL_dsig, dL_drgb, n, idx, cnt, s)
    denc = torch.empty(n, 32, device=dev)
    K.ngp_field_backward_mlp_act(dirs, n, cnt, idx, enc, 0, params16, dL_dsig, dL_drgb, denc, mlp_grad, int(rgb_act), s)
    dx = dd = None
    if want_in:
        dx, dd = field_input_grad(xyzs, dirs, grid, params16, enc, dL_drgb, denc, rgb_act=rgb_act, n_dev=cnt,
                                  sample_idx=idx, want_dirs=want_dirs)
    if grad is None:
        return dx, dd
    listed = (xyzs, n, cnt, idx, grid.desc, denc, grad[MLP_PARAMS:])
    K.ngp_hash_backward_levels_rep(*listed, 0, BIN_LEVEL_LO, _rep_buffer(grid, dev), COARSE_REP_LEVELS, COARSE_REP, 1,
                                   s)
    K.ngp_hash_backward_binned(*listed, _binned_workspace(dev), BIN_WS_SAMPLES, BIN_LEVEL_LO, BIN_MERGE_HI, s)
    return dx, dd


class FP16Shadow:
    """fp16 copy of an fp32 master parameter, refreshed when the master changes."""

    def __init__(self, master: torch.Tensor):
        self.master = master
        self.version = None
        self.half = None

    def get(self):
        v = self.master._version
        if self.half is None or v != self.version or self.half.data_ptr() == 0:
            self.half = self.master.detach().to(torch.float16)
            self.version = v
        return self.half


class _FieldFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyzs, dirs, params, grid, shadow, rgb_act=0):
        p16 = shadow.get()
        sig, rgb, enc, _ = field_forward(xyzs.contiguous(), dirs.contiguous(), grid, p16, save_enc=True,
                                         rgb_act=rgb_act)
        ctx.save_for_backward(xyzs, dirs, enc)
        ctx.grid, ctx.p16, ctx.rgb_act = grid, p16, rgb_act
        return sig, rgb

    @staticmethod
    def backward(ctx, dsig, drgb):
        xyzs, dirs, enc = ctx.saved_tensors
        grid = ctx.grid
        dsig = torch.zeros(xyzs.shape[0], device=xyzs.device) if dsig is None else dsig.float().contiguous()
        drgb = torch.zeros(xyzs.shape[0], 3, device=xyzs.device) if drgb is None else drgb.float().contiguous()
        need_x, need_d, need_p = ctx.needs_input_grad[:3]
        grad = torch.zeros(grid.n_params, device=xyzs.device) if need_p else None
        dx, dd = field_backward_sparse(xyzs.contiguous(), dirs.contiguous(), grid, ctx.p16, enc, dsig, drgb, grad,
                                       rgb_act=ctx.rgb_act, want_xyzs=need_x, want_dirs=need_d)
        return (dx if need_x else None), dd, grad, None, None, None


def field(xyzs, dirs, params, grid, shadow, rgb_act=0):
    """Differentiable fused field (w.r.t. params, and xyzs / dirs where they require grad:
    pose refinement) -> sigmas (n), rgbs (n,3)."""
    return _FieldFn.apply(xyzs, dirs, params, grid, shadow, rgb_act)


# ------------------------------------------------------------ exposure tonemappers
TONE_LDR, TONE_RADIANCE, TONE_PARAMS = C["NGP_TONE_LDR"], C["NGP_TONE_RADIANCE"], C["NGP_TONE_PARAMS"]
TONE_NET = TONE_PARAMS // 3  # one channel: A 64x16 | B 16x64


def init_tone_params(generator):
    """The three tonemapper nets (networks.py:80-93), Xavier-uniform per matrix as init_params does,
    drawn from `generator` -> (TONE_PARAMS) f32 on the CPU."""
    parts = []
    for _ in range(3):
        for out_d, in_d in ((64, 16), (16, 64)):
            a = math.sqrt(6.0 / (in_d + out_d))
            parts.append((torch.rand(out_d * in_d, generator=generator) * 2 - 1) * a)
    return torch.cat(parts)


def tone_exposure(exposure, n, device):
    """The `exposure` argument of the model surface as the kernels take it -> (tensor | None,
    n_exposure): None: none; a 0-d / one-element tensor or a number: one value; (n,) / (n,1): per row."""
    if exposure is None:
        return None, 0
    if not isinstance(exposure, torch.Tensor):
        if not isinstance(exposure, (int, float)):
            raise ValueError(f"exposure must be a tensor or a number, got {type(exposure).__name__}")
        exposure = torch.tensor(float(exposure))
    if exposure.numel() == 1:
        return exposure.detach().reshape(1).to(device=device, dtype=torch.float32), 1
    if exposure.shape in ((n,), (n, 1)):
        return exposure.detach().reshape(n).to(device=device, dtype=torch.float32).contiguous(), n
    raise ValueError(f"exposure must have one element or shape ({n},) / ({n}, 1), got {tuple(exposure.shape)}")


def _tone_args(log_rad, exposure, n_exposure, tone16, mode):
    n = log_rad.shape[0]
    _check(log_rad, "log_rad", torch.float32, 3 * n)
    if mode == TONE_LDR:
        _check(tone16, "tone16", torch.float16, TONE_PARAMS)
    if n_exposure:
        _check(exposure, "exposure", torch.float32)
        if n_exposure not in (1, n) or exposure.numel() != n_exposure:
            raise RuntimeError(f"exposure must hold 1 or {n} values, got {exposure.numel()} for n_exposure {n_exposure}")
    return n


def tonemap_forward(log_rad, exposure, n_exposure, tone16, mode=TONE_LDR, n_dev=None, sample_idx=None, out=None):
    """ngp_tonemap_forward: log radiance (n,3) -> rgbs (n,3) (`out`: written in place on the counted /
    listed rows, and may be log_rad; None: a new tensor, zero on the other rows)."""
    n = _tone_args(log_rad, exposure, n_exposure, tone16, mode)
    if sample_idx is not None:
        _check(sample_idx, "sample_idx", torch.int32)
        if n_dev is None:
            raise RuntimeError("sample_idx needs its count in n_dev")
    if out is None:
        out = torch.zeros_like(log_rad) if (n_dev is not None) else torch.empty_like(log_rad)
    else:
        _check(out, "rgbs", torch.float32, 3 * n)
    _K().ngp_tonemap_forward(log_rad, exposure if n_exposure else None, n_exposure, n, n_dev, sample_idx,
                             tone16 if mode == TONE_LDR else None, int(mode), out, vren._stream())
    return out


def tonemap_backward(log_rad, exposure, n_exposure, tone16, dL_drgbs, grad_tone, n_dev=None, out=None, workspace=None):
    """ngp_tonemap_backward -> dL/dlog_rad (n,3) (`out`, which may be dL_drgbs); dL/dtone is ADDED to
    grad_tone (TONE_PARAMS f32)."""
    n = _tone_args(log_rad, exposure, n_exposure, tone16, TONE_LDR)
    _check(dL_drgbs, "dL_drgbs", torch.float32, 3 * n)
    _check(grad_tone, "grad_tone", torch.float32, TONE_PARAMS)
    if out is None:
        out = torch.zeros_like(log_rad) if (n_dev is not None) else torch.empty_like(log_rad)
    else:
        _check(out, "dL_dlog_rad", torch.float32, 3 * n)
    if n == 0:
        return out
    nbytes = _K().ngp_tonemap_backward_workspace(n)
    if workspace is None:
        workspace = torch.empty((nbytes + 3) // 4, device=log_rad.device)
    elif workspace.numel() * workspace.element_size() < nbytes:
        raise RuntimeError(f"workspace must hold {nbytes} bytes")
    _K().ngp_tonemap_backward(log_rad, exposure if n_exposure else None, n_exposure, n, n_dev, tone16, dL_drgbs, out,
                              grad_tone, workspace, vren._stream())
    return out


# ---- the forms the fused training step takes
def sample_exposure(rays_a, out, img_idxs=None, img_exposure=None, ray_exposure=None):
    """ngp_sample_exposure / ngp_sample_exposure_rays: every row (ray, start, N) of rays_a writes its
    ray's exposure -- img_exposure[img_idxs[ray]], or ray_exposure[ray] -- to out[start : start + N];
    the other slots of `out` (n) f32 keep their bits."""
    _check(out, "sample_exposure", torch.float32)
    n_rays, n = rays_a.shape[0], out.numel()
    if ray_exposure is not None:
        _check(ray_exposure, "ray_exposure", torch.float32, n_rays)
        _K().ngp_sample_exposure_rays(rays_a, n_rays, ray_exposure, n, out, vren._stream())
    else:
        _check(img_idxs, "img_idxs", torch.int64, n_rays)
        _check(img_exposure, "img_exposure", torch.float32)
        _K().ngp_sample_exposure(rays_a, n_rays, img_idxs, img_exposure, img_exposure.numel(), n, out, vren._stream())
    return out


def tonemap_forward_rows(log_rad, rays_a, rows, n_rows_dev, first, exposure, tone16, out):
    """ngp_tonemap_forward_rows: the first min(N_r, first) samples of the listed rows of rays_a, each at
    its own exposure (n) -> `out` (n,3), which may be log_rad; every other row of `out` keeps its bits."""
    n = _tone_args(log_rad, exposure, log_rad.shape[0], tone16, TONE_LDR)
    _check(out, "rgbs", torch.float32, 3 * n)
    _K().ngp_tonemap_forward_rows(log_rad, n, rays_a, rows, n_rows_dev, rays_a.shape[0], int(first), exposure, tone16,
                                  out, vren._stream())
    return out


def tonemap_backward_indexed(log_rad, exposure, tone16, dL_drgbs, grad_tone, n_dev, sample_idx, out, workspace=None):
    """ngp_tonemap_backward_indexed over the rows sample_idx[:min(n, *n_dev)], each at its own exposure
    (n) -> dL/dlog_rad on those rows of `out` (which may be dL_drgbs); dL/dtone ADDED to grad_tone."""
    n = _tone_args(log_rad, exposure, log_rad.shape[0], tone16, TONE_LDR)
    _check(dL_drgbs, "dL_drgbs", torch.float32, 3 * n)
    _check(grad_tone, "grad_tone", torch.float32, TONE_PARAMS)
    _check(out, "dL_dlog_rad", torch.float32, 3 * n)
    if n == 0:
        return out
    nbytes = _K().ngp_tonemap_backward_indexed_workspace(n)
    if workspace is None:
        workspace = torch.empty((nbytes + 3) // 4, device=log_rad.device)
    elif workspace.numel() * workspace.element_size() < nbytes:
        raise RuntimeError(f"workspace must hold {nbytes} bytes")
    _K().ngp_tonemap_backward_indexed(log_rad, exposure, n, n_dev, sample_idx, tone16, dL_drgbs, out, grad_tone,
                                      workspace, vren._stream())
    return out


def unit_exposure_term(tone16, target, grad_tone, out_loss=None):
    """ngp_unit_exposure_term -> (1) f32: mean_c 0.5 (tonemap(0, exposure 1)_c - target)^2; its gradient
    ADDED to grad_tone."""
    _check(tone16, "tone16", torch.float16, TONE_PARAMS)
    _check(grad_tone, "grad_tone", torch.float32, TONE_PARAMS)
    out_loss = torch.zeros(1, device=grad_tone.device) if out_loss is None else out_loss
    _K().ngp_unit_exposure_term(tone16, float(target), grad_tone, out_loss, vren._stream())
    return out_loss


class _ToneFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_rad, tone_params, exposure, n_exposure, shadow):
        t16 = shadow.get()
        log_rad = log_rad.float().contiguous()
        ctx.save_for_backward(log_rad, exposure)
        ctx.t16, ctx.n_exposure = t16, n_exposure
        return tonemap_forward(log_rad, exposure, n_exposure, t16)

    @staticmethod
    def backward(ctx, drgb):
        log_rad, exposure = ctx.saved_tensors
        need_x, need_t = ctx.needs_input_grad[:2]
        grad = torch.zeros(TONE_PARAMS, device=log_rad.device)
        dx = tonemap_backward(log_rad, exposure, ctx.n_exposure, ctx.t16, drgb.float().contiguous(), grad)
        return (dx if need_x else None), (grad if need_t else None), None, None, None


def tonemap(log_rad, exposure, tone_params, shadow, mode=TONE_LDR):
    """The tonemappers on log radiance (n,3) -> rgbs (n,3), differentiable in log_rad and tone_params
    (not in the exposure: it is data).  exposure: as tone_exposure takes it.  mode TONE_RADIANCE
    (output_radiance): exp(clamp(x, 0, 20)), forward only."""
    exposure, n_exposure = tone_exposure(exposure, log_rad.shape[0], log_rad.device)
    wants_grad = torch.is_grad_enabled() and (log_rad.requires_grad or tone_params.requires_grad)
    if mode == TONE_RADIANCE:
        if torch.is_grad_enabled() and log_rad.requires_grad:
            raise NotImplementedError("output_radiance is forward-only: the radiance mode of the tonemapper has no "
                                      "backward (call it under torch.no_grad())")
        return tonemap_forward(log_rad.detach().float().contiguous(), None, 0, None, TONE_RADIANCE)
    if wants_grad:
        return _ToneFn.apply(log_rad, tone_params, exposure, n_exposure, shadow)
    return tonemap_forward(log_rad.detach().float().contiguous(), exposure, n_exposure, shadow.get())
