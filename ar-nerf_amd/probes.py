"""Light probes: what the insertion app asks of the NeRF beyond plain frames
(insert/main.py:306-407, insert/insert_utils.py:61-147 of the reference).

From each of P scene points R rays are rendered over the sphere (random
directions) or a cube map; the estimated global light can be blended in behind
them as a 9-coefficient spherical-harmonic background (`SH_bkg`); the radiance
and `1 - opacity` are then projected onto the SH9 basis.  The app's shading
and shadow steps consume the resulting (P,9,3) and (P,9,1) tensors.

The helpers keep the reference's names, semantics and spelling
(`clamp_postive`); they work on any device and run the HIP kernels
(csrc/probe.hip) on CUDA fp32 contiguous inputs.  `sh_probes` renders and
projects whole batches of probes on the device; `sg_probe` renders one cube
map and fits the SG lights of the SG shading path to it (sg_probe.py).
"""
from __future__ import annotations

import math

import torch

import vren
from models import rendering as RND

SH9_C = (0.2820947918, 0.4886025119, 1.0925484306, 0.3153915653, 0.5462742153)


# ------------------------------------------------------------------ rays
def get_sphere_rays(probe_num, ray_num, generator=None, device=None):
    """insert_utils.py:61-70: (probe_num, ray_num, 3) directions uniform on the
    sphere (cos theta ~ U(-1,1], phi ~ U[0,2pi)).  The random numbers are drawn
    on the CPU (reproducible under `generator`), then moved to `device`."""
    rds = torch.rand((2, probe_num, ray_num), generator=generator)
    cos_t = 1.0 - 2.0 * rds[0]
    phi = 2.0 * torch.pi * rds[1]
    sin_t = torch.sqrt(1.0 - torch.clamp(cos_t * cos_t, 0.0, 1.0))
    dirs = torch.stack([sin_t * torch.cos(phi), sin_t * torch.sin(phi), cos_t], dim=-1)
    return dirs if device is None else dirs.to(device)


def get_cubemap_rays(probe_num, resolution, keep_raw_dim=False):
    """insert_utils.py:83-100: unit directions through the texel grid of a cube
    map, faces in the order +z, -z, +x, -x, +y, -y: (6, res, res, 3) with
    keep_raw_dim, else (probe_num, 6*res*res, 3) (one set, expanded)."""
    res = int(resolution)
    x = torch.linspace(0, 1, res) * 2 - 1
    X, Y = torch.meshgrid(x, x, indexing="ij")
    X, Y = X.unsqueeze(-1), Y.unsqueeze(-1)
    one = torch.ones((res, res, 1))
    faces = [torch.cat([X, Y, one], -1), torch.cat([X, Y, -one], -1), torch.cat([one, X, Y], -1),
             torch.cat([-one, X, Y], -1), torch.cat([X, one, Y], -1), torch.cat([X, -one, Y], -1)]
    dirs = torch.stack(faces, dim=0)
    dirs = dirs / torch.norm(dirs, dim=-1, keepdim=True)
    if keep_raw_dim:
        return dirs
    dirs = dirs.reshape(-1, 3).unsqueeze(0)
    return dirs.expand(probe_num, *dirs.shape[1:])


# -------------------------------------------------------------------- SH
def sh9_basis(dirs):
    """The nine SH functions of insert_utils.py:102-127 at dirs (...,3) -> (...,9)."""
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    c0, c1, c2, c3, c4 = SH9_C
    return torch.stack([c0 * torch.ones_like(x), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z,
                        c3 * (3.0 * z ** 2 - 1), c2 * x * z, c4 * (x ** 2 - y ** 2)], dim=-1)


def _kernel_ok(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)


def get_SH_val(shec, dirs, clamp_postive=False, kernel=None):
    """insert_utils.py:142-147: the SH function `shec` (9,C) along dirs (...,3)
    -> (...,C), clamped at zero with clamp_postive.  The clamped value of a
    (9,3) light on CUDA comes from ngp_render_test_finish_sh (blended over
    black at zero opacity); everything else, and kernel=False, is evaluated
    with fp32 torch expressions (no matmul: under autocast it would round the
    light to fp16)."""
    if kernel is None:
        kernel = clamp_postive and dirs.numel() > 0 and tuple(shec.shape) == (9, 3) and _kernel_ok(shec, dirs)
    if kernel:
        flat = dirs.reshape(-1, 3)
        vals = torch.zeros_like(flat)
        vren.render_test_finish_sh(torch.zeros(flat.shape[0], device=dirs.device), flat, shec, vals)
        return vals.reshape(dirs.shape)
    vals = (sh9_basis(dirs).unsqueeze(-1) * shec).sum(-2)
    return torch.relu(vals) if clamp_postive else vals


def get_SH_coeff(rays_d, rays_rgb):
    """insert_utils.py:132-136: rays_d (P,R,3), rays_rgb (P,R,C) -> (P,9,C),
    (4 pi / R) sum_r Y_k(d_r) rgb_r.  C = 3 on CUDA runs ngp_probe_sh9_project."""
    if rays_rgb.shape[-1] == 3 and rays_d.numel() > 0 and _kernel_ok(rays_d, rays_rgb):
        return vren.probe_sh9_project(rays_d, rays_rgb)[0]
    shs = sh9_basis(rays_d)
    res = (shs.unsqueeze(-1) * rays_rgb.unsqueeze(-2)).sum(dim=1)
    return res * 4 * torch.pi / rays_d.shape[1]


# --------------------------------------------------------------- probes
@torch.no_grad()
def sh_probes(model, pts, dirs=None, n_rays=2048, SH_bkg=None, blend_bkg=True, probes_per_batch=64,
              return_rays=False, **render_kwargs):
    """SH9 light probes at the points pts (P,3) (main.py:355-407).

    dirs: one shared (R,3) set of directions, (P,R,3) per probe, or None for
    get_sphere_rays(P, n_rays).  SH_bkg: a (9,3) global light blended in behind
    the rays (clamped at zero) unless blend_bkg is False.  render_kwargs:
    T_threshold, max_samples, exp_step_factor, output_radiance, as render()
    takes them (output_radiance: a raw-HDR model's relu radiance, what
    generate_SH_probes asks for under use_EXR; on a model built with
    use_exposure, the tonemapped colour at the one `exposure` given, unit by
    default, or its radiance).

    Returns {'rgb_sh': (P,9,3), 'trans_sh': (P,9,1)}: the projections of the
    radiance and of 1 - opacity; with return_rays also 'rgb' (P,R,3),
    'opacity' (P,R) and 'dirs'.

    The probes are rendered in fixed batches of probes_per_batch through one
    cached renderer.TestRenderer of probes_per_batch * R rays: probe rays
    (ngp_probe_rays), the device loop, the closing blend and the projection
    (ngp_probe_sh9_project), nothing in between on the host but the loop's own
    check.  The last batch is filled up by repeating the last point (and its
    directions); those rows are dropped.  Each batch equals
    render(test_time=True) on exactly those B*R rays bit for bit.  The loop's
    samples-per-iteration budget depends on how many rays of the batch are
    still alive, so a probe's rays are NOT independent of the batch they are
    rendered in: another probes_per_batch gives slightly different values.
    """
    unknown = set(render_kwargs) - {'T_threshold', 'max_samples', 'exp_step_factor', 'output_radiance', 'exposure'}
    if unknown:
        raise TypeError(f"sh_probes: unexpected arguments {sorted(unknown)}")
    if not hasattr(model, '_shadow'):
        raise RuntimeError("sh_probes needs a models.networks.NGP on the GPU")
    dev = model.density_bitfield.device
    pts = torch.as_tensor(pts, dtype=torch.float32, device=dev).reshape(-1, 3)
    P, B = pts.shape[0], int(probes_per_batch)
    if P < 1 or B < 1:
        raise ValueError("sh_probes needs at least one probe and probes_per_batch >= 1")
    if dirs is None:
        dirs = get_sphere_rays(P, int(n_rays), device=dev)
    dirs = torch.as_tensor(dirs, dtype=torch.float32, device=dev)
    if dirs.dim() not in (2, 3) or dirs.shape[-1] != 3 or (dirs.dim() == 3 and dirs.shape[0] != P):
        raise ValueError("dirs must be (R,3) or (P,R,3)")
    R, per_probe = dirs.shape[-2], dirs.dim() == 3
    if R < 1:
        raise ValueError("sh_probes needs at least one ray per probe")
    n_batches = (P + B - 1) // B
    pad = n_batches * B - P
    pts_all = torch.cat([pts, pts[-1:].expand(pad, 3)]).contiguous()
    dirs_all = dirs.contiguous()
    if per_probe and pad:
        dirs_all = torch.cat([dirs_all, dirs_all[-1:].expand(pad, R, 3)]).contiguous()
    bg_sh = None
    if SH_bkg is not None and blend_bkg:
        bg_sh = torch.as_tensor(SH_bkg, dtype=torch.float32, device=dev).reshape(9, 3).contiguous()
    rr = RND._test_renderer(model, B * R, render_kwargs.get('exp_step_factor', 0.),
                            render_kwargs.get('T_threshold', 1e-4), render_kwargs.get('max_samples', RND.MAX_SAMPLES),
                            model.rgb_mode(render_kwargs.get('output_radiance', False)),
                            model.tone_mode(render_kwargs.get('output_radiance', False)))
    if rr.tone_mode is not None:
        rr.set_exposure(render_kwargs.get('exposure', None))
    rgb_sh = torch.empty(n_batches * B, 9, 3, device=dev)
    trans_sh = torch.empty(n_batches * B, 9, device=dev)
    rays = {'rgb': [], 'opacity': []}
    for b in range(n_batches):
        sl = slice(b * B, (b + 1) * B)
        vren.probe_rays(pts_all[sl], dirs_all[sl] if per_probe else dirs_all, model.center, model.half_size,
                        RND.NEAR_DISTANCE, out=(rr.rays_o, rr.rays_d, rr.hits_t))
        out = rr.render_loaded(bg_sh)
        vren.probe_sh9_project(rr.rays_d.view(B, R, 3), out['rgb'].view(B, R, 3), out['opacity'].view(B, R),
                               rgb_sh[sl], trans_sh[sl])
        if return_rays:
            rays['rgb'].append(out['rgb'].view(B, R, 3).clone())
            rays['opacity'].append(out['opacity'].view(B, R).clone())
    res = {'rgb_sh': rgb_sh[:P], 'trans_sh': trans_sh[:P].unsqueeze(-1)}
    if return_rays:
        res['rgb'] = torch.cat(rays['rgb'])[:P]
        res['opacity'] = torch.cat(rays['opacity'])[:P]
        res['dirs'] = dirs
    return res


@torch.no_grad()
def sg_probe(model, pt, env_opt, SH_bkg=None, resolution=32, env_hw=(128, 128), **render_kwargs):
    """The SG light probe at the point pt (3,) (main.py:306-352 with SH_probe=False): a cube map of
    6 * resolution^2 rays rendered from pt through sh_probes (one probe, probes_per_batch=1, SH_bkg blended in
    behind the rays), resampled to an env_hw equirectangular map (sg_probe.cubemap2env_map), to which env_opt
    (an sg_probe.EnvOptim: warm-started, N_iter Adam steps) fits its lights; trans_raw_sg normalises a copy of
    them into the rows shading.sg_shade and sg_shadow.SGShadow take.

    Returns {'lSGs': (L,7) axis, sharpness, rgb; 'envmap': (H,W,3); 'cubemap_rgb': (6*resolution^2,3)}."""
    import sg_probe as SGP
    res, (H, W) = int(resolution), (int(v) for v in env_hw)
    dirs = get_cubemap_rays(1, res)[0]
    out = sh_probes(model, torch.as_tensor(pt, dtype=torch.float32).reshape(1, 3), dirs=dirs, SH_bkg=SH_bkg,
                    probes_per_batch=1, return_rays=True, **render_kwargs)
    cubemap_rgb = out['rgb'][0].contiguous()
    envmap = SGP.cubemap2env_map(cubemap_rgb, res, H, W)
    lSGs = SGP.trans_raw_sg(env_opt.eval(envmap).clone())
    return {'lSGs': lSGs, 'envmap': envmap, 'cubemap_rgb': cubemap_rgb}
