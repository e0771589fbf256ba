"""Drop-in for the reference's models/rendering.py:1-319 (render,
__render_rays_train, __render_rays_test) on the MI355X kernels."""
import torch

import vren
from .custom_functions import RayAABBIntersector, RayMarcher, VolumeRenderer

MAX_SAMPLES = 1024
NEAR_DISTANCE = 0.01


@torch.amp.autocast("cuda")
def render(model, rays_o, rays_d, **kwargs):
    """models/rendering.py:13-54: AABB intersection + near clamp, then the
    train or test render function; optional to_cpu / to_numpy."""
    rays_o = rays_o.contiguous()
    rays_d = rays_d.contiguous()
    _, hits_t, _ = RayAABBIntersector.apply(rays_o, rays_d, model.center, model.half_size, 1)
    # (the reference's boolean-mask assignment, as a select: a mask index_put lists the mask's
    # nonzeros first, which waits for the device every call)
    h0 = hits_t[:, 0, 0]
    hits_t[:, 0, 0] = torch.where((h0 >= 0) & (h0 < NEAR_DISTANCE), torch.full_like(h0, NEAR_DISTANCE), h0)
    render_func = __render_rays_test if kwargs.get('test_time', False) else __render_rays_train
    mesh_depth_map = kwargs.get('mesh_depth_map', None)
    if mesh_depth_map is not None:  # rendering.py:38-44
        valid_depth = mesh_depth_map >= 1e-6
        hits_t_s = hits_t[valid_depth]
        update_min = torch.min(hits_t_s[:, 0, 1], mesh_depth_map[valid_depth])
        update_min = torch.max(update_min, hits_t_s[:, 0, 0])
        hits_t[valid_depth, 0, 1] = update_min
    results = render_func(model, rays_o, rays_d, hits_t, **kwargs)
    for k, v in results.items():
        if kwargs.get('to_cpu', False):
            v = v.cpu()
            if kwargs.get('to_numpy', False):
                v = v.numpy()
        results[k] = v
    return results


# BASELINE.json's north_star names the drop-in surface models.rendering.render_rays;
# the reference module's entry point is render() (rendering.py:13), so both names bind it
render_rays = render


def _sh_light(kwargs, device):
    """The SH_bkg kwarg as a device (9,3) fp32 tensor, or None when the frame
    does not blend it: IM_bkg overrides it and blend_bkg=False skips both
    (rendering.py:240-250)."""
    sh = kwargs.get('SH_bkg', None)
    if sh is None or kwargs.get('IM_bkg', None) is not None or not kwargs.get('blend_bkg', True):
        return None
    return torch.as_tensor(sh, dtype=torch.float32, device=device).reshape(9, 3).contiguous()


def _background(kwargs, rays_d, default):
    """rgb_bg of rendering.py:240-247 for the torch blend: IM_bkg, else the
    clamped SH_bkg light along rays_d (fp32 torch expressions), else default."""
    im = kwargs.get('IM_bkg', None)
    if im is not None:
        return im
    sh = _sh_light(kwargs, rays_d.device)
    if sh is not None:
        import probes
        return probes.get_SH_val(sh, rays_d.float(), clamp_postive=True, kernel=False)
    return default


def _test_renderer(model, n_rays, esf, T_threshold, max_samples, rgb_act=0, tone_mode=None):
    """TestRenderer cached on the model per (rays, loop settings, bitfield,
    colour mode, tonemap mode: the modes are baked into the captured graphs)."""
    import renderer as RD
    cache = model.__dict__.setdefault('_test_renderers', {})
    key = (n_rays, float(esf), float(T_threshold), int(max_samples), model.density_bitfield.data_ptr(), int(rgb_act),
           tone_mode)
    rr = cache.get(key)
    p16 = model._shadow.get()
    t16 = model._tone_shadow.get() if tone_mode is not None else None
    if rr is None:
        if len(cache) >= 4:
            cache.clear()
        rr = RD.TestRenderer(n_rays, model.grid, p16.clone(), model.density_bitfield, model.cascades, model.scale,
                             model.grid_size, exp_step_factor=esf, T_threshold=T_threshold, max_samples=max_samples,
                             iters_per_graph=16, iters_tail=8, rgb_act=int(rgb_act),
                             tone16=None if t16 is None else t16.clone(), tone_mode=tone_mode)
        rr._src = rr._tone_src = None
        cache[key] = rr
    _refresh_shadows(rr, p16, t16)
    return rr


def _refresh_shadows(rr, p16, t16):
    """A cached renderer's own copies of the model's fp16 shadows, refreshed when the model made new ones."""
    if rr._src is not p16:  # parameters changed since the last frame: refresh the renderer's copy
        rr.params16.copy_(p16)
        rr._src = p16
    if t16 is not None and rr._tone_src is not t16:  # (the tone shadow likewise)
        rr.tone16.copy_(t16)
        rr._tone_src = t16


def _frame_exposure(kwargs):
    """The `exposure` kwarg of a test-time frame for the device loop: None or one value
    (the viewer's slider, show_gui.py:86); per-ray exposures take the host loop."""
    e = kwargs.get('exposure', None)
    if e is None or not isinstance(e, torch.Tensor) or e.numel() == 1:
        return True, e
    return False, e


@torch.no_grad()
def __render_rays_test(model, rays_o, rays_d, hits_t, **kwargs):
    """models/rendering.py:162-253 (grows samples per alive ray, composites
    until T < T_threshold; black background by default, SH_bkg / IM_bkg
    blended behind the rays when given).  For an NGP on the
    GPU the loop runs device-resident in HIP graphs (renderer.TestRenderer,
    bit-identical results); device_loop=False keeps the host-driven loop."""
    exp_step_factor = kwargs.get('exp_step_factor', 0.)
    tone_mode = model.tone_mode(kwargs.get('output_radiance', False)) if hasattr(model, 'tone_mode') else None
    uniform, exposure = _frame_exposure(kwargs) if tone_mode is not None else (True, None)
    if kwargs.get('device_loop', True) and hasattr(model, '_shadow') and rays_o.is_cuda and len(rays_o) > 0 \
            and uniform:
        rr = _test_renderer(model, len(rays_o), exp_step_factor, kwargs.get('T_threshold', 1e-4),
                            kwargs.get('max_samples', MAX_SAMPLES),
                            model.rgb_mode(kwargs.get('output_radiance', False)), tone_mode)
        if tone_mode is not None:
            rr.set_exposure(exposure)
        # SH_bkg: blended by the frame's closing launch (ngp_render_test_finish_sh)
        bg_sh = _sh_light(kwargs, rays_o.device)
        out = rr.render(rays_o, rays_d, hits_t[:, 0], bg_sh=bg_sh)
        results = {k: v.clone() for k, v in out.items()}
        if bg_sh is None and kwargs.get('blend_bkg', True):
            rgb_bg = _background(kwargs, rays_d, torch.zeros(3, device=rays_o.device))
            results['rgb'] += rgb_bg * (1 - results['opacity'])[:, None]
        return results
    results = {}
    N_rays = len(rays_o)
    device = rays_o.device
    opacity = torch.zeros(N_rays, device=device)
    depth = torch.zeros(N_rays, device=device)
    rgb = torch.zeros(N_rays, 3, device=device)
    samples = total_samples = 0
    alive_indices = torch.arange(N_rays, device=device)
    min_samples = 1 if exp_step_factor == 0 else 4
    ht = hits_t[:, 0]
    while samples < kwargs.get('max_samples', MAX_SAMPLES):
        N_alive = len(alive_indices)
        if N_alive == 0:
            break
        N_samples = max(min(N_rays // N_alive, 64), min_samples)
        samples += N_samples
        xyzs, dirs, deltas, ts, N_eff_samples = vren.raymarching_test(
            rays_o, rays_d, ht, alive_indices, model.density_bitfield, model.cascades, model.scale, exp_step_factor,
            model.grid_size, MAX_SAMPLES, N_samples)
        total_samples += N_eff_samples.sum()
        xyzs = xyzs.reshape(-1, 3)
        dirs = dirs.reshape(-1, 3)
        valid_mask = ~torch.all(dirs == 0, dim=1)
        if valid_mask.sum() == 0:
            break
        sigmas = torch.zeros(len(xyzs), device=device)
        rgbs = torch.zeros(len(xyzs), 3, device=device)
        xyzs = xyzs[valid_mask]
        dirs = dirs[valid_mask]
        pts_num = xyzs.shape[0]
        val_batch_size = kwargs.get('val_batch_size', pts_num)
        sig_res, rgb_res = [], []
        for i in range(0, pts_num, val_batch_size):
            s, c = model(xyzs[i:i + val_batch_size], dirs[i:i + val_batch_size], **kwargs)
            sig_res.append(s)
            rgb_res.append(c)
        sigmas[valid_mask] = torch.cat(sig_res, 0).float()
        rgbs[valid_mask] = torch.cat(rgb_res, 0).float()
        sigmas = sigmas.view(-1, N_samples)
        rgbs = rgbs.view(-1, N_samples, 3)
        vren.composite_test_fw(sigmas, rgbs, deltas, ts, ht, alive_indices, kwargs.get('T_threshold', 1e-4),
                               N_eff_samples, opacity, depth, rgb)
        alive_indices = alive_indices[alive_indices >= 0].contiguous()
    results['opacity'] = opacity
    results['depth'] = depth
    results['rgb'] = rgb
    results['total_samples'] = total_samples
    if kwargs.get('blend_bkg', True):
        rgb_bg = _background(kwargs, rays_d, torch.zeros(3, device=device))
        results['rgb'] += rgb_bg * (1 - opacity)[:, None]
    return results


@torch.no_grad()
def render_insert(model, c2w, directions, H, W, rect, obj_rgb, obj_depth, **kwargs):
    """The body of the insertion app's Insertor.render_insert_object
    (insert/main.py:632-660) in one call: the rays of the screen rectangle
    rect = (hs, ws, hl, wl) of the H x W camera `directions` (H*W,3) at the
    (3,4) pose c2w, render(test_time=True, IM_bkg=obj_rgb[hs:hl, ws:wl],
    mesh_depth_map=obj_depth[hs:hl, ws:wl]) and the write into the persistent
    last_rgb / last_depth canvases, plus pts = rays_o + rays_d * depth
    (main.py:429).  obj_rgb (H,W,3) / obj_depth (H,W): the shaded object and
    its depth over the whole frame.  kwargs as the app's render takes them:
    T_threshold, max_samples, exp_step_factor, exposure (None or one value),
    output_radiance.

    One renderer.InsertRenderer is cached on the model per (H, W, camera,
    loop settings, bitfield, modes) and serves every rectangle without
    re-capture.  Returns views of its canvases: rgb (H,W,3), depth (H,W), pts
    (H,W,3) -- pixels outside the rectangle keep the last frame's values -- and
    total_samples."""
    import renderer as RD
    esf = kwargs.get('exp_step_factor', 0.)
    T_threshold, max_samples = kwargs.get('T_threshold', 1e-4), kwargs.get('max_samples', MAX_SAMPLES)
    radiance = kwargs.get('output_radiance', False)
    rgb_act = int(model.rgb_mode(radiance))
    tone_mode = model.tone_mode(radiance)
    directions = directions.reshape(-1, 3)
    cache = model.__dict__.setdefault('_insert_renderers', {})
    key = (int(H), int(W), directions.data_ptr(), float(esf), float(T_threshold), int(max_samples),
           model.density_bitfield.data_ptr(), rgb_act, tone_mode)
    rr = cache.get(key)
    p16 = model._shadow.get()
    t16 = model._tone_shadow.get() if tone_mode is not None else None
    if rr is None:
        if len(cache) >= 4:
            cache.clear()
        rr = RD.InsertRenderer(H, W, directions, model.center, model.half_size, model.grid, p16.clone(),
                               model.density_bitfield, model.cascades, model.scale, model.grid_size,
                               exp_step_factor=esf, T_threshold=T_threshold, max_samples=max_samples,
                               iters_per_graph=16, iters_tail=8, rgb_act=rgb_act,
                               tone16=None if t16 is None else t16.clone(), tone_mode=tone_mode)
        rr._src = rr._tone_src = None
        cache[key] = rr
    _refresh_shadows(rr, p16, t16)
    if tone_mode is not None:
        uniform, exposure = _frame_exposure(kwargs)
        if not uniform:
            raise ValueError("render_insert takes one exposure per frame")
        rr.set_exposure(exposure)
    return rr.render_rect(c2w, rect, obj_rgb, obj_depth)


def _insert_renderer(model, directions, H, W, kwargs):
    """render_insert's cached InsertRenderer for these settings (the same key
    and construction, so both calls share one renderer per camera), with the
    model's current parameters and the frame's exposure set."""
    import renderer as RD
    esf = kwargs.get('exp_step_factor', 0.)
    T_threshold, max_samples = kwargs.get('T_threshold', 1e-4), kwargs.get('max_samples', MAX_SAMPLES)
    radiance = kwargs.get('output_radiance', False)
    rgb_act = int(model.rgb_mode(radiance))
    tone_mode = model.tone_mode(radiance)
    directions = directions.reshape(-1, 3)
    cache = model.__dict__.setdefault('_insert_renderers', {})
    key = (int(H), int(W), directions.data_ptr(), float(esf), float(T_threshold), int(max_samples),
           model.density_bitfield.data_ptr(), rgb_act, tone_mode)
    rr = cache.get(key)
    p16 = model._shadow.get()
    t16 = model._tone_shadow.get() if tone_mode is not None else None
    if rr is None:
        if len(cache) >= 4:
            cache.clear()
        rr = RD.InsertRenderer(H, W, directions, model.center, model.half_size, model.grid, p16.clone(),
                               model.density_bitfield, model.cascades, model.scale, model.grid_size,
                               exp_step_factor=esf, T_threshold=T_threshold, max_samples=max_samples,
                               iters_per_graph=16, iters_tail=8, rgb_act=rgb_act,
                               tone16=None if t16 is None else t16.clone(), tone_mode=tone_mode)
        rr._src = rr._tone_src = None
        cache[key] = rr
    _refresh_shadows(rr, p16, t16)
    if tone_mode is not None:
        uniform, exposure = _frame_exposure(kwargs)
        if not uniform:
            raise ValueError("render_insert_sg takes one exposure per frame")
        rr.set_exposure(exposure)
    return rr


@torch.no_grad()
def render_insert_sg(model, c2w, directions, H, W, rect, bbox, normals, obj_depth, lSGs, **kwargs):
    """render_insert with the object shaded on the device: the app's
    Insertor.render_object under SG lights (insert/main.py:521-594,
    shading.sg_shade) into the cached InsertRenderer's own obj_rgb buffer,
    then the rectangle.  bbox: the model's box (hs, ws, hl, wl), in which the
    object is shaded; rect: the update range that is rendered (main.py:632);
    each four ints or a device int32[4] tensor.  normals (H,W,3), obj_depth
    (H,W), lSGs (L,7).  kwargs: render_insert's, and the materials metal,
    rough, albedo, decay, clamp01 (default: not output_radiance, the app's
    `not render_HDR_mapping`)."""
    shade = {k: kwargs.pop(k) for k in ('metal', 'rough', 'albedo', 'decay') if k in kwargs}
    shade['clamp01'] = kwargs.pop('clamp01', not kwargs.get('output_radiance', False))
    rr = _insert_renderer(model, directions, H, W, kwargs)
    rr.shade_sg(c2w, bbox, normals, obj_depth, lSGs, **shade)
    return rr.render_rect(c2w, rect)


@torch.no_grad()
def render_insert_sg_shadow(model, c2w, directions, H, W, rect, bbox, normals, obj_depth, lSGs, shadow, scale,
                            model_pos, rot_inv=None, self_shadow=True, gen_shadow=True, **kwargs):
    """render_insert_sg with the SSDF soft shadows of an SG-lit frame
    (insert/sg_shadow.py; sg_shadow.SGShadow `shadow`) on the
    cached InsertRenderer: the self-shadow decay of the object's pixels
    (self_shadow; main.py:558-567) feeds the shade, the rectangle is rendered,
    and the cast shadow over the whole screen's surface points (gen_shadow;
    main.py:662-672) is blurred 3 x 3 and multiplied into a NEW image: the
    canvases stay unshadowed, as the reference's last_rgb does.  scale: the
    model's radius; model_pos (3); rot_inv (3,3) or None -- the lights are
    given unrotated and rotated here for the cast pass (main.py:496-499).
    Returns render_insert_sg's canvases and, with gen_shadow, `shadowed`
    (H,W,3), a view of the renderer's buffer.  A `decay` in kwargs is used as
    given when self_shadow is off."""
    shade = {k: kwargs.pop(k) for k in ('metal', 'rough', 'albedo', 'decay') if k in kwargs}
    shade['clamp01'] = kwargs.pop('clamp01', not kwargs.get('output_radiance', False))
    rr = _insert_renderer(model, directions, H, W, kwargs)
    if self_shadow:
        shade['decay'] = rr.self_shadow_decay(c2w, bbox, obj_depth, shadow, lSGs, scale, model_pos, rot_inv)
    rr.shade_sg(c2w, bbox, normals, obj_depth, lSGs, **shade)
    out = rr.render_rect(c2w, rect)
    if gen_shadow:
        lights = lSGs
        if rot_inv is not None:
            lights = lSGs.clone()
            lights[:, :3] = (rot_inv @ lights[:, :3].T).T
        out['shadowed'] = rr.cast_shadow(shadow, lights, scale, model_pos, rot_inv)
    return out


def __render_rays_train(model, rays_o, rays_d, hits_t, **kwargs):
    """models/rendering.py:255-298."""
    exp_step_factor = kwargs.get('exp_step_factor', 0.)
    results = {}
    (rays_a, xyzs, dirs, results['deltas'], results['ts'], results['rm_samples']) = RayMarcher.apply(
        rays_o, rays_d, hits_t[:, 0], model.density_bitfield, model.cascades, model.scale, exp_step_factor,
        model.grid_size, MAX_SAMPLES)
    for k, v in kwargs.items():  # supply additional inputs, repeated per ray
        if isinstance(v, torch.Tensor):
            kwargs[k] = torch.repeat_interleave(v[rays_a[:, 0]], rays_a[:, 2], 0)
    sigmas, rgbs = model(xyzs, dirs, **kwargs)
    (results['vr_samples'], results['opacity'], results['depth'], results['rgb'], results['ws']) = \
        VolumeRenderer.apply(sigmas, rgbs.contiguous(), results['deltas'], results['ts'], rays_a,
                             kwargs.get('T_threshold', 1e-4))
    results['rays_a'] = rays_a
    if kwargs.get('random_bg', False):
        rgb_bg = torch.rand(3, device=rays_o.device)
    elif exp_step_factor == 0:  # synthetic
        rgb_bg = torch.ones(3, device=rays_o.device)
    else:  # real
        rgb_bg = torch.zeros(3, device=rays_o.device)
    results['rgb'] = results['rgb'] + rgb_bg * (1 - results['opacity'])[:, None]
    return results


@torch.no_grad()
def render_surface_rgb(model, pts, rays_d, **kwargs):
    """models/rendering.py:314-319."""
    H, W, _ = pts.shape
    _, rgbs = model(pts.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous(), **kwargs)
    return rgbs.reshape(H, W, 3)


def normalize_eps(vec, eps=1e-6):
    """insert/insert_utils.py:18-19"""
    return vec / (torch.norm(vec, dim=-1, keepdim=True) + eps)


@torch.enable_grad()
def render_surface_normal(model, pts, **kwargs):
    """models/rendering.py:300-313: normals = -normalize(d sigma / d x) at the
    surface points, the input gradient taken through the hash grid by
    autograd (NGP.density -> ngp_density_input_grad)."""
    H, W, _ = pts.shape
    pts_grad = pts.reshape(-1, 3).detach().clone().requires_grad_(True)
    sigmas = model.density(pts_grad)
    normals = torch.autograd.grad(sigmas, pts_grad, torch.ones_like(sigmas))[0]
    normals = normals.reshape(H, W, 3).nan_to_num(0.0, 1.0, -1.0).detach()
    return -normalize_eps(normals)
