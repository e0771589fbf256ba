"""`vren` for MI355X: the reference's pybind extension surface
(models/csrc/binding.cpp:234-250) re-implemented over the C-ABI library
libngp_amd.so (include/ngp_amd.h, hand-written gfx950 HIP kernels).

Same function names, argument order and meaning, same output tensors and
the same CHECK_INPUT error behaviour ("x must be a CUDA tensor" /
"x must be contiguous" as RuntimeError, models/csrc/include/utils.h:4-6).
There is NO CPU fallback: importing works on any host (so the library can
be inspected), but every call needs the library and GPU tensors, and fails
loudly otherwise.

Differences from the reference, all deliberate and documented in DESIGN.md:
  * raymarching_train returns exact-size outputs in a deterministic
    RAY-ORDERED layout (rays_a[r] = [r, start_r, n_r]); the reference fills
    a N_rays*1024 zero-initialised scratch in atomic order.
  * composite_train_fw's first output is the per-ray sample count, as in
    the reference (the autograd wrapper sums it).
"""
from __future__ import annotations

import contextlib
import ctypes
import gc
import os
from ctypes import c_float, c_void_p  # noqa: F401  (c_float: callers wrap float arguments as vren.c_float)

import torch

import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NGP_AMD_LIB", os.path.join(_HERE, "lib", "libngp_amd.so"))

_lib = _kernels = None


class NGPError(RuntimeError):
    status = None  # the C function's return, when that is what failed


def _load(errcheck=None):
    if not os.path.exists(LIB_PATH):
        raise NGPError(f"libngp_amd.so not found at {LIB_PATH}: run `make -C ar-nerf_amd` "
                       "(or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    capi.declare(L, errcheck=errcheck)
    return L


def lib():
    """The raw view of libngp_amd.so (raises if it was not built): every entry
    point's signature as include/ngp_amd.h declares it (capi.py), the status
    handed back as the return value (tests, bench, diagnostics)."""
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def _raise_status(rc, fn, args):
    if rc != 0:
        e = NGPError(f"{fn.__name__} failed with status {rc}")
        e.status = rc
        raise e
    return rc


def kernels():
    """The checked view, which all product code calls: a second handle on the
    same loaded library with the same signatures, whose status-returning
    functions raise NGPError (.status) instead of returning nonzero.  Tensors,
    Python numbers and grid.desc are passed as they are (capi.POINTER_TO)."""
    global _kernels
    if _kernels is None:
        _kernels = _load(_raise_status)
    return _kernels


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def graph_capture(g):
    """torch.cuda.graph(g) with the cyclic garbage collector kept out of the
    capture.  torch no longer collects before a capture, and a collection that
    fires inside one may free an unreachable trainer or renderer whose
    CUDAGraph destructor synchronises the device on ROCm: not allowed while a
    stream is capturing, and thrown from a destructor it aborts the process.
    So: collect first (dead graphs go now), no automatic collection inside."""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            yield
    finally:
        if was_on:
            gc.enable()


def _check(name, x, dtype=None):
    # models/csrc/include/utils.h:4-6 (CHECK_CUDA, CHECK_CONTIGUOUS)
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not x.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if dtype is not None and x.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {x.dtype}")
    return c_void_p(x.data_ptr())


def _checks(dtype, **named):
    """_check(name, x, dtype) of every name=x, in order"""
    for name, x in named.items():
        _check(name, x, dtype)


def _ok(st, what):  # (callers of the raw view: tests, diagnostics)
    if st != 0:
        raise NGPError(f"{what} failed with status {st}")


# ------------------------------------------------------------------ rays
def ray_aabb_intersect(rays_o, rays_d, centers, half_sizes, max_hits):
    """intersection.cu:59-100 -> [hit_cnt (N) i32, hits_t (N,max_hits,2), hits_voxel_idx (N,max_hits) i64]"""
    _checks(torch.float32, rays_o=rays_o, rays_d=rays_d, centers=centers, half_sizes=half_sizes)
    n, nv = rays_o.shape[0], centers.numel() // 3
    dev = rays_o.device
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    ht = torch.empty(n, max_hits, 2, dtype=torch.float32, device=dev)
    hv = torch.empty(n, max_hits, dtype=torch.int64, device=dev)
    kernels().ngp_ray_aabb_intersect(rays_o, rays_d, n, centers, half_sizes, nv, int(max_hits), cnt, ht, hv, _stream())
    return [cnt, ht, hv]


def raygen_aabb(directions, poses, img_idxs, pix_idxs, center, half_size, near_distance):
    """Fused get_rays (datasets/ray_utils.py:45-70) on the gathered training
    batch (train.py:85-87) + AABB + near clamp (models/rendering.py:29-31).
    Returns rays_o, rays_d (N,3) and hits_t (N,2)."""
    n = img_idxs.shape[0]
    dev = directions.device
    rays_o = torch.empty(n, 3, device=dev)
    rays_d = torch.empty(n, 3, device=dev)
    hits_t = torch.empty(n, 2, device=dev)
    _checks(torch.float32, directions=directions, poses=poses)
    _checks(torch.int64, img_idxs=img_idxs, pix_idxs=pix_idxs)
    _checks(torch.float32, center=center, half_size=half_size)
    kernels().ngp_raygen_aabb(directions, poses, img_idxs, pix_idxs, n, center, half_size, float(near_distance),
                              rays_o, rays_d, hits_t, _stream())
    return rays_o, rays_d, hits_t


# --------------------------------------------------------- light probes
def probe_rays(pts, dirs, center, half_size, near_distance, out=None):
    """ngp_probe_rays: R rays from each of the P points `pts` (P,3) along
    `dirs`, one shared (R,3) set or (P,R,3) per probe; AABB + near clamp as
    models/rendering.py:29-31.  Returns rays_o, rays_d (P*R,3) and hits_t
    (P*R,2), written into `out` = (rays_o, rays_d, hits_t) when given."""
    _checks(torch.float32, pts=pts, dirs=dirs)
    if pts.dim() != 2 or pts.shape[1] != 3 or dirs.dim() not in (2, 3) or dirs.shape[-1] != 3:
        raise RuntimeError("pts must be (P,3) and dirs (R,3) or (P,R,3)")
    P, R, per_probe = pts.shape[0], dirs.shape[-2], int(dirs.dim() == 3)
    if per_probe and dirs.shape[0] != P:
        raise RuntimeError(f"dirs holds {dirs.shape[0]} probes, pts {P}")
    n = P * R
    if out is None:
        out = tuple(torch.empty(n, k, device=pts.device) for k in (3, 3, 2))
    rays_o, rays_d, hits_t = out
    for name, t, k in (("rays_o", rays_o, 3), ("rays_d", rays_d, 3), ("hits_t", hits_t, 2)):
        _check(name, t, torch.float32)
        if t.numel() != n * k:
            raise RuntimeError(f"{name} must hold {n} rays")
    _checks(torch.float32, center=center, half_size=half_size)
    kernels().ngp_probe_rays(pts, dirs, per_probe, P, R, center, half_size, float(near_distance), rays_o, rays_d,
                             hits_t, _stream())
    return rays_o, rays_d, hits_t


def render_test_finish_sh(opacity, rays_d, shec, rgb):
    """ngp_render_test_finish_sh, in place on rgb (N,3):
    rgb += relu(get_SH_val(shec, rays_d)) * (1 - opacity)."""
    n = opacity.numel()
    if rays_d.numel() != 3 * n or rgb.numel() != 3 * n:
        raise RuntimeError("opacity (N), rays_d (N,3) and rgb (N,3) must agree")
    _checks(torch.float32, opacity=opacity, rays_d=rays_d, shec=shec)
    if tuple(shec.shape) != (9, 3):
        raise RuntimeError(f"shec must be (9,3), got {tuple(shec.shape)}")
    _check("rgb", rgb, torch.float32)
    kernels().ngp_render_test_finish_sh(opacity, rays_d, n, shec, rgb, _stream())
    return rgb


def probe_sh9_project(rays_d, rgb, opacity=None, rgb_sh=None, trans_sh=None):
    """ngp_probe_sh9_project: rays_d, rgb (P,R,3) [, opacity (P,R)] ->
    rgb_sh (P,9,3) [, trans_sh (P,9) of 1 - opacity; None without opacity].
    Outputs are written into rgb_sh / trans_sh when given."""
    if rays_d.dim() != 3 or rays_d.shape[-1] != 3 or rgb.shape != rays_d.shape:
        raise RuntimeError("rays_d and rgb must be (P,R,3)")
    P, R = rays_d.shape[:2]
    _checks(torch.float32, rays_d=rays_d, rgb=rgb)
    if opacity is not None:
        _check("opacity", opacity, torch.float32)
        if opacity.numel() != P * R:
            raise RuntimeError("opacity must be (P,R)")
        if trans_sh is None:
            trans_sh = torch.empty(P, 9, device=rays_d.device)
    elif trans_sh is not None:
        raise RuntimeError("trans_sh needs opacity")
    if rgb_sh is None:
        rgb_sh = torch.empty(P, 9, 3, device=rays_d.device)
    _check("rgb_sh", rgb_sh, torch.float32)
    if rgb_sh.numel() != P * 27 or (trans_sh is not None and trans_sh.numel() != P * 9):
        raise RuntimeError("rgb_sh must be (P,9,3) and trans_sh (P,9)")
    if trans_sh is not None:
        _check("trans_sh", trans_sh, torch.float32)
    kernels().ngp_probe_sh9_project(rays_d, rgb, opacity, P, R, rgb_sh, trans_sh, _stream())
    return rgb_sh, trans_sh


# -------------------------------------------------------- occupancy grid
def morton3D(coords):
    _check("coords", coords, torch.int32)
    out = torch.empty(coords.shape[0], dtype=torch.int32, device=coords.device)
    kernels().ngp_morton3d(coords, coords.shape[0], out, _stream())
    return out


def morton3D_invert(indices):
    _check("indices", indices, torch.int32)
    out = torch.empty(indices.shape[0], 3, dtype=torch.int32, device=indices.device)
    kernels().ngp_morton3d_invert(indices, indices.shape[0], out, _stream())
    return out


def packbits(density_grid, density_threshold, density_bitfield):
    """In place on density_bitfield.  density_threshold may be a float or a
    1-element device tensor (then no host sync is needed)."""
    _check("density_grid", density_grid, torch.float32)
    _check("density_bitfield", density_bitfield, torch.uint8)
    if density_grid.numel() != 8 * density_bitfield.numel():
        raise RuntimeError("density_grid must hold 8 cells per bitfield byte")
    if isinstance(density_threshold, torch.Tensor):
        _check("density_threshold", density_threshold, torch.float32)
        thr_dev, thr = density_threshold, 0.0
    else:
        thr_dev, thr = None, float(density_threshold)
    kernels().ngp_packbits(density_grid, density_bitfield.numel(), thr, thr_dev, density_bitfield, _stream())


def bitfield_summary(density_bitfield, grid_size=128, out=None):
    """ngp_bitfield_summary: 2 x (n_bytes/256) i32 words: bit w = (64-bit word w
    of the bitfield != 0), then the same dilated by one 4^3 block.  The
    marchers keep it in LDS to skip empty blocks without a global load and
    rays that pass no occupied block (same results with or without it)."""
    _check("density_bitfield", density_bitfield, torch.uint8)
    n = density_bitfield.numel()
    if out is None:
        out = torch.empty(2 * ((n + 255) // 256), dtype=torch.int32, device=density_bitfield.device)
    kernels().ngp_bitfield_summary(density_bitfield, n, int(grid_size), out, _stream())
    return out


def _summary_arg(density_bitfield, cascades, grid_size):
    """Summary for a marcher launch, or None when the grid is not whole
    2048-cell words (the marcher then reads the bitfield directly)."""
    if (int(cascades) * int(grid_size) ** 3) % 2048 != 0 or density_bitfield.numel() % 8 != 0:
        return None
    return bitfield_summary(density_bitfield, grid_size)


# ----------------------------------------------------------- marching
def _march_args(rays_o, rays_d, hits_t, density_bitfield, cascades, scale, exp_step_factor, noise, grid_size,
                max_samples):
    """The training marchers' shared leading arguments, checked"""
    _checks(torch.float32, rays_o=rays_o, rays_d=rays_d, hits_t=hits_t)
    _check("density_bitfield", density_bitfield, torch.uint8)
    _check("noise", noise, torch.float32)
    return (rays_o, rays_d, hits_t, rays_o.shape[0], density_bitfield, int(cascades), int(grid_size), float(scale),
            float(exp_step_factor), noise, int(max_samples))


def march_train_count(rays_o, rays_d, hits_t, density_bitfield, cascades, scale, exp_step_factor, noise,
                      grid_size, max_samples):
    """Pass 1 -> (counts i32 (N), rays_a i64 (N,3) ray-ordered, total i64 (1)), no host sync."""
    n = rays_o.shape[0]
    dev = rays_o.device
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    rays_a = torch.empty(n, 3, dtype=torch.int64, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    kernels().ngp_march_train_count(*_march_args(rays_o, rays_d, hits_t, density_bitfield, cascades, scale,
                                                 exp_step_factor, noise, grid_size, max_samples),
                                    counts, rays_a, total, _stream())
    return counts, rays_a, total


def march_train_write(rays_o, rays_d, hits_t, density_bitfield, cascades, scale, exp_step_factor, noise,
                      grid_size, max_samples, rays_a, xyzs, dirs, deltas, ts):
    """Pass 2 into caller buffers (capacity >= total)."""
    args = _march_args(rays_o, rays_d, hits_t, density_bitfield, cascades, scale, exp_step_factor, noise, grid_size,
                       max_samples)
    _check("rays_a", rays_a, torch.int64)
    _checks(torch.float32, xyzs=xyzs, dirs=dirs, deltas=deltas, ts=ts)
    kernels().ngp_march_train_write(*args, rays_a, xyzs, dirs, deltas, ts, _stream())


def raymarching_train(rays_o, rays_d, hits_t, density_bitfield, cascades, scale, exp_step_factor, noise,
                      grid_size, max_samples):
    """raymarching.cu:283-332 -> [rays_a, xyzs, dirs, deltas, ts, counter].
    counter = [total_samples, n_rays] (int32, like the reference's).  Single
    walk per ray into slot scratch, then one host sync to size the outputs
    (the reference syncs on counter[0] slicing, custom_functions.py:91-96)."""
    n = rays_o.shape[0]
    dev = rays_o.device
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    rays_a = torch.empty(n, 3, dtype=torch.int64, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    slot_t = torch.empty(n * int(max_samples), device=dev)
    slot_dt = torch.empty(n * int(max_samples), device=dev)
    args = _march_args(rays_o, rays_d, hits_t, density_bitfield, cascades, scale, exp_step_factor, noise, grid_size,
                       max_samples)
    summ = _summary_arg(density_bitfield, cascades, grid_size)
    K = kernels()
    K.ngp_march_train_slots(*args, counts, rays_a, total, slot_t, slot_dt, summ, _stream())
    N = int(total.item())
    xyzs = torch.empty(N, 3, device=dev)
    dirs = torch.empty(N, 3, device=dev)
    deltas = torch.empty(N, device=dev)
    ts = torch.empty(N, device=dev)
    if N > 0:
        K.ngp_march_train_compact(rays_o, rays_d, rays_a, n, slot_t, slot_dt, int(max_samples), xyzs, dirs, deltas, ts,
                                  _stream())
    counter = torch.stack([total[0].to(torch.int32), torch.full_like(total[0], n, dtype=torch.int32)])
    return [rays_a, xyzs, dirs, deltas, ts, counter]


def raymarching_test(rays_o, rays_d, hits_t, alive_indices, density_bitfield, cascades, scale, exp_step_factor,
                     grid_size, max_samples, N_samples):
    """raymarching.cu:407-454; hits_t (N_rays,2) is updated in place."""
    n = alive_indices.shape[0]
    dev = rays_o.device
    xyzs = torch.empty(n, N_samples, 3, device=dev)
    dirs = torch.empty(n, N_samples, 3, device=dev)
    deltas = torch.empty(n, N_samples, device=dev)
    ts = torch.empty(n, N_samples, device=dev)
    neff = torch.empty(n, dtype=torch.int32, device=dev)
    summ = _summary_arg(density_bitfield, cascades, grid_size)
    _checks(torch.float32, rays_o=rays_o, rays_d=rays_d, hits_t=hits_t)
    _check("alive_indices", alive_indices, torch.int64)
    _check("density_bitfield", density_bitfield, torch.uint8)
    kernels().ngp_march_test(rays_o, rays_d, hits_t, alive_indices, n, density_bitfield, int(cascades), int(grid_size),
                             float(scale), float(exp_step_factor), int(N_samples), int(max_samples), xyzs, dirs,
                             deltas, ts, neff, summ, _stream())
    return [xyzs, dirs, deltas, ts, neff]


# ---------------------------------------------------------- compositing
def composite_train_fw(sigmas, rgbs, deltas, ts, rays_a, T_threshold):
    """volumerendering.cu:47-83 -> [total_samples (N_rays) i64, opacity, depth, rgb, ws]"""
    nr, N = rays_a.shape[0], sigmas.shape[0]
    dev = sigmas.device
    op = torch.empty(nr, device=dev)
    dep = torch.empty(nr, device=dev)
    rgb = torch.empty(nr, 3, device=dev)
    ws = torch.empty(N, device=dev)
    tot = torch.empty(nr, dtype=torch.int64, device=dev)
    _checks(torch.float32, sigmas=sigmas, rgbs=rgbs, deltas=deltas, ts=ts)
    _check("rays_a", rays_a, torch.int64)
    kernels().ngp_composite_train_fw(sigmas, rgbs, deltas, ts, rays_a, nr, float(T_threshold), tot, op, dep, rgb, ws,
                                     _stream())
    return [tot, op, dep, rgb, ws]


def composite_train_bw(dL_dopacity, dL_ddepth, dL_drgb, dL_dws, sigmas, rgbs, ws, deltas, ts, rays_a, opacity,
                       depth, rgb, T_threshold):
    """volumerendering.cu:153-201 -> [dL_dsigmas (N), dL_drgbs (N,3)]"""
    N, nr = sigmas.shape[0], rays_a.shape[0]
    dev = sigmas.device
    dsig = torch.empty(N, device=dev)
    drgbs = torch.empty(N, 3, device=dev)
    _checks(torch.float32, dL_dopacity=dL_dopacity, dL_ddepth=dL_ddepth, dL_drgb=dL_drgb, dL_dws=dL_dws, sigmas=sigmas,
            rgbs=rgbs, ws=ws, deltas=deltas, ts=ts)
    _check("rays_a", rays_a, torch.int64)
    _checks(torch.float32, opacity=opacity, depth=depth, rgb=rgb)
    kernels().ngp_composite_train_bw(dL_dopacity, dL_ddepth, dL_drgb, dL_dws, sigmas, rgbs, ws, deltas, ts, rays_a, nr,
                                     opacity, depth, rgb, float(T_threshold), dsig, drgbs, _stream())
    return [dsig, drgbs]


def ray_segment_sum(dL_dxyzs, dL_ddirs, ts, rays_a, n_rays=None):
    """RayMarcher.backward's segment sums (custom_functions.py:107-110) -> [dL_drays_o, dL_drays_d] (n_rays,3):
    per row (ray, start, N) of rays_a, sum dL_dxyzs and sum (ts * dL_dxyzs + dL_ddirs) over the ray's
    samples (dL_ddirs may be None).  Run-to-run bit-identical (no atomics)."""
    nr = rays_a.shape[0] if n_rays is None else int(n_rays)
    if rays_a.shape[0] > nr:
        raise RuntimeError("rays_a has more rows than n_rays")
    N = dL_dxyzs.shape[0]
    if ts.numel() != N or (dL_ddirs is not None and dL_ddirs.numel() != 3 * N):
        raise RuntimeError("dL_dxyzs (N,3), dL_ddirs (N,3) and ts (N) must agree")
    dev = dL_dxyzs.device
    do = torch.zeros(nr, 3, device=dev)
    dd = torch.zeros(nr, 3, device=dev)
    _check("dL_dxyzs", dL_dxyzs, torch.float32)
    if dL_ddirs is not None:
        _check("dL_ddirs", dL_ddirs, torch.float32)
    _check("ts", ts, torch.float32)
    _check("rays_a", rays_a, torch.int64)
    kernels().ngp_ray_segment_sum(dL_dxyzs, dL_ddirs, ts, N, rays_a, rays_a.shape[0], do, dd, _stream())
    return [do, dd]


def composite_test_fw(sigmas, rgbs, deltas, ts, hits_t, alive_indices, T_threshold, N_eff_samples, opacity, depth,
                      rgb):
    """volumerendering.cu:251-284; alive/opacity/depth/rgb updated in place."""
    n = alive_indices.shape[0]
    Ns = sigmas.shape[1] if sigmas.dim() == 2 else 1
    _checks(torch.float32, sigmas=sigmas, rgbs=rgbs, deltas=deltas, ts=ts)
    _check("alive_indices", alive_indices, torch.int64)
    _check("N_eff_samples", N_eff_samples, torch.int32)
    _checks(torch.float32, opacity=opacity, depth=depth, rgb=rgb)
    kernels().ngp_composite_test_fw(sigmas, rgbs, deltas, ts, n, Ns, alive_indices, float(T_threshold), N_eff_samples,
                                    opacity, depth, rgb, _stream())


def ray_sphere_intersect(*args, **kwargs):
    raise NotImplementedError("ray_sphere_intersect is never called by the reference (intersection.cu:103-197); "
                              "out of scope (SURVEY.md §2 row 3)")


def distortion_loss_fw(ws, deltas, ts, rays_a):
    """losses.cu:62-107 -> [loss (N_rays), ws_inclusive_scan (N), wts_inclusive_scan (N)]
    (zero-initialised like the reference's torch::zeros outputs)."""
    _checks(torch.float32, ws=ws, deltas=deltas, ts=ts)
    _check("rays_a", rays_a, torch.int64)
    nr, N = rays_a.shape[0], ws.shape[0]
    loss = torch.zeros(nr, device=ws.device)
    wsi, wtsi = torch.zeros(N, device=ws.device), torch.zeros(N, device=ws.device)
    kernels().ngp_distortion_loss_fw(ws, deltas, ts, rays_a, nr, loss, wsi, wtsi, _stream())
    return [loss, wsi, wtsi]


def distortion_loss_bw(dL_dloss, ws_inclusive_scan, wts_inclusive_scan, ws, deltas, ts, rays_a):
    """losses.cu:143-173 -> dL_dws (N)"""
    _checks(torch.float32, dL_dloss=dL_dloss, ws_inclusive_scan=ws_inclusive_scan,
            wts_inclusive_scan=wts_inclusive_scan, ws=ws, deltas=deltas, ts=ts)
    _check("rays_a", rays_a, torch.int64)
    dws = torch.zeros(ws.shape[0], device=ws.device)
    kernels().ngp_distortion_loss_bw(dL_dloss, ws_inclusive_scan, wts_inclusive_scan, ws, deltas, ts, rays_a,
                                     rays_a.shape[0], dws, _stream())
    return dws


def density_scatter_last(tmp, indices, sigmas):
    """tmp.view(-1)[indices] = sigmas (models/networks.py:268) with torch's
    sequential index_put_ semantics on duplicate indices (the last one in
    list order wins), deterministically on the GPU (a device index_put_
    leaves the winner to the scheduler): ngp_density_scatter_last's 64-bit
    (position, sigma) keys, then the winners' sigmas into tmp (f32, in place;
    cells not listed keep their value; sigma is clamped at 0)."""
    _check("tmp", tmp, torch.float32)
    idx = indices.reshape(-1).long().contiguous()
    sig = sigmas.reshape(-1).float().contiguous()
    key = torch.zeros(tmp.numel(), dtype=torch.int64, device=tmp.device)
    kernels().ngp_density_scatter_last(idx, sig, idx.numel(), 0, key, _stream())
    hit = key != 0
    val = (key & 0xFFFFFFFF).to(torch.int32).view(torch.float32)
    flat = tmp.view(-1)
    flat.copy_(torch.where(hit, val, flat))
    return tmp


def erode_decay(count_grid, decay=0.95):
    """Per-cell erode decay clamp(decay**(1/count_grid), 0.1, 0.95)
    (models/networks.py:270-272), for ngp_density_grid_ema's decay_cells.
    count_grid is fixed once mark_invisible_cells ran, so this is evaluated
    once, with torch on the host: the values are the reference expression's
    CPU evaluation bit for bit (a device pow may differ in the last ulp).
    Cells no camera sees (count 0 -> 0.1) hold density -1 and never decay."""
    return torch.clamp(decay ** (1 / count_grid.detach().float().cpu()), 0.1, 0.95)
