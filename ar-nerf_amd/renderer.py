"""Graph-captured test-time renderer (BASELINE config 5).

The reference renders a frame with the host loop of __render_rays_test
(models/rendering.py:162-253): per iteration a host-side N_samples decision,
vren.raymarching_test, model(xyzs, dirs) on the valid samples,
vren.composite_test_fw and a boolean-mask compaction of the alive rays --
a host sync and ~10 launches per iteration, ~20-40 iterations per frame.

TestRenderer runs the same loop with every decision in device memory
(include/ngp_amd.h "device-resident test-time render"): one iteration is
  ngp_render_test_march   (loop test, N_samples, march, valid-sample list)
  ngp_field_encode_mlp over the list (NGP.forward: encode + MLPs in one launch)
  [ngp_tonemap_forward over the same list, in place on the colours: a model
   built with use_exposure, whose field output is log radiance]
  ngp_render_test_composite (composite_test_fw + survivor compaction)
and the iterations are captured in HIP graphs: a frame is graph A (begin +
summary + `iters_per_graph` iterations), then graph B (`iters_tail` more)
only while the device says the loop is still running -- one host sync per
graph; iterations after the loop ends are no-ops (early exits).
Results (opacity, depth, rgb, total_samples) equal the host loop's bit for
bit: tests/test_renderer_gpu.py.

InsertRenderer is the same loop for the insertion app's frames:
the ray count comes from device memory (ngp_insert_frame_begin,
ngp_render_test_march_n, ngp_insert_frame_finish), so one renderer sized for
the frame renders any screen rectangle without re-capture:
tests/test_insert_gpu.py.
"""
from __future__ import annotations

import ctypes

import torch

import hashgrid as HG
import vren
from capi import C

MAX_SAMPLES = 1024     # models/rendering.py:7
NEAR_DISTANCE = 0.01   # models/rendering.py:8
STATE_WORDS = C["NGP_RENDER_STATE_WORDS"]
RS_ACTIVE, RS_VALID, RS_TOTAL, RS_ITERS = 4, 5, 6, 7


class TestRenderer:
    """Fixed-shape renderer for batches of n_rays rays (a full frame:
    n_rays = W*H).  params16 / density_bitfield are read through stable
    device buffers: `params16` is used in place (refresh it with copy_), the
    bitfield is re-read every frame (its summary is rebuilt inside graph A)."""

    def __init__(self, n_rays, grid: HG.HashGrid, params16, density_bitfield, cascades, scale, grid_size=128,
                 exp_step_factor=0.0, T_threshold=1e-4, max_samples=MAX_SAMPLES, iters_per_graph=16,
                 bg_rgb=(0.0, 0.0, 0.0), use_graphs=True, iters_tail=None, rgb_act=0, tone16=None, tone_mode=None):
        iters_tail = iters_per_graph if iters_tail is None else iters_tail
        if min(iters_per_graph, iters_tail) < 2 or iters_per_graph % 2 or iters_tail % 2:
            raise ValueError("iters_per_graph / iters_tail must be even (alive lists alternate per iteration)")
        if int(rgb_act) not in (HG.RGB_SIGMOID, HG.RGB_NONE, HG.RGB_LEAKY_RELU, HG.RGB_RELU):
            raise ValueError(f"rgb_act must be one of hashgrid.RGB_*, got {rgb_act}")
        self.rgb_act = int(rgb_act)  # colour-output mode of the field (baked into the captured graphs)
        dev = params16.device
        # exposure tonemappers between the field and the composite: tone16 is read through
        # a stable buffer like params16, the exposure through a one-element device buffer (set_exposure)
        self.tone_mode = None if tone_mode is None else int(tone_mode)
        self.tone16 = tone16
        if self.tone_mode is not None:
            if self.tone_mode not in (HG.TONE_LDR, HG.TONE_RADIANCE):
                raise ValueError(f"tone_mode must be hashgrid.TONE_LDR / TONE_RADIANCE or None, got {tone_mode}")
            if self.rgb_act != HG.RGB_NONE:
                raise ValueError("the tonemappers take the colour net's raw output: rgb_act must be hashgrid.RGB_NONE")
            if self.tone_mode == HG.TONE_LDR:
                vren._check("tone16", tone16, torch.float16)
                if tone16.numel() != HG.TONE_PARAMS:
                    raise ValueError(f"tone16 must hold {HG.TONE_PARAMS} values, got {tone16.numel()}")
        elif tone16 is not None:
            raise ValueError("tone16 needs a tone_mode")
        self.exposure = torch.ones(1, dtype=torch.float32, device=dev)
        vren._check("params16", params16, torch.float16)
        vren._check("density_bitfield", density_bitfield, torch.uint8)
        self.n_rays, self.grid, self.params16, self.bitfield = int(n_rays), grid, params16, density_bitfield
        self.cascades, self.scale, self.grid_size = int(cascades), float(scale), int(grid_size)
        self.esf, self.T_threshold, self.max_samples = float(exp_step_factor), float(T_threshold), int(max_samples)
        # rendering.py:185: min_samples = 1 if exp_step_factor == 0 else 4
        self.min_samples = 1 if self.esf == 0 else 4
        # graph A: frame opening + K iterations; graph B (replayed while the loop runs): K_tail
        self.K, self.K_tail, self.use_graphs = int(iters_per_graph), int(iters_tail), bool(use_graphs)
        self.bg = (ctypes.c_float * 3)(*[float(b) for b in bg_rgb])
        self.cap = int(vren.kernels().ngp_render_test_capacity(self.n_rays, self.min_samples))
        n, cap = self.n_rays, self.cap
        f = dict(device=dev, dtype=torch.float32)
        self.rays_o = torch.zeros(n, 3, **f)
        self.rays_d = torch.zeros(n, 3, **f)
        self.hits_t = torch.zeros(n, 2, **f)
        self.opacity = torch.zeros(n, **f)
        self.depth = torch.zeros(n, **f)
        self.rgb = torch.zeros(n, 3, **f)
        self.state = torch.zeros(STATE_WORDS, dtype=torch.int64, device=dev)
        self.alive = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)]
        self.n_eff = torch.zeros(n, dtype=torch.int32, device=dev)
        self.xyzs = torch.zeros(cap, 3, **f)
        self.dirs = torch.zeros(cap, 3, **f)
        self.deltas = torch.zeros(cap, **f)
        self.ts = torch.zeros(cap, **f)
        self.sigmas = torch.zeros(cap, **f)
        self.rgbs = torch.zeros(cap, 3, **f)
        self.sample_idx = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.enc = torch.zeros(8 * cap * 4, dtype=torch.float16, device=dev)  # pair-major (8, cap, 4)
        self.summary = torch.zeros(2 * ((density_bitfield.numel() + 255) // 256), dtype=torch.int32, device=dev)
        self.n_valid = self.state[RS_VALID:]  # (the valid-sample list's length, where the field kernel reads it)
        self._graphs = {}
        self.n_captures = 0  # graphs captured so far (two per renderer: A and B)
        self.last_iterations = 0
        # full-frame camera (render_pose)
        self._dirs = None

    # ------------------------------------------------------------ pieces
    def _march(self, par):
        """Loop test, N_samples and the march of one iteration (rendering.py:186-203)."""
        vren.kernels().ngp_render_test_march(
            self.rays_o, self.rays_d, self.hits_t, self.n_rays, self.bitfield, self.cascades, self.grid_size,
            self.scale, self.esf, MAX_SAMPLES, self.min_samples, self.max_samples, par, self.state, self.alive[par],
            self.summary, self.xyzs, self.dirs, self.deltas, self.ts, self.n_eff, self.sample_idx, vren._stream())

    def _iteration(self, k):
        """One loop iteration (rendering.py:186-236) on the current stream."""
        K, s, par = vren.kernels(), vren._stream(), k & 1
        self._march(par)
        # model(xyzs[valid], dirs[valid]) (rendering.py:204-218): NGP.forward over the list
        # (encode + MLPs in one launch; no encoding kept: nothing goes backward)
        K.ngp_field_encode_mlp_act(self.xyzs, self.dirs, self.cap, self.n_valid, self.sample_idx, self.grid.desc,
                                   self.params16[HG.MLP_PARAMS:], self.params16, None, self.sigmas, self.rgbs, None,
                                   self.rgb_act, s)
        if self.tone_mode is not None:  # log radiance -> colour on the valid samples (networks.py:158-163)
            K.ngp_tonemap_forward(self.rgbs, self.exposure, 1, self.cap, self.n_valid, self.sample_idx, self.tone16,
                                  self.tone_mode, self.rgbs, s)
        K.ngp_render_test_composite(self.sigmas, self.rgbs, self.deltas, self.ts, self.n_eff, self.n_rays, par,
                                    self.state, self.alive[par], self.alive[par ^ 1], self.T_threshold, self.opacity,
                                    self.depth, self.rgb, s)

    def _begin(self):
        vren.kernels().ngp_render_test_begin(self.n_rays, self.state, self.alive[0], self.opacity, self.depth, self.rgb,
                                             vren._stream())
        vren.bitfield_summary(self.bitfield, self.grid_size, out=self.summary)

    def _run(self, first):
        """K iterations (graph A, which also opens the frame) or K_tail (graph B)."""
        if first:
            self._begin()
        for k in range(self.K if first else self.K_tail):
            self._iteration(k)

    def _launch(self, first):
        if not self.use_graphs:
            self._run(first)
            return
        self._graph(first).replay()

    def _graph(self, first):
        """Graph A (first) or B, captured on first use (capture does not execute)."""
        g = self._graphs.get(first)
        if g is None:
            g = torch.cuda.CUDAGraph()
            torch.cuda.current_stream().synchronize()
            with vren.graph_capture(g):
                self._run(first)
            self._graphs[first] = g
            self.n_captures += 1
        return g

    # --------------------------------------------------------------- API
    @torch.no_grad()
    def render_loaded(self, bg_sh=None):
        """Render the rays already in self.rays_o / rays_d / hits_t.  bg_sh: a
        device (9,3) SH9 light blended in behind the rays (SH_bkg,
        rendering.py:241-250) in place of the constant background colour."""
        self._launch(True)
        while int(self.state[RS_ACTIVE].item()):
            self._launch(False)
        self.last_iterations = int(self.state[RS_ITERS].item())
        # (the finish runs outside the captured graphs: either one, no re-capture)
        if bg_sh is not None:
            vren.render_test_finish_sh(self.opacity, self.rays_d, bg_sh, self.rgb)
        else:
            vren.kernels().ngp_render_test_finish(self.opacity, self.n_rays, self.bg, self.rgb, vren._stream())
        return {"opacity": self.opacity, "depth": self.depth, "rgb": self.rgb,
                "total_samples": self.state[RS_TOTAL]}

    @torch.no_grad()
    def render(self, rays_o, rays_d, hits_t, bg_sh=None):
        """__render_rays_test(model, rays_o, rays_d, hits_t) for hits_t (n_rays,2)
        (the caller's hits_t[:, 0], near-clamped): returns views of the
        renderer's buffers (copy them to keep them past the next frame).
        bg_sh: see render_loaded."""
        if rays_o.shape[0] != self.n_rays:
            raise RuntimeError(f"TestRenderer was built for {self.n_rays} rays, got {rays_o.shape[0]}")
        self.rays_o.copy_(rays_o.reshape(-1, 3))
        self.rays_d.copy_(rays_d.reshape(-1, 3))
        self.hits_t.copy_(hits_t.reshape(-1, 2))
        return self.render_loaded(bg_sh)

    def set_exposure(self, e):
        """The frame's exposure (a number or a one-element tensor; None: unit): written to the device
        scalar the captured tonemap launches read, so the next frame follows it without re-capture."""
        if e is None:
            self.exposure.fill_(1.0)
        elif isinstance(e, torch.Tensor):
            if e.numel() != 1:
                raise ValueError(f"the device loop takes one exposure per frame, got {tuple(e.shape)}")
            self.exposure.copy_(e.detach().reshape(1))
        else:
            self.exposure.fill_(float(e))

    def set_camera(self, directions, center, half_size):
        """Per-pixel camera directions (H*W, 3) (datasets/ray_utils.py:7-42)
        and the scene box, for render_pose."""
        if directions.shape[0] != self.n_rays:
            raise RuntimeError("directions must have n_rays rows")
        self._dirs = directions.float().contiguous()
        self._center, self._half = center.float().contiguous(), half_size.float().contiguous()
        dev = self._dirs.device
        self._img = torch.zeros(self.n_rays, dtype=torch.int64, device=dev)
        self._pix = torch.arange(self.n_rays, dtype=torch.int64, device=dev)
        self._pose = torch.zeros(1, 3, 4, device=dev)

    @torch.no_grad()
    def render_pose(self, c2w):
        """get_rays(directions, c2w) (ray_utils.py:45-70) + AABB + near clamp
        (rendering.py:25-31) + the test loop, for one (3,4) camera-to-world pose."""
        if self._dirs is None:
            raise RuntimeError("call set_camera() first")
        self._pose.copy_(c2w.reshape(1, 3, 4))
        vren.kernels().ngp_raygen_aabb(self._dirs, self._pose, self._img, self._pix, self.n_rays, self._center,
                                       self._half, NEAR_DISTANCE, self.rays_o, self.rays_d, self.hits_t, vren._stream())
        return self.render_loaded()


def _model_kwargs(model, output_radiance, kwargs):
    """The model's colour mode (relu for a raw-HDR model with output_radiance) and,
    for an exposure model, its tonemap mode and tone shadow, as renderer kwargs."""
    kwargs.setdefault('rgb_act', model.rgb_mode(output_radiance))
    if getattr(model, 'use_exposure', False):  # (its tone shadow in place: refresh with rr.tone16.copy_)
        kwargs.setdefault('tone_mode', model.tone_mode(output_radiance))
        kwargs.setdefault('tone16', model._tone_shadow.get())
    return kwargs


def for_model(model, n_rays, output_radiance=False, **kwargs):
    """TestRenderer over a models.networks.NGP (its fp16 shadow and bitfield;
    the model's colour mode, relu for a raw-HDR model with output_radiance)."""
    kwargs = _model_kwargs(model, output_radiance, kwargs)
    return TestRenderer(n_rays, model.grid, model._shadow.get(), model.density_bitfield, model.cascades,
                        model.scale, model.grid_size, **kwargs)


HEADER_WORDS = C["NGP_INSERT_HEADER_WORDS"]


class InsertRenderer(TestRenderer):
    """The insertion app's per-frame render (insert/main.py:620-684,
    Insertor.render_insert_object) for one camera: a screen rectangle of the
    H x W frame, every ray ended at the virtual object's surface
    (mesh_depth_map, rendering.py:38-44), the shaded object blended in behind
    what is left (IM_bkg, rendering.py:245-250), scattered into the persistent
    canvases frame_rgb / frame_depth (main.py:652-654) with the surface points
    frame_pts = rays_o + rays_d * depth (main.py:429).

    The rectangle is a device value: buffers and graphs are
    sized for the whole frame and captured once, whatever rectangles follow
    (n_captures stays at 2); a rectangle's pixels equal those of a TestRenderer
    built for its ray count, bit for bit.

    directions (H*W,3); center / half_size: the model's box.  `buffers` may
    give preallocated obj_rgb (H*W,3), obj_depth (H*W), frame_rgb (H*W,3),
    frame_depth (H*W), frame_pts (H*W,3) tensors (contiguous fp32, e.g. views
    of an application's own allocations)."""

    def __init__(self, H, W, directions, center, half_size, grid, params16, density_bitfield, cascades, scale,
                 grid_size=128, buffers=None, **kwargs):
        H, W = int(H), int(W)
        if H < 1 or W < 1 or H * W >= 2 ** 31:
            raise ValueError(f"bad frame size {H} x {W}")
        super().__init__(H * W, grid, params16, density_bitfield, cascades, scale, grid_size, **kwargs)
        self.H, self.W = H, W
        dev, n = params16.device, H * W
        vren._check("directions", directions, torch.float32)
        if directions.numel() != 3 * n:
            raise ValueError(f"directions must hold H*W = {n} rows of 3, got {tuple(directions.shape)}")
        self._dirs = directions
        self._center, self._half = center.float().contiguous(), half_size.float().contiguous()
        self._pose = torch.zeros(3, 4, dtype=torch.float32, device=dev)
        buffers = dict(buffers or {})
        for name, cols in (("obj_rgb", 3), ("obj_depth", 1), ("frame_rgb", 3), ("frame_depth", 1), ("frame_pts", 3)):
            t = buffers.pop(name, None)
            if t is None:
                t = torch.zeros((n, 3) if cols == 3 else (n,), dtype=torch.float32, device=dev)
            vren._check(name, t, torch.float32)
            if t.numel() != n * cols:
                raise ValueError(f"{name} must hold {n * cols} values, got {tuple(t.shape)}")
            setattr(self, name, t)
        if buffers:
            raise ValueError(f"unknown buffers {sorted(buffers)}")
        self.rect = torch.zeros(4, dtype=torch.int32, device=dev)  # (hs, ws, hl, wl): graph A reads it, the kernel clamps it
        self._rect_host = torch.zeros(4, dtype=torch.int32).pin_memory()
        self.header = torch.zeros(HEADER_WORDS, dtype=torch.int64, device=dev)
        # the shadow steps' buffers: the cast-shadow factor of every pixel's surface point, the
        # shadowed copy of frame_rgb (the canvas itself stays unshadowed), and the (H*W, L) self-shadow decay,
        # which self_shadow_decay sizes for the frame's number of lights
        self.frame_factor = torch.zeros(n, dtype=torch.float32, device=dev)
        self.frame_shadowed = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        self.decay = None

    # ------------------------------------------------------------ pieces
    def _begin(self):
        vren.kernels().ngp_insert_frame_begin(
            self.rect, self.H, self.W, self._dirs, self._pose, self._center, self._half, NEAR_DISTANCE,
            self.obj_depth, self.rays_o, self.rays_d, self.hits_t, self.state, self.alive[0], self.opacity,
            self.depth, self.rgb, self.header, vren._stream())
        vren.bitfield_summary(self.bitfield, self.grid_size, out=self.summary)

    def _march(self, par):
        vren.kernels().ngp_render_test_march_n(
            self.rays_o, self.rays_d, self.hits_t, self.header, self.n_rays, self.bitfield, self.cascades,
            self.grid_size, self.scale, self.esf, MAX_SAMPLES, self.min_samples, self.max_samples, par, self.state,
            self.alive[par], self.summary, self.xyzs, self.dirs, self.deltas, self.ts, self.n_eff, self.sample_idx,
            vren._stream())

    # --------------------------------------------------------------- API
    def _set_rect(self, rect):
        if isinstance(rect, torch.Tensor):
            if rect.dtype != torch.int32 or rect.numel() != 4 or not rect.is_cuda:
                raise ValueError("rect must be four ints or a device int32[4] tensor (hs, ws, hl, wl)")
            if rect.data_ptr() != self.rect.data_ptr():
                self.rect.copy_(rect.reshape(4))  # (device to device: no host wait)
            return
        hs, ws, hl, wl = (int(v) for v in rect)
        if not (0 <= hs <= hl <= self.H and 0 <= ws <= wl <= self.W):
            raise ValueError(f"rect (hs, ws, hl, wl) = {(hs, ws, hl, wl)} does not lie in the {self.H} x {self.W} frame")
        # (the previous frame ended in a host sync after its copy: the pinned words are free again)
        self._rect_host.copy_(torch.tensor([hs, ws, hl, wl], dtype=torch.int32))
        self.rect.copy_(self._rect_host, non_blocking=True)

    @torch.no_grad()
    def render_rect(self, c2w, rect, obj_rgb=None, obj_depth=None):
        """One insertion frame: rows hs..hl, columns ws..wl (rect = (hs, ws, hl, wl): four ints, checked here,
        or a device int32[4] tensor, clamped to the frame by the kernel) seen from the (3,4) pose c2w, with the
        whole-frame object images obj_rgb (H,W,3) / obj_depth (H,W) (None: what the renderer's buffers hold).
        Returns views of the canvases (pixels outside the rectangle keep the last frame's values) and
        total_samples; copy them to keep them past the next frame."""
        self._pose.copy_(c2w.reshape(3, 4))
        self._set_rect(rect)
        if obj_rgb is not None:
            self.obj_rgb.copy_(obj_rgb.reshape(self.obj_rgb.shape))
        if obj_depth is not None:
            self.obj_depth.copy_(obj_depth.reshape(self.obj_depth.shape))
        if self.use_graphs and not self._graphs:  # both graphs now: no later frame, whatever its rectangle, captures
            self._graph(True)
            self._graph(False)
        self._launch(True)
        while int(self.state[RS_ACTIVE].item()):
            self._launch(False)
        self.last_iterations = int(self.state[RS_ITERS].item())
        # (the closing launch runs outside the captured graphs, like TestRenderer's finish)
        vren.kernels().ngp_insert_frame_finish(
            self.header, self.H, self.W, self.opacity, self.depth, self.rgb, self.rays_o, self.rays_d, self.obj_rgb,
            self.frame_rgb, self.frame_depth, self.frame_pts, vren._stream())
        H, W = self.H, self.W
        return {"rgb": self.frame_rgb.view(H, W, 3), "depth": self.frame_depth.view(H, W),
                "pts": self.frame_pts.view(H, W, 3), "total_samples": self.state[RS_TOTAL]}

    @torch.no_grad()
    def shade_sg(self, c2w, bbox, normals, obj_depth, lSGs, metal=0.9, rough=0.2, albedo=None, decay=None,
                 clamp01=True):
        """The frame's object image on the device (shading.sg_shade): obj_depth (H,W) is
        written to the renderer's buffer and the object, seen from the (3,4) pose c2w inside the model's box
        bbox = (hs, ws, hl, wl) (four ints or a device int32[4] tensor; not the update rectangle), is shaded
        under the lights lSGs (L,7) straight into the obj_rgb buffer: no host copy.  A frame is then
        shade_sg(...) and render_rect(c2w, rect) with obj_rgb = obj_depth = None.  The launch is outside the
        captured graphs, so L may change from frame to frame.  Returns the obj_rgb buffer as (H,W,3)."""
        import shading
        self._pose.copy_(c2w.reshape(3, 4))
        shading._arg("obj_depth", obj_depth, torch.float32, self.n_rays, f"(H,W) = ({self.H},{self.W})")
        if obj_depth.data_ptr() != self.obj_depth.data_ptr():
            self.obj_depth.copy_(obj_depth.reshape(self.obj_depth.shape))
        return shading.sg_shade(self.H, self.W, self._dirs, self._pose, bbox, normals, self.obj_depth, lSGs,
                                metal=metal, rough=rough, albedo=albedo, decay=decay, clamp01=clamp01,
                                out=self.obj_rgb)

    @torch.no_grad()
    def self_shadow_decay(self, c2w, bbox, obj_depth, shadow, lSGs, scale, model_pos, rot_inv=None):
        """The frame's self-shadow decay on the device (sg_shadow.SGShadow.frame_decay):
        obj_depth (H,W) is written to the renderer's buffer and, for every pixel the object covers inside the
        model's box bbox, row p of the renderer's persistent (H*W, L) decay buffer is written (the buffer is
        reallocated when L changes and starts as ones; sg_shade reads covered rows only).  scale: the
        model's radius; model_pos (3); rot_inv (3,3) or None.  Returns the buffer: shade_sg(..., decay=it)
        follows.  Outside the captured graphs."""
        import shading
        self._pose.copy_(c2w.reshape(3, 4))
        shading._arg("obj_depth", obj_depth, torch.float32, self.n_rays, f"(H,W) = ({self.H},{self.W})")
        if obj_depth.data_ptr() != self.obj_depth.data_ptr():
            self.obj_depth.copy_(obj_depth.reshape(self.obj_depth.shape))
        import sg_shadow
        L = sg_shadow._lights_arg(lSGs)
        buf = self.decay
        if buf is None or buf.shape[1] != L:
            buf = self.decay = torch.ones(self.n_rays, L, dtype=torch.float32, device=self._pose.device)
        return shadow.frame_decay(self.H, self.W, self._dirs, self._pose, bbox, self.obj_depth, scale, model_pos,
                                  lSGs, buf, rot_inv)

    @torch.no_grad()
    def cast_shadow(self, shadow, lSGs, scale, model_pos, rot_inv=None):
        """The cast shadow of the frame the canvases hold (ssdf_shadow, main.py:492-519): the factor of
        every surface point of frame_pts (lSGs (L,7) with axes already rotated where rot_inv is given) into
        the frame_factor buffer, then frame_rgb times its 3 x 3 blur into the frame_shadowed buffer, which
        is returned as (H,W,3).  Eager, outside the captured graphs; frame_rgb / frame_depth / frame_pts
        keep their bits (later frames re-render rectangles of them)."""
        import sg_shadow
        shadow.calc_shadow_factor(scale, self.frame_pts, model_pos, lSGs, rot_inv, out=self.frame_factor)
        return sg_shadow.shadow_apply(self.frame_rgb, self.frame_factor, self.H, self.W, out=self.frame_shadowed)

    def render_frame(self, c2w, obj_rgb=None, obj_depth=None):
        """render_rect over the whole screen (the app's frame after a camera move)."""
        return self.render_rect(c2w, (0, 0, self.H, self.W), obj_rgb, obj_depth)

    def render_loaded(self, bg_sh=None):
        raise RuntimeError("InsertRenderer renders rectangles of its camera: use render_rect / render_frame")

    def set_camera(self, directions, center, half_size):
        raise RuntimeError("InsertRenderer is built for its camera")


def insert_for_model(model, H, W, directions, output_radiance=False, **kwargs):
    """InsertRenderer over a models.networks.NGP and its box, as for_model."""
    kwargs = _model_kwargs(model, output_radiance, kwargs)
    return InsertRenderer(H, W, directions, model.center, model.half_size, model.grid, model._shadow.get(),
                          model.density_bitfield, model.cascades, model.scale, model.grid_size, **kwargs)
