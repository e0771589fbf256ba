"""Insertion frames on the device loop (renderer.InsertRenderer,
models.rendering.render_insert; csrc/insert.hip) against the composed path they
replace: vren.raygen_aabb on the rectangle's pixels, the HOST loop
render(test_time=True, device_loop=False, IM_bkg=clip, mesh_depth_map=clip) with
the app's settings, and a torch scatter into the canvases.  Every comparison is
torch.equal on the rgb / depth / pts canvases and total_samples as an integer;
the golden fixture of the reference's own glue (tests/golden/insert_frame.npz)
is held within the project's 2e-3."""
import numpy as np
import pytest
import torch

import insert_ref as IR
import renderer as R
import synthetic as S
import vren
from fixture_model import load
from models.rendering import NEAR_DISTANCE, render, render_insert
from test_golden_gpu import _product_model
from test_renderer_gpu import _scene_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 48, 40                                      # W no multiple of 64, H != W
APP = dict(T_threshold=1e-2, max_samples=100)      # insert/main.py's render settings
SENTINEL = 1234.5


def _camera(scale):
    """directions (H*W,3) and one (3,4) pose looking at the box of half size `scale`"""
    sc = S.AnalyticScene(W=W, H=H, n_images=3)
    pose = sc.poses[1].clone()
    pose[:, 3] *= 2 * scale
    return sc.directions.to(DEV).contiguous(), pose.to(DEV).contiguous()


def _full_rays(model, dirs, pose, h=H, w=W):
    n = h * w
    return vren.raygen_aabb(dirs, pose.reshape(1, 3, 4), torch.zeros(n, dtype=torch.int64, device=DEV),
                            torch.arange(n, device=DEV), model.center, model.half_size, NEAR_DISTANCE)


def _object(model, dirs, pose, seed, h=H, w=W):
    """A synthetic object over the middle of the frame: colour (h,w,3) and a depth map (h,w) that puts pixels before
    the box (zero length), inside it, behind it, at 0 (no object) and at the fp32 numbers around 1e-6."""
    g = torch.Generator().manual_seed(seed)
    _, _, ht = _full_rays(model, dirs, pose, h, w)
    t1, t2 = ht[:, 0].reshape(h, w), ht[:, 1].reshape(h, w)
    frac = (torch.rand(h, w, generator=g) * 1.6 - 0.3).to(DEV)
    depth = t1 + (t2 - t1) * frac
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    disc = (((yy - h / 2) / (0.42 * h)) ** 2 + ((xx - w / 2) / (0.42 * w)) ** 2 < 1).to(DEV)
    depth = torch.where(disc & (t1 >= 0), depth, torch.zeros_like(depth)).clamp_min(0)
    eps = np.float32(1e-6)
    special = [0.0, 5e-7, float(eps), float(np.nextafter(eps, np.float32(0))), float(np.nextafter(eps, np.float32(1)))]
    flat = depth.reshape(-1)
    idx = torch.randperm(h * w, generator=g)[:5 * len(special)].to(DEV)
    flat[idx] = torch.tensor(special, device=DEV).repeat(5)
    flat[:4] = torch.tensor([0.3, 0.0, float(eps), 0.7], device=DEV)  # (the corners' neighbourhood is not all zero)
    flat[-2:] = 0.25
    return torch.rand(h, w, 3, generator=g).to(DEV), depth.contiguous()


def _junk(seed, h=H, w=W):
    g = torch.Generator().manual_seed(seed)
    return {"rgb": (torch.rand(h, w, 3, generator=g) + 2).to(DEV), "depth": (torch.rand(h, w, generator=g) + 2).to(DEV),
            "pts": (torch.rand(h, w, 3, generator=g) + 2).to(DEV)}


def _reference(model, dirs, pose, rect, obj_rgb, obj_depth, canvas, h=H, w=W, **kw):
    """The composed path, in place on the `canvas` dict -> total_samples (int)"""
    pix = torch.from_numpy(IR.rect_pixels(rect, h, w)).to(DEV)
    n = pix.numel()
    if n == 0:
        return 0
    o, d, _ = vren.raygen_aabb(dirs, pose.reshape(1, 3, 4), torch.zeros(n, dtype=torch.int64, device=DEV), pix,
                               model.center, model.half_size, NEAR_DISTANCE)
    with torch.no_grad():
        res = render(model, o, d, test_time=True, device_loop=False, IM_bkg=obj_rgb.reshape(-1, 3)[pix],
                     mesh_depth_map=obj_depth.reshape(-1)[pix], **APP, **kw)
    canvas["rgb"].view(-1, 3)[pix] = res["rgb"]
    canvas["depth"].view(-1)[pix] = res["depth"]
    canvas["pts"].view(-1, 3)[pix] = o + d * res["depth"][:, None]
    return int(res["total_samples"])


def _load_canvas(rr, canvas):
    rr.frame_rgb.copy_(canvas["rgb"].reshape(-1, 3))
    rr.frame_depth.copy_(canvas["depth"].reshape(-1))
    rr.frame_pts.copy_(canvas["pts"].reshape(-1, 3))


def _assert_frame(out, canvas, total, what=""):
    for k in ("rgb", "depth", "pts"):
        assert torch.equal(out[k], canvas[k]), (what, k)
    assert int(out["total_samples"]) == total, what


RECTS = [(0, 0, H, W),                                                       # the whole frame
         (0, 0, 1, 1), (0, W - 1, 1, W), (H - 1, 0, H, 1), (H - 1, W - 1, H, W),  # 1x1 at the four corners
         (20, 0, 21, W),                                                     # one full row
         (0, 13, H, 14),                                                     # one full column
         (9, 5, 26, 28),                                                     # 17 x 23 in the interior
         (10, 4, 10, 30),                                                    # empty: hl == hs
         (0, 0, H, W)]                                                       # the whole frame again


@pytest.mark.parametrize("scale,esf,occ", [(0.5, 0.0, 0.02), (16.0, 1 / 256, 0.01)])
def test_rectangle_sequence_through_one_renderer(scale, esf, occ):
    model = _scene_model(scale, occ, seed=5)
    dirs, pose = _camera(scale)
    obj_rgb, obj_depth = _object(model, dirs, pose, seed=3)
    # (short graphs: the full frames need graph A and several replays of graph B)
    rr = R.insert_for_model(model, H, W, dirs, exp_step_factor=esf, iters_per_graph=4, iters_tail=2, **APP)
    assert rr.min_samples == (1 if esf == 0 else 4)
    canvas = _junk(7)
    _load_canvas(rr, canvas)
    totals = []
    for rect in RECTS:
        total = _reference(model, dirs, pose, rect, obj_rgb, obj_depth, canvas, exp_step_factor=esf)
        out = rr.render_rect(pose, rect, obj_rgb, obj_depth)
        _assert_frame(out, canvas, total, rect)       # (the whole canvases: pixels outside keep the last call's bits)
        assert rr.n_captures == 2, rect
        assert int(rr.header[0]) == (rect[2] - rect[0]) * (rect[3] - rect[1])
        if rect[2] == rect[0]:
            assert rr.last_iterations == 0 and total == 0
        if rect == (0, 0, H, W) and esf == 0:  # (the cascaded frame, at >= 4 samples an iteration, ends inside graph A)
            assert rr.last_iterations > rr.K + rr.K_tail
        totals.append(total)
    assert totals[0] == totals[-1] > 0 and totals[7] > 0
    assert bool((canvas["rgb"] < 2).all())             # the full frames left no junk
    out = rr.render_frame(pose, obj_rgb, obj_depth)
    _assert_frame(out, canvas, totals[0], "render_frame")
    # Python-side checks of the rectangle
    for bad in [(-1, 0, 4, 4), (0, 0, H + 1, 4), (5, 0, 4, 4), (0, 9, 4, 8), (0, 0, 4, W + 1)]:
        with pytest.raises(ValueError):
            rr.render_rect(pose, bad, obj_rgb, obj_depth)


def _guarded(n, cols, pad=4096):
    """a contiguous (n, cols) view in the middle of a larger sentinel-filled allocation"""
    big = torch.full(((n + 2 * pad) * cols,), SENTINEL, device=DEV)
    view = big[pad * cols:(pad + n) * cols]
    return big, (view.view(n, cols) if cols > 1 else view)


def test_device_rectangle_is_clamped_by_the_kernel():
    model = _scene_model(0.5, 0.02, seed=5)
    dirs, pose = _camera(0.5)
    obj_rgb, obj_depth = _object(model, dirs, pose, seed=4)
    n = H * W
    bigs, bufs = {}, {}
    for name, cols in (("obj_rgb", 3), ("obj_depth", 1), ("frame_rgb", 3), ("frame_depth", 1), ("frame_pts", 3)):
        bigs[name], bufs[name] = _guarded(n, cols)
    rr = R.insert_for_model(model, H, W, dirs, buffers=bufs, **APP)
    canvas = _junk(8)
    _load_canvas(rr, canvas)
    # overhang by three pixels on two sides; on the other two; inverted; wholly outside -> (the clamped one, n)
    cases = [((-3, 5, 30, W + 3), (0, 5, 30, W), 30 * (W - 5)), ((7, -3, H + 3, 22), (7, 0, H, 22), (H - 7) * 22),
             ((30, 10, 20, 25), (30, 10, 20, 25), 0), ((H + 2, 0, H + 9, 5), (H, 0, H, 5), 0)]
    for given, clamped, n_rect in cases:
        assert IR.rect_clamp(given, H, W) == (clamped, n_rect)
        total = _reference(model, dirs, pose, clamped, obj_rgb, obj_depth, canvas)
        out = rr.render_rect(pose, torch.tensor(given, dtype=torch.int32, device=DEV), obj_rgb, obj_depth)
        _assert_frame(out, canvas, total, given)
        assert rr.header.tolist() == [n_rect, *clamped, H, W, 0]
        assert (total > 0) == (n_rect > 0)
    assert rr.n_captures == 2
    pad = 4096
    for name, big in bigs.items():
        cols = 3 if name in ("obj_rgb", "frame_rgb", "frame_pts") else 1
        assert bool((big[:pad * cols] == SENTINEL).all()) and bool((big[(pad + n) * cols:] == SENTINEL).all()), name
    with pytest.raises(ValueError):
        rr.render_rect(pose, torch.tensor([0, 0, 4, 4], device=DEV), obj_rgb, obj_depth)  # int64


def test_golden_fixture_of_the_reference_glue():
    fx = load("insert_frame")
    model = _product_model(fx)
    h, w = int(fx["H"]), int(fx["W"])
    rect = tuple(int(v) for v in fx["rect"])
    dirs, pose = torch.from_numpy(fx["directions"]).to(DEV), torch.from_numpy(fx["pose"]).to(DEV)
    obj_rgb, obj_depth = torch.from_numpy(fx["obj_rgb"]).to(DEV), torch.from_numpy(fx["obj_depth"]).to(DEV)
    rr = R.insert_for_model(model, h, w, dirs, **APP)
    rr.frame_rgb.copy_(torch.from_numpy(fx["canvas0_rgb"]).reshape(-1, 3))
    rr.frame_depth.copy_(torch.from_numpy(fx["canvas0_depth"]).reshape(-1))
    canvas = {"rgb": rr.frame_rgb.clone().view(h, w, 3), "depth": rr.frame_depth.clone().view(h, w),
              "pts": rr.frame_pts.clone().view(h, w, 3)}
    total = _reference(model, dirs, pose, rect, obj_rgb, obj_depth, canvas, h, w)
    out = rr.render_rect(pose, rect, obj_rgb, obj_depth)
    _assert_frame(out, canvas, total)
    pix = torch.from_numpy(fx["pix"])
    d_rgb = float((out["rgb"].cpu() - torch.from_numpy(fx["canvas_rgb"])).abs().max())
    d_depth = float((out["depth"].cpu() - torch.from_numpy(fx["canvas_depth"])[..., 0]).abs().max())
    d_pts = float((out["pts"].cpu().view(-1, 3)[pix] - torch.from_numpy(fx["pts"])).abs().max())
    print(f"insert_frame.npz: max |rgb| {d_rgb:.3e} |depth| {d_depth:.3e} |pts| {d_pts:.3e} "
          f"total_samples {total} (fixture {int(fx['total_samples'])})")
    assert d_rgb <= 2e-3 and d_depth <= 2e-3 and d_pts <= 2e-3
    # the rays themselves: the kernel's rows against the reference's get_rays and clipped hits_t
    # (rays_d: three-term fp32 dot products summed in another order than the reference's matmul, <= 6u * 1.7)
    n = pix.numel()
    assert float((rr.rays_d[:n].cpu() - torch.from_numpy(fx["rays_d"])).abs().max()) <= 1e-6
    assert torch.equal(rr.rays_o[:n].cpu(), torch.from_numpy(fx["rays_o"]))


def _mode_case(model, seed, **kw):
    dirs, pose = _camera(0.5)
    obj_rgb, obj_depth = _object(model, dirs, pose, seed=seed)
    canvas = _junk(seed + 1)
    rect = (6, 3, 41, 37)
    for k in range(2):  # (twice: the second call is all replay)
        total = _reference(model, dirs, pose, rect, obj_rgb, obj_depth, canvas, **kw)
        out = render_insert(model, pose, dirs, H, W, rect, obj_rgb, obj_depth, **APP, **kw)
        if k == 0:
            rr = next(iter(model._insert_renderers.values()))
            inside = torch.zeros(H, W, dtype=torch.bool, device=DEV)
            inside[rect[0]:rect[2], rect[1]:rect[3]] = True
            for name in ("rgb", "depth", "pts"):  # outside the rectangle: the renderer's zero-initialised canvases
                assert not bool(out[name][~inside].any()), name
                canvas[name][~inside] = 0
        _assert_frame(out, canvas, total, kw)
    assert total > 0 and len(model._insert_renderers) == 1 and rr.n_captures == 2
    return rr


def test_raw_hdr_model_with_output_radiance():
    from test_hdr_gpu import _hdr_scene_model
    import hashgrid as HG
    rr = _mode_case(_hdr_scene_model(), 11, output_radiance=True)
    assert rr.rgb_act == HG.RGB_RELU and rr.tone_mode is None


def test_exposure_model_with_an_exposure():
    from test_tonemap_gpu import _exposure_model
    import hashgrid as HG
    rr = _mode_case(_exposure_model(), 13, exposure=1.0)
    assert rr.tone_mode == HG.TONE_LDR and float(rr.exposure) == 1.0


def test_replays_are_independent_of_the_last_frame():
    """The same rectangle twice with different object depths: no object at all, then the designed map."""
    model = _scene_model(0.5, 0.02, seed=5)
    dirs, pose = _camera(0.5)
    obj_rgb, obj_depth = _object(model, dirs, pose, seed=5)
    rr = R.insert_for_model(model, H, W, dirs, **APP)
    rect = (4, 2, 44, 39)
    outs = []
    for depth in (torch.zeros_like(obj_depth), obj_depth):
        canvas = _junk(9)
        _load_canvas(rr, canvas)
        total = _reference(model, dirs, pose, rect, obj_rgb, depth, canvas)
        out = rr.render_rect(pose, rect, obj_rgb, depth)
        _assert_frame(out, canvas, total)
        outs.append(({k: out[k].clone() for k in ("rgb", "depth", "pts")}, total))
    assert not torch.equal(outs[0][0]["rgb"], outs[1][0]["rgb"])
    assert not torch.equal(outs[0][0]["depth"], outs[1][0]["depth"])
    assert outs[0][1] != outs[1][1] and rr.n_captures == 2


def test_render_insert_caches_one_renderer_and_follows_the_parameters():
    model = _scene_model(0.5, 0.02, seed=6)
    dirs, pose = _camera(0.5)
    obj_rgb, obj_depth = _object(model, dirs, pose, seed=6)
    canvas = {k: torch.zeros_like(v) for k, v in _junk(1).items()}  # (the cached renderer's canvases start at zero)
    first = None
    for i, rect in enumerate([(0, 0, H, W), (5, 5, 30, 31), (40, 2, 47, 9)]):
        if i == 2:
            with torch.no_grad():
                model.params.mul_(0.5)
        total = _reference(model, dirs, pose, rect, obj_rgb, obj_depth, canvas)
        out = render_insert(model, pose, dirs, H, W, rect, obj_rgb, obj_depth, **APP)
        _assert_frame(out, canvas, total, rect)
        first = first if first is not None else out["rgb"].clone()
    assert len(model._insert_renderers) == 1
    rr = next(iter(model._insert_renderers.values()))
    assert rr.n_captures == 2
    # the halved parameters reached the frame: the whole screen again differs from the first one
    total = _reference(model, dirs, pose, (0, 0, H, W), obj_rgb, obj_depth, canvas)
    out = render_insert(model, pose, dirs, H, W, (0, 0, H, W), obj_rgb, obj_depth, **APP)
    _assert_frame(out, canvas, total)
    assert not torch.equal(out["rgb"], first)
    assert not hasattr(model, "_test_renderers")     # render()'s own cache was not touched


def test_entry_point_statuses_on_the_device():
    """Argument errors of the new entry points with real buffers in every other place: still NGP_EINVAL, before any
    launch (the buffers keep their bits)."""
    L = vren.lib()
    f = lambda *s: torch.full(s, SENTINEL, device=DEV)  # noqa: E731
    rect = torch.tensor([0, 0, 4, 4], dtype=torch.int32, device=DEV)
    i64 = torch.full((8,), 77, dtype=torch.int64, device=DEV)
    i32 = torch.full((16,), 77, dtype=torch.int32, device=DEV)
    bufs = dict(d=f(16, 3), pose=f(3, 4), c=f(3), h=f(3), od=f(16), o=f(16, 3), rd=f(16, 3), ht=f(16, 2), op=f(16),
                dp=f(16), rgb=f(16, 3))
    b = bufs
    cf = vren.c_float

    def begin(Hh, Ww, state=i64, header=i64.clone()):
        return L.ngp_insert_frame_begin(rect, Hh, Ww, b["d"], b["pose"], b["c"], b["h"], cf(0.01), b["od"], b["o"],
                                        b["rd"], b["ht"], state, i32, b["op"], b["dp"], b["rgb"], header, None)
    assert begin(0, 4) == -1 and begin(4, -4) == -1 and begin(1 << 16, 1 << 15) == -1
    assert begin(4, 4, state=None) == -1 and begin(4, 4, header=None) == -1
    assert L.ngp_insert_frame_finish(None, 4, 4, b["op"], b["dp"], b["rgb"], b["o"], b["rd"], b["d"], b["o"], b["op"],
                                     None, None) == -1
    assert L.ngp_insert_frame_finish(i64, 4, 0, b["op"], b["dp"], b["rgb"], b["o"], b["rd"], b["d"], b["o"], b["op"],
                                     None, None) == -1
    torch.cuda.synchronize()
    for t in bufs.values():
        assert bool((t == SENTINEL).all())
    assert bool((i64 == 77).all()) and bool((i32 == 77).all())
