"""ngp_image_metrics (csrc/metrics.hip) and the metrics module on it, against
the fp64 reference tests/metrics_ref.py (direct 11x11 windows in numpy).

Bars.  The kernel is fp64 between its fp32 loads and stores, so what separates
it from the reference is (a) the one rounding of each stored value to fp32,
2^-24 relative, and (b) fp64 summation order (separable passes against the
direct window; tile slots against numpy's pairwise mean): about 24 roundings
of 2^-53 E[x^2] per moment, divided by C2 = 9e-4, i.e. <= 1e-11 for values in
[0, 2] -- capped by 1e-9.  Every window, the SSIM and the MSE are held to
2^-24 |ref| + 1e-9.  (A torch fp32 SSIM is no comparator here: its
E[x^2] - mu^2 cancels in fp32 and misses by up to 4.7e-4 on the bright flat
inputs below.)

Shapes: one window, one row / one column of windows, sizes at and one past
multiples of the 32 x 16 tile (both divide 64, so 74 = 64 + 10 fills tiles
exactly), non-square frames, several tiles per axis.
"""
import functools

import numpy as np
import pytest
import torch

import metrics
import metrics_ref as MR
import vren

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

SHAPES = [(11, 11), (11, 75), (75, 11), (12, 43), (42, 42), (43, 44), (64, 64), (74, 74), (33, 140), (75, 139),
          (200, 200)]
KINDS = ["noise", "noisy_copy", "const", "white", "bright", "ramp", "clone"]
EINVAL, ERANGE = -1, -2


@functools.lru_cache(maxsize=None)
def _inputs(kind, h, w):
    """(pred, gt) fp32 (h*w, 3) on the host"""
    g = torch.Generator().manual_seed(100003 * h + 17 * w + KINDS.index(kind))
    n = h * w
    if kind == "noise":
        return torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    if kind == "noisy_copy":  # falls outside [0, 1]: the clamp matters
        gt = torch.rand(n, 3, generator=g)
        return gt + 0.1 * torch.randn(n, 3, generator=g), gt
    if kind == "const":
        return torch.full((n, 3), 0.75), torch.full((n, 3), 0.5)
    if kind == "white":
        return torch.ones(n, 3), torch.ones(n, 3)
    if kind == "bright":
        return 1 - 1e-3 * torch.rand(n, 3, generator=g), 1 - 1e-3 * torch.rand(n, 3, generator=g)
    if kind == "ramp":  # bilinear in (u, v), another one per channel; + 0.02 passes 1 in a corner
        v, u = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
        ramp = torch.stack([0.6 * u + 0.4 * v, 1 - 0.5 * u - 0.5 * v + 0.3 * u * v, u * v], -1).reshape(n, 3)
        return (ramp + 0.02).contiguous(), ramp.contiguous()
    x = torch.rand(n, 3, generator=g)
    return x, x.clone()


@functools.lru_cache(maxsize=None)
def _ref(kind, h, w, clamp):
    pred, gt = _inputs(kind, h, w)
    if clamp and bool(((pred >= 0) & (pred <= 1)).all()):
        return _ref(kind, h, w, False)  # nothing to clamp
    return MR.image_metrics(pred, gt, h, w, clamp=clamp)


def _ws(h, w, margin=0):
    nbytes = vren.lib().ngp_image_metrics_ws_bytes(h, w)
    assert nbytes > 0 and nbytes % 16 == 0
    return torch.empty(nbytes // 8 + 2 * margin, dtype=torch.float64, device=DEV)


def _run(pred, gt, h, w, clamp, with_map=True):
    out = torch.full((2,), float("nan"), device=DEV)
    smap = torch.full((3, h - 10, w - 10), float("nan"), device=DEV) if with_map else None
    st = vren.lib().ngp_image_metrics(pred, gt, h, w, int(clamp), _ws(h, w), out, smap, vren._stream())
    assert st == 0
    return out, smap


def _bits(t):
    return t.detach().cpu().reshape(-1).contiguous().view(torch.int32)


def _within(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err, bar = np.abs(got - ref), 2.0 ** -24 * np.abs(ref) + 1e-9
    worst = int(np.argmax(err - bar))
    return bool(np.all(err <= bar)), f"worst |got - ref| {err.flat[worst]:.3e} against a bar of {bar.flat[worst]:.3e}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_kernel_against_fp64_reference(h, w, kind):
    pred, gt = (t.to(DEV) for t in _inputs(kind, h, w))
    for clamp in (False, True):
        ref_map, ref_ssim, ref_mse = _ref(kind, h, w, clamp)
        out, smap = _run(pred, gt, h, w, clamp)
        ok, msg = _within(smap.cpu().numpy(), ref_map)
        assert ok, f"ssim_map {kind} {h}x{w} clamp={clamp}: {msg}"
        ok, msg = _within(out[1].item(), ref_ssim)
        assert ok, f"ssim {kind} {h}x{w} clamp={clamp}: {msg}"
        ok, msg = _within(out[0].item(), ref_mse)
        assert ok, f"mse {kind} {h}x{w} clamp={clamp}: {msg}"
        if kind == "clone":  # identical images: exactly 1 in every window, exactly no error
            assert bool((smap == 1.0).all()) and out[1].item() == 1.0 and out[0].item() == 0.0
        # without the map: the same out; a second call: the same bits everywhere
        out_nomap, _ = _run(pred, gt, h, w, clamp, with_map=False)
        assert torch.equal(_bits(out_nomap), _bits(out))
        out2, smap2 = _run(pred, gt, h, w, clamp)
        assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(smap2), _bits(smap))


def test_clamp_changes_the_noisy_copy():
    """the two settings of clamp01 are told apart by the inputs that need it"""
    a, b = _ref("noisy_copy", 43, 44, False), _ref("noisy_copy", 43, 44, True)
    assert abs(a[1] - b[1]) > 1e-4 and abs(a[2] - b[2]) > 1e-5
    a, b = _ref("ramp", 43, 44, False), _ref("ramp", 43, 44, True)
    assert abs(a[2] - b[2]) > 1e-7


@pytest.mark.parametrize("h,w", [(43, 44), (75, 139)])
def test_writes_stay_inside_map_and_workspace(h, w):
    """ssim_map and ws carved out of junk-filled buffers: the margins keep their bits"""
    pred, gt = (t.to(DEV) for t in _inputs("noise", h, w))
    M, n_map = 64, 3 * (h - 10) * (w - 10)
    g = torch.Generator().manual_seed(5)
    junk_map = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_map + 2 * M,), dtype=torch.int32, generator=g)
    map_buf = junk_map.to(DEV)
    ws_buf = _ws(h, w, margin=M)
    junk_ws = torch.randint(-2 ** 62, 2 ** 62, (ws_buf.numel(),), dtype=torch.int64, generator=g)
    ws_buf.view(torch.int64).copy_(junk_ws)
    out = torch.empty(2, device=DEV)
    smap = map_buf.view(torch.float32)[M:M + n_map]
    ws = ws_buf[M:ws_buf.numel() - M]
    assert ws.numel() * 8 == vren.lib().ngp_image_metrics_ws_bytes(h, w)
    assert vren.lib().ngp_image_metrics(pred, gt, h, w, 0, ws, out, smap, vren._stream()) == 0
    got_map, got_ws = map_buf.cpu(), ws_buf.view(torch.int64).cpu()
    assert torch.equal(got_map[:M], junk_map[:M]) and torch.equal(got_map[-M:], junk_map[-M:])
    assert torch.equal(got_ws[:M], junk_ws[:M]) and torch.equal(got_ws[-M:], junk_ws[-M:])
    want, _ = _run(pred, gt, h, w, False)
    assert torch.equal(_bits(out), _bits(want))
    ok, msg = _within(smap.cpu().numpy().reshape(3, h - 10, w - 10), _ref("noise", h, w, False)[0])
    assert ok, msg


def test_argument_errors_come_before_any_launch():
    L = vren.lib()
    x = torch.rand(20 * 20, 3, device=DEV)
    out = torch.full((2,), 7.0, device=DEV)
    ws = _ws(20, 20)
    s = vren._stream()
    for args in ((None, x, 20, 20, 0, ws, out, None), (x, None, 20, 20, 0, ws, out, None),
                 (x, x, 20, 20, 0, None, out, None), (x, x, 20, 20, 0, ws, None, None)):
        assert L.ngp_image_metrics(*args, s) == EINVAL
    assert L.ngp_image_metrics(x, x, 5, 80, 0, ws, out, None, s) == EINVAL
    assert L.ngp_image_metrics(x, x, 80, 5, 0, ws, out, None, s) == EINVAL
    assert L.ngp_image_metrics(x, x, 100000, 100000, 0, ws, out, None, s) == ERANGE  # 3 h w = 3e10
    assert L.ngp_image_metrics_ws_bytes(5, 80) == 0 and L.ngp_image_metrics_ws_bytes(100000, 100000) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [7.0, 7.0]  # nothing ran
    with pytest.raises(vren.NGPError) as e:
        vren.kernels().ngp_image_metrics(x, x, 100000, 100000, 0, ws, out, None, s)
    assert e.value.status == ERANGE


def test_ssim_function():
    h, w = 33, 140
    pred, gt = (t.to(DEV) for t in _inputs("noisy_copy", h, w))
    for clamp in (False, True):
        ref_map, ref_ssim, _ = _ref("noisy_copy", h, w, clamp)
        s, smap = metrics.ssim(pred, gt, (w, h), clamp=clamp, return_map=True)
        assert s.shape == () and smap.shape == (3, h - 10, w - 10)
        assert _within(s.item(), ref_ssim)[0] and _within(smap.cpu().numpy(), ref_map)[0]
        s2 = metrics.ssim(pred.view(h, w, 3), gt.view(h, w, 3), (w, h), clamp=clamp)
        assert torch.equal(_bits(s2), _bits(s))
    with pytest.raises(RuntimeError, match="image_gt must be a CUDA tensor"):
        metrics.ssim(pred, gt.cpu(), (w, h))
    with pytest.raises(RuntimeError, match="image_pred must be"):
        metrics.ssim(pred.view(h, w, 3), gt.view(h, w, 3), (h, w))  # img_wh is (w, h)
    with pytest.raises(RuntimeError, match="float32"):
        metrics.ssim(pred.double(), gt, (w, h))


def test_image_metrics_accumulates_frames_without_touching_other_slots():
    h, w = 43, 44
    frames = [("noisy_copy", True), ("bright", True), ("noise", False)]
    im = metrics.ImageMetrics((w, h), 5, DEV)
    junk = torch.tensor([[1.5, -2.5]] * 5, device=DEV)
    im.values.copy_(junk)
    for i, (kind, clamp) in enumerate(frames):
        pred, gt = (t.to(DEV) for t in _inputs(kind, h, w))
        im.update(pred, gt, clamp=clamp)
        single, _ = _run(pred, gt, h, w, clamp, with_map=False)
        assert torch.equal(_bits(im.values[i]), _bits(single))  # a frame of the series = a single call
        assert torch.equal(_bits(im.values[i + 1:]), _bits(junk[i + 1:]))  # the slots after it: untouched
        if i:
            assert torch.equal(_bits(im.values[:i]), _bits(before[:i]))  # and the ones before it
        before = im.values.clone()
    res = im.compute()
    assert len(res["psnr"]) == len(res["ssim"]) == 3
    for i, (kind, clamp) in enumerate(frames):
        _, ref_ssim, ref_mse = _ref(kind, h, w, clamp)
        assert abs(res["psnr"][i] - -10 * np.log10(max(ref_mse, 1e-12))) <= 1e-4
        assert _within(res["ssim"][i], ref_ssim)[0]
    assert abs(res["mean_psnr"] - sum(res["psnr"]) / 3) < 1e-12
    assert abs(res["mean_ssim"] - sum(res["ssim"]) / 3) < 1e-12
    im.update(*(t.to(DEV) for t in _inputs("clone", h, w)))
    im.update(*(t.to(DEV) for t in _inputs("white", h, w)))
    res = im.compute()
    assert abs(res["psnr"][3] - 120.0) < 1e-9 and res["ssim"][3] == 1.0  # mse 0 -> the 1e-12 floor
    with pytest.raises(RuntimeError, match="holds 5 frames"):
        im.update(*(t.to(DEV) for t in _inputs("white", h, w)))
    with pytest.raises(RuntimeError, match="pred must be a CUDA tensor"):
        metrics.ImageMetrics((w, h), 1, DEV).update(torch.rand(h * w, 3), torch.rand(h * w, 3, device=DEV))


def test_rendered_frames_end_to_end():
    """two 40 x 30 views of an untrained model rendered by NGPTrainer.render
    and scored on the device, against the reference on the same frames"""
    import synthetic as S
    from trainer import NGPTrainer
    W, H = 40, 30
    sc = S.AnalyticScene(W=W, H=H, n_images=2)
    tr = NGPTrainer(scale=0.5, batch_size=256, sample_capacity=256 * 64, device=DEV, seed=2)
    tr.density_bitfield.copy_(sc.bitfield.to(DEV))  # the scene's shell: the rays go through the (untrained) field
    gts = sc.gt_images(device="cpu").float().div(255).to(DEV)
    im = metrics.ImageMetrics((W, H), 2, DEV)
    frames = []
    for i in range(2):
        o, d = sc.rays(torch.full((W * H,), i, dtype=torch.int64), torch.arange(W * H))
        out = tr.render(o.to(DEV).contiguous(), d.to(DEV).contiguous(), bg=1.0)
        frames.append(out["rgb"].clone())
        im.update(out["rgb"], gts[i].contiguous(), clamp=True)
    res = im.compute()
    for i in range(2):
        assert bool(torch.isfinite(frames[i]).all()) and float(frames[i].std()) > 0
        _, ref_ssim, ref_mse = MR.image_metrics(frames[i], gts[i], H, W, clamp=True)
        assert abs(res["psnr"][i] - -10 * np.log10(max(ref_mse, 1e-12))) <= 1e-4
        assert _within(res["ssim"][i], ref_ssim)[0] and _within(res["mse"][i], ref_mse)[0]
