"""The fp64 SSIM / MSE reference (tests/metrics_ref.py) against known answers,
metrics.mse / metrics.psnr against the reference module's semantics
(metrics.py:4-15), and the image-metrics entry points in the parsed C ABI.
No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import capi
import metrics
import metrics_ref as MR


def _rand(h, w, seed):
    return np.random.default_rng(seed).random((h, w, 3), dtype=np.float32)


# ------------------------------------------------------------ the reference
def test_window_is_the_normalised_gaussian():
    g = MR.window1d()
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15
    assert np.array_equal(g, g[::-1]) and g.argmax() == 5
    np.testing.assert_allclose(g[4] / g[5], np.exp(-0.5 / 1.5 ** 2), rtol=1e-14)
    assert abs(MR.window2d().sum() - 1) < 1e-15


def test_identical_images_give_exactly_one():
    x = _rand(23, 31, 0)
    smap, s, m = MR.image_metrics(x, x.copy(), 23, 31)
    assert smap.shape == (3, 13, 21)
    assert np.all(smap == 1.0) and s == 1.0 and m == 0.0


def test_constant_images_closed_form():
    a, b = 0.75, 0.5
    x, y = np.full((17, 29, 3), a, np.float32), np.full((17, 29, 3), b, np.float32)
    smap, s, m = MR.image_metrics(x, y, 17, 29)
    want = (2 * a * b + MR.C1) / (a * a + b * b + MR.C1)  # both variances and the covariance vanish
    assert abs(want - 0.92308638936746) < 1e-13
    assert np.abs(smap - want).max() <= 1e-12 and abs(s - want) <= 1e-12
    assert abs(m - (a - b) ** 2) <= 1e-15


def test_one_window_by_hand():
    x, y = _rand(11, 11, 1), _rand(11, 11, 2)
    smap, s, m = MR.image_metrics(x, y, 11, 11)
    assert smap.shape == (3, 1, 1)
    W = MR.window2d()
    for c in range(3):
        X, Y = x[..., c].astype(np.float64), y[..., c].astype(np.float64)
        mx, my = (W * X).sum(), (W * Y).sum()
        vx, vy, cxy = (W * X * X).sum() - mx ** 2, (W * Y * Y).sum() - my ** 2, (W * X * Y).sum() - mx * my
        want = (2 * mx * my + 1e-4) * (2 * cxy + 9e-4) / ((mx ** 2 + my ** 2 + 1e-4) * (vx + vy + 9e-4))
        assert abs(smap[c, 0, 0] - want) <= 1e-12
    assert abs(s - smap.mean()) <= 1e-15
    assert abs(m - ((x.astype(np.float64) - y.astype(np.float64)) ** 2).mean()) <= 1e-15


def test_symmetric_in_its_two_images():
    x, y = _rand(19, 26, 3), _rand(19, 26, 4)
    a, b = MR.image_metrics(x, y, 19, 26), MR.image_metrics(y, x, 19, 26)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_transposing_both_images_transposes_the_map():
    h, w = 14, 37
    x, y = _rand(h, w, 5), _rand(h, w, 6)
    xt, yt = np.ascontiguousarray(x.transpose(1, 0, 2)), np.ascontiguousarray(y.transpose(1, 0, 2))
    a, b = MR.image_metrics(x, y, h, w), MR.image_metrics(xt, yt, w, h)
    assert a[0].shape == (3, h - 10, w - 10) and b[0].shape == (3, w - 10, h - 10)
    assert np.abs(a[0] - b[0].transpose(0, 2, 1)).max() <= 1e-12  # (the taps are added in another order)
    assert abs(a[1] - b[1]) <= 1e-12 and abs(a[2] - b[2]) <= 1e-15


def test_clamp_touches_pred_only():
    x = _rand(12, 15, 7) * 1.6 - 0.3
    y = _rand(12, 15, 8) * 1.6 - 0.3
    a = MR.image_metrics(x, y, 12, 15, clamp=True)
    b = MR.image_metrics(np.clip(x, 0, 1), y, 12, 15)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    assert MR.image_metrics(x, y, 12, 15)[2] != a[2]


# ------------------------------------------------- metrics.mse / metrics.psnr
def test_mse_psnr_reference_semantics():
    g = torch.Generator().manual_seed(0)
    p, t = torch.rand(50, 3, generator=g), torch.rand(50, 3, generator=g)
    sq = (p - t) ** 2
    assert torch.equal(metrics.mse(p, t), sq.mean())
    assert torch.equal(metrics.mse(p, t, reduction='none'), sq)
    assert torch.equal(metrics.psnr(p, t), -10 * torch.log10(sq.mean()))
    assert torch.equal(metrics.psnr(p, t, reduction='none'), -10 * torch.log10(sq))
    mask = torch.rand(50, generator=g) > 0.5
    assert torch.equal(metrics.mse(p, t, mask), sq[mask].mean())
    assert torch.equal(metrics.mse(p, t, valid_mask=mask, reduction='none'), sq[mask])
    assert metrics.mse(p, t, mask, 'none').shape == (int(mask.sum()), 3)
    assert torch.equal(metrics.psnr(p, t, mask), -10 * torch.log10(sq[mask].mean()))
    # psnr is the no_grad one of the two (metrics.py:13)
    q = p.clone().requires_grad_()
    assert metrics.mse(q, t).requires_grad and not metrics.psnr(q, t).requires_grad


def test_ssim_has_no_cpu_fallback():
    x = torch.rand(11 * 12, 3)
    with pytest.raises(RuntimeError, match="image_pred must be a CUDA tensor"):
        metrics.ssim(x, x, (12, 11))
    with pytest.raises(ValueError, match="11 x 11"):
        metrics.ssim(x, x, (10, 11))


# ------------------------------------------------------------------ the ABI
def test_image_metrics_in_the_parsed_header():
    P = capi.POINTER_TO
    assert capi.FUNCS["ngp_image_metrics_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    assert capi.FUNCS["ngp_image_metrics"] == (ctypes.c_int, [
        P["float"], P["float"], ctypes.c_int, ctypes.c_int, ctypes.c_int, P["void"], P["float"], P["float"],
        P["void"]])


def test_fp32_torch_ssim_is_the_same_index_but_no_reference():
    """the timing comparator (metrics_ref.ssim_torch_fp32) computes the same
    quantity: close on noise, visibly off where fp32 cancels"""
    h, w = 43, 75
    x, y = _rand(h, w, 9), _rand(h, w, 10)
    smap, s = MR.ssim_torch_fp32(torch.from_numpy(x), torch.from_numpy(y), h, w)
    ref = MR.image_metrics(x, y, h, w)
    assert smap.shape == (3, h - 10, w - 10)
    assert np.abs(smap.numpy() - ref[0]).max() < 1e-5 and abs(float(s) - ref[1]) < 1e-6
    xb, yb = 1 - 1e-3 * x, 1 - 1e-3 * y
    smap, _ = MR.ssim_torch_fp32(torch.from_numpy(xb), torch.from_numpy(yb), h, w)
    assert np.abs(smap.numpy() - MR.image_metrics(xb, yb, h, w)[0]).max() > 1e-5
