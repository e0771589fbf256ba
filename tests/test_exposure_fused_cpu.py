"""Exposure-conditioned models in the fused training step, the
parts that need no GPU: the new entry points' argument checks, the NumPy
restatements the GPU tests use (tests/tonemap_step_ref.py), the size of the
ReLU-ambiguous set on the GPU tests' lists, and NGPTrainer's refusals."""
import ctypes

import numpy as np
import pytest
import torch

import hashgrid as HG
import tonemap_ref as T
import tonemap_step_ref as TS
import vren


# ------------------------------------------------------------ 1. argument checks
def test_step_entry_points_refuse_bad_arguments_without_launching():
    L = vren.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # (host memory: a launch would fault, a refusal never reads it)
    q = ctypes.c_void_p(p.value + 4)  # not 16-byte aligned
    z = None
    # ngp_sample_exposure(rays_a, n_rays, img_idxs, img_exposure, n_img, n, sample_exposure, stream)
    se = L.ngp_sample_exposure
    assert se(z, 0, z, z, 0, 8, z, z) == 0 and se(z, 4, z, z, 0, 0, z, z) == 0  # empty: no-ops, also with nulls
    assert se(p, -1, p, p, 2, 8, p, z) == -1 and se(p, 4, p, p, 2, -1, p, z) == -1 and se(p, 4, p, p, -1, 8, p, z) == -1
    for hole in range(4):
        a = [p] * 4
        a[hole] = z
        assert se(a[0], 4, a[1], a[2], 2, 8, a[3], z) == -1
    # ngp_sample_exposure_rays(rays_a, n_rays, ray_exposure, n, sample_exposure, stream)
    sr = L.ngp_sample_exposure_rays
    assert sr(z, 0, z, 8, z, z) == 0 and sr(z, 4, z, 0, z, z) == 0
    assert sr(p, -1, p, 8, p, z) == -1 and sr(p, 4, p, -1, p, z) == -1
    for hole in range(3):
        a = [p] * 3
        a[hole] = z
        assert sr(a[0], 4, a[1], 8, a[2], z) == -1
    # ngp_tonemap_forward_rows(log_rad, n, rays_a, rows, n_rows_dev, n_rows, first, sample_exposure, tone, rgbs, stream)
    fr = L.ngp_tonemap_forward_rows
    assert fr(z, 0, z, z, z, 4, 64, z, z, z, z) == 0 and fr(z, 8, z, z, z, 0, 64, z, z, z, z) == 0
    assert fr(z, 8, z, z, z, 4, 0, z, z, z, z) == 0
    assert fr(p, -1, p, z, z, 4, 64, p, p, p, z) == -1 and fr(p, 8, p, z, z, -1, 64, p, p, p, z) == -1
    assert fr(p, 8, p, z, z, 4, -1, p, p, p, z) == -1
    for hole in range(5):  # log_rad, rays_a, sample_exposure, tone, rgbs (rows and n_rows_dev may be null)
        a = [p] * 5
        a[hole] = z
        assert fr(a[0], 8, a[1], z, z, 4, 64, a[2], a[3], a[4], z) == -1
    # ngp_tonemap_backward_indexed(log_rad, sample_exposure, n, n_dev, sample_idx, tone, dL_drgbs, dL_dlog_rad,
    #                              grad_tone, workspace, stream)
    bi = L.ngp_tonemap_backward_indexed
    assert bi(z, z, 0, z, z, z, z, z, z, z, z) == 0
    assert bi(p, p, -1, p, p, p, p, p, p, p, z) == -1
    for hole in range(7):  # log_rad, sample_exposure, tone, dL_drgbs, dL_dlog_rad, grad_tone, workspace
        a = [p] * 7
        a[hole] = z
        assert bi(a[0], a[1], 4, p, p, a[2], a[3], a[4], a[5], a[6], z) == -1
    assert bi(p, p, 4, z, p, p, p, p, p, p, z) == -1  # sample_idx without its count
    assert bi(p, p, 4, p, p, p, p, p, p, q, z) == -1  # a misaligned workspace
    # ngp_unit_exposure_term(tone, target, grad_tone, out_loss, stream)
    ue = L.ngp_unit_exposure_term
    for hole in range(3):
        a = [p] * 3
        a[hole] = z
        assert ue(a[0], 0.5, a[1], a[2], z) == -1
    with pytest.raises(vren.NGPError):
        vren.kernels().ngp_tonemap_backward_indexed(p, p, 4, z, p, p, p, p, p, p, z)


def test_indexed_workspace_is_the_backwards():
    L = vren.lib()
    ws, ws0 = L.ngp_tonemap_backward_indexed_workspace, L.ngp_tonemap_backward_workspace
    assert ws(0) == 0 and ws(-3) == 0
    for n in (1, 256, 257, 4099, 512 * 256, 1 << 24):
        assert ws(n) == ws0(n) > 0
    assert ws(512 * 256) == ws(1 << 24) == 512 * 384 * 4


# ------------------------------------------------------------ 2. the restatements
@pytest.mark.parametrize("n", [1, 65, 257])
def test_indexed_restatement_equals_the_reference_on_the_whole_range(n):
    c = T.case(n)
    ref = T.backward(c["w"], c["x"], c["e"], c["dy"])
    got = TS.backward_indexed(c["w"], c["x"], c["e"], c["dy"], np.arange(n, dtype=np.int32))
    for k in ("dx", "dx_bar", "grad", "grad_bar"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["n_amb"] == ref["n_amb"]
    # the count cuts the list, indices outside [0, n) are skipped
    idx = np.concatenate([np.arange(n), [n, -1, n + 5]]).astype(np.int32)
    assert np.array_equal(TS.list_selection(idx, n + 3, n), np.arange(n))  # (the count is capped at n)
    big = np.concatenate([[n, -1, n + 5], np.arange(n)]).astype(np.int32)
    assert np.array_equal(TS.list_selection(big, n + 3, n + 3)[-n:], np.arange(n))
    assert np.array_equal(TS.list_selection(idx, 1, n), [0])


def test_indexed_restatement_leaves_rows_off_the_list_alone():
    c, idx = TS.list_case(65)
    x = c["x"].copy()
    off = np.ones(c["n"], bool)
    off[idx] = False
    x[off] = np.nan  # never read
    got = TS.backward_indexed(c["w"], x, c["e"], c["dy"], idx)
    assert np.isnan(got["dx"][off]).all() and np.isfinite(got["dx"][idx]).all() and np.isfinite(got["grad"]).all()
    gathered = T.backward(c["w"], c["x"][idx], c["e"][idx], c["dy"][idx])
    assert np.array_equal(got["grad"], gathered["grad"]) and np.array_equal(got["dx"][idx], gathered["dx"])


def test_sample_exposure_and_row_selection_restatements():
    rays_a, n = TS.rays_case()
    assert sorted(rays_a[:, 2]) == sorted(TS.ROW_SAMPLES * 2) and sorted(rays_a[:, 0]) == list(range(len(rays_a)))
    assert not np.array_equal(rays_a[:, 0], np.arange(len(rays_a)))  # shuffled ray order
    own = TS.owned(rays_a, n)
    assert own.sum() == rays_a[:, 2].sum() and not own[:3].any() and not own[-3:].any()
    R = len(rays_a)
    per_ray = np.arange(1, R + 1, dtype=np.float32)
    e = TS.expand_exposure(rays_a, np.full(n, np.nan, np.float32), ray_exposure=per_ray)
    assert np.isnan(e[~own]).all()
    for ray, start, N in rays_a:
        assert np.all(e[start:start + N] == per_ray[ray])
    img = np.arange(R)[::-1] % 5
    table = np.asarray(T.EXPOSURES, np.float32)
    e2 = TS.expand_exposure(rays_a, np.full(n, np.nan, np.float32), img_idxs=img, img_exposure=table)
    assert np.array_equal(e2[own], TS.expand_exposure(rays_a, np.zeros(n), ray_exposure=table[img])[own])
    full = TS.rows_selection(rays_a, None, None, 64, n)
    assert full.sum() == np.minimum(rays_a[:, 2], 64).sum() and not (full & ~own).any()
    rows = np.array([r for r in range(R) if r % 3 != 1], np.int32)
    part = TS.rows_selection(rays_a, rows, len(rows) - 2, 64, n)
    assert part.sum() == np.minimum(rays_a[rows[:-2], 2], 64).sum() and not (part & ~full).any()


# ------------------------------------------------------------ 3. the ambiguous set on the GPU tests' lists
@pytest.mark.parametrize("length", TS.LIST_LENGTHS)
def test_the_relu_ambiguous_set_is_small_on_every_list(length):
    c, idx = TS.list_case(length)
    assert c["n"] == 2 * length + 21 and len(idx) == length == len(np.unique(idx))
    amb = T.ambiguous(c["w"], c["x"][idx], c["e"][idx])
    print(f"list of {length}: {int(amb.sum())} of {amb.size} pairs")
    assert float(amb.mean()) <= T.AMBIGUOUS_CAP
    assert TS.backward_indexed(c["w"], c["x"], c["e"], c["dy"], idx)["n_amb"] == int(amb.sum())


def test_unit_exposure_restatement_is_the_mean_over_channels():
    w = T.xavier_fp16(3)
    loss, grad, bar = TS.unit_exposure(w, 0.73)
    y = T.forward(w, np.zeros((1, 3)), np.ones(1))[0]
    assert abs(loss - sum(0.5 * (y - 0.73) ** 2) / 3) < 1e-15 and np.abs(grad).max() > 0 and bar.shape == grad.shape
    eps, k = 1e-6, 1024  # B[0, 0] of channel 0, by finite differences
    wp, wm = w.astype(np.float64), w.astype(np.float64)
    wp[k] += eps
    wm[k] -= eps
    fd = (TS.unit_exposure(wp, 0.73)[0] - TS.unit_exposure(wm, 0.73)[0]) / (2 * eps)
    assert abs(fd - grad[k]) <= 1e-6 * max(abs(fd), 1e-3)


# ------------------------------------------------------------ 4. the trainer's refusals
def test_trainer_refuses_the_combinations_it_does_not_have():
    from trainer import NGPTrainer
    with pytest.raises(ValueError, match="raw-HDR"):
        NGPTrainer(use_exposure=True, use_raw_HDR=True, device="cpu")
    with pytest.raises(NotImplementedError, match="pose gradient"):
        NGPTrainer(use_exposure=True, optimize_ext=True, device="cpu")
    with pytest.raises(NotImplementedError, match="ZeRO-1 bucket"):
        NGPTrainer(use_exposure=True, emulate_dp=2, device="cpu")
