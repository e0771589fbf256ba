"""The training step's forms of the exposure tonemapper kernels (DESIGN.md §19:
ngp_sample_exposure*, ngp_tonemap_forward_rows, ngp_tonemap_backward_indexed,
ngp_unit_exposure_term) against ngp_tonemap_forward / _backward bit for bit and
against the fp64 restatements of tests/tonemap_step_ref.py.  Every buffer has a
NaN tail, and NaN in every row a call must not touch."""
import numpy as np
import pytest
import torch

import hashgrid as HG
import tonemap_ref as T
import tonemap_step_ref as TS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PAYLOAD = 0x7FC00123  # a NaN with a payload: "kept its bits" is more than "is NaN"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _sentinel(*shape):
    t = torch.empty(*shape, device=DEV)
    t.view(torch.int32)[:] = PAYLOAD
    return t


# ------------------------------------------------------------ 1. sample exposure
@pytest.fixture(scope="module")
def rays():
    """TS.rays_case on the device, with TAIL more slots no row owns, a per-ray exposure and a per-image
    table with the rays' images."""
    rays_a, n = TS.rays_case()
    R = len(rays_a)
    g = np.random.default_rng(5)
    table = np.asarray(T.EXPOSURES + (0.75, 3.0), np.float32)
    img = g.integers(0, len(table), R)
    per_ray = g.uniform(0.1, 30, R).astype(np.float32)
    return {"rays_a": rays_a, "n": n, "cap": n + T.TAIL, "R": R, "table": table, "img": img, "per_ray": per_ray,
            "d_rays_a": torch.from_numpy(rays_a).to(DEV), "d_table": torch.from_numpy(table).to(DEV),
            "d_img": torch.from_numpy(img).to(DEV), "d_per_ray": torch.from_numpy(per_ray).to(DEV)}


def test_sample_exposure_both_forms_equal_numpy_and_keep_unowned_slots(rays):
    r = rays
    own = torch.from_numpy(TS.owned(r["rays_a"], r["cap"])).to(DEV)
    assert 0 < int(own.sum()) < r["n"]
    for kw, ref_kw in ((dict(img_idxs=r["d_img"], img_exposure=r["d_table"]), dict(img_idxs=r["img"], img_exposure=r["table"])),
                       (dict(ray_exposure=r["d_per_ray"]), dict(ray_exposure=r["per_ray"]))):
        out = _sentinel(r["cap"])
        assert HG.sample_exposure(r["d_rays_a"], out, **kw) is out
        ref = torch.from_numpy(TS.expand_exposure(r["rays_a"], np.zeros(r["cap"], np.float32), **ref_kw)).to(DEV)
        assert _same_bits(out[own], ref[own])
        assert bool((_bits(out[~own]) == PAYLOAD).all())
    # a buffer shorter than the rows claim is never written past its end
    short = r["n"] - 150
    out = _sentinel(r["cap"])
    HG.sample_exposure(r["d_rays_a"], out[:short], ray_exposure=r["d_per_ray"])
    assert bool((_bits(out[short:]) == PAYLOAD).all())


# ------------------------------------------------------------ 2. rows forward
def _rows_inputs(r):
    g = np.random.default_rng(11)
    x = g.uniform(-8, 4, (r["cap"], 3)).astype(np.float16).astype(np.float32)
    x[~TS.owned(r["rays_a"], r["cap"])] = np.nan  # gaps and the tail
    e = TS.expand_exposure(r["rays_a"], np.ones(r["cap"], np.float32), img_idxs=r["img"], img_exposure=r["table"])
    return torch.from_numpy(x).to(DEV), torch.from_numpy(e).to(DEV), torch.from_numpy(T.xavier_fp16(11)).to(DEV).half()


def test_rows_forward_is_the_forward_on_the_rows_first_chunks_and_nothing_else(rays):
    r = rays
    x, e, t16 = _rows_inputs(r)
    finite = torch.nan_to_num(x)  # (the whole-buffer forward as the per-row reference)
    direct = HG.tonemap_forward(finite, e, r["cap"], t16)
    R = r["R"]
    rows = np.array([j for j in range(R) if j % 3 != 1], np.int32)
    d_rows = torch.from_numpy(rows).to(DEV)
    # (a list always comes with its device count: without one the kernel walks n_rows entries)
    for use_rows, count in ((None, None), (d_rows, len(rows)), (d_rows, len(rows) - 2), (None, R - 3)):
        sel = torch.from_numpy(TS.rows_selection(r["rays_a"], None if use_rows is None else rows, count, 64, r["cap"])).to(DEV)
        assert 0 < int(sel.sum()) < r["n"]
        cnt = None if count is None else torch.tensor([count], dtype=torch.int64, device=DEV)
        rr = use_rows  # (null with a device count: the rows [0, count))
        out = _sentinel(r["cap"], 3)
        HG.tonemap_forward_rows(x, r["d_rays_a"], rr, cnt, 64, e, t16, out)
        assert _same_bits(out[sel], direct[sel])
        assert bool((_bits(out[~sel]) == PAYLOAD).all())  # samples >= 64 of long rows, unlisted rows, gaps, the tail
        inplace = x.clone()
        HG.tonemap_forward_rows(inplace, r["d_rays_a"], rr, cnt, 64, e, t16, inplace)
        assert _same_bits(inplace[sel], direct[sel]) and _same_bits(inplace[~sel], x[~sel])
    # the long rows really are cut at 64, and another `first` moves the cut
    long_rows = r["rays_a"][r["rays_a"][:, 2] > 64]
    assert len(long_rows) >= 2
    sel64 = TS.rows_selection(r["rays_a"], None, None, 64, r["cap"])
    for _, start, N in long_rows:
        assert sel64[start:start + 64].all() and not sel64[start + 64:start + N].any()
    for first in (1, 100, 1000):
        sel = torch.from_numpy(TS.rows_selection(r["rays_a"], None, None, first, r["cap"])).to(DEV)
        out = _sentinel(r["cap"], 3)
        HG.tonemap_forward_rows(x, r["d_rays_a"], None, None, first, e, t16, out)
        assert _same_bits(out[sel], direct[sel]) and bool((_bits(out[~sel]) == PAYLOAD).all())


# ------------------------------------------------------------ 3. indexed backward
_lists = {}


def _list_dev(length):
    """TS.list_case on the device: buffers of n + TAIL rows, NaN in every row off the list (and in the
    tail), the list followed by TAIL out-of-range entries past its count."""
    if length not in _lists:
        c, idx = TS.list_case(length)
        n = c["n"]
        cap = n + T.TAIL
        off = np.ones(cap, bool)
        off[idx] = False

        def pad(a, fill):
            full = np.full((cap,) + a.shape[1:], fill, np.float32)
            full[:n] = a
            full[off] = np.nan
            return torch.from_numpy(full).to(DEV)

        d_idx = torch.from_numpy(np.concatenate([idx, np.full(T.TAIL, cap + 5, np.int32)])).to(DEV)
        _lists[length] = {"c": c, "idx": idx, "n": n, "cap": cap, "x": pad(c["x"], np.nan), "e": pad(c["e"], np.nan),
                          "dy": pad(c["dy"], np.nan), "t16": torch.from_numpy(c["w"]).to(DEV).half(), "d_idx": d_idx,
                          "cnt": torch.tensor([length], dtype=torch.int64, device=DEV),
                          "listed": torch.from_numpy(~off).to(DEV),
                          "ref": TS.backward_indexed(c["w"], c["x"], c["e"], c["dy"], idx)}
    return _lists[length]


def _run_indexed(D, alias=False, grad=None, **over):
    D = dict(D, **over)
    grad = torch.zeros(HG.TONE_PARAMS, device=DEV) if grad is None else grad
    if alias:
        dx = D["dy"].clone()
        assert HG.tonemap_backward_indexed(D["x"], D["e"], D["t16"], dx, grad, D["cnt"], D["d_idx"], dx) is dx
    else:
        dx = HG.tonemap_backward_indexed(D["x"], D["e"], D["t16"], D["dy"], grad, D["cnt"], D["d_idx"],
                                         _sentinel(D["cap"], 3))
    return dx, grad


@pytest.mark.parametrize("length", TS.LIST_LENGTHS)
def test_indexed_backward_equals_the_backward_on_the_gathered_rows(length):
    D = _list_dev(length)
    ref, idx = D["ref"], torch.from_numpy(D["idx"]).long().to(DEV)
    dx, grad = _run_indexed(D)
    # dL/dlog_rad: the bits ngp_tonemap_backward writes for the same rows, gathered
    gx, ge, gdy = (D[k][idx].contiguous() for k in ("x", "e", "dy"))
    g_grad = torch.zeros(HG.TONE_PARAMS, device=DEV)
    g_dx = HG.tonemap_backward(gx, ge, length, D["t16"], gdy, g_grad)
    assert _same_bits(dx[idx], g_dx)
    assert bool((_bits(dx[~D["listed"]]) == PAYLOAD).all())  # written only on listed rows; NaN inputs off the list never read
    # the weight gradients: §18's bar against the fp64 restatement
    eg = np.abs(grad.double().cpu().numpy() - ref["grad"])
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.nanmax(np.where(ref["grad_bar"] > 0, eg / ref["grad_bar"], 0.0))
    print(f"list of {length} of {D['n']} rows: dL/dtone max err {eg.max():.3e} (largest share of its bar {share:.4f}); "
          f"{ref['n_amb']} ambiguous pairs")
    assert np.all(eg <= ref["grad_bar"]) and float(np.abs(ref["grad"]).max()) > 0 and bool(torch.isfinite(grad).all())
    # structure: the fifteen padding columns of a unit are one bit pattern, dB[1..15] exactly 0
    A, B = T.split(grad.cpu().numpy())
    assert np.all(A[:, :, 1:].view(np.int32) == A[:, :, 1:2].view(np.int32))
    assert np.all(B[:, 1:].view(np.int32) == 0) and np.abs(B[:, 0]).max() > 0
    # two runs: the same bits; a second call leaves exactly twice the first
    dx_b, grad_b = _run_indexed(D)
    assert _same_bits(dx_b, dx) and _same_bits(grad_b, grad)
    _, twice = _run_indexed(D, grad=grad_b)
    assert twice is grad_b and _same_bits(twice, 2 * grad)
    # dL_dlog_rad written over dL_drgbs: the same bits on the list, dL_drgbs' own off it
    dx_a, grad_a = _run_indexed(D, alias=True)
    assert _same_bits(dx_a[idx], dx[idx]) and _same_bits(dx_a[~D["listed"]], D["dy"][~D["listed"]])
    assert _same_bits(grad_a, grad)
    # listed rows with a zero gradient add nothing, whatever their log radiance holds
    if length >= 2:
        zero = torch.from_numpy((D["c"]["dy"][D["idx"]] == 0).all(1)).to(DEV)
        assert 0 < int(zero.sum()) < length
        x_nan = D["x"].clone()
        x_nan[idx[zero]] = float("nan")
        dx_c, grad_c = _run_indexed(D, x=x_nan)
        assert _same_bits(grad_c, grad) and bool((dx_c[idx[zero]] == 0).all())
    else:  # the one listed row, its gradient zeroed and its log radiance NaN: nothing is added at all
        x_nan = D["x"].clone()
        x_nan[idx] = float("nan")
        dy_zero = D["dy"].clone()
        dy_zero[idx] = 0.0
        dx_c, grad_c = _run_indexed(D, x=x_nan, dy=dy_zero)
        assert bool((grad_c == 0).all()) and bool((dx_c[idx] == 0).all())
    # a shorter device count walks the head of the list only
    if length > 64:
        m = length // 2
        head = idx[:m]
        dx_h, grad_h = _run_indexed(D, cnt=torch.tensor([m], dtype=torch.int64, device=DEV))
        rest = torch.ones(D["cap"], dtype=torch.bool, device=DEV)
        rest[head] = False
        assert _same_bits(dx_h[head], dx[head]) and bool((_bits(dx_h[rest]) == PAYLOAD).all())
        ref_h = TS.backward_indexed(D["c"]["w"], D["c"]["x"], D["c"]["e"], D["c"]["dy"], D["idx"], m)
        assert np.all(np.abs(grad_h.double().cpu().numpy() - ref_h["grad"]) <= ref_h["grad_bar"])


def test_indexed_backward_without_a_list_is_the_backward():
    n = 257
    c = T.case(n)
    x, e, dy = (torch.from_numpy(c[k]).to(DEV) for k in ("x", "e", "dy"))
    t16 = torch.from_numpy(c["w"]).to(DEV).half()
    g0, g1 = torch.zeros(HG.TONE_PARAMS, device=DEV), torch.zeros(HG.TONE_PARAMS, device=DEV)
    dx0 = HG.tonemap_backward(x, e, n, t16, dy, g0)
    dx1 = HG.tonemap_backward_indexed(x, e, t16, dy, g1, None, None, torch.empty_like(x))
    assert _same_bits(dx0, dx1) and _same_bits(g0, g1)


# ------------------------------------------------------------ 4. unit-exposure term
@pytest.mark.parametrize("target", [0.73, 0.5])
def test_unit_exposure_term_equals_the_models_expression(target):
    """train.py:182-187 as scripts/train_exposure.py states it on the drop-in model, through torch's
    0.5 (y - t)^2 .mean() and backward."""
    from models.networks import NGP
    m = NGP(0.5, 'None', False, seed=8, use_exposure=True).to(DEV)
    unit = m.log_radiance_to_rgb(torch.zeros(1, 3, device=DEV), exposure=torch.ones(1, 1, device=DEV))
    loss = (0.5 * (unit - target) ** 2).mean()
    loss.backward()
    loss = loss.detach()
    t16 = m._tone_shadow.get()
    grad = torch.zeros(HG.TONE_PARAMS, device=DEV)
    out = HG.unit_exposure_term(t16, target, grad, torch.full((1,), float("nan"), device=DEV))
    ref_loss, ref_grad, bar = TS.unit_exposure(t16.float().cpu().numpy(), target)
    print(f"unit-exposure loss {float(out):.8e}, torch {float(loss):.8e}, fp64 {ref_loss:.8e}")
    assert abs(float(out) - float(loss)) <= 1e-6 * abs(float(loss)) and abs(float(out) - ref_loss) <= 1e-6 * ref_loss
    g = grad.double().cpu().numpy()
    assert np.all(np.abs(g - ref_grad) <= bar + 1e-9) and float(grad.abs().max()) > 0
    # against torch's tone_params.grad: the same per-element bar (both run the same arithmetic on one row)
    err_t = np.abs(g - m.tone_params.grad.double().cpu().numpy())
    print(f"gradient vs torch's: max err {err_t.max():.3e}, largest share of the bar {(err_t / (bar + 1e-9)).max():.4f}")
    assert np.all(err_t <= bar + 1e-9)
    # it adds: a second call leaves twice the first
    HG.unit_exposure_term(t16, target, grad, out)
    assert _same_bits(grad, 2 * torch.from_numpy(g).float().to(DEV))
    A, B = T.split(grad.cpu().numpy())
    assert np.all(A[:, :, 1:].view(np.int32) == A[:, :, 1:2].view(np.int32)) and np.all(B[:, 1:] == 0)
