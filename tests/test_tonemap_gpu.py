"""The exposure tonemapper kernels (ngp_tonemap_forward / _backward;
DESIGN.md §18) against the fp64 restatement of tests/tonemap_ref.py, and the
model, renderer and training surface built on them (NGP(use_exposure=True))."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import hashgrid as HG
import tonemap_ref as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _padded(a, fill=float("nan")):
    """a's rows followed by T.TAIL rows of `fill`, on the device"""
    a = torch.as_tensor(a)
    return torch.cat([a, torch.full((T.TAIL,) + tuple(a.shape[1:]), fill, dtype=a.dtype)]).to(DEV).contiguous()


_cases = {}


def _dev(n):
    """Case n on the device: buffers of capacity n + TAIL (NaN past n), the count in device memory,
    the weights as the fp16 shadow."""
    if n not in _cases:
        c = T.case(n)
        _cases[n] = {"n": n, "cap": n + T.TAIL, "x": _padded(c["x"]), "e": _padded(c["e"], 1.0), "dy": _padded(c["dy"]),
                     "t16": torch.from_numpy(c["w"]).to(DEV).half(), "cnt": torch.tensor([n], dtype=torch.int64, device=DEV)}
    return _cases[n]


def _exposure(D, kind):
    """(tensor | None, n_exposure) of the three ways to give the exposure"""
    if kind == "absent":
        return None, 0
    if kind == "uniform":
        return torch.tensor([8.0], device=DEV), 1
    return D["e"], D["cap"]


def _ref_exposure(c, kind):
    return {"absent": None, "uniform": np.full(c["n"], 8.0), "per row": c["e"]}[kind]


# ------------------------------------------------------------ 1. forward
# The worst-case bar of tonemap_ref.forward is never approached: the largest |y - y_ref| measured on an MI355X
# over every case below is 1.45e-7, the largest share of the bar 0.010.  Under a tenth of the
# bar, so the bar is tightened to 4 x what was measured: 0.04 of the worst case.
FORWARD_BAR_SHARE = 0.04


@pytest.mark.parametrize("kind", ["absent", "uniform", "per row"])
@pytest.mark.parametrize("n", T.SIZES)
def test_forward_is_within_the_dot_products_bar(n, kind):
    c, D = T.case(n), _dev(n)
    e, ne = _exposure(D, kind)
    y = HG.tonemap_forward(D["x"], e, ne, D["t16"], n_dev=D["cnt"], out=torch.full_like(D["x"], float("nan")))
    ref, bar = T.forward(c["w"], c["x"], _ref_exposure(c, kind), with_bound=True)
    err = np.abs(y[:n].double().cpu().numpy() - ref)
    print(f"n = {n}, exposure {kind}: max |y - y_ref| {err.max():.3e}, max share of the bar {(err / bar).max():.3f}, "
          f"smallest bar {bar.min():.3e}")
    assert np.all(err <= FORWARD_BAR_SHARE * bar)
    assert bool(torch.isnan(y[n:]).all())  # rows past the count keep their bits
    # in place equals out of place, bit for bit
    x2 = D["x"].clone()
    assert HG.tonemap_forward(x2, e, ne, D["t16"], n_dev=D["cnt"], out=x2) is x2
    assert _same_bits(x2[:n], y[:n]) and _same_bits(x2[n:], D["x"][n:])
    if kind == "absent":  # exposure absent equals exposure 1.0, bit for bit
        one = HG.tonemap_forward(D["x"], torch.ones(1, device=DEV), 1, D["t16"], n_dev=D["cnt"], out=torch.zeros_like(D["x"]))
        ones = HG.tonemap_forward(D["x"], torch.ones(D["cap"], device=DEV), D["cap"], D["t16"], n_dev=D["cnt"],
                                  out=torch.zeros_like(D["x"]))
        assert _same_bits(one[:n], y[:n]) and _same_bits(ones[:n], y[:n])
    if n == 257:  # without a device-side count every row of the buffer is a row
        e_n, ne_n = (e[:n].contiguous(), n) if kind == "per row" else (e, ne)
        assert _same_bits(HG.tonemap_forward(D["x"][:n].contiguous(), e_n, ne_n, D["t16"]), y[:n])


@pytest.mark.parametrize("kind", ["absent", "uniform", "per row"])
@pytest.mark.parametrize("n", [65, 4099])
def test_forward_through_a_shuffled_partial_sample_list(n, kind):
    c, D = T.case(n), _dev(n)
    e, ne = _exposure(D, kind)
    direct = HG.tonemap_forward(D["x"], e, ne, D["t16"], n_dev=D["cnt"], out=torch.full_like(D["x"], float("nan")))
    g = torch.Generator().manual_seed(n)
    perm = torch.randperm(n, generator=g)
    m = (2 * n) // 3
    idx = torch.cat([perm, torch.full((T.TAIL,), n + 1, dtype=torch.int64)]).to(torch.int32).to(DEV)  # (only m of them count)
    cnt = torch.tensor([m], dtype=torch.int64, device=DEV)
    sentinel = torch.full_like(D["x"], float("nan"))
    sentinel.view(torch.int32)[:] = 0x7FC00123  # a NaN with a payload: "kept its bits" is more than "is NaN"
    out = sentinel.clone()
    HG.tonemap_forward(D["x"], e, ne, D["t16"], n_dev=cnt, sample_idx=idx, out=out)
    listed = torch.zeros(D["cap"], dtype=torch.bool, device=DEV)
    listed[perm[:m].to(DEV)] = True
    assert _same_bits(out[listed], direct[listed]) and _same_bits(out[~listed], sentinel[~listed])
    ref, bar = T.forward(c["w"], c["x"], _ref_exposure(c, kind), with_bound=True)
    rows = perm[:m].numpy()
    assert np.all(np.abs(out[:n].double().cpu().numpy()[rows] - ref[rows]) <= FORWARD_BAR_SHARE * bar[rows])
    inplace = D["x"].clone()
    HG.tonemap_forward(inplace, e, ne, D["t16"], n_dev=cnt, sample_idx=idx, out=inplace)
    assert _same_bits(inplace[listed], direct[listed]) and _same_bits(inplace[~listed], D["x"][~listed])


# ------------------------------------------------------------ 2. radiance mode
def test_radiance_mode_clamps_and_is_within_4_ulp():
    g = np.random.default_rng(7)
    x = np.concatenate([g.uniform(-30, 0, 300), g.uniform(0, 20, 3000), g.uniform(20, 60, 300),
                        [0.0, -0.0, 20.0, np.nextafter(np.float32(20), np.float32(0)), -np.inf, np.inf]])
    x = x.astype(np.float32).reshape(-1, 3)
    n = x.shape[0]
    X = _padded(x)
    cnt = torch.tensor([n], dtype=torch.int64, device=DEV)
    y = HG.tonemap_forward(X, None, 0, None, mode=HG.TONE_RADIANCE, n_dev=cnt, out=torch.full_like(X, float("nan")))
    assert bool(torch.isnan(y[n:]).all())
    y = y[:n].cpu().numpy()
    assert np.all(y[x <= 0] == 1.0) and np.all(y[x >= 20] == y[x == 20][0])  # (exp(20) itself: within the 4 ulp below)
    ref = T.radiance(x)
    ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
    err = np.abs(y.astype(np.float64) - ref) / ulp
    print(f"radiance: max error {err.max():.2f} ulp over {x.size} values")
    assert err.max() <= 4
    # the exposure and the weights play no part; in place is allowed
    X2 = X.clone()
    HG.tonemap_forward(X2, torch.full((1,), 8.0, device=DEV), 1, None, mode=HG.TONE_RADIANCE, n_dev=cnt, out=X2)
    assert _same_bits(X2[:n], torch.from_numpy(y).to(DEV)) and _same_bits(X2[n:], X[n:])


# ------------------------------------------------------------ 3. backward
_bwd = {}


def _backward_ref(n, kind):
    if (n, kind) not in _bwd:
        c = T.case(n)
        _bwd[n, kind] = T.backward(c["w"], c["x"], _ref_exposure(c, kind), c["dy"])
    return _bwd[n, kind]


def _run_backward(D, e, ne, alias=False, grad=None):
    grad = torch.zeros(HG.TONE_PARAMS, device=DEV) if grad is None else grad
    if alias:
        dx = D["dy"].clone()
        assert HG.tonemap_backward(D["x"], e, ne, D["t16"], dx, grad, n_dev=D["cnt"], out=dx) is dx
    else:
        dx = HG.tonemap_backward(D["x"], e, ne, D["t16"], D["dy"], grad, n_dev=D["cnt"],
                                 out=torch.full_like(D["x"], float("nan")))
    return dx, grad


# every size with per-row exposures; the exposure's other forms at n = 1, 257 and 4099
_BWD_CASES = [(n, "per row") for n in T.SIZES] + [(n, k) for n in (1, 257, 4099) for k in ("absent", "uniform")]


@pytest.mark.parametrize("n,kind", _BWD_CASES)
def test_backward_is_within_the_summation_bars(n, kind):
    """dL/dlog_rad and all 6144 weight gradients, elementwise: |dev - ref| <= 2^-23 (n_terms + 64) S + Bamb."""
    c, D = T.case(n), _dev(n)
    e, ne = _exposure(D, kind)
    ref = _backward_ref(n, kind)
    dx, grad = _run_backward(D, e, ne)
    edx = np.abs(dx[:n].double().cpu().numpy() - ref["dx"])
    eg = np.abs(grad.double().cpu().numpy() - ref["grad"])
    with np.errstate(divide="ignore", invalid="ignore"):
        sdx = np.nanmax(np.where(ref["dx_bar"] > 0, edx / ref["dx_bar"], 0.0))
        sg = np.nanmax(np.where(ref["grad_bar"] > 0, eg / ref["grad_bar"], 0.0))
    print(f"n = {n}, exposure {kind}: dL/dx max err {edx.max():.3e} (largest share of its bar {sdx:.3f}); "
          f"dL/dtone max err {eg.max():.3e} (share {sg:.4f}); {ref['n_amb']} ambiguous pairs")
    assert np.all(edx <= ref["dx_bar"]) and np.all(eg <= ref["grad_bar"])
    assert float(np.abs(ref["grad"]).max()) > 0 and bool(torch.isnan(dx[n:]).all())
    # dL_dlog_rad written over dL_drgbs: the same bits
    dx2, grad2 = _run_backward(D, e, ne, alias=True)
    assert _same_bits(dx2[:n], dx[:n]) and _same_bits(dx2[n:], D["dy"][n:]) and _same_bits(grad2, grad)


# ------------------------------------------------------------ 4. structure
@pytest.mark.parametrize("n", [65, 4099, T.SIZES[-1]])
def test_backward_structure(n):
    c, D = T.case(n), _dev(n)
    e, ne = _exposure(D, "per row")
    dx, grad = _run_backward(D, e, ne)
    A, B = T.split(grad.cpu().numpy())
    assert np.all(A[:, :, 1:].view(np.int32) == A[:, :, 1:2].view(np.int32))  # the fifteen padding columns: one value
    assert np.all(B[:, 1:].view(np.int32) == 0) and np.abs(B[:, 0]).max() > 0  # dB[1..15] untouched
    # two runs: the same bits; a second call adds onto the first
    dx_b, grad_b = _run_backward(D, e, ne)
    assert _same_bits(dx_b[:n], dx[:n]) and _same_bits(grad_b, grad)
    _, twice = _run_backward(D, e, ne, grad=grad_b)
    assert twice is grad_b and _same_bits(twice, 2 * grad)
    # rows with a zero dL_drgbs change nothing: drop them (and garble their inputs) and the sums stay
    zero = torch.from_numpy((c["dy"] == 0).all(1))
    assert 0 < int(zero.sum()) < n or n < 8
    assert bool((dx[:n][zero.to(DEV)] == 0).all())
    D2 = dict(D, x=D["x"].clone())
    D2["x"][:n][zero.to(DEV)] = float("nan")
    dx_c, grad_c = _run_backward(D2, e, ne)
    assert _same_bits(grad_c, grad) and bool((dx_c[:n][zero.to(DEV)] == 0).all())
    nothing = dict(D, dy=torch.zeros_like(D["dy"]))
    dx_z, grad_z = _run_backward(nothing, e, ne)
    assert bool((grad_z == 0).all()) and bool((dx_z[:n] == 0).all())


def test_workspace_is_bounded_and_a_short_one_is_refused():
    K = HG._K()
    assert K.ngp_tonemap_backward_workspace(1 << 30) == K.ngp_tonemap_backward_workspace(512 * 256) == 512 * 384 * 4
    D = _dev(4099)
    with pytest.raises(RuntimeError, match="workspace"):
        HG.tonemap_backward(D["x"], None, 0, D["t16"], D["dy"], torch.zeros(HG.TONE_PARAMS, device=DEV), n_dev=D["cnt"],
                            workspace=torch.empty(16, device=DEV))


# ------------------------------------------------------------ 5. autograd surface
def _exposure_model(seed=5, occ_frac=0.02):
    """An exposure-conditioned NGP with a seeded table and a ~2 % random bitfield."""
    from models.networks import NGP
    m = NGP(0.5, 'None', False, use_exposure=True)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.params[HG.MLP_PARAMS:].uniform_(-1, 1, generator=g)
        bits = (torch.rand(m.density_bitfield.numel() * 8, generator=g) < occ_frac).to(torch.uint8)
        m.density_bitfield.copy_((bits.view(-1, 8) << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8))
    return m.to(DEV)


@pytest.fixture(scope="module")
def model():
    return _exposure_model()


def _points(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = ((torch.rand(n, 3, generator=g) - 0.5) * 0.9).to(DEV)
    d = torch.randn(n, 3, generator=g)
    return x.contiguous(), (d / d.norm(dim=1, keepdim=True)).to(DEV).contiguous()


@pytest.mark.parametrize("kind", ["absent", "none", "uniform", "per row", "per row flat"])
def test_model_forward_equals_field_then_kernels_bit_for_bit(model, kind):
    n = 1000
    x, d = _points(n, 11)
    g = torch.Generator().manual_seed(12)
    dsig, drgb = torch.randn(n, generator=g).to(DEV), torch.randn(n, 3, generator=g).to(DEV)
    per_row = torch.tensor(T.EXPOSURES)[torch.randint(5, (n,), generator=g)].to(DEV)
    kw = {"absent": {}, "none": {"exposure": None}, "uniform": {"exposure": torch.tensor([2.0], device=DEV)},
          "per row": {"exposure": per_row[:, None]}, "per row flat": {"exposure": per_row}}[kind]
    e, ne = HG.tone_exposure(kw.get("exposure"), n, DEV)
    model.zero_grad()
    sig, rgb = model(x, d, **kw)
    ((sig * dsig).sum() + (rgb * drgb).sum()).backward()
    # by hand: the field in RGB_NONE, then the kernels
    p16, t16 = model._shadow.get(), model._tone_shadow.get()
    s2, raw, enc, _ = HG.field_forward(x, d, model.grid, p16, rgb_act=HG.RGB_NONE)
    y2 = HG.tonemap_forward(raw, e, ne, t16)
    assert _same_bits(sig.detach(), s2) and _same_bits(rgb.detach(), y2)
    gt = torch.zeros(HG.TONE_PARAMS, device=DEV)
    draw = HG.tonemap_backward(raw, e, ne, t16, drgb, gt)
    gp = torch.zeros_like(model.params)
    HG.field_backward_sparse(x, d, model.grid, p16, enc, dsig, draw, gp, rgb_act=HG.RGB_NONE)
    assert _same_bits(model.tone_params.grad, gt) and float(gt.abs().max()) > 0
    # (the field's backward adds with fp32 atomics: the same terms -- dL/dlog_rad is the same bits -- in another
    # order from run to run, as in test_hdr_gpu.py)
    assert float((model.params.grad - gp).abs().max()) <= 1e-5 * float(gp.abs().max())
    with torch.no_grad():
        s3, r3 = model(x, d, **kw)
    assert _same_bits(s3, s2) and _same_bits(r3, y2)
    if kind == "absent":
        assert _same_bits(model.log_radiance_to_rgb(raw), y2)
        with torch.no_grad():
            _, rad = model(x, d, output_radiance=True, exposure=per_row)
        assert _same_bits(rad, HG.tonemap_forward(raw, None, 0, None, mode=HG.TONE_RADIANCE))
        with pytest.raises(NotImplementedError, match="forward-only"):
            model(x, d, output_radiance=True)
    for bad in (torch.ones(n - 1, device=DEV), torch.ones(n, 2, device=DEV)):
        with pytest.raises(ValueError, match="exposure"):
            model(x, d, exposure=bad)


def test_unit_exposure_term_reaches_the_tonemappers_only(model):
    """train.py:182-187: log_radiance_to_rgb(zeros(1,3), exposure=ones(1,1)), N = 1, with grad."""
    model.zero_grad()
    unit = model.log_radiance_to_rgb(torch.zeros(1, 3, device=DEV), exposure=torch.ones(1, 1, device=DEV))
    assert unit.shape == (1, 3) and unit.requires_grad
    (0.5 * (unit - 0.73) ** 2).mean().backward()
    assert model.params.grad is None
    gt = model.tone_params.grad
    w = model._tone_shadow.get().float().cpu().numpy()
    one = np.zeros((1, 3), np.float32)
    y = T.forward(w, one, np.ones(1))
    assert np.abs(unit.detach().cpu().numpy() - y).max() < 1e-6
    ref = T.backward(w, one, np.ones(1), ((y - 0.73) / 3).astype(np.float32))
    assert np.all(np.abs(gt.double().cpu().numpy() - ref["grad"]) <= ref["grad_bar"] + 1e-9) and float(gt.abs().max()) > 0


def test_fused_adam_steps_the_tone_parameters_and_their_shadow():
    from optimizers import FusedAdam
    m = _exposure_model(seed=6)
    opt = FusedAdam([m.params, m.tone_params], 1e-2, eps=1e-15)
    x, d = _points(500, 13)
    t0, p0 = m.tone_params.detach().clone(), m.params.detach().clone()
    sig, rgb = m(x, d, exposure=torch.full((500, 1), 2.0, device=DEV))
    (sig.mean() + rgb.sum()).backward()
    opt.step()
    moved = (m.tone_params.detach() != t0).view(3, 2, 1024)
    A_moved = moved[:, 0].view(3, 64, 16)
    # a unit that fired on some row moves in all sixteen columns (the padding columns carry the bias's
    # gradient), one that never fired in none; of B only row 0 moves
    assert bool((A_moved.all(-1) | ~A_moved.any(-1)).all()) and float(A_moved.float().mean()) > 0.25
    assert bool(moved[:, 1, :64].any()) and not bool(moved[:, 1, 64:].any())
    assert float((m.params.detach() - p0).abs().max()) > 0
    half = m._tone_shadow.half
    assert m._tone_shadow.get() is half  # current: no re-cast
    assert torch.equal(half, m.tone_params.detach().half())
    assert torch.equal(m._shadow.get(), m.params.detach().half())


# ------------------------------------------------------------ 6. render()
def _rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = ((torch.rand(n, 3, generator=g) - 0.5) * 0.8).to(DEV)
    d = torch.randn(n, 3, generator=g)
    return o.contiguous(), (d / d.norm(dim=1, keepdim=True)).to(DEV).contiguous()


def test_training_render_with_per_ray_exposure_equals_the_hand_composition(model):
    from models.custom_functions import RayAABBIntersector, RayMarcher, VolumeRenderer
    from models.rendering import MAX_SAMPLES, NEAR_DISTANCE, render
    n = 512
    o, d = _rays(n, 31)
    g = torch.Generator().manual_seed(32)
    e = torch.tensor(T.EXPOSURES)[torch.randint(5, (n, 1), generator=g)].to(DEV)
    torch.manual_seed(33)
    res = render(model, o, d, test_time=False, exposure=e)
    torch.manual_seed(33)  # (the marcher's jitter)
    with torch.no_grad():
        _, hits_t, _ = RayAABBIntersector.apply(o, d, model.center, model.half_size, 1)
        h0 = hits_t[:, 0, 0]
        hits_t[:, 0, 0] = torch.where((h0 >= 0) & (h0 < NEAR_DISTANCE), torch.full_like(h0, NEAR_DISTANCE), h0)
        rays_a, xyzs, dirs, deltas, ts, _ = RayMarcher.apply(o, d, hits_t[:, 0], model.density_bitfield, model.cascades,
                                                             model.scale, 0., model.grid_size, MAX_SAMPLES)
        per_sample = torch.repeat_interleave(e[rays_a[:, 0]], rays_a[:, 2], 0)
        assert per_sample.shape == (xyzs.shape[0], 1) and xyzs.shape[0] > n
        sig, raw, _, _ = HG.field_forward(xyzs, dirs, model.grid, model._shadow.get(), rgb_act=HG.RGB_NONE)
        rgbs = HG.tonemap_forward(raw, per_sample.reshape(-1).contiguous(), xyzs.shape[0], model._tone_shadow.get())
        _, opacity, depth, rgb, _ = VolumeRenderer.apply(sig, rgbs, deltas, ts, rays_a, 1e-4)
        rgb = rgb + torch.ones(3, device=DEV) * (1 - opacity)[:, None]
    assert _same_bits(res["opacity"].detach(), opacity) and _same_bits(res["rgb"].detach(), rgb)
    assert res["rgb"].requires_grad


def test_device_loop_follows_the_exposure_without_recapture(model):
    from models.rendering import render
    n = 4096
    o, d = _rays(n, 3)
    model.__dict__.pop('_test_renderers', None)
    frames = {}
    with torch.no_grad():
        for e in (0.5, 4.0, 0.5):
            ex = torch.tensor([e], device=DEV)
            dev = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in render(model, o, d, test_time=True, exposure=ex).items()}
            host = render(model, o, d, test_time=True, exposure=ex, device_loop=False)
            for k in ("rgb", "opacity", "depth"):
                assert torch.equal(dev[k], host[k]), (e, k)
            assert int(dev["total_samples"]) == int(host["total_samples"])
            if e in frames:
                assert torch.equal(frames[e]["rgb"], dev["rgb"])
            frames[e] = dev
        assert len(model._test_renderers) == 1
        rr = next(iter(model._test_renderers.values()))
        graphs = dict(rr._graphs)
        assert 1 <= len(graphs) <= 2 and rr.tone_mode == HG.TONE_LDR
        assert torch.equal(frames[0.5]["opacity"], frames[4.0]["opacity"])  # sigma knows no exposure
        assert not torch.equal(frames[0.5]["rgb"], frames[4.0]["rgb"])
        # the slider moves: another exposure, the very same captured graphs
        again = render(model, o, d, test_time=True, exposure=torch.tensor([1.0], device=DEV))["rgb"].clone()
        unit = render(model, o, d, test_time=True)["rgb"].clone()  # no exposure: unit
        assert len(model._test_renderers) == 1 and len(rr._graphs) == len(graphs)
        assert all(rr._graphs[k] is g for k, g in graphs.items())
        assert torch.equal(again, unit) and not torch.equal(again, frames[0.5]["rgb"])
        # the renderer's copy of the tone shadow follows the parameters
        with torch.no_grad():
            model.tone_params.mul_(1.5)
        moved = render(model, o, d, test_time=True, exposure=torch.tensor([1.0], device=DEV))["rgb"].clone()
        host = render(model, o, d, test_time=True, exposure=torch.tensor([1.0], device=DEV), device_loop=False)["rgb"]
        with torch.no_grad():
            model.tone_params.div_(1.5)
        assert torch.equal(moved, host) and not torch.equal(moved, again) and len(model._test_renderers) == 1
        # radiance through the device loop: its own renderer, exp(clamp) of the log radiance >= 1 where opaque
        rad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in render(model, o, d, test_time=True, output_radiance=True).items()}
        rad_host = render(model, o, d, test_time=True, output_radiance=True, device_loop=False)
        assert torch.equal(rad["rgb"], rad_host["rgb"]) and torch.equal(rad["opacity"], frames[0.5]["opacity"])
        assert len(model._test_renderers) == 2
        # every sample's radiance is >= 1 and every tonemapped colour <= 1: so are the composites, per unit opacity
        op = frames[4.0]["opacity"][:, None]
        assert float(op.max()) > 0
        assert bool((rad["rgb"] >= op * (1 - 1e-4)).all()) and bool((frames[4.0]["rgb"] <= op * (1 + 1e-4) + 1e-6).all())
        assert not torch.equal(rad["rgb"], frames[4.0]["rgb"])


def test_sh_probes_pass_the_mode_through(model):
    import probes
    from models.rendering import render
    P, R, B = 2, 65, 64
    g = torch.Generator().manual_seed(21)
    pts = ((torch.rand(P, 3, generator=g) - 0.5) * 0.8).to(DEV)
    dirs = probes.get_sphere_rays(P, R, generator=g, device=DEV)
    res = {k: v.clone() for k, v in probes.sh_probes(model, pts, dirs, return_rays=True, exposure=2.0).items()}
    idx = [min(i, P - 1) for i in range(B)]
    o = pts[idx][:, None].expand(B, R, 3).reshape(-1, 3).contiguous()
    dd = dirs[idx].reshape(-1, 3).contiguous()
    with torch.no_grad():
        out = render(model, o, dd, test_time=True, exposure=torch.tensor([2.0], device=DEV))
    assert torch.equal(res["rgb"], out["rgb"].view(B, R, 3)[:P])


# ------------------------------------------------------------ 7. a short training run
# Seed-to-seed spread of the torch-op path's held-out PSNR over 3 seeds, measured once on an MI355X
# (28.72, 28.76, 29.34 dB at seeds 4, 5, 6): the margin is twice that, at least 0.3 dB.
TORCH_PATH_SPREAD_DB = 0.623
MARGIN_DB = max(2 * TORCH_PATH_SPREAD_DB, 0.3)
TRAIN_STEPS = 300


def _train_exposure_module():
    spec = importlib.util.spec_from_file_location("train_exposure", os.path.join(ROOT, "scripts", "train_exposure.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _held_out_psnr(TE, data, seed=4, **kw):
    loop = TE.ExposureLoop(data, batch=1024, seed=seed, **kw)
    for _ in range(TRAIN_STEPS):
        loss, _ = loop.step()
    assert bool(torch.isfinite(loss))
    psnr = loop.test_psnr()
    assert sorted(psnr) == [0.5, 2.0]
    return sum(psnr.values()) / len(psnr), loop


def test_short_training_run_matches_the_torch_restatement_and_uses_the_exposure():
    """The analytic scene, radiance = 4 x colour through a fixed response curve, trained at exposures
    {1/4, 1, 4} for a few hundred steps of 1024 rays; PSNR on held-out views at the held-out exposures
    {1/2, 2}: the kernels against the tonemappers restated in torch ops (same weights, same seeds), and
    against the same run blind to the exposure."""
    TE = _train_exposure_module()
    data = TE.synthetic_data(res=64, n_train=12, n_test=2, device=DEV)
    assert data.train_rays.shape == (36, 4096, 4) and data.test_rays.shape == (4, 4096, 4)
    kernels, loop = _held_out_psnr(TE, data)
    assert torch.equal(loop.model._tone_shadow.get(), loop.model.tone_params.detach().half())
    torch_ops, _ = _held_out_psnr(TE, data, torch_ops=True)
    blind, _ = _held_out_psnr(TE, data, zero_exposure=True)
    print(f"held-out PSNR after {TRAIN_STEPS} steps: kernels {kernels:.2f} dB, torch ops {torch_ops:.2f} dB "
          f"(margin {MARGIN_DB:.2f} dB), exposure-blind {blind:.2f} dB")
    assert kernels >= torch_ops - MARGIN_DB
    assert kernels > blind
