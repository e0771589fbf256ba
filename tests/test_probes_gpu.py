"""Light probes on the GPU: ngp_probe_rays, ngp_render_test_finish_sh,
ngp_probe_sh9_project, render(SH_bkg=...) and probes.sh_probes.

Error bounds (u = 2^-24, fp32 unit roundoff), both against an fp64 evaluation
of the same fp32 inputs:
  projection  (R + 16) u (4 pi / R) sum_r |Y_k(d_r) v_r|   -- the worst case of
              an fp32 sum of R terms in ANY order (R u sum|terms|) plus 16
              roundings for the basis, the products and the scale;
  finish      32 u ((1 - opacity) sum_k |Y_k shec_k| + |rgb|) -- nine products
              summed, the clamp, the blend.
Neither is measured from the kernels.  A dropped or doubled ray moves a
coefficient by about 1/R of its magnitude: 1e5 bounds at the sizes used here.
"""
import math

import pytest
import torch

import probes
import synthetic as S
import vren
from models.rendering import NEAR_DISTANCE, render
from test_renderer_gpu import _scene_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
CANARY = 12345.0


def _basis64(d):
    """SH9 basis in fp64 from fp32 directions (the constants of the C-ABI header)."""
    d = d.double()
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return torch.stack([0.2820947918 * torch.ones_like(x), 0.4886025119 * y, 0.4886025119 * z, 0.4886025119 * x,
                        1.0925484306 * x * y, 1.0925484306 * y * z, 0.3153915653 * (3 * z * z - 1),
                        1.0925484306 * x * z, 0.5462742153 * (x * x - y * y)], -1)


def _project64(dirs, vals):
    """fp64 get_SH_coeff of vals (P,R,C) and the projection bound per coefficient."""
    R = dirs.shape[1]
    Y, v = _basis64(dirs), vals.double()
    ref = torch.einsum("prk,prc->pkc", Y, v) * (4 * math.pi / R)
    mag = torch.einsum("prk,prc->pkc", Y.abs(), v.abs()) * (4 * math.pi / R)
    return ref, (R + 16) * U * mag


def _assert_projection(name, out, ref, bound):
    err = (out.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max error {float(err.max()):.3e}, max error/bound {ratio:.4f}")
    assert bool((err <= bound).all()), name


@pytest.fixture(scope="module")
def model():
    return _scene_model(0.5, 0.02, seed=5)


# ------------------------------------------------------------ probe rays
@pytest.mark.parametrize("per_probe", [False, True])
def test_probe_rays_bit_identical_to_expand_intersect_clamp(model, per_probe):
    P, R = 3, 65
    # inside the box; outside it; outside, 0.005 (< NEAR_DISTANCE) in front of the +x face
    pts = torch.tensor([[0.1, -0.2, 0.05], [0.9, 0.1, -0.2], [0.505, 0.0, 0.1]], device=DEV)
    g = torch.Generator().manual_seed(11)
    dirs = probes.get_sphere_rays(P if per_probe else 1, R, generator=g, device=DEV)
    dirs = dirs.contiguous() if per_probe else dirs[0].contiguous()
    o = pts[:, None].expand(P, R, 3).reshape(-1, 3).contiguous()
    d = (dirs if per_probe else dirs[None].expand(P, R, 3)).reshape(-1, 3).contiguous()
    _, ht, _ = vren.ray_aabb_intersect(o, d, model.center, model.half_size, 1)
    raw = ht[:, 0].contiguous()
    ref = raw.clone()
    ref[(ref[:, 0] >= 0) & (ref[:, 0] < NEAR_DISTANCE), 0] = NEAR_DISTANCE
    # the cases are all there: misses, hits from outside, t1 = 0, 0 < t1 < near
    assert (raw[:, 0] == -1).any() and (raw[:, 0] > NEAR_DISTANCE).any() and (raw[:R, 0] == 0).all()
    assert ((raw[2 * R:, 0] > 0) & (raw[2 * R:, 0] < NEAR_DISTANCE)).any()
    ro, rd, hits = vren.probe_rays(pts, dirs, model.center, model.half_size, NEAR_DISTANCE)
    assert torch.equal(ro, o) and torch.equal(rd, d)
    assert torch.equal(hits, ref)


# ------------------------------------------------------------ projection
@pytest.mark.parametrize("R", [1, 63, 64, 65, 257, 2048])
@pytest.mark.parametrize("P", [1, 3])
def test_projection_bound_determinism_and_margins(P, R):
    g = torch.Generator().manual_seed(100 * P + R)
    dirs = probes.get_sphere_rays(P, R, generator=g, device=DEV).contiguous()
    rgb = torch.rand(P, R, 3, generator=g).to(DEV)
    opa = torch.rand(P, R, generator=g).to(DEV)
    keep = [t.clone() for t in (dirs, rgb, opa)]
    pad = 64

    def run(with_trans):
        buf_c = torch.full((P * 27 + 2 * pad,), CANARY, device=DEV)
        buf_t = torch.full((P * 9 + 2 * pad,), CANARY, device=DEV)
        c, t = buf_c[pad:pad + P * 27].view(P, 9, 3), buf_t[pad:pad + P * 9].view(P, 9)
        if with_trans:
            vren.probe_sh9_project(dirs, rgb, opa, rgb_sh=c, trans_sh=t)
        else:
            vren.probe_sh9_project(dirs, rgb, rgb_sh=c)
        torch.cuda.synchronize()
        for buf, n in ((buf_c, P * 27), (buf_t, P * 9)):
            assert bool((buf[:pad] == CANARY).all()) and bool((buf[pad + n:] == CANARY).all()), "margin overwritten"
        return c.clone(), t.clone()

    c1, t1 = run(True)
    c2, t2 = run(True)
    assert torch.equal(c1, c2) and torch.equal(t1, t2), "not run-to-run bit-identical"
    c3, t3 = run(False)  # trans_sh = None: same radiance coefficients, transmittance output untouched
    assert torch.equal(c3, c1) and bool((t3 == CANARY).all())
    for t, k in zip((dirs, rgb, opa), keep):
        assert torch.equal(t, k), "input modified"
    ref, bound = _project64(dirs, rgb)
    _assert_projection(f"rgb_sh P={P} R={R}", c1, ref, bound)
    ref, bound = _project64(dirs, (1 - opa.double())[..., None])
    _assert_projection(f"trans_sh P={P} R={R}", t1[..., None], ref, bound)
    # the public helper takes the same path
    assert torch.equal(probes.get_SH_coeff(dirs, rgb), c1)


# --------------------------------------------------- render() with SH_bkg
def _frame(scale, W=64):
    sc = S.AnalyticScene(W=W, H=W, n_images=2)
    n = W * W
    o, d = sc.rays(torch.zeros(n, dtype=torch.int64), torch.arange(n))
    return (o * (2 * scale)).to(DEV).contiguous(), d.to(DEV).contiguous()


def _light(seed=3):
    g = torch.Generator().manual_seed(seed)
    sh = torch.rand(9, 3, generator=g) - 0.5
    sh[0] = torch.tensor([2.0, -3.0, 1.0])  # DC: green's is negative, the clamp works there
    return sh.to(DEV)


@pytest.mark.parametrize("device_loop", [True, False])
def test_render_sh_bkg_inside_finish_bound(model, device_loop):
    o, d = _frame(0.5)
    sh = _light()
    kw = dict(test_time=True, device_loop=device_loop)
    with torch.no_grad():
        base = render(model, o, d, blend_bkg=False, **kw)
        res = render(model, o, d, SH_bkg=sh, **kw)
        res_cpu_light = render(model, o, d, SH_bkg=sh.cpu(), **kw)
    assert torch.equal(res["opacity"], base["opacity"]) and torch.equal(res["depth"], base["depth"])
    assert torch.equal(res_cpu_light["rgb"], res["rgb"])
    m = 1 - base["opacity"].double()
    assert float(m.max()) > 0.5, "the frame must show background"
    terms = _basis64(d)[:, :, None] * sh.double()[None]          # (N,9,3)
    bg, bg_mag = terms.sum(1), terms.abs().sum(1)
    ref = base["rgb"].double() + bg.clamp_min(0) * m[:, None]
    bound = 32 * U * (m[:, None] * bg_mag + base["rgb"].double().abs())
    err = (res["rgb"].double() - ref).abs()
    print(f"finish device_loop={device_loop}: max error {float(err.max()):.3e}, "
          f"max error/bound {float((err / bound.clamp_min(1e-300)).max()):.4f}")
    assert bool((err <= bound).all())
    # where the light is negative (by more than its own rounding) the clamp leaves the pixel as it was
    neg = bg[:, 1] < -32 * U * bg_mag[:, 1]
    assert bool(neg.any()) and bool((bg[:, 0] > 0).any())
    assert torch.equal(res["rgb"][neg, 1], base["rgb"][neg, 1])
    assert not torch.equal(res["rgb"][:, 0], base["rgb"][:, 0])


@pytest.mark.parametrize("device_loop", [True, False])
def test_render_background_precedence(model, device_loop):
    o, d = _frame(0.5)
    sh = _light()
    im = torch.rand(o.shape[0], 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    kw = dict(test_time=True, device_loop=device_loop)
    with torch.no_grad():
        both = render(model, o, d, SH_bkg=sh, IM_bkg=im, **kw)
        im_only = render(model, o, d, IM_bkg=im, **kw)
        off = render(model, o, d, SH_bkg=sh, blend_bkg=False, **kw)
        none = render(model, o, d, blend_bkg=False, **kw)
        black = render(model, o, d, **kw)
    assert torch.equal(both["rgb"], im_only["rgb"])       # IM_bkg overrides SH_bkg
    assert torch.equal(off["rgb"], none["rgb"])           # blend_bkg=False skips both
    assert torch.equal(black["rgb"], none["rgb"])         # and the default is black
    assert not torch.equal(im_only["rgb"], none["rgb"])


# ------------------------------------------------------ sh_probes end to end
@pytest.mark.parametrize("scale,esf,with_sh", [(0.5, 0.0, False), (0.5, 0.0, True), (16.0, 1 / 256, True)])
def test_sh_probes_equal_render_per_batch(model, scale, esf, with_sh):
    """P = 5 probes in batches of 2: two full batches and one filled up with a
    repeat of the last point."""
    mdl = model if scale == 0.5 else _scene_model(scale, 0.01, seed=5)
    P, R, B = 5, 256, 2
    g = torch.Generator().manual_seed(21)
    pts = ((torch.rand(P, 3, generator=g) - 0.5) * 0.8 * (2 * scale)).to(DEV)
    dirs = probes.get_sphere_rays(P, R, generator=g, device=DEV)
    sh = _light() if with_sh else None
    rk = dict(exp_step_factor=esf) if esf else {}
    res = probes.sh_probes(mdl, pts, dirs, SH_bkg=sh, probes_per_batch=B, return_rays=True, **rk)
    assert res["rgb_sh"].shape == (P, 9, 3) and res["trans_sh"].shape == (P, 9, 1)
    assert res["rgb"].shape == (P, R, 3) and res["opacity"].shape == (P, R) and torch.equal(res["dirs"], dirs)
    res = {k: v.clone() for k, v in res.items()}
    # render() on the same batches with the same padding
    rgb, opa = [], []
    for b0 in range(0, P, B):
        idx = [min(i, P - 1) for i in range(b0, b0 + B)]
        o = pts[idx][:, None].expand(B, R, 3).reshape(-1, 3).contiguous()
        d = dirs[idx].reshape(-1, 3).contiguous()
        with torch.no_grad():
            out = render(mdl, o, d, test_time=True, **({"SH_bkg": sh} if with_sh else {}), **rk)
        valid = min(B, P - b0)
        rgb.append(out["rgb"].view(B, R, 3)[:valid])
        opa.append(out["opacity"].view(B, R)[:valid])
    rgb, opa = torch.cat(rgb), torch.cat(opa)
    assert torch.equal(res["rgb"], rgb) and torch.equal(res["opacity"], opa)
    assert 0 < float(opa.mean()) < 1
    ref, bound = _project64(dirs, rgb)
    _assert_projection(f"sh_probes rgb_sh scale={scale}", res["rgb_sh"], ref, bound)
    ref, bound = _project64(dirs, (1 - opa.double())[..., None])
    _assert_projection(f"sh_probes trans_sh scale={scale}", res["trans_sh"], ref, bound)
    again = probes.sh_probes(mdl, pts, dirs, SH_bkg=sh, probes_per_batch=B, return_rays=True, **rk)
    for k in ("rgb_sh", "trans_sh", "rgb", "opacity"):
        assert torch.equal(again[k], res[k]), k
    if with_sh:  # the light reaches the probes
        dark = probes.sh_probes(mdl, pts, dirs, SH_bkg=sh, blend_bkg=False, probes_per_batch=B, **rk)
        assert torch.equal(dark["trans_sh"], res["trans_sh"]) and not torch.equal(dark["rgb_sh"], res["rgb_sh"])


def test_get_SH_val_kernel_path_inside_finish_bound():
    g = torch.Generator().manual_seed(9)
    d = probes.get_sphere_rays(1, 1000, generator=g, device=DEV)[0].contiguous()
    sh = _light()
    out = probes.get_SH_val(sh, d, clamp_postive=True)
    assert torch.equal(out, probes.get_SH_val(sh, d, clamp_postive=True, kernel=True))
    terms = _basis64(d)[:, :, None] * sh.double()[None]
    err = (out.double() - terms.sum(1).clamp_min(0)).abs()
    assert bool((err <= 32 * U * terms.abs().sum(1)).all())
    torch.testing.assert_close(probes.get_SH_val(sh, d, clamp_postive=True, kernel=False), out, atol=1e-5, rtol=0)
    assert float(probes.get_SH_val(sh, d).min()) < 0  # unclamped: torch expressions
