"""composite_ref.py on the CPU: the analytic fp64 backward equals fp64 autograd
through the truncated forward; the input sets meet their precondition and
cover what they claim; and the project's fp32 CPU path (the oracle's
restatement of volumerendering.cu / losses.cu plus the reference's torch
expressions for the loss, all fp32) lies inside the bounds with the same
termination counts -- so the bounds hold for a correct fp32 implementation."""
import math

import pytest
import torch

import composite_ref as CR
import oracle as O
from test_composite_gpu import _DistortionCPU
from test_distortion_cpu import _closed_form

SETS = [("thr1e-4", 0), ("thr1e-2", 1)]
CONFIGS = [  # loss_type, bg, lambda_depth, depth_scale, lambda_distortion
    (0, "zero", 0.0, 1.0, 0.0), (0, "colour", 1e-2, 0.5, 1e-2), (1, "colour", 0.0, 1.0, 1e-2),
    (1, "zero", 1e-2, 0.5, 0.0), (2, "colour", 1e-2, 0.5, 0.0), (2, "zero", 0.0, 1.0, 1e-2),
    (3, "zero", 1e-2, 0.5, 1e-2), (3, "colour", 0.0, 1.0, 0.0),
]


@pytest.mark.parametrize("name,seed", SETS)
def test_input_sets_meet_precondition_and_coverage(name, seed):
    inp = CR.rows(name, seed)
    bad, _ = CR.margin_violations(inp.sig, inp.deltas, inp.rays_a, inp.T_thr)
    assert not bool(bad.any())
    f = CR.composite_ref64(inp.sig, inp.rgbs, inp.deltas, inp.ts, inp.rays_a, inp.T_thr)
    # the issue's form of the precondition, spelled out once more from scratch
    for r in range(inp.n_rows):
        s, N = int(inp.rays_a[r, 1]), int(inp.rays_a[r, 2])
        lnT = -torch.cumsum(inp.sig[s:s + N].double() * inp.deltas[s:s + N].double(), 0)
        upto = min(int(f.K[r]) + 1, N)
        k = torch.arange(upto).double()
        assert bool(((lnT[:upto] - math.log(inp.T_thr)).abs() >= 4 * (k + 2) * 2.0 ** -20).all()), r
    N, K = f.N, f.K
    term = K < N
    assert set(CR.LENGTHS) <= set(N.tolist())
    for p in CR.TERM_POS:
        assert bool((term & (K == p)).any()), p
    assert bool((term & (K == N - 1) & (N > 256)).any())  # the row's last sample, in a spilled chunk
    for n in CR.LENGTHS:  # transparent to the end on both sides of every chunk boundary
        assert bool((~term & (N == n)).any()), n
    fam = [k[0] for k in inp.kind]
    assert fam.count("gradual") >= 10 and all(bool(term[r]) for r in range(inp.n_rows) if fam[r] == "gradual")
    op = [r for r in range(inp.n_rows) if fam[r] == "opaque"]
    x32 = (inp.sig * inp.deltas)  # fp32 product
    for r in op + inp.v1_rows.tolist():  # alpha == 1 exactly in fp32: 1 - exp(-x) with exp(-x) < 2^-25
        assert float(x32[int(inp.rays_a[r, 1]) + int(K[r])]) > 18.0
    # ray != row, storage order != row order
    assert not torch.equal(inp.rays_a[:, 0], torch.arange(inp.n_rows))
    assert not bool((inp.rays_a[1:, 1] >= inp.rays_a[:-1, 1]).all())
    assert [fam[r] for r in range(5)] == ["term", "never", "never", "v1", "gradual"]
    # the depth term: both sides of the clip, and the v == 1 rows give exactly 1.0f in fp32
    sc = torch.tensor(CR.DEPTH_SCALE, dtype=torch.float32)
    v = f.D / float(sc) + CR.C_EPS
    rest = torch.ones(inp.n_rows, dtype=torch.bool)
    rest[inp.v1_rows] = False
    assert int((v[rest] > 1 + 1e-3).sum()) > 20 and int((v[rest] < 1 - 1e-3).sum()) > 20
    assert bool(((v[rest] - 1).abs() >= 1e-3).all())
    tot, _, dep32, _, _ = O.composite_train_fw(inp.sig, inp.rgbs, inp.deltas, inp.ts, inp.rays_a, inp.T_thr)
    v32 = dep32 / sc + torch.tensor(1e-10, dtype=torch.float32)
    assert v32.dtype == torch.float32 and inp.v1_rows.numel() >= 3
    assert bool((v32[inp.rays_a[inp.v1_rows, 0]] == 1.0).all())
    x = v32.clone().requires_grad_(True)
    torch.log(x.clip(max=1.0)).sum().backward()
    assert bool((x.grad[inp.rays_a[inp.v1_rows, 0]] == 1.0).all())  # torch's clip passes the gradient at equality
    assert bool(CR.clip_pass(v)[inp.v1_rows].all())


def test_distortion_scan_form_is_the_closed_form():
    inp = CR.rows("thr1e-4", 0)
    f = CR.composite_ref64(inp.sig, inp.rgbs, inp.deltas, inp.ts, inp.rays_a, inp.T_thr)
    ld, AB, _, _ = CR._dist_scan(f.w, f.Ts, f.Dl)
    ws = CR.flat(f, f.w)
    pick = torch.tensor([r for r in range(inp.n_rows) if int(f.N[r]) <= 200][:60])
    ra = inp.rays_a[pick].clone()
    ra[:, 0] = torch.arange(pick.numel())
    w64 = ws.clone().requires_grad_(True)
    ref = _closed_form(w64, inp.deltas.double(), inp.ts.double(), ra)
    torch.testing.assert_close(ld.sum(1)[pick], ref.detach(), rtol=1e-11, atol=1e-14)
    ref.sum().backward()
    gw = CR.flat(f, 2 * (AB + f.w * f.Dl / 3) * f.m)
    sel = torch.cat([torch.arange(int(s), int(s) + int(n)) for _, s, n in inp.rays_a[pick].tolist()])
    keep = CR.flat(f, f.m.double())[sel] > 0
    torch.testing.assert_close(gw[sel][keep], w64.grad[sel][keep], rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_analytic_backward_equals_autograd(cfg):
    """to 1e-11 of mag = bound / (C u), for the four loss types with and without bg / depth / distortion"""
    for name, seed in SETS:
        r = CR.reference(name, seed, *cfg, None)
        mag_s, mag_c = r.b_dsig / (2 * CR.U), r.b_drgbs / (2 * CR.U)
        es, ec = (r.dsig_an - r.dsig).abs(), (r.drgbs_an - r.drgbs).abs()
        assert bool((es <= 1e-11 * mag_s).all()), float((es / mag_s.clamp(min=1e-300)).max())
        assert bool((ec <= 1e-11 * mag_c).all()), float((ec / mag_c.clamp(min=1e-300)).max())
        assert float(r.dsig.abs().max()) > 0 and float(r.drgbs.abs().max()) > 0
        if cfg[2] != 0:  # the depth gradient is there on the v == 1 rows and on no clipped ray
            assert bool((r.gdep[CR.rows(name, seed).v1_rows] != 0).all())
            assert bool((r.gdep[~r.clip_pass] == 0).all()) and int((~r.clip_pass).sum()) > 20


def _torch_loss32(loss_type, rgb, gt, op, dep, ws, inp, lam_op, lam_depth, scale, lam_dist):
    """the reference's torch expressions (losses.py:63-82, the mse of upstream ngp_pl for type 1), fp32, per ray"""
    n = rgb.shape[0]
    if loss_type == 0:
        l = ((rgb - gt) / (rgb.detach() + 1e-3)) ** 2
    elif loss_type == 1:
        l = (rgb - gt) ** 2
    elif loss_type == 2:
        l = (torch.log((0.2935 + rgb) / (0.2935 + gt)) * 0.7607) ** 2
    else:
        l = (torch.tanh(rgb) - torch.tanh(gt)) ** 2
    o = op + 1e-10
    per = l.sum(1) / (3 * n) + lam_op * (-o * torch.log(o)) / n
    if lam_depth:
        per = per + (-lam_depth * torch.log((dep / scale + 1e-10).clip(max=1.0))) / n
    if lam_dist:
        per = per + lam_dist * _DistortionCPU.apply(ws, inp.deltas, inp.ts, inp.rays_a) / n
    return per


@pytest.mark.parametrize("name,seed", SETS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_fp32_cpu_path_inside_bounds(name, seed, cfg):
    loss_type, bgn, lam_depth, scale, lam_dist = cfg
    inp = CR.rows(name, seed)
    r = CR.reference(name, seed, *cfg, None, "serial")
    f, ray = r.f, r.f.ray
    s_ = inp.sig.clone().requires_grad_(True)
    c_ = inp.rgbs.clone().requires_grad_(True)
    _, op, dep, rgb, ws = O._VolumeRendererCPU.apply(s_, c_, inp.deltas, inp.ts, inp.rays_a, inp.T_thr)
    bg = CR.bg_tensor(bgn)
    xc = rgb + bg[None, :] * (1 - op)[:, None]
    per = _torch_loss32(loss_type, xc, inp.gt, op, dep, ws, inp, 1e-3, lam_depth, scale, lam_dist)
    per.sum().backward()
    tot = O.composite_train_fw(inp.sig, inp.rgbs, inp.deltas, inp.ts, inp.rays_a, inp.T_thr)[0]
    assert torch.equal(tot[ray], f.count)  # termination: exact on every row
    ra = {
        "rgb": CR.ratio((xc.detach().double()[ray] - r.xc).abs(), r.b_xc),
        "opacity": CR.ratio((op.detach().double()[ray] - f.O).abs(), r.b_O),
        "depth": CR.ratio((dep.detach().double()[ray] - f.D).abs(), r.b_D),
        "loss": CR.ratio((per.detach().double()[ray] - r.loss).abs(), r.b_loss),
        "ws": CR.ratio((ws.detach().double() - CR.flat(f, f.w)).abs(), CR.flat(f, r.fb.dw * 2 * CR.SLACK)),
        "dsig": CR.ratio((s_.grad.double() - CR.flat(f, r.dsig)).abs(), CR.flat(f, r.b_dsig)),
        "drgbs": CR.ratio((c_.grad.double() - CR.flat(f, r.drgbs)).abs(), CR.flat(f, r.b_drgbs)),
    }
    print(f"fp32 CPU path {name} {cfg}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ra.items()))
    assert all(v <= 1 for v in ra.values()), ra


@pytest.mark.parametrize("name,seed", SETS)
def test_fp32_cpu_compositing_backward_inside_bounds(name, seed):
    """O.composite_train_bw fed its own forward outputs and four non-zero upstream gradients"""
    inp = CR.rows(name, seed)
    g = torch.Generator().manual_seed(9)
    gop, gdep, grgb = (torch.randn(inp.n_rows, generator=g), torch.randn(inp.n_rows, generator=g),
                       torch.randn(inp.n_rows, 3, generator=g))
    gws = torch.randn(inp.n, generator=g)
    f = CR.composite_ref64(inp.sig, inp.rgbs, inp.deltas, inp.ts, inp.rays_a, inp.T_thr)
    dsig, drgbs, b_sig, b_rgb, fb = CR.train_bw_ref64(f, "serial", gop, gdep, grgb, gws)
    tot, op, dep, rgb, ws = O.composite_train_fw(inp.sig, inp.rgbs, inp.deltas, inp.ts, inp.rays_a, inp.T_thr)
    out = O.composite_train_bw(gop, gdep, grgb, gws, inp.sig, inp.rgbs, ws, inp.deltas, inp.ts, inp.rays_a, op, dep, rgb,
                               inp.T_thr)
    rs = CR.ratio((out[0].double() - CR.flat(f, dsig)).abs(), CR.flat(f, b_sig))
    rc = CR.ratio((out[1].double() - CR.flat(f, drgbs)).abs(), CR.flat(f, b_rgb))
    print(f"fp32 CPU composite_train_bw {name}: worst err / bound dsig {rs:.3f}, drgbs {rc:.3f}")
    assert rs <= 1 and rc <= 1 and torch.equal(tot[f.ray], f.count)
    assert float(CR.flat(f, dsig).abs().max()) > 0


@pytest.mark.parametrize("Ns", [1, 4, 8])
def test_alive_rows_and_fp32_cpu_test_compositing(Ns):
    t = CR.alive_rows(Ns, 3)
    bad, f = CR.margin_violations(t.sig.reshape(-1), t.deltas.reshape(-1), t.rays_a, t.T_thr, t.T0)
    assert not bool(bad.any())
    assert int((t.n_eff == 0).sum()) >= 3 and int((t.n_eff == Ns).sum()) >= 3 and float(t.op0.min()) >= 0
    if Ns > 1:
        assert int(((t.n_eff > 0) & (t.n_eff < Ns)).sum()) >= 3
    ref = CR.alive_ref64(t)
    assert int((ref.alive < 0).sum()) > 20 and int((ref.alive >= 0).sum()) > 20
    al, op, dep, rgb = t.alive.clone(), t.op0.clone(), t.dep0.clone(), t.rgb0.clone()
    O.composite_test_fw(t.sig, t.rgbs, t.deltas, t.ts, None, al, t.T_thr, t.n_eff, op, dep, rgb)
    assert torch.equal(al, ref.alive)
    ra = {"opacity": CR.ratio((op.double() - ref.op).abs(), ref.b_op),
          "depth": CR.ratio((dep.double() - ref.dep).abs(), ref.b_dep),
          "rgb": CR.ratio((rgb.double() - ref.rgb).abs(), ref.b_rgb)}
    print(f"fp32 CPU composite_test_fw Ns {Ns}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ra.items()))
    assert all(v <= 1 for v in ra.values()), ra
