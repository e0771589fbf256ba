"""The compositing kernels and the fused NeRF loss against the fp64 per-sample
references and derived per-element bounds of composite_ref.py, on its
designed input sets (shuffled rows, ray != row, every chunk boundary and
termination position, the v == 1 depth edge): ngp_composite_loss in every
loss type / bg / depth / distortion / n_rays combination of CASES, with its
sample list, counters and nullable outputs; vren.composite_train_fw / _bw fed
their own outputs; vren.composite_test_fw; losses.NeRFLoss per element and on
the shapes the fused path must not take.  Termination (n_active, counts,
alive) is compared exactly on every row: the inputs keep every transmittance
a margin away from the threshold (composite_ref.enforce_margin)."""
import ctypes

import pytest
import torch

import composite_ref as CR
import vren

pytestmark = pytest.mark.gpu
DEV = "cuda"
JUNK = 12345.0

# loss_type, bg, (lambda_depth, depth_scale), lambda_distortion, n_rays, input set: every value with the distortion
# term both off and on
CASES = [
    (0, "zero", (0.0, 1.0), 0.0, None, ("thr1e-4", 0)),
    (0, "colour", (1e-2, 0.5), 1e-2, None, ("thr1e-4", 0)),
    (1, "colour", (0.0, 1.0), 1e-2, None, ("thr1e-2", 1)),
    (1, "zero", (1e-2, 0.5), 0.0, None, ("thr1e-2", 1)),
    (2, "colour", (1e-2, 0.5), 0.0, None, ("thr1e-4", 0)),
    (2, "zero", (0.0, 1.0), 1e-2, None, ("thr1e-2", 1)),
    (3, "zero", (1e-2, 0.5), 1e-2, None, ("thr1e-2", 1)),
    (3, "colour", (0.0, 1.0), 0.0, None, ("thr1e-4", 0)),
    (0, "colour", (1e-2, 0.5), 0.0, 1, ("thr1e-4", 0)),
    (1, "zero", (0.0, 1.0), 1e-2, 1, ("thr1e-4", 0)),
    (2, "colour", (1e-2, 0.5), 1e-2, 5, ("thr1e-4", 0)),
    (3, "zero", (1e-2, 0.5), 0.0, 5, ("thr1e-4", 0)),
]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(inp):
    return [t.to(DEV).contiguous() for t in (inp.sig, inp.rgbs, inp.deltas, inp.ts, inp.rays_a, inp.gt)]


def _composite_loss(inp, dev, cfg, bg, n_rays, with_lists):
    """one ngp_composite_loss call into junk-filled outputs -> dict of CPU tensors"""
    S, C, Dl, Ts, RA, GT = dev
    nr, n = inp.n_rows, inp.n
    junk = lambda *s: torch.full(s, JUNK, device=DEV)  # noqa: E731
    o = dict(dsig=junk(n), drgb=junk(n, 3), rgb=junk(nr, 3), op=junk(nr), dep=junk(nr), loss=junk(nr))
    na = torch.full((nr,), -7, dtype=torch.int32, device=DEV) if with_lists else None
    sidx = torch.full((n,), -7, dtype=torch.int32, device=DEV) if with_lists else None
    ws = torch.zeros(2, dtype=torch.int64, device=DEV) if with_lists else None
    tot = torch.full((1,), -7, dtype=torch.int64, device=DEV) if with_lists else None
    stats = torch.zeros(32 * 16, dtype=torch.int64, device=DEV) if with_lists else None

    def call():
        vren._ok(vren.lib().ngp_composite_loss(
            _p(S), _p(C), _p(Dl), _p(Ts), _p(RA), n_rays, _p(GT), _p(bg), cfg.loss_type, cfg.lambda_opacity,
            cfg.lambda_depth, cfg.lambda_distortion, cfg.depth_scale, inp.T_thr, _p(o["dsig"]), _p(o["drgb"]),
            _p(o["rgb"]), _p(o["op"]), _p(o["dep"]), _p(o["loss"]), _p(na), _p(sidx), _p(ws), _p(tot), _p(stats),
            vren._stream()), "composite_loss")
        torch.cuda.synchronize()

    call()
    out = {k: v.cpu() for k, v in o.items()}
    if with_lists:
        out.update(n_active=na.cpu(), sample_idx=sidx.cpu(), alloc_ws=ws.cpu(), total=int(tot.item()), stats=stats.cpu())
        sidx.fill_(-7); tot.fill_(-7)
        call()  # the same workspace again, as the kernel left it
        out.update(sample_idx2=sidx.cpu(), alloc_ws2=ws.cpu(), total2=int(tot.item()), stats2=stats.cpu(),
                   again={k: v.cpu() for k, v in o.items()})
    return out


def _check_list(f, lst, total):
    """the sample list: a permutation of the expected set, each row's entries contiguous and ascending"""
    na = f.n_active
    assert total == int(na.sum())
    want = torch.cat([f.start[r] + torch.arange(int(na[r])) for r in range(na.numel())]) if total else torch.zeros(0)
    got = lst[:total].long()
    assert torch.equal(got.sort().values, want.long().sort().values)
    assert bool((lst[total:] == -7).all())
    pos = torch.full((f.n,), -1, dtype=torch.int64)
    pos[got] = torch.arange(total)
    for r in range(na.numel()):
        s, k = int(f.start[r]), int(na[r])
        if k:
            assert torch.equal(pos[s:s + k], pos[s] + torch.arange(k)), r


@pytest.mark.parametrize("loss_type,bgn,depth,lam_dist,n_rays,iset", CASES,
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_composite_loss_per_element(loss_type, bgn, depth, lam_dist, n_rays, iset):
    inp = CR.rows(*iset)
    r = CR.reference(iset[0], iset[1], loss_type, bgn, depth[0], depth[1], lam_dist, n_rays, "tree")
    f, cfg = r.f, CR.config(loss_type, 1e-3, depth[0], depth[1], lam_dist)
    nr = r.n_rays
    dev = _dev(inp)
    bg = CR.bg_tensor(bgn).to(DEV)
    out = _composite_loss(inp, dev, cfg, bg, nr, True)
    # ---- termination, exact on every row, indexed by ROW
    want_na = torch.full((inp.n_rows,), -7, dtype=torch.int32)
    want_na[:nr] = f.n_active.int()
    assert torch.equal(out["n_active"], want_na)
    # ---- per-ray outputs, indexed by RAY; rays of other rows keep the junk
    def by_ray(v, b):
        e = torch.full((inp.n_rows,) + tuple(v.shape[1:]), JUNK, dtype=torch.float64)
        bb = torch.zeros_like(e)
        e[f.ray], bb[f.ray] = v, b
        return e, bb
    ratios = {}
    for key, v, b in (("rgb", r.xc, r.b_xc), ("op", f.O, r.b_O), ("dep", f.D, r.b_D), ("loss", r.loss, r.b_loss)):
        e, bb = by_ray(v, b)
        ratios[key] = CR.ratio((out[key].double() - e).abs(), bb)
    # ---- gradients: every element of each row's first n_active samples; samples of other rows keep the junk
    act = CR.flat(f, f.m.double()) > 0
    other = ~(CR.flat(f, f.valid.double()) > 0)
    ratios["dsig"] = CR.ratio((out["dsig"].double() - CR.flat(f, r.dsig)).abs()[act], CR.flat(f, r.b_dsig)[act])
    ratios["drgbs"] = CR.ratio((out["drgb"].double() - CR.flat(f, r.drgbs)).abs()[act], CR.flat(f, r.b_drgbs)[act])
    assert bool((out["dsig"][other] == JUNK).all()) and bool((out["drgb"][other] == JUNK).all())
    print(f"composite_loss {loss_type} {bgn} {depth} {lam_dist} n_rays {nr} {iset[0]}: worst err / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1 for v in ratios.values()), ratios
    assert float(CR.flat(f, r.dsig).abs().max()) > 0
    # ---- the sample list, its total, the workspace, the counters
    _check_list(f, out["sample_idx"], out["total"])
    assert bool((out["alloc_ws"] == 0).all()) and bool((out["alloc_ws2"] == 0).all())
    _check_list(f, out["sample_idx2"], out["total2"])
    for k, v in out["again"].items():
        assert torch.equal(v, out[k]), k
    st = out["stats"].view(32, 16)
    assert st[:, :3].sum(0).tolist() == [int(f.N.sum()), int(f.count.sum()), int(f.n_active.sum())]
    assert int(st[:, 3:].abs().sum()) == 0 and torch.equal(out["stats2"], 2 * out["stats"])
    # ---- n_active, sample_idx and stats are optional
    bare = _composite_loss(inp, dev, cfg, bg, nr, False)
    for k in ("rgb", "op", "dep", "loss"):
        assert torch.equal(bare[k], out[k]), k
    assert torch.equal(bare["dsig"][act], out["dsig"][act]) and torch.equal(bare["drgb"][act], out["drgb"][act])


@pytest.mark.parametrize("iset", [("thr1e-4", 0), ("thr1e-2", 1)], ids=lambda v: v[0])
def test_composite_train_fw_bw_per_element(iset):
    """vren.composite_train_fw, then _bw fed the kernel's OWN outputs and four non-zero upstream gradients"""
    inp = CR.rows(*iset)
    S, C, Dl, Ts, RA, _ = _dev(inp)
    f = CR.composite_ref64(inp.sig, inp.rgbs, inp.deltas, inp.ts, inp.rays_a, inp.T_thr)
    g = torch.Generator().manual_seed(11)
    gop, gdep, grgb = (torch.randn(inp.n_rows, generator=g), torch.randn(inp.n_rows, generator=g),
                       torch.randn(inp.n_rows, 3, generator=g))
    gws = torch.randn(inp.n, generator=g)
    dsig, drgbs, b_sig, b_rgb, fb = CR.train_bw_ref64(f, "serial", gop, gdep, grgb, gws)
    tot, op, dep, rgb, ws = vren.composite_train_fw(S, C, Dl, Ts, RA, inp.T_thr)
    c = CR.C_PATH["serial"] * CR.SLACK
    assert torch.equal(tot.cpu()[f.ray], f.count)  # total_samples: exact on every row
    ratios = {
        "rgb": CR.ratio((rgb.cpu().double()[f.ray] - f.R).abs(), fb.dR * c),
        "op": CR.ratio((op.cpu().double()[f.ray] - f.O).abs(), fb.dO * c),
        "dep": CR.ratio((dep.cpu().double()[f.ray] - f.D).abs(), fb.dD * c),
        "ws": CR.ratio((ws.cpu().double() - CR.flat(f, f.w)).abs(), CR.flat(f, fb.dw * c)),  # (0 past the termination)
    }
    empty = f.ray[f.N == 0]
    assert empty.numel() > 0 and float(rgb.cpu()[empty].abs().max()) == 0 and float(op.cpu()[empty].abs().max()) == 0 \
        and float(dep.cpu()[empty].abs().max()) == 0 and int(tot.cpu()[empty].abs().max()) == 0
    D = lambda t: t.to(DEV)  # noqa: E731
    out = vren.composite_train_bw(D(gop), D(gdep), D(grgb), D(gws), S, C, ws, Dl, Ts, RA, op, dep, rgb, inp.T_thr)
    ratios["dsig"] = CR.ratio((out[0].cpu().double() - CR.flat(f, dsig)).abs(), CR.flat(f, b_sig))
    ratios["drgbs"] = CR.ratio((out[1].cpu().double() - CR.flat(f, drgbs)).abs(), CR.flat(f, b_rgb))
    past = ~(CR.flat(f, f.m.double()) > 0)
    assert int(past.sum()) > 1000
    assert float(ws.cpu()[past].abs().max()) == 0 and float(out[0].cpu()[past].abs().max()) == 0 \
        and float(out[1].cpu()[past].abs().max()) == 0
    print(f"composite_train_fw/bw {iset[0]}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1 for v in ratios.values()), ratios


@pytest.mark.parametrize("Ns", [1, 4, 8])
def test_composite_test_fw_per_element(Ns):
    t = CR.alive_rows(Ns, 3)
    ref = CR.alive_ref64(t)
    D = lambda x: x.to(DEV).contiguous()  # noqa: E731
    al, op, dep, rgb = D(t.alive.clone()), D(t.op0.clone()), D(t.dep0.clone()), D(t.rgb0.clone())
    vren.composite_test_fw(D(t.sig), D(t.rgbs), D(t.deltas), D(t.ts), None, al, t.T_thr, D(t.n_eff), op, dep, rgb)
    torch.cuda.synchronize()
    assert torch.equal(al.cpu(), ref.alive)  # exact: n_eff == 0 and terminated rays leave, no other
    # (a bound of 0 -- rays not listed, rays with n_eff == 0 -- means untouched)
    ratios = {"op": CR.ratio((op.cpu().double() - ref.op).abs(), ref.b_op),
              "dep": CR.ratio((dep.cpu().double() - ref.dep).abs(), ref.b_dep),
              "rgb": CR.ratio((rgb.cpu().double() - ref.rgb).abs(), ref.b_rgb)}
    print(f"composite_test_fw Ns {Ns}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1 for v in ratios.values()), ratios
    assert int((ref.b_op == 0).sum()) >= 700 and float((ref.op - t.op0.double()).abs().max()) > 0.1


# ------------------------------------------------------------------ NeRFLoss
def _loss_inputs(n=1500, scale=0.5):
    g = torch.Generator().manual_seed(13)
    rgb, gt = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    rgb[:6] = torch.tensor([[0.0, 1.0, 0.5], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 0.0, 1.0],
                            [0.0, 0.5, 1.0]])
    gt[:4] = torch.tensor([[0.0, 1.0, 1.0], [0.0, 1.0, 0.5], [1.0, 0.0, 0.5], [1.0, 0.0, 0.0]])
    op = torch.rand(n, generator=g)
    op[:4] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    v = torch.rand(n, generator=g) * 2.4
    v = torch.where((v - 1).abs() < 1e-3, v + 0.01, v)  # a margin from the clip, except the exact rows
    dep = (v * scale).float()
    dep[:3] = scale  # depth / scale + 1e-10 == 1.0f: the gradient passes
    dep[3], dep[4], dep[5] = 0.0, scale * 0.999, scale * 1.001
    return rgb, gt, op, dep


@pytest.mark.parametrize("lam_depth", [1e-2, 0.0])
@pytest.mark.parametrize("loss_set", ["raw", "log", "tanh"])
def test_nerf_loss_per_element(loss_set, lam_depth):
    from losses import NeRFLoss, _LOSS_TYPE
    scale = 0.5
    rgb, gt, op, dep = _loss_inputs(scale=scale)
    n = rgb.shape[0]
    g = torch.Generator().manual_seed(14)
    up = [torch.randn(n, 3, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)]
    for skip in (None, 1):  # a term no gradient flows into
        R, Op, Dp = (t.to(DEV).requires_grad_(True) for t in (rgb, op, dep))
        L = NeRFLoss(30, loss_set, scale, lam_depth, lambda_opacity=1e-3, lambda_distortion=0.0)
        d = L({"rgb": R, "opacity": Op, "depth": Dp}, {"rgb": gt.to(DEV)})
        assert type(d["rgb"].grad_fn).__name__.startswith("_NeRFLossFn")  # the fused path
        terms = [d["rgb"], d["opacity"], d["depth"]]
        tot = sum((t * u.to(DEV)).sum() for i, (t, u) in enumerate(zip(terms, up)) if i != skip)
        gr = torch.autograd.grad(tot, (R, Op, Dp))
        ups = [None if i == skip else u for i, u in enumerate(up)]
        ref = CR.nerf_loss_ref64(_LOSS_TYPE[loss_set], rgb, gt, op, dep, 1e-3, lam_depth, scale, *ups)
        ratios = {}
        for key, got in (("l_rgb", d["rgb"]), ("l_op", d["opacity"]), ("l_dep", d["depth"]), ("d_rgb", gr[0]),
                         ("d_op", gr[1]), ("d_dep", gr[2])):
            val, b = getattr(ref, key)
            ratios[key] = CR.ratio((got.detach().cpu().double() - val).abs(), b)
        print(f"NeRFLoss {loss_set} lambda_depth {lam_depth} skip {skip}: worst err / bound "
              + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        assert all(v <= 1 for v in ratios.values()), ratios
        if lam_depth and skip is None:
            assert bool(ref.clip_pass[:3].all()) and bool((gr[2][:3] != 0).all())       # at the clip: passes
            assert int((~ref.clip_pass).sum()) > 100 and bool((gr[2].cpu()[~ref.clip_pass] == 0).all())
        if skip == 1:
            assert float(gr[1].abs().max()) == 0
    # the entry point itself with a NULL upstream gradient (what a caller without that term passes)
    D = lambda t: t.to(DEV).contiguous()  # noqa: E731
    Rg, Gt, Op, Dp, Ur, Ud = D(rgb), D(gt), D(op), D(dep), D(up[0]), D(up[2])
    o3, o1, o2 = torch.full((n, 3), JUNK, device=DEV), torch.full((n,), JUNK, device=DEV), torch.full((n,), JUNK, device=DEV)
    vren._ok(vren.lib().ngp_nerf_loss_bw(_p(Rg), _p(Gt), _p(Op), _p(Dp), n, _LOSS_TYPE[loss_set], 1e-3, lam_depth, scale,
                                         _p(Ur), None, _p(Ud), _p(o3), _p(o1), _p(o2), vren._stream()), "nerf_loss_bw")
    torch.cuda.synchronize()
    assert float(o1.abs().max()) == 0 and torch.equal(o3, gr[0]) and torch.equal(o2, gr[2])


def _torch_terms(L, rgb, gt, op, dep):
    d = {"rgb": L.rgb_loss(rgb, gt) ** 2}
    o = op + 1e-10
    d["opacity"] = L.lambda_opacity * (-o * torch.log(o))
    d["depth"] = -L.lambda_depth * torch.log((dep / L.grid_scale + 1e-10).clip(max=1.0))
    return d


@pytest.mark.parametrize("case", ["gt_1x3", "gt_3", "opacity_nx1", "opacity_longer", "depth_shorter", "gt_n+1"])
def test_nerf_loss_shapes_the_fused_path_must_not_take(case, monkeypatch):
    """A broadcast gt, or an opacity / depth of another length, gives what the reference's torch expressions give on
    the same tensors (or raises as they raise) -- the fused kernels, which index every tensor by ray without looking
    at its shape, are not launched on them; opacity (n, 1) stays on the fused path and keeps its shape."""
    import losses
    from losses import NeRFLoss
    n = 257
    rgb, gt, op, dep = (t.to(DEV) for t in _loss_inputs(n))
    fused = case == "opacity_nx1"
    if case == "gt_1x3":
        gt = gt[:1].contiguous()
    elif case == "gt_3":
        gt = gt[0].contiguous()
    elif case == "opacity_nx1":
        op = op[:, None].contiguous()
    elif case == "opacity_longer":
        op = torch.cat([op, op[:5]])
    elif case == "depth_shorter":
        dep = dep[:n // 2].contiguous()
    elif case == "gt_n+1":
        gt = torch.cat([gt, gt[:1]])
    L = NeRFLoss(30, "raw", 0.5, 1e-2, lambda_opacity=1e-3, lambda_distortion=0.0)
    if not fused:
        def boom(*a, **k):
            raise AssertionError("the fused kernels were launched on tensors of mismatched shapes")
        monkeypatch.setattr(losses._NeRFLossFn, "apply", boom)
    if case == "gt_n+1":
        with pytest.raises(RuntimeError) as want:
            _torch_terms(L, rgb, gt, op, dep)
        with pytest.raises(RuntimeError) as got:
            L({"rgb": rgb, "opacity": op, "depth": dep}, {"rgb": gt})
        assert str(got.value) == str(want.value)
        return
    R = rgb.clone().requires_grad_(True)
    d = L({"rgb": R, "opacity": op, "depth": dep}, {"rgb": gt})
    ref = _torch_terms(L, rgb, gt, op, dep)
    for k in ("rgb", "opacity", "depth"):
        assert d[k].shape == ref[k].shape, k
        if fused:
            torch.testing.assert_close(d[k], ref[k], rtol=2e-6, atol=1e-9)
        else:
            assert torch.equal(d[k].detach(), ref[k]), k
    gr, = torch.autograd.grad(d["rgb"].sum(), R)
    R2 = rgb.clone().requires_grad_(True)
    gref, = torch.autograd.grad((L.rgb_loss(R2, gt) ** 2).sum(), R2)
    torch.testing.assert_close(gr, gref, rtol=2e-5, atol=1e-12)
