"""GPU parity of the fused hash-grid + MLP field (libngp_amd.so) against the
CPU oracle with tcnn semantics (oracle/oracle.py OracleNGPField).

* hash encoding: BIT-EXACT (same fmaf order, same fp16 rounding);
* sigma / rgb: the MLPs accumulate in a different order (MFMA vs CPU GEMM),
  so an fp16 layer output can flip by one ulp, and a flipped hidden unit
  moves the next layer's sums.  Bar, for EVERY point: |h - h_oracle| within
  oracle.mlp_forward_bound (one fp16 ulp at every storage point + fp32
  accumulation in any order, propagated through |W|), so |ln sigma -
  ln sigma_oracle| <= that bound on h0 (+ fp32 exp rounding) and rgb within
  sigmoid's 1/4 x the colour net's output bound + one fp16 ulp; rgb also
  within north_star's 1e-3.  The share of h0 within one fp16 ulp is
  reported (a single ulp per point cannot be guaranteed by any
  implementation whose summation order differs from the oracle's);
* gradients (fp16 MFMA backward with per-stage power-of-two scaling vs the
  oracle's fp32 autograd): relative L2 error <= 1e-2 per parameter group;
  against the oracle with the backward's fp16 gradient storage points
  modelled (oracle.rg16): <= 2e-3 per weight matrix and for the table.
"""
import pytest
import torch

import hashgrid as HG
import oracle as O
import synthetic as S
import vren

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _oracle_and_params(scale=0.5, table_init=1.0, seed=4):
    f = O.OracleNGPField(scale=scale, seed=seed, table_init=table_init)
    nd = f.n_dens
    flat = torch.cat([f.xyz_params.detach()[:nd], f.rgb_params.detach(), f.xyz_params.detach()[nd:]])
    return f, flat


def _points(n, scale, seed=0):
    sc = S.SyntheticScene(W=200, H=200, n_images=10, scale=scale)
    g = torch.Generator().manual_seed(seed)
    img, pix = sc.sample_batch(4096, g)
    o, d = sc.rays(img, pix)
    c = torch.zeros(1, 3); h = torch.ones(1, 3) * scale
    _, ht, _ = O.ray_aabb_intersect(o, d, c, h, 1)
    ht = ht[:, 0].contiguous()
    ht[(ht[:, 0] >= 0) & (ht[:, 0] < 0.01), 0] = 0.01
    noise = torch.rand(4096, generator=g)
    _, xyzs, dirs, _, _, _ = O.raymarching_train(o, d, ht, sc.bitfield, sc.cascades, scale,
                                                 0.0 if scale <= 0.5 else 1 / 256, noise, 128, 1024)
    xyzs, dirs = xyzs[:n], dirs[:n]
    # plus random points incl. the box faces / corners
    xr = (torch.rand(512, 3, generator=g) * 2 - 1) * scale
    xr[:8] = torch.tensor([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * scale
    dr = torch.randn(512, 3, generator=g)
    return torch.cat([xyzs, xr]).contiguous(), torch.cat([dirs, dr]).contiguous()


@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_hashgrid_levels_match_oracle(scale):
    g = HG.HashGrid(scale)
    spec = O.HashGridSpec(16, 19, 16, scale=scale)
    assert g.n_entries == spec.n_entries
    assert g.resolutions == spec.res.tolist()
    assert g.offsets == spec.offsets.tolist()


@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_split_encode_mlp_equals_fused(scale):
    """ngp_hash_encode (level pair per XCD, pair-major) + ngp_field_mlp_forward
    (the training path) give the fused ngp_field_forward's encoding, sigma
    and rgb bit for bit."""
    import ctypes
    _, flat = _oracle_and_params(scale=scale)
    x, d = _points(20000, scale)
    n = x.shape[0]
    grid = HG.HashGrid(scale)
    p16 = flat.to(DEV).half()
    x, d = x.to(DEV), d.to(DEV)
    sig, rgb, enc, _ = HG.field_forward(x, d, grid, p16)
    enc_pm = torch.empty(8, n, 4, dtype=torch.float16, device=DEV)
    sig2, rgb2 = torch.empty(n, device=DEV), torch.empty(n, 3, device=DEV)
    L = HG._lib()
    vp = ctypes.c_void_p
    vren._ok(L.ngp_hash_encode(vp(x.data_ptr()), n, None, None, ctypes.byref(grid.desc), vp(p16[HG.MLP_PARAMS:].data_ptr()),
                               vp(enc_pm.data_ptr()), vren._stream()), "hash_encode")
    vren._ok(L.ngp_field_mlp_forward(vp(enc_pm.data_ptr()), vp(d.data_ptr()), n, None, None, vp(p16.data_ptr()),
                                     vp(sig2.data_ptr()), vp(rgb2.data_ptr()), None, vren._stream()), "mlp_forward")
    assert torch.equal(enc_pm.permute(1, 0, 2).reshape(n, 32).view(torch.int16), enc.view(torch.int16))
    assert torch.equal(sig2, sig)
    assert torch.equal(rgb2, rgb)
    # density net only (occupancy updates): ngp_density_forward's sigmas
    sig3 = torch.empty(n, device=DEV)
    vren._ok(L.ngp_field_mlp_forward(vp(enc_pm.data_ptr()), None, n, None, None, vp(p16.data_ptr()),
                                     vp(sig3.data_ptr()), None, None, vren._stream()), "density_mlp")
    assert torch.equal(sig3, HG.density_forward(x, grid, p16)[0])
    # indexed: only the listed samples (rows = samples), the others untouched
    g = torch.Generator().manual_seed(1)
    sidx = torch.randperm(n, generator=g)[: n // 3].to(torch.int32).to(DEV)
    m = torch.tensor([sidx.numel()], dtype=torch.int64, device=DEV)
    enc_pm.fill_(7.0); sig2.fill_(-1.0); rgb2.fill_(-1.0)
    vren._ok(L.ngp_hash_encode(vp(x.data_ptr()), n, vp(m.data_ptr()), vp(sidx.data_ptr()), ctypes.byref(grid.desc),
                               vp(p16[HG.MLP_PARAMS:].data_ptr()), vp(enc_pm.data_ptr()), vren._stream()), "encode_ix")
    vren._ok(L.ngp_field_mlp_forward(vp(enc_pm.data_ptr()), vp(d.data_ptr()), n, vp(m.data_ptr()),
                                     vp(sidx.data_ptr()), vp(p16.data_ptr()), vp(sig2.data_ptr()), vp(rgb2.data_ptr()),
                                     None, vren._stream()), "mlp_ix")
    ix = sidx.long()
    rows = enc_pm.permute(1, 0, 2).reshape(n, 32)
    assert torch.equal(rows[ix].view(torch.int16), enc[ix].view(torch.int16))
    assert torch.equal(sig2[ix], sig[ix]) and torch.equal(rgb2[ix], rgb[ix])
    rest = torch.ones(n, dtype=torch.bool, device=DEV)
    rest[ix] = False
    assert bool((sig2[rest] == -1.0).all()) and bool((rows[rest] == 7.0).all())
    # encode + MLPs in one launch (ngp_field_encode_mlp, the trainer's forward): same values, listed rows only
    enc_pm.fill_(7.0); sig2.fill_(-1.0); rgb2.fill_(-1.0)
    vren._ok(L.ngp_field_encode_mlp(vp(x.data_ptr()), vp(d.data_ptr()), n, vp(m.data_ptr()), vp(sidx.data_ptr()),
                                    ctypes.byref(grid.desc), vp(p16[HG.MLP_PARAMS:].data_ptr()), vp(p16.data_ptr()),
                                    vp(enc_pm.data_ptr()), vp(sig2.data_ptr()), vp(rgb2.data_ptr()), None,
                                    vren._stream()), "encode_mlp_ix")
    rows = enc_pm.permute(1, 0, 2).reshape(n, 32)
    assert torch.equal(rows[ix].view(torch.int16), enc[ix].view(torch.int16))
    assert torch.equal(sig2[ix], sig[ix]) and torch.equal(rgb2[ix], rgb[ix])
    assert bool((sig2[rest] == -1.0).all()) and bool((rows[rest] == 7.0).all())
    # all rows, density net only
    sig3.fill_(-1.0)
    vren._ok(L.ngp_field_encode_mlp(vp(x.data_ptr()), None, n, None, None, ctypes.byref(grid.desc),
                                    vp(p16[HG.MLP_PARAMS:].data_ptr()), vp(p16.data_ptr()), vp(enc_pm.data_ptr()),
                                    vp(sig3.data_ptr()), None, None, vren._stream()), "encode_density")
    assert torch.equal(sig3, HG.density_forward(x, grid, p16)[0])


@pytest.mark.parametrize("shrink", [(), (7, 12)])
def test_encoding_outside_the_box_wraps_like_tcnn(shrink):
    """Inputs outside the grid's box (negative or past-the-end cell coordinates:
    the API takes arbitrary points) index every level modulo its size, as tcnn's
    grid_index does -- each forward kernel (fused field, split encode, the
    trainer's one-launch encode + MLPs) gives the oracle's encoding bit for bit,
    with no read outside the table.  shrink: hashed levels given a size that is
    no power of two (2^19 - 8, still a multiple of 8; offsets and table as they
    are), which only a hand-built descriptor can state: the generic modulo."""
    import ctypes
    f, flat = _oracle_and_params(0.5)
    g = torch.Generator().manual_seed(21)
    x = (torch.rand(8192, 3, generator=g) * 2 - 1) * 1.5  # up to 3x the box half-size, every octant
    x[:6] = torch.tensor([[-40.0, 0, 0], [0, 55.0, 0], [0, 0, -70.0], [1e3, -1e3, 1e3], [0.5, 0.5, 0.5],
                          [-0.5, -0.5, -0.5]])
    d = torch.randn(8192, 3, generator=g)
    n = x.shape[0]
    grid = HG.HashGrid(0.5)
    for l in shrink:
        grid.desc.sizes[l] = 2 ** 19 - 8
        f.spec.sizes[l] = 2 ** 19 - 8
    p16 = flat.to(DEV).half()
    xd, dd = x.to(DEV), d.to(DEV)
    enc_ref = O.hash_encode_fwd(f.spec, x, f.xyz_min, f.xyz_max, f.xyz_params.detach()[f.n_dens:])
    _, _, enc, _ = HG.field_forward(xd, dd, grid, p16)
    assert torch.equal(enc.cpu().view(torch.int16), enc_ref.view(torch.int16))
    L = HG._lib()
    vp = ctypes.c_void_p
    for fused in (False, True):
        enc_pm = torch.empty(8, n, 4, dtype=torch.float16, device=DEV)
        if fused:
            sig, rgb = torch.empty(n, device=DEV), torch.empty(n, 3, device=DEV)
            vren._ok(L.ngp_field_encode_mlp(vp(xd.data_ptr()), vp(dd.data_ptr()), n, None, None, ctypes.byref(grid.desc),
                                            vp(p16[HG.MLP_PARAMS:].data_ptr()), vp(p16.data_ptr()),
                                            vp(enc_pm.data_ptr()), vp(sig.data_ptr()), vp(rgb.data_ptr()), None,
                                            vren._stream()), "encode_mlp")
        else:
            vren._ok(L.ngp_hash_encode(vp(xd.data_ptr()), n, None, None, ctypes.byref(grid.desc),
                                       vp(p16[HG.MLP_PARAMS:].data_ptr()), vp(enc_pm.data_ptr()), vren._stream()),
                     "hash_encode")
        torch.cuda.synchronize()
        got = enc_pm.permute(1, 0, 2).reshape(n, 32).cpu()
        assert torch.equal(got.view(torch.int16), enc_ref.view(torch.int16)), fused


@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_field_forward_parity(scale):
    f, flat = _oracle_and_params(scale)
    x, d = _points(20000, scale)
    grid = HG.HashGrid(scale)
    p16 = flat.to(DEV).half()
    sig, rgb, enc, h = HG.field_forward(x.to(DEV), d.to(DEV), grid, p16, save_enc=True, want_h=True)
    # encoding: bit-exact
    table = f.xyz_params.detach()[f.n_dens:]
    enc_ref = O.hash_encode_fwd(f.spec, x, f.xyz_min, f.xyz_max, table)
    assert torch.equal(enc.cpu().view(torch.int16), enc_ref.view(torch.int16))
    with torch.no_grad():
        sig_ref, rgb_ref = f(x, d)
        h_ref = f.density_feat(x)
    hg = h.cpu().float()
    Wd, _ = O.mlp_layers(f.xyz_params.detach()[:f.n_dens], f.dens_dims)
    _, hb = O.mlp_forward_bound(enc_ref, Wd)
    dh = (hg - h_ref).abs()
    assert bool((dh <= hb).all()), float((dh / hb).max())
    one_ulp = float((dh[:, 0] <= O.ulp16(h_ref[:, 0])).float().mean())
    print(f"h0 within one fp16 ulp of the oracle: {one_ulp:.4%} of {dh.shape[0]} points; "
          f"max |dh0| / bound {float((dh[:, 0] / hb[:, 0]).max()):.3f}")
    assert one_ulp > 0.99
    dls = (torch.log(sig.cpu()) - torch.log(sig_ref)).abs()
    assert bool((dls <= hb[:, 0] + 4 * 2.0 ** -24).all())
    # colour net: input [SH (exact), h (bounded above)] -> logits bound -> sigmoid (1/4-Lipschitz) + fp16 ulp
    Wc, _ = O.mlp_layers(f.rgb_params.detach(), f.color_dims)
    cin = torch.cat([O.sh4(d).float(), h_ref], 1)
    _, lb = O.mlp_forward_bound(cin.half(), Wc, d_in=torch.cat([torch.zeros(cin.shape[0], 16), hb], 1))
    rb = 0.25 * lb[:, :3] + O.ulp16(rgb_ref)
    assert bool(((rgb.cpu() - rgb_ref).abs() <= rb).all())
    torch.testing.assert_close(rgb.cpu(), rgb_ref, atol=1e-3, rtol=0)
    # density-only kernel agrees with the full one
    sig2, h2 = HG.density_forward(x.to(DEV), grid, p16, want_h=True)
    assert torch.equal(sig2.cpu(), sig.cpu()) and torch.equal(h2.cpu(), h.cpu())


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("table_init", [1.0, 1e-4])
def test_field_backward_parity(table_init):
    f, flat = _oracle_and_params(0.5, table_init=table_init)
    x, d = _points(30000, 0.5, seed=1)
    g = torch.Generator().manual_seed(9)
    dsig = torch.randn(x.shape[0], generator=g) * 1e-3
    drgb = torch.randn(x.shape[0], 3, generator=g) * 1e-2
    sig_ref, rgb_ref = f(x, d)
    (sig_ref * dsig).sum().backward(retain_graph=True)
    (rgb_ref * drgb).sum().backward()
    nd = f.n_dens
    ref = torch.cat([f.xyz_params.grad[:nd], f.rgb_params.grad, f.xyz_params.grad[nd:]])
    grid = HG.HashGrid(0.5)
    p16 = flat.to(DEV).half()
    _, _, enc, _ = HG.field_forward(x.to(DEV), d.to(DEV), grid, p16)
    grad = torch.zeros(grid.n_params, device=DEV)
    HG.field_backward(x.to(DEV), d.to(DEV), grid, p16, enc, dsig.to(DEV), drgb.to(DEV), grad)
    gc = grad.cpu()
    for name, (o, od, idim) in HG.OW.items():
        sl = slice(o, o + od * idim)
        if name == "W5":  # only the 3 used output rows carry gradient
            sl = slice(o, o + 3 * idim)
            assert gc[o + 3 * idim:o + 16 * idim].abs().max() == 0
        assert _rel(gc[sl], ref[sl]) < 1e-2, name
    assert _rel(gc[HG.MLP_PARAMS:], ref[HG.MLP_PARAMS:]) < 1e-2
    # untouched table entries stay exactly zero
    assert torch.equal(gc[HG.MLP_PARAMS:] == 0, ref[HG.MLP_PARAMS:] == 0)


@pytest.mark.parametrize("table_init", [1.0, 1e-4])
def test_field_backward_matches_the_fp16_storage_model(table_init):
    """The same backward against the oracle with tcnn's fp16 gradient storage
    points modelled (OracleNGPField.grad16: each layer's pre-activation
    gradient rounded to fp16's 11 significant bits, oracle.rg16) instead of
    fp32 autograd throughout.  What remains is the kernel's fp32 summation
    order (MFMA tiles vs the CPU GEMM), the fp16 ulp flips of the forward
    recompute (the forward's own bound), and the weight gradients' block-common
    re-scale (a sample's fp16 G tile shifted down to the block's largest
    sample's exponent loses the bits below fp16's subnormal floor).  Bar: every
    weight matrix and the table within 2e-3 relative L2 (the fp32-autograd
    test above: 1e-2).  Measured (round 6, profiles/r06/r6ae_fp16_storage_model.log):
    table_init 1.0 -- W1-W4 and the table 0.85-1.25e-3 against the model
    (0.90-1.32e-3 against fp32 autograd), W5 2.7e-5 (2.1e-4); table_init 1e-4
    -- 1.1-3.7e-4 (2.6-4.8e-4), W5 1.6e-5 (9.7e-5)."""
    f, flat = _oracle_and_params(0.5, table_init=table_init)
    f.grad16 = True
    x, d = _points(30000, 0.5, seed=1)
    g = torch.Generator().manual_seed(9)
    dsig = torch.randn(x.shape[0], generator=g) * 1e-3
    drgb = torch.randn(x.shape[0], 3, generator=g) * 1e-2
    sig_ref, rgb_ref = f(x, d)
    (sig_ref * dsig).sum().backward(retain_graph=True)
    (rgb_ref * drgb).sum().backward()
    nd = f.n_dens
    ref = torch.cat([f.xyz_params.grad[:nd], f.rgb_params.grad, f.xyz_params.grad[nd:]])
    f.grad16 = False
    f.zero_grad()
    s32, r32 = f(x, d)
    (s32 * dsig).sum().backward(retain_graph=True)
    (r32 * drgb).sum().backward()
    ref32 = torch.cat([f.xyz_params.grad[:nd], f.rgb_params.grad, f.xyz_params.grad[nd:]])
    grid = HG.HashGrid(0.5)
    p16 = flat.to(DEV).half()
    _, _, enc, _ = HG.field_forward(x.to(DEV), d.to(DEV), grid, p16)
    grad = torch.zeros(grid.n_params, device=DEV)
    HG.field_backward(x.to(DEV), d.to(DEV), grid, p16, enc, dsig.to(DEV), drgb.to(DEV), grad)
    gc = grad.cpu()
    groups = []
    for name, (o, od, idim) in HG.OW.items():
        groups.append((name, slice(o, o + (3 if name == "W5" else od) * idim)))
    groups.append(("table", slice(HG.MLP_PARAMS, None)))
    worst = 0.0
    for name, sl in groups:
        e16, e32, m = _rel(gc[sl], ref[sl]), _rel(gc[sl], ref32[sl]), _rel(ref[sl], ref32[sl])
        print(f"{name}: vs fp16-storage model {e16:.2e}, vs fp32 autograd {e32:.2e} "
              f"(model vs fp32 autograd {m:.2e})")
        worst = max(worst, e16)
    assert worst < 2e-3, worst


def test_field_backward_per_sample_scales():
    """dL/denc per sample when the per-sample gradient magnitudes span nine
    decades (composited weights of a batch do): the MLP backward scales each
    sample's gradient column by its own power of two before the fp16 cast (at
    the chain's inputs; after each inner layer the exponent drops by the block's
    bound exponent of W^T, round 5), so small-gradient samples keep full
    precision beside large ones.  Oracle: fp32 autograd through the oracle's MLP
    from the same fp16 encoding; then the same with the backward's fp16
    gradient storage points modelled (oracle.rg16), where the product agrees to
    fp32 roundoff for the median sample (bars: median 1e-6, 99th percentile
    1e-4, 99.9 % of samples within 2e-3, per decade)."""
    f, flat = _oracle_and_params(0.5)
    x, d = _points(20000, 0.5, seed=3)
    g = torch.Generator().manual_seed(11)
    mag = 10.0 ** (torch.rand(x.shape[0], generator=g) * 9 - 7)  # 1e-7 .. 1e2 per sample
    dsig = torch.randn(x.shape[0], generator=g) * mag * 1e-2
    drgb = torch.randn(x.shape[0], 3, generator=g) * mag[:, None]
    grid = HG.HashGrid(0.5)
    p16 = flat.to(DEV).half()
    _, _, enc, _ = HG.field_forward(x.to(DEV), d.to(DEV), grid, p16)
    grad = torch.zeros(grid.n_params, device=DEV)
    denc = torch.empty(x.shape[0], 32, device=DEV)
    HG.field_backward(x.to(DEV), d.to(DEV), grid, p16, enc, dsig.to(DEV), drgb.to(DEV), grad, denc_ws=denc)
    e = enc.cpu().float().requires_grad_()
    nd = f.n_dens
    Wd, _ = O.mlp_layers(f.xyz_params.detach()[:nd], f.dens_dims)
    Wc, _ = O.mlp_layers(f.rgb_params.detach(), f.color_dims)
    h = O.mlp_forward(e, Wd)
    sig = O.TruncExpCPU.apply(h[:, 0])
    out = O.mlp_forward(torch.cat([O.sh4(d).float(), h], 1), Wc)
    rgb = O.rh(torch.sigmoid(out[:, :3]))
    ((sig * dsig).sum() + (rgb * drgb).sum()).backward()
    ref, got = e.grad, denc.cpu()
    assert bool(torch.isfinite(got).all())
    rn = ref.norm(dim=1)
    rel = (got - ref).norm(dim=1) / rn.clamp_min(1e-38)
    live = rn > 0
    frac = float((rel[live] <= 2e-2).float().mean())
    print(f"dL/denc per sample: {frac:.2%} of {int(live.sum())} samples within 2e-2 relative, "
          f"median {float(rel[live].median()):.1e}")
    assert frac >= 0.99
    # the smallest-gradient decade as well as the largest
    lo, hi = live & (mag < 1e-6), live & (mag > 10)
    assert float((rel[lo] <= 2e-2).float().mean()) >= 0.99 and float((rel[hi] <= 2e-2).float().mean()) >= 0.99
    # against the fp16 gradient-storage model (oracle.rg16): the per-sample scales make the product's
    # rounding the model's in every decade
    e16 = enc.cpu().float().requires_grad_()
    h16 = O.mlp_forward(e16, Wd, grad16=True)
    out16 = O.mlp_forward(torch.cat([O.sh4(d).float(), h16], 1), Wc, grad16=True)
    ((O.TruncExpCPU.apply(h16[:, 0]) * dsig).sum() + (O.rh(torch.sigmoid(out16[:, :3])) * drgb).sum()).backward()
    rel16 = (got - e16.grad).norm(dim=1) / e16.grad.norm(dim=1).clamp_min(1e-38)
    # (measured, profiles/r06/r6ak_pytest_per_sample.log: median 9.7e-8 -- fp32 roundoff --, 99th percentile
    # 1.2e-5, 99.98 % within 2e-3; the same in the smallest and the largest decade)
    for name, m in (("all", live), ("mag < 1e-6", lo), ("mag > 10", hi)):
        r = rel16[m]
        print(f"dL/denc vs the fp16-storage model, {name}: median {float(r.median()):.1e}, "
              f"99th percentile {float(r.quantile(0.99)):.1e}, within 2e-3 {float((r <= 2e-3).float().mean()):.2%}")
        assert float(r.median()) <= 1e-6 and float(r.quantile(0.99)) <= 1e-4, name
        assert float((r <= 2e-3).float().mean()) >= 0.999, name


def test_field_autograd_function():
    f, flat = _oracle_and_params(0.5)
    x, d = _points(5000, 0.5, seed=2)
    grid = HG.HashGrid(0.5)
    params = torch.nn.Parameter(flat.to(DEV))
    shadow = HG.FP16Shadow(params)
    sig, rgb = HG.field(x.to(DEV), d.to(DEV), params, grid, shadow)
    (sig.sum() * 1e-3 + rgb.sum()).backward()
    assert params.grad is not None and torch.isfinite(params.grad).all()
    assert params.grad[:HG.MLP_PARAMS].abs().sum() > 0


def _ray_points(n_rays, per_ray, scale, seed):
    """samples along rays, consecutive per ray (a march's layout): runs of
    equal corner pairs on the coarse levels"""
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(n_rays, 3, generator=g) * 2 - 1) * scale * 0.9
    d = torch.randn(n_rays, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    t = torch.arange(per_ray).float() * (3 ** 0.5 / 1024) * scale * 2
    x = (o[:, None] + t[None, :, None] * d[:, None]).clamp(-scale, scale).reshape(-1, 3)
    return x.contiguous()


@pytest.mark.parametrize("scale", [0.5, 16.0])
@pytest.mark.parametrize("level_cap,level_lo,merge_hi,rays", [(1 << 20, 0, 0, False), (3000, 0, 0, False),
                                                             (1 << 20, 8, 8, False), (1 << 20, 0, 12, True),
                                                             (3000, 0, 16, True), (1 << 20, 4, 12, True)])
def test_hash_backward_binned_matches_atomic(scale, level_cap, level_lo, merge_hi, rays):
    """ngp_hash_backward_binned (records + LDS range sums) == ngp_hash_backward
    (per-sample atomics) up to fp32 summation order, through a sample_idx
    subset, onto a non-zero gradient (+= contract).  max_samples=3000 sends
    most tiles through the overflow path (direct atomics); level_lo=8 bins the
    fine levels only, the coarse ones going through ngp_hash_backward_levels;
    merge_hi > level_lo merges runs of equal corner pairs on samples laid out
    along rays (rays=True, where runs exist)."""
    x = _ray_points(400, 100, scale, seed=3) if rays else _points(40000, scale, seed=3)[0]
    n = x.shape[0]
    grid = HG.HashGrid(scale)
    g = torch.Generator().manual_seed(5)
    sidx = torch.randperm(n, generator=g)[: n * 3 // 4].sort().values.to(torch.int32)
    m = sidx.numel()
    denc = (torch.randn(m, 32, generator=g) * 1e-2).to(DEV)
    x, sidx = x.to(DEV), sidx.to(DEV)
    n_dev = torch.tensor([m], dtype=torch.int64, device=DEV)
    base = torch.randn(grid.n_entries * 2, generator=g).to(DEV)
    L = HG._lib()
    p = lambda t: vren.c_void_p(t.data_ptr())  # noqa: E731
    ref = base.clone()
    vren._ok(L.ngp_hash_backward(p(x), n, p(n_dev), p(sidx), HG.ctypes.byref(grid.desc), p(denc), p(ref),
                                 vren._stream()), "hash_backward")
    ws = torch.empty((L.ngp_hash_backward_binned_workspace(level_cap) + 255) // 256, 64, dtype=torch.int32,
                     device=DEV)
    out = base.clone()
    for _ in range(2):  # the workspace is reusable: counters reset per call
        out.copy_(base)
        vren._ok(L.ngp_hash_backward_binned(p(x), n, p(n_dev), p(sidx), HG.ctypes.byref(grid.desc), p(denc), p(out),
                                            p(ws), level_cap, level_lo, merge_hi, vren._stream()), "hash_backward_binned")
        vren._ok(L.ngp_hash_backward_levels(p(x), n, p(n_dev), p(sidx), HG.ctypes.byref(grid.desc), p(denc), p(out),
                                            0, level_lo, vren._stream()), "hash_backward_levels")
    torch.cuda.synchronize()
    d_ref, d_out = (ref - base).cpu().double(), (out - base).cpu().double()
    assert float(d_ref.abs().max()) > 0
    assert _rel(d_out, d_ref) < 5e-5  # product order (1-fx)*((wy*wz)*g) vs ((wx*wy)*wz)*g + sum order
    # rtol: a coarse entry sums thousands of terms in another order
    torch.testing.assert_close(out.cpu(), ref.cpu(), rtol=1e-4, atol=1e-6 * float(d_ref.abs().max()))


def test_forward_first_with_preencoded_coarse_levels_is_bit_identical():
    """ngp_field_encode_first_coarse (levels 0-7 of the first chunks, ahead of
    time) + ngp_field_forward_first_pre(pre_levels = 8) == ngp_field_forward_first:
    the encoding, sigma, rgb, round-2 counts and evaluated count bit for bit;
    the pre-encode touches only pairs 0-3 of the first-chunk samples."""
    import ctypes
    _, flat = _oracle_and_params(scale=0.5)
    x, d = _points(20000, 0.5)
    n = x.shape[0]
    grid = HG.HashGrid(0.5)
    p16 = flat.to(DEV).half()
    x, d = x.to(DEV), d.to(DEV)
    g = torch.Generator().manual_seed(7)
    R = 400
    N = torch.randint(1, 150, (R,), generator=g)
    N[torch.rand(R, generator=g) < 0.4] = 0
    while int(N.sum()) > n:
        N = N // 2
    start = torch.cumsum(N, 0) - N
    rays_a = torch.stack([torch.arange(R), start, N], 1).to(DEV)
    deltas = ((torch.rand(n, generator=g) + 0.5) * 1e-2).to(DEV)
    L, Lv = HG._lib(), vren.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    rows = torch.empty(R, dtype=torch.int32, device=DEV)
    n_ne = torch.zeros(1, dtype=torch.int64, device=DEV)
    vren._ok(Lv.ngp_rays_nonempty(vp(rays_a), R, vp(rows), vp(n_ne), None, None, vren._stream()), "nonempty")
    first = torch.cat([torch.arange(int(s), int(s) + min(int(k), 64)) for s, k in zip(start, N)]).to(DEV)
    outs = []
    for pre in (0, 8):
        enc_pm = torch.full((8, n, 4), 7.0, dtype=torch.float16, device=DEV)
        sig, rgb = torch.full((n,), -1.0, device=DEV), torch.full((n, 3), -1.0, device=DEV)
        rest = torch.full((R,), -9, dtype=torch.int32, device=DEV)
        ev = torch.zeros(1, dtype=torch.int64, device=DEV)
        if pre:
            vren._ok(L.ngp_field_encode_first_coarse(vp(x), vp(rays_a), vp(rows), vp(n_ne), R, n,
                                                     ctypes.byref(grid.desc), vp(p16[HG.MLP_PARAMS:]), vp(enc_pm),
                                                     vren._stream()), "encode_first_coarse")
            torch.cuda.synchronize()
            rows_enc = enc_pm.permute(1, 0, 2).reshape(n, 32)
            touched = torch.zeros(n, dtype=torch.bool, device=DEV)
            touched[first] = True
            assert bool((rows_enc[~touched] == 7.0).all()) and bool((rows_enc[touched][:, 16:] == 7.0).all())
        vren._ok(L.ngp_field_forward_first_pre(vp(x), vp(d), vp(deltas), vp(rays_a), vp(rows), vp(n_ne), R, n,
                                               ctypes.c_float(1e-4), ctypes.byref(grid.desc), vp(p16[HG.MLP_PARAMS:]),
                                               vp(p16), vp(enc_pm), vp(sig), vp(rgb), vp(rest), None, None, vp(ev),
                                               pre, vren._stream()), "forward_first_pre")
        torch.cuda.synchronize()
        outs.append((enc_pm.clone(), sig.clone(), rgb.clone(), rest.clone(), int(ev)))
    (e0, s0, r0, c0, v0), (e1, s1, r1, c1, v1) = outs
    assert torch.equal(e0.view(torch.int16), e1.view(torch.int16))
    assert torch.equal(s0, s1) and torch.equal(r0, r1) and torch.equal(c0, c1) and v0 == v1 == first.numel()
    assert L.ngp_field_forward_first_pre(vp(x), vp(d), vp(deltas), vp(rays_a), vp(rows), vp(n_ne), R, n,
                                         ctypes.c_float(1e-4), ctypes.byref(grid.desc), vp(p16[HG.MLP_PARAMS:]),
                                         vp(p16), vp(enc_pm), vp(sig), vp(rgb), vp(rest), None, None, vp(ev), 4,
                                         vren._stream()) == -1


@pytest.mark.parametrize("layout", ["rays", "scattered"])
def test_coarse_scatter_matches_oracle(layout):
    """ngp_hash_backward_levels(_rep) over levels 0-7 (runs merged per wave,
    memory-side atomics per run head; levels 0-3 into 8 replicas in the _rep
    form) against the oracle's hash backward (oracle.hash_encode_bwd, tcnn's
    scatter restated in C) on the same samples: rel-L2 per level <= 1e-5
    (fp32 summation order only); "scattered": no runs to merge; the replicated
    call leaves its replicas zero and nothing outside levels 0-7 is touched."""
    if layout == "rays":
        x = _ray_points(600, 120, 0.5, seed=11)
    else:  # marched samples in random order: no two consecutive ones on one ray
        x = _points(60000, 0.5, seed=11)[0]
        x = x[torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(12))].contiguous()
    n = x.shape[0]
    grid = HG.HashGrid(0.5)
    g = torch.Generator().manual_seed(13)
    sidx = torch.randperm(n, generator=g)[: n * 3 // 4].sort().values.to(torch.int32)
    m = sidx.numel()
    denc = torch.randn(m, 32, generator=g) * 1e-2
    denc[:, 16:] = 0  # levels 8-15 are not scattered here
    spec = O.HashGridSpec(scale=0.5)
    ref = O.hash_encode_bwd(spec, x[sidx.long()], -0.5 * torch.ones(3), 0.5 * torch.ones(3), denc).double()
    L = HG._lib()
    p = lambda t: vren.c_void_p(t.data_ptr())  # noqa: E731
    desc = HG.ctypes.byref(grid.desc)
    xd, sd, dd = x.to(DEV), sidx.to(DEV), denc.to(DEV)
    n_dev = torch.tensor([m], dtype=torch.int64, device=DEV)
    rep = torch.zeros(L.ngp_hash_backward_rep_floats(desc, 4, 8), device=DEV)
    for replicated in (False, True):
        out = torch.zeros(grid.n_entries * 2, device=DEV)
        if replicated:
            vren._ok(L.ngp_hash_backward_levels_rep(p(xd), n, p(n_dev), p(sd), desc, p(dd), p(out), 0, 8,
                                                    p(rep), 4, 8, 1, vren._stream()), "levels_rep")
        else:
            vren._ok(L.ngp_hash_backward_levels(p(xd), n, p(n_dev), p(sd), desc, p(dd), p(out), 0, 8,
                                                vren._stream()), "levels")
        torch.cuda.synchronize()
        assert float(rep.abs().max()) == 0.0
        got = out.cpu().double()
        for lv in range(8):
            a, b = 2 * int(grid.offsets[lv]), 2 * int(grid.offsets[lv + 1])
            assert float(ref[a:b].abs().max()) > 0
            assert _rel(got[a:b], ref[a:b]) < 1e-5, (replicated, lv, _rel(got[a:b], ref[a:b]))
        assert float(got[2 * int(grid.offsets[8]):].abs().max()) == 0.0  # nothing outside levels 0-7


@pytest.mark.parametrize("rep_levels,n_rep", [(4, 8), (8, 16), (2, 1)])
def test_hash_backward_levels_replicated(rep_levels, n_rep):
    """ngp_hash_backward_levels_rep (levels < rep_levels into n_rep replicas,
    folded afterwards) == ngp_hash_backward_levels up to fp32 summation order,
    onto a non-zero gradient (+= contract); the replicas are left zero, so a
    second call gives the same result."""
    x = _ray_points(400, 100, 0.5, seed=7)
    n = x.shape[0]
    grid = HG.HashGrid(0.5)
    g = torch.Generator().manual_seed(9)
    sidx = torch.randperm(n, generator=g)[: n * 3 // 4].sort().values.to(torch.int32)
    m = sidx.numel()
    denc = (torch.randn(m, 32, generator=g) * 1e-2).to(DEV)
    x, sidx = x.to(DEV), sidx.to(DEV)
    n_dev = torch.tensor([m], dtype=torch.int64, device=DEV)
    base = torch.randn(grid.n_entries * 2, generator=g).to(DEV)
    L = HG._lib()
    p = lambda t: vren.c_void_p(t.data_ptr())  # noqa: E731
    desc = HG.ctypes.byref(grid.desc)
    ref = base.clone()
    vren._ok(L.ngp_hash_backward_levels(p(x), n, p(n_dev), p(sidx), desc, p(denc), p(ref), 0, 8, vren._stream()),
             "hash_backward_levels")
    rep = torch.zeros(L.ngp_hash_backward_rep_floats(desc, rep_levels, n_rep), device=DEV)
    assert rep.numel() == n_rep * 2 * grid.offsets[rep_levels]
    for _ in range(2):
        out = base.clone()
        vren._ok(L.ngp_hash_backward_levels_rep(p(x), n, p(n_dev), p(sidx), desc, p(denc), p(out), 0, 8, p(rep),
                                                rep_levels, n_rep, 1, vren._stream()), "hash_backward_levels_rep")
        torch.cuda.synchronize()
        assert float(rep.abs().max()) == 0.0
        d_ref, d_out = (ref - base).cpu().double(), (out - base).cpu().double()
        assert float(d_ref[: 2 * grid.offsets[rep_levels]].abs().max()) > 0
        assert _rel(d_out, d_ref) < 1e-5
        torch.testing.assert_close(out.cpu(), ref.cpu(), rtol=1e-4, atol=1e-6 * float(d_ref.abs().max()))
    # argument checks: replicas beyond the atomic levels, replica count bounds
    assert L.ngp_hash_backward_levels_rep(p(x), n, p(n_dev), p(sidx), desc, p(denc), p(out), 0, 8, p(rep), 9, 8, 1,
                                          vren._stream()) < 0
    assert L.ngp_hash_backward_levels_rep(p(x), n, p(n_dev), p(sidx), desc, p(denc), p(out), 0, 8, p(rep), 4, 0, 1,
                                          vren._stream()) < 0


@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_forward_first_chunk_matches_encode_mlp_and_chunk_counts(scale):
    """ngp_field_forward_first (the row forward's round 1: a wave per row, its
    first min(N, 64) samples, the row's transmittance in the epilogue): the
    evaluated samples' encoding / sigma / rgb bit-identical to
    ngp_field_encode_mlp, no other sample touched; rest = the counts
    ngp_chunk_counts_range(first 64) gives from the full forward's sigmas; and
    with ngp_rays_nonempty's row list, the appended round-2 list holds exactly
    ngp_ray_segments' samples (each row's run contiguous and ascending)."""
    import ctypes
    _, flat = _oracle_and_params(scale=scale)
    x, d = _points(20000, scale)
    n = x.shape[0]
    grid = HG.HashGrid(scale)
    p16 = flat.to(DEV).half()
    x, d = x.to(DEV), d.to(DEV)
    sig, rgb, enc, _ = HG.field_forward(x, d, grid, p16)
    g = torch.Generator().manual_seed(5)
    R = 400
    N = torch.randint(1, 200, (R,), generator=g)
    N[torch.rand(R, generator=g) < 0.5] = 0
    N[3], N[4] = 64, 65  # chunk-boundary rows
    while int(N.sum()) > n:
        N = N // 2
    start = torch.cumsum(N, 0) - N
    rays_a = torch.stack([torch.arange(R), start, N], 1).to(DEV)
    row = torch.repeat_interleave(torch.arange(R), N)
    scale_row = torch.where(torch.rand(R, generator=g) < 0.5, 1.0, 1e-6)  # terminating vs transparent rows
    deltas = torch.zeros(n)
    deltas[:row.numel()] = (torch.rand(row.numel(), generator=g) + 0.5) * scale_row[row]
    deltas = deltas.to(DEV)
    L, Lv = HG._lib(), vren.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    cnt_ref = torch.empty(R, dtype=torch.int32, device=DEV)
    vren._ok(Lv.ngp_chunk_counts_range(vp(rays_a), R, 64, 0, vp(sig), vp(deltas), ctypes.c_float(1e-4), vp(cnt_ref),
                                       vren._stream()), "counts")
    first = torch.cat([torch.arange(int(s), int(s) + min(int(k), 64)) for s, k in zip(start, N)]).to(DEV)
    # 1) every row (rows NULL), counts out
    enc_pm = torch.full((8, n, 4), 7.0, dtype=torch.float16, device=DEV)
    sig2, rgb2 = torch.full((n,), -1.0, device=DEV), torch.full((n, 3), -1.0, device=DEV)
    rest = torch.full((R,), -9, dtype=torch.int32, device=DEV)
    ev = torch.zeros(1, dtype=torch.int64, device=DEV)
    vren._ok(L.ngp_field_forward_first(vp(x), vp(d), vp(deltas), vp(rays_a), None, None, R, n, ctypes.c_float(1e-4),
                                       ctypes.byref(grid.desc), vp(p16[HG.MLP_PARAMS:]), vp(p16), vp(enc_pm), vp(sig2),
                                       vp(rgb2), vp(rest), None, None, vp(ev), vren._stream()), "forward_first")
    torch.cuda.synchronize()
    rows_enc = enc_pm.permute(1, 0, 2).reshape(n, 32)
    assert torch.equal(rows_enc[first].view(torch.int16), enc[first].view(torch.int16))
    assert torch.equal(sig2[first], sig[first]) and torch.equal(rgb2[first], rgb[first])
    untouched = torch.ones(n, dtype=torch.bool, device=DEV)
    untouched[first] = False
    assert bool((sig2[untouched] == -1.0).all()) and bool((rows_enc[untouched] == 7.0).all())
    assert torch.equal(rest, cnt_ref) and int(ev) == first.numel()
    assert 0 < int((cnt_ref > 0).sum()) < int((N > 64).sum())  # some long rows stop, some go on
    # 2) the non-empty row list, round-2 list appended
    rows = torch.empty(R, dtype=torch.int32, device=DEV)
    n_ne, total2 = torch.zeros(1, dtype=torch.int64, device=DEV), torch.full((1,), 3, dtype=torch.int64, device=DEV)
    vren._ok(Lv.ngp_rays_nonempty(vp(rays_a), R, vp(rows), vp(n_ne), None, vp(total2), vren._stream()), "nonempty")
    list2 = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ev.zero_()
    vren._ok(L.ngp_field_forward_first(vp(x), vp(d), vp(deltas), vp(rays_a), vp(rows), vp(n_ne), R, n,
                                       ctypes.c_float(1e-4), ctypes.byref(grid.desc), vp(p16[HG.MLP_PARAMS:]), vp(p16),
                                       vp(enc_pm), vp(sig2), vp(rgb2), None, vp(list2), vp(total2), vp(ev),
                                       vren._stream()), "forward_first_list")
    st = torch.empty(R, dtype=torch.int64, device=DEV)
    tot_ref, idx_ref = torch.zeros(1, dtype=torch.int64, device=DEV), torch.full((n,), -1, dtype=torch.int32, device=DEV)
    vren._ok(Lv.ngp_ray_segments(vp(cnt_ref), vp(rays_a), R, 64, vp(st), vp(tot_ref), None, vp(idx_ref),
                                 vren._stream()), "segments")
    torch.cuda.synchronize()
    T = int(tot_ref)
    assert int(total2) == T and int(ev) == first.numel() + T
    got = list2[:T].long()
    assert torch.equal(torch.sort(got)[0], torch.sort(idx_ref[:T].long())[0])
    # runs of a row are contiguous and ascending: every step inside the list is +1 or a jump to another row's start
    steps = got[1:] - got[:-1]
    assert int((steps == 1).sum()) == T - int((cnt_ref > 0).sum())


def test_sparse_field_backward_matches_the_dense_one():
    """The drop-in autograd backward (HG.field_backward_sparse: the rows with a
    nonzero upstream gradient listed on the device, then the MLP backward and
    the hybrid atomic / binned hash backward over them) against field_backward
    over every row, with 70 % of the rows exactly zero as past a ray's
    termination: per weight matrix and for the table within 2e-3 relative L2
    (fp32 summation order and the MLP backward's per-block fp16 scales, which
    depend on which samples share a block), and against the oracle's autograd
    within the dense test's 1e-2."""
    f, flat = _oracle_and_params(0.5, table_init=1.0)
    x, d = _points(30000, 0.5, seed=3)
    g = torch.Generator().manual_seed(5)
    keep = (torch.rand(x.shape[0], generator=g) < 0.3).float()
    dsig = torch.randn(x.shape[0], generator=g) * 1e-3 * keep
    drgb = torch.randn(x.shape[0], 3, generator=g) * 1e-2 * keep[:, None]
    sig_ref, rgb_ref = f(x, d)
    (sig_ref * dsig).sum().backward(retain_graph=True)
    (rgb_ref * drgb).sum().backward()
    nd = f.n_dens
    ref = torch.cat([f.xyz_params.grad[:nd], f.rgb_params.grad, f.xyz_params.grad[nd:]])
    grid = HG.HashGrid(0.5)
    p16 = flat.to(DEV).half()
    xd, dd = x.to(DEV), d.to(DEV)
    _, _, enc, _ = HG.field_forward(xd, dd, grid, p16)
    dense = torch.zeros(grid.n_params, device=DEV)
    HG.field_backward(xd, dd, grid, p16, enc, dsig.to(DEV), drgb.to(DEV), dense)
    sparse = torch.zeros(grid.n_params, device=DEV)
    HG.field_backward_sparse(xd, dd, grid, p16, enc, dsig.to(DEV), drgb.to(DEV), sparse)
    ds, sp = dense.cpu(), sparse.cpu()
    for name, (o, od, idim) in HG.OW.items():
        sl = slice(o, o + (3 if name == "W5" else od) * idim)
        assert _rel(sp[sl], ds[sl]) < 2e-3, name
        assert _rel(sp[sl], ref[sl]) < 1e-2, name
    assert _rel(sp[HG.MLP_PARAMS:], ds[HG.MLP_PARAMS:]) < 2e-3
    assert _rel(sp[HG.MLP_PARAMS:], ref[HG.MLP_PARAMS:]) < 1e-2
    assert torch.equal(sp[HG.MLP_PARAMS:] == 0, ds[HG.MLP_PARAMS:] == 0)
    # the list holds exactly the nonzero rows
    idx = torch.empty(x.shape[0], dtype=torch.int32, device=DEV)
    cnt = torch.empty(1, dtype=torch.int64, device=DEV)
    import vren
    dsd, drd = dsig.to(DEV).contiguous(), drgb.to(DEV).contiguous()  # (held: the launch reads them later)
    vren._ok(vren.lib().ngp_gradient_rows(HG._ptr(dsd), HG._ptr(drd), x.shape[0], HG._ptr(idx), HG._ptr(cnt),
                                          vren._stream()), "gradient_rows")
    n = int(cnt)
    nz = torch.nonzero((dsig != 0) | (drgb != 0).any(1))[:, 0]
    assert n == nz.numel() and torch.equal(torch.sort(idx[:n].cpu().long())[0], nz)
