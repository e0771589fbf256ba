"""Raw-HDR colour modes on the GPU (NGP_RGB_* of include/ngp_amd.h; the
reference's NGP(rgb_act='None', use_raw_HDR=True), networks.py:68-78, 152-157)
through every layer: the _act entry points against the oracle composition of
tests/hdr_ref.py, the modes against each other bit for bit, the backward at
the existing sigmoid tests' bars, the autograd surface, the device-resident
renderer and probes, and the trainer (one step against the oracle, the forward
paths against each other, and a short training run on 4x ground truth).

The input sets are hdr_ref.CASES (test_hdr_cpu.py shows that the
sign-ambiguous set A = {|o_ref| <= d} is below 5 % on each).  Inside A the
branch of leaky_relu / relu is taken from the device's own forward; outside it
the device's sign must be the oracle's.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import hashgrid as HG
import hdr_ref as H
import oracle as O
import vren

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = [c[0] for c in H.CASES]
BIG = [c[0] for c in H.CASES if c[4] is None]
TAIL = 21  # rows between the device count and the capacity (NaN inputs; outputs must keep their bits)
MODES = {"none": H.NONE, "leaky_relu": H.LEAKY_RELU, "relu": H.RELU}


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _padded(t, fill=float("nan")):
    """t with TAIL more rows of `fill` (the rows past the device count)."""
    pad = torch.full((TAIL,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    return torch.cat([t, pad]).contiguous().to(DEV)


_dev_cache = {}


def _dev(name):
    """The case on the device: capacity n + TAIL, NaN rows past the count n."""
    if name not in _dev_cache:
        c = H.case(name)
        n = c["x"].shape[0]
        _dev_cache[name] = dict(c=c, n=n, cap=n + TAIL, grid=HG.HashGrid(c["scale"]), p16=c["flat"].to(DEV).half(),
                                x=_padded(c["x"]), d=_padded(c["d"]),
                                n_dev=torch.tensor([n], dtype=torch.int64, device=DEV))
    return _dev_cache[name]


def _field_forward(D, act, old_symbol=False):
    """ngp_field_forward_act (or the old symbol) over the count n of capacity
    cap -> sig, rgb, enc (n,32), h; the rows past n must keep their NaN bits."""
    cap, n, grid, p16 = D["cap"], D["n"], D["grid"], D["p16"]
    sig, rgb = torch.full((cap,), float("nan"), device=DEV), torch.full((cap, 3), float("nan"), device=DEV)
    enc = torch.full((cap, 32), float("nan"), dtype=torch.float16, device=DEV)
    h = torch.full((cap, 16), float("nan"), dtype=torch.float16, device=DEV)
    args = [vp(D["x"]), vp(D["d"]), cap, vp(D["n_dev"]), ctypes.byref(grid.desc), vp(p16[HG.MLP_PARAMS:]), vp(p16),
            vp(sig), vp(rgb), vp(enc), vp(h)]
    L = HG._lib()
    if old_symbol:
        vren._ok(L.ngp_field_forward(*args, vren._stream()), "field_forward")
    else:
        vren._ok(L.ngp_field_forward_act(*args, act, vren._stream()), "field_forward_act")
    torch.cuda.synchronize()
    for t in (sig, rgb, enc.float(), h.float()):
        assert bool(torch.isnan(t[n:]).all()) and bool(torch.isfinite(t[:n]).all())
    assert _same_bits(sig[n:], torch.full((TAIL,), float("nan"), device=DEV))
    assert _same_bits(rgb[n:], torch.full((TAIL, 3), float("nan"), device=DEV))
    return sig[:n], rgb[:n], enc[:n], h[:n]


def _encode_mlp(D, act, old_symbol=False):
    """ngp_field_encode_mlp_act over the count n -> sig, rgb, enc (n,32) from the pair-major planes, h."""
    cap, n, grid, p16 = D["cap"], D["n"], D["grid"], D["p16"]
    sig, rgb = torch.full((cap,), float("nan"), device=DEV), torch.full((cap, 3), float("nan"), device=DEV)
    enc_pm = torch.full((8, cap, 4), float("nan"), dtype=torch.float16, device=DEV)
    h = torch.full((cap, 16), float("nan"), dtype=torch.float16, device=DEV)
    args = [vp(D["x"]), vp(D["d"]), cap, vp(D["n_dev"]), None, ctypes.byref(grid.desc), vp(p16[HG.MLP_PARAMS:]), vp(p16),
            vp(enc_pm), vp(sig), vp(rgb), vp(h)]
    L = HG._lib()
    if old_symbol:
        vren._ok(L.ngp_field_encode_mlp(*args, vren._stream()), "field_encode_mlp")
    else:
        vren._ok(L.ngp_field_encode_mlp_act(*args, act, vren._stream()), "field_encode_mlp_act")
    torch.cuda.synchronize()
    rows = enc_pm.permute(1, 0, 2).reshape(cap, 32)
    for t in (sig, rgb, rows.float(), h.float()):
        assert bool(torch.isnan(t[n:]).all()) and bool(torch.isfinite(t[:n]).all())
    assert _same_bits(rgb[n:], torch.full((TAIL, 3), float("nan"), device=DEV))
    return sig[:n], rgb[:n], rows[:n].contiguous(), h[:n]


def _forward_first(D, act):
    """ngp_field_forward_first_pre_act on a small rays_a covering the n samples
    in rows of at most 47 (every sample is in a first chunk) -> sig, rgb."""
    cap, n, grid, p16 = D["cap"], D["n"], D["grid"], D["p16"]
    N = torch.full(((n + 46) // 47,), 47, dtype=torch.int64)
    N[-1] = n - 47 * (N.numel() - 1)
    start = torch.cumsum(N, 0) - N
    R = N.numel()
    rays_a = torch.stack([torch.arange(R), start, N], 1).contiguous().to(DEV)
    deltas = torch.full((cap,), 1e-3, device=DEV)
    sig, rgb = torch.full((cap,), float("nan"), device=DEV), torch.full((cap, 3), float("nan"), device=DEV)
    rest = torch.full((R,), -9, dtype=torch.int32, device=DEV)
    vren._ok(HG._lib().ngp_field_forward_first_pre_act(
        vp(D["x"]), vp(D["d"]), vp(deltas), vp(rays_a), None, None, R, cap, ctypes.c_float(1e-4),
        ctypes.byref(grid.desc), vp(p16[HG.MLP_PARAMS:]), vp(p16), None, vp(sig), vp(rgb), vp(rest), None, None, None, 0,
        act, vren._stream()), "field_forward_first_pre_act")
    torch.cuda.synchronize()
    assert bool(torch.isnan(rgb[n:]).all()) and bool((rest == 0).all())  # (no row longer than its first chunk)
    return sig[:n], rgb[:n]


# ------------------------------------------------------------ 1. NONE vs oracle
@pytest.mark.parametrize("name", ALL)
def test_raw_colour_is_within_the_oracles_bound(name):
    """NGP_RGB_NONE through ngp_field_forward_act and ngp_field_encode_mlp_act:
    every channel within d + ulp16(|o_ref| + d) of the oracle's raw output;
    sigmas, enc and h bit-equal to the sigmoid call's."""
    D = _dev(name)
    c = D["c"]
    tol = c["bound"] + O.ulp16(c["o_ref"].abs() + c["bound"])
    s0, _, e0, h0 = _field_forward(D, H.SIGMOID, old_symbol=True)
    for fn in (_field_forward, _encode_mlp):
        sig, rgb, enc, h = fn(D, H.NONE)
        err = (rgb.cpu() - c["o_ref"]).abs()
        print(f"{name} {fn.__name__}: worst |rgb - o_ref| / bound {float((err / tol).max()):.3f} over {err.numel()} "
              f"channels, max |o| {float(rgb.abs().max()):.2f}")
        assert bool((err <= tol).all())
        assert _same_bits(sig, s0)
        assert torch.equal(enc.view(torch.int16), e0.view(torch.int16)) and torch.equal(h.view(torch.int16),
                                                                                         h0.view(torch.int16))
    assert torch.equal(e0.cpu().view(torch.int16), c["enc_ref"].view(torch.int16))  # (the encoding: the oracle's bits)


# -------------------------------------------- 2. the other modes vs NONE, bit for bit
@pytest.mark.parametrize("name", ALL)
def test_modes_are_functions_of_the_raw_output_bit_for_bit(name):
    D = _dev(name)
    _, raw, _, _ = _field_forward(D, H.NONE)
    o16 = raw.half()
    assert torch.equal(o16.float(), raw)  # the raw colour is an fp16 value
    _, old_sig, _, _ = _field_forward(D, H.SIGMOID, old_symbol=True)
    _, old_sig2, _, _ = _encode_mlp(D, H.SIGMOID, old_symbol=True)
    want = {
        H.SIGMOID: old_sig,
        H.NONE: raw,
        H.LEAKY_RELU: torch.where(o16 > 0, o16, (o16.float() * 0.01).half()).float(),
        H.RELU: torch.relu(o16).float(),
    }
    assert torch.equal(want[H.LEAKY_RELU], F.leaky_relu(o16).float())  # torch's own evaluation on the device
    assert _same_bits(want[H.LEAKY_RELU], F.leaky_relu(o16).float())
    assert _same_bits(old_sig, old_sig2)
    if raw.numel() > 300:
        assert bool((raw < 0).any()) and bool((raw > 0).any())  # both branches are exercised
    for act, ref in want.items():
        outs = []
        for fn in (_field_forward, _encode_mlp, _forward_first):
            out = fn(D, act)
            outs.append(out)
            assert torch.equal(out[1], ref), (act, fn.__name__)
            if act != H.RELU:  # (relu(-0) keeps the sign in torch; the mode's `o > 0 ? o : 0` gives +0)
                assert _same_bits(out[1], ref), (act, fn.__name__)
        # the three kernels agree with each other bit for bit, sigma and colour
        for k in (0, 1):
            assert _same_bits(outs[0][k], outs[1][k]) and _same_bits(outs[0][k], outs[2][k]), (act, k)


# ------------------------------------------------------------ 3. backward
def _grads(n, seed, spread):
    g = torch.Generator().manual_seed(seed)
    if spread:  # nine decades of per-sample magnitude (test_field_backward_per_sample_scales)
        mag = 10.0 ** (torch.rand(n, generator=g) * 9 - 7)
        return torch.randn(n, generator=g) * mag * 1e-2, torch.randn(n, 3, generator=g) * mag[:, None], mag
    return torch.randn(n, generator=g) * 1e-3, torch.randn(n, 3, generator=g) * 1e-2, None


def _device_mask(D, mode):
    """The branch mask from the device's own forward; equal to the oracle's outside A."""
    c = D["c"]
    _, rgb, enc, _ = _field_forward(D, mode)
    _, raw, _, _ = _field_forward(D, H.NONE)
    mask = (raw > 0).cpu()
    if mode != H.NONE:
        assert torch.equal(rgb > 0, raw > 0)  # the sign survives leaky_relu / relu
    outside = ~c["A"]
    assert torch.equal(mask[outside], (c["o_ref"] > 0)[outside])
    return mask, enc


def _groups():
    gs = [(name, slice(o, o + (3 if name == "W5" else od) * idim)) for name, (o, od, idim) in HG.OW.items()]
    return gs + [("table", slice(HG.MLP_PARAMS, None))]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ALL)
def test_backward_matches_the_fp16_storage_model(name, mode):
    """ngp_field_backward_act (device count, NaN rows past it) and
    field_backward_sparse(rgb_act=) against hdr_ref with grad16=True and the
    mask of the device's forward: every weight matrix and the table within
    2e-3 relative L2 (test_field_backward_matches_the_fp16_storage_model's bar;
    measured values: DESIGN.md "Raw-HDR colour modes")."""
    act = MODES[mode]
    D = _dev(name)
    c, n, cap, grid, p16 = D["c"], D["n"], D["cap"], D["grid"], D["p16"]
    mask, enc = _device_mask(D, act)
    print(f"{name} {mode}: |A| = {int(c['A'].sum())} of {c['A'].numel()} channels")
    dsig, drgb, _ = _grads(n, 9, False)
    f = c["f"]
    f.zero_grad()
    sig_ref, rgb_ref, _ = H.forward(f, c["x"], c["d"], act, mask=mask, grad16=True)
    ((sig_ref * dsig).sum() + (rgb_ref * drgb).sum()).backward()
    nd = f.n_dens
    ref = torch.cat([f.xyz_params.grad[:nd], f.rgb_params.grad, f.xyz_params.grad[nd:]]).clone()
    f.zero_grad()
    # a) the fused entry point over the device count; the rows past it hold NaN everywhere
    enc_cap = torch.full((cap, 32), float("nan"), dtype=torch.float16, device=DEV)
    enc_cap[:n] = enc
    ds, dr = _padded(dsig), _padded(drgb)
    grad = torch.zeros(grid.n_params, device=DEV)
    denc = torch.full((cap, 32), float("nan"), device=DEV)
    vren._ok(HG._lib().ngp_field_backward_act(vp(D["x"]), vp(D["d"]), cap, vp(D["n_dev"]), ctypes.byref(grid.desc),
                                              vp(enc_cap), vp(p16), vp(ds), vp(dr), vp(denc), vp(grad),
                                              vp(grad[HG.MLP_PARAMS:]), act, vren._stream()), "field_backward_act")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()) and bool(torch.isnan(denc[n:]).all())  # nothing from / to the rows past n
    # b) the same without the tail rows: they contribute exactly nothing (fp32 atomic order apart)
    exact = torch.zeros(grid.n_params, device=DEV)
    HG.field_backward(D["x"][:n].contiguous(), D["d"][:n].contiguous(), grid, p16, enc.contiguous(), ds[:n].contiguous(),
                      dr[:n].contiguous(), exact, rgb_act=act)
    # c) the sparse backward (backward_mlp_act over the nonzero rows + both hash paths)
    sparse = torch.zeros(grid.n_params, device=DEV)
    HG.field_backward_sparse(D["x"][:n].contiguous(), D["d"][:n].contiguous(), grid, p16, enc.contiguous(),
                             ds[:n].contiguous(), dr[:n].contiguous(), sparse, rgb_act=act)
    torch.cuda.synchronize()
    gc, ge, gs = grad.cpu(), exact.cpu(), sparse.cpu()
    for gname, sl in _groups():
        if float(ref[sl].norm()) == 0:
            assert float(gc[sl].abs().max()) == 0 and float(gs[sl].abs().max()) == 0
            continue
        e1, e2, e3 = _rel(gc[sl], ref[sl]), _rel(gs[sl], ref[sl]), _rel(gc[sl], ge[sl])
        print(f"  {gname}: backward_act {e1:.2e}, sparse {e2:.2e} vs the fp16-storage model; tail rows {e3:.1e}")
        assert e1 < 2e-3 and e2 < 2e-3, (gname, e1, e2)
        assert e3 < 1e-5, (gname, e3)
    o5 = HG.OW["W5"][0]
    assert float(gc[o5 + 3 * 64:o5 + 16 * 64].abs().max()) == 0  # W5's padding rows carry nothing
    assert torch.equal(gc[HG.MLP_PARAMS:] == 0, ref[HG.MLP_PARAMS:] == 0)  # untouched entries stay exactly zero


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", BIG)
def test_backward_per_sample_gradients_over_nine_decades(name, mode):
    """dL/denc per sample with per-sample gradient magnitudes over nine decades,
    against the fp16-storage model from the device's encoding (as
    test_field_backward_per_sample_scales): over the set, median <= 1e-6, 99th
    percentile <= 1e-4 relative and 99.9 % of the samples within 2e-3.  The
    smallest and the largest decade hold ~150 of the 1512 samples each, so
    their 99th percentile would be their second-largest value -- a statement
    about single samples, for which that test's bar is the 2e-3 one: per
    decade the median bar and every sample within 2e-3.  (Measured: one sample
    of 147 at 1.2e-4 in `table 1e-2, relu, mag > 10`, the set's 99th percentile
    there 5.8e-7; a forward-recompute fp16 ulp flip, as in the sigmoid test.)"""
    act = MODES[mode]
    D = _dev(name)
    c, n, grid, p16 = D["c"], D["n"], D["grid"], D["p16"]
    mask, enc = _device_mask(D, act)
    dsig, drgb, mag = _grads(n, 11, True)
    grad = torch.zeros(grid.n_params, device=DEV)
    denc = torch.empty(n, 32, device=DEV)
    HG.field_backward(D["x"][:n].contiguous(), D["d"][:n].contiguous(), grid, p16, enc.contiguous(), dsig.to(DEV),
                      drgb.to(DEV), grad, denc_ws=denc, rgb_act=act)
    f = c["f"]
    Wd, _ = O.mlp_layers(f.xyz_params.detach()[:f.n_dens], f.dens_dims)
    Wc, _ = O.mlp_layers(f.rgb_params.detach(), f.color_dims)
    e16 = enc.cpu().float().requires_grad_()
    h16 = O.mlp_forward(e16, Wd, grad16=True)
    out16 = O.mlp_forward(torch.cat([O.sh4(c["d"]).float(), h16], 1), Wc, grad16=True)[:, :3]
    ((O.TruncExpCPU.apply(h16[:, 0]) * dsig).sum() + (H.activate(out16, act, mask) * drgb).sum()).backward()
    got = denc.cpu()
    assert bool(torch.isfinite(got).all())
    rn = e16.grad.norm(dim=1)
    live = rn > 0
    rel16 = (got - e16.grad).norm(dim=1) / rn.clamp_min(1e-38)
    for label, m in (("all", live), ("mag < 1e-6", live & (mag < 1e-6)), ("mag > 10", live & (mag > 10))):
        r = rel16[m]
        print(f"{name} {mode} dL/denc vs the fp16-storage model, {label} ({int(m.sum())}): median "
              f"{float(r.median()):.1e}, 99th percentile {float(r.quantile(0.99)):.1e}")
        assert float(r.median()) <= 1e-6, label
        if label == "all":
            assert float(r.quantile(0.99)) <= 1e-4 and float((r <= 2e-3).float().mean()) >= 0.999
        else:
            assert float(r.max()) <= 2e-3, (label, float(r.max()))


@pytest.mark.parametrize("mode", list(MODES))
def test_backward_mlp_rows_outside_sample_idx_contribute_nothing(mode):
    """ngp_field_backward_mlp_act over a sample_idx subset with NaN gradients
    in every unlisted row == the same with zeros there (up to fp32 atomic
    order), and the listed rows' dL/denc bit for bit."""
    act = MODES[mode]
    D = _dev("marched+random s0.5")
    n, grid, p16 = D["n"], D["grid"], D["p16"]
    _, enc = _device_mask(D, act)
    dsig, drgb, _ = _grads(n, 9, False)
    g = torch.Generator().manual_seed(5)
    sidx = torch.randperm(n, generator=g)[: n * 3 // 4].sort().values
    m = sidx.numel()
    listed = torch.zeros(n, dtype=torch.bool)
    listed[sidx] = True
    cnt = torch.tensor([m], dtype=torch.int64, device=DEV)
    sd = torch.cat([sidx.to(torch.int32), torch.full((n - m,), -1, dtype=torch.int32)]).to(DEV)  # (capacity n)
    outs = []
    for fill in (0.0, float("nan")):
        ds, dr = dsig.clone(), drgb.clone()
        ds[~listed] = fill
        dr[~listed] = fill
        ds, dr = ds.to(DEV), dr.to(DEV)
        gm = torch.zeros(HG.MLP_PARAMS, device=DEV)
        denc = torch.full((n, 32), 7.0, device=DEV)
        vren._ok(HG._lib().ngp_field_backward_mlp_act(vp(D["d"]), n, vp(cnt), vp(sd), vp(enc.contiguous()), 0, vp(p16),
                                                      vp(ds), vp(dr), vp(denc), vp(gm), act, vren._stream()), "bwd_mlp_act")
        torch.cuda.synchronize()
        outs.append((gm.cpu(), denc.cpu()))
    (g0, d0), (g1, d1) = outs
    assert bool(torch.isfinite(g1).all()) and float(g0.abs().max()) > 0
    assert _rel(g1, g0) < 1e-5
    assert torch.equal(d0[:m], d1[:m]) and bool((d1[m:] == 7.0).all())  # compact rows j < count only


# ------------------------------------------------------------ 4. autograd surface
@pytest.mark.parametrize("radiance", [False, True])
def test_ngp_forward_under_grad_and_without(radiance):
    from models.networks import NGP
    m = NGP(0.5, 'None', True).to(DEV)
    c = H.case("table 1e-2 s0.5")
    with torch.no_grad():
        m.params.copy_(c["flat"].to(DEV))
    x, d = c["x"].to(DEV), c["d"].to(DEV)
    n = x.shape[0]
    dsig, drgb, _ = _grads(n, 9, False)
    dsig, drgb = dsig.to(DEV), drgb.to(DEV)
    kw = dict(output_radiance=True) if radiance else {}
    sig, rgb = m(x, d, exposure=None, **kw)
    ((sig * dsig).sum() + (rgb * drgb).sum()).backward()
    act = HG.RGB_RELU if radiance else HG.RGB_LEAKY_RELU
    p16 = m._shadow.get()
    s2, r2, enc, _ = HG.field_forward(x, d, m.grid, p16, rgb_act=act)
    direct = torch.zeros_like(m.params)
    HG.field_backward_sparse(x, d, m.grid, p16, enc, dsig, drgb, direct, rgb_act=act)
    assert float(direct.abs().max()) > 0
    assert _rel(m.params.grad, direct) < 1e-5  # (fp32 atomic summation order only)
    with torch.no_grad():
        s3, r3 = m(x, d, **kw)
    assert _same_bits(s3, sig.detach()) and _same_bits(r3, rgb.detach()) and _same_bits(r3, r2)
    assert float(r3.min()) == 0.0 if radiance else float(r3.min()) < 0
    # a sigmoid model ignores the flag
    ms = NGP(0.5).to(DEV)
    with torch.no_grad():
        assert _same_bits(ms(x, d)[1], ms(x, d, output_radiance=True)[1])


# ------------------------------------------------------------ 5. renderer
def _hdr_scene_model(seed=5, occ_frac=0.02):
    """An HDR NGP with a seeded table and a ~2 % random bitfield (scripts/probe_bench.py's scene)."""
    from models.networks import NGP
    m = NGP(0.5, 'None', True)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.params[HG.MLP_PARAMS:].uniform_(-1, 1, generator=g)
        bits = (torch.rand(m.density_bitfield.numel() * 8, generator=g) < occ_frac).to(torch.uint8)
        m.density_bitfield.copy_((bits.view(-1, 8) << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8))
    return m.to(DEV)


@pytest.fixture(scope="module")
def hdr_model():
    return _hdr_scene_model()


def _rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = ((torch.rand(n, 3, generator=g) - 0.5) * 0.8).to(DEV)
    d = torch.randn(n, 3, generator=g)
    return o.contiguous(), (d / d.norm(dim=1, keepdim=True)).to(DEV).contiguous()


def test_render_device_loop_equals_host_loop_in_both_modes(hdr_model):
    from models.rendering import render
    o, d = _rays(4096, 3)
    frames = {}
    for radiance in (False, True, False):  # F, T, F on one model: a stale cached graph would repeat a frame
        with torch.no_grad():
            dev = render(hdr_model, o, d, test_time=True, output_radiance=radiance)
            dev = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in dev.items()}
            host = render(hdr_model, o, d, test_time=True, output_radiance=radiance, device_loop=False)
        for k in ("rgb", "opacity", "depth"):
            assert torch.equal(dev[k], host[k]), (radiance, k)
        assert int(dev["total_samples"]) == int(host["total_samples"])
        if radiance in frames:
            assert torch.equal(frames[radiance]["rgb"], dev["rgb"]) and torch.equal(frames[radiance]["opacity"], dev["opacity"])
        frames[radiance] = dev
    Ff, Tf = frames[False], frames[True]
    assert torch.equal(Ff["opacity"], Tf["opacity"]) and torch.equal(Ff["depth"], Tf["depth"])  # sigma has no mode
    differ = (Ff["rgb"] != Tf["rgb"]).any(1)
    print(f"{int(differ.sum())} of 4096 rays composite a negative raw colour")
    assert int(differ.sum()) >= 1
    assert float(Tf["rgb"].min()) >= 0
    # relu >= leaky_relu sample by sample, composited with non-negative weights
    assert bool((Tf["rgb"] >= Ff["rgb"]).all())
    assert len(hdr_model._test_renderers) == 2  # one renderer (captured graphs) per mode


def test_sh_probes_output_radiance_equals_render(hdr_model):
    import probes
    from models.rendering import render
    P, R, B = 3, 65, 64
    g = torch.Generator().manual_seed(21)
    pts = ((torch.rand(P, 3, generator=g) - 0.5) * 0.8).to(DEV)
    dirs = probes.get_sphere_rays(P, R, generator=g, device=DEV)
    res = probes.sh_probes(hdr_model, pts, dirs, output_radiance=True, return_rays=True)
    res = {k: v.clone() for k, v in res.items()}
    idx = [min(i, P - 1) for i in range(B)]  # the batch is filled up with the last probe
    o = pts[idx][:, None].expand(B, R, 3).reshape(-1, 3).contiguous()
    d = dirs[idx].reshape(-1, 3).contiguous()
    with torch.no_grad():
        out = render(hdr_model, o, d, test_time=True, output_radiance=True)
        leaky = render(hdr_model, o, d, test_time=True)
    assert torch.equal(res["rgb"], out["rgb"].view(B, R, 3)[:P]) and torch.equal(res["opacity"], out["opacity"].view(B, R)[:P])
    assert float(res["rgb"].min()) >= 0 and not torch.equal(out["rgb"], leaky["rgb"])
    assert res["rgb_sh"].shape == (P, 9, 3) and bool(torch.isfinite(res["rgb_sh"]).all())
    with pytest.raises(TypeError):
        probes.sh_probes(hdr_model, pts, dirs, radiance=True)


# ------------------------------------------------------------ 6.-8. trainer
def _hdr_setup(**kw):
    from test_trainer_gpu import _setup
    return _setup(use_raw_HDR=True, **kw)


def test_hdr_training_step_matches_oracle():
    """test_training_step_matches_oracle's shape and bars with
    NGPTrainer(use_raw_HDR=True), ground truth 4 gt, and the oracle trainer's
    field forward replaced by hdr_ref (leaky_relu, mask from the device)."""
    sc, tr, img, pix, noise = _hdr_setup(chunk_first=0)
    assert tr.rgb_act == HG.RGB_LEAKY_RELU
    dirs, poses = sc.directions.to(DEV), sc.poses.to(DEV)
    o, d = sc.rays(img, pix)
    gt = 4 * sc.gt_rgb_rays(o, d)
    p0 = tr.params.detach().cpu().clone()
    loss = tr.step(img.to(DEV), pix.to(DEV), gt.to(DEV), dirs, poses, noise=noise.to(DEV), apply_adam=False)
    torch.cuda.synchronize()
    rays_o, rays_d, hits_t = tr.rays_o.cpu(), tr.rays_d.cpu(), tr.hits_t.cpu()
    n = int(tr.n_samples.item())
    mask = (tr.rgbs[:n] > 0).cpu()  # (chunk_first = 0: every marched sample is written)
    assert bool(mask.any()) and bool((~mask).any())
    g_gpu = tr.grad.cpu()
    for grad16, bar in ((False, 1e-3), (True, 5e-4)):
        ot = O.OracleTrainer(p0, 0.5, tr.density_bitfield.cpu(), 1)
        ot.field.grad16 = grad16
        ot.field.forward = lambda x, dd, f=ot.field, g16=grad16: H.forward(f, x, dd, H.LEAKY_RELU, mask=mask,
                                                                           grad16=g16)[:2]
        l_ref, n_ref = ot.step(rays_o, rays_d, hits_t, gt, noise, torch.ones(3), apply_adam=False)
        assert n == n_ref and torch.equal(tr.rays_a.cpu(), ot.last["rays_a"])
        if not grad16:
            l_gpu = float(loss.sum())
            print(f"loss {l_gpu:.6e} vs the oracle's {l_ref:.6e}, relative {abs(l_gpu - l_ref) / abs(l_ref):.2e}; "
                  f"rgb max |diff| {float((tr.out_rgb.cpu() - ot.last['rgb']).abs().max()):.2e}, opacity "
                  f"{float((tr.out_op.cpu() - ot.last['opacity']).abs().max()):.2e}")
            assert abs(l_gpu - l_ref) <= 1e-5 * abs(l_ref)
            torch.testing.assert_close(tr.out_rgb.cpu(), ot.last["rgb"], atol=1e-5, rtol=0)
            torch.testing.assert_close(tr.out_op.cpu(), ot.last["opacity"], atol=1e-5, rtol=0)
        g_ref = ot.flat_grad()
        rels = []
        for lo, hi in ((0, 3072), (3072, 10240), (10240, g_ref.numel())):
            rels.append(float((g_gpu[lo:hi] - g_ref[lo:hi]).norm() / g_ref[lo:hi].norm()))
        print(f"gradients vs {'the fp16-storage model' if grad16 else 'fp32 autograd'}: " +
              " / ".join(f"{r:.1e}" for r in rels))
        assert max(rels) < bar, (grad16, rels)


@pytest.mark.parametrize("table_init", [0.2, 2.0])
def test_hdr_trainer_forward_paths_agree(table_init):
    """Full forward, two chunked rounds and the row forward of an HDR trainer:
    loss / out_rgb / out_op bit-identical, gradients within 1e-5 relative L2,
    a second step repeats the first (test_chunked_forward_matches_full,
    test_row_forward_matches_two_rounds_and_full)."""
    runs = []
    for chunk, rows in ((0, 0), (64, 0), (64, 1)):
        sc, tr, img, pix, noise = _hdr_setup(table_init=table_init)
        tr.chunk_first, tr.row_forward = chunk, rows
        dirs, poses = sc.directions.to(DEV), sc.poses.to(DEV)
        o, d = sc.rays(img, pix)
        gt = (4 * sc.gt_rgb_rays(o, d)).to(DEV)
        loss = tr.step(img.to(DEV), pix.to(DEV), gt, dirs, poses, noise=noise.to(DEV), apply_adam=False)
        torch.cuda.synchronize()
        out = (loss.clone(), tr.out_rgb.clone(), tr.out_op.clone(), tr.grad.clone())
        tr.grad.zero_()
        loss2 = tr.step(img.to(DEV), pix.to(DEV), gt, dirs, poses, noise=noise.to(DEV), apply_adam=False)
        torch.cuda.synchronize()
        assert torch.equal(loss2, out[0]) and torch.equal(tr.out_rgb, out[1]) and torch.equal(tr.out_op, out[2])
        n = int(tr.n_samples.item())
        if chunk == 0:
            assert bool((tr.rgbs[:n] < 0).any())  # the leaky branch is taken in this step
        runs.append(out)
    for other in runs[1:]:
        assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1]) and torch.equal(runs[0][2], other[2])
        assert float((other[3] - runs[0][3]).norm() / runs[0][3].norm()) < 1e-5


def test_hdr_training_converges_above_one():
    """300 graph-replayed steps of 4096 rays on 4x the analytic scene's colours
    (fp32 ground truth, loss 'log'): finite losses, the last 20 below half the
    first 20; the radiance render afterwards is non-negative and exceeds 1."""
    import synthetic as S
    from trainer import NGPTrainer
    sc = S.AnalyticScene(W=200, H=200, n_images=10)
    dirs, poses = sc.directions.to(DEV), sc.poses.to(DEV)
    gt = (sc.gt_images(device=DEV).float() / 255 * 4).contiguous()
    assert float(gt.max()) > 1
    tr = NGPTrainer(scale=0.5, batch_size=4096, device=DEV, seed=3, loss="log", use_raw_HDR=True)
    losses = [float(tr.train_step(gt, dirs, poses).sum()) for _ in range(300)]
    tr.drain()
    assert all(torch.isfinite(torch.tensor(losses)))
    first, last = sum(losses[:20]) / 20, sum(losses[-20:]) / 20
    print(f"HDR training: mean loss of the first 20 steps {first:.4f}, of the last 20 {last:.4f}")
    assert last < 0.5 * first
    g = torch.Generator().manual_seed(2)
    img, pix = sc.sample_batch(1024, g)
    o, d = sc.rays(img, pix)
    out = tr.render(o.to(DEV).contiguous(), d.to(DEV).contiguous(), output_radiance=True)
    leaky = tr.render(o.to(DEV).contiguous(), d.to(DEV).contiguous())
    print(f"radiance render: min {float(out['rgb'].min()):.3f}, max {float(out['rgb'].max()):.3f}")
    assert float(out["rgb"].min()) >= 0 and float(out["rgb"].max()) > 1
    assert bool((out["rgb"] >= leaky["rgb"]).all())


# ------------------------------------------------------------ scripts/train_scene.py --use_raw_HDR
def _train_scene_module():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_scene", os.path.join(root, "scripts", "train_scene.py"))
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    return ts


def test_train_scene_use_raw_hdr_end_to_end(tmp_path, monkeypatch):
    """test_nsvf_scene_trains_to_a_useful_psnr's scene and criterion through
    --use_raw_HDR (HDR trainer, evaluated with output_radiance=True, no clamp);
    a dataset that holds 8-bit pixels only is refused with a clear message."""
    import synthetic as S
    root = tmp_path / "Synthetic_Test" / "Sphere"
    S.write_nsvf_scene(str(root), res=100, n_train=24, n_test=2)
    ts = _train_scene_module()
    res = ts.main(["--dataset", "nsvf", "--root", str(root), "--downsample", "0.125", "--steps", "1500",
                   "--use_raw_HDR"])
    assert res["use_raw_HDR"] is True and res["test_views"] == 2
    assert res["test_psnr"] > 22.0, res
    import datasets

    class U8Only:
        def __init__(self, root, split="train", downsample=1.0):
            self.rays = torch.zeros(2, 16, 3, dtype=torch.uint8)

    monkeypatch.setitem(datasets.dataset_dict, "u8only", U8Only)
    with pytest.raises(SystemExit, match="fp32"):
        ts.main(["--dataset", "u8only", "--root", str(root), "--use_raw_HDR"])
