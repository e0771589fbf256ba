"""Input gradients of the field down to rays and poses (csrc/inputgrad.hip:
ngp_field_input_grad, ngp_ray_segment_sum; hashgrid._FieldFn, RayMarcher.backward,
pose_refine.PoseRefiner) against the fp64 restatement tests/input_grad_ref.py
(checked on the CPU by test_pose_cpu.py).  tcnn's own input-gradient arithmetic
is not available: parity unpinned, the restatement is the specification.

Bars (u = 2^-24; every figure is printed before it is asserted):
* position part: per component |err| <= POS_C u sum|terms| over the 16*8*2 terms
  scale_l dw_c/dpos_d denc_lf t_cf / (max - min).  POS_C = 20 is the kernel's own
  operation count, first order (the issue's 256 + 16 is the any-order worst case of
  a 256-term sum; this kernel adds in a fixed shallow order): a term passes through
  at most 2 roundings of 1 - pos, 1 of the weight product, 2 of denc_0 t_0 + denc_1
  t_1, 8 corner fmaf, 4 level fmaf, 2 butterfly adds and the final division.
  Measured on an MI355X: worst err / bound = 0.094 (n = 4113).
* direction part: relative error per row <= TAU_DIR for >= 99 % of rows, all four
  colour modes (the remaining rows: a ReLU whose pre-activation sits within rounding
  of 0 flips between the MFMA forward and the fp64 one).  TAU_DIR = 4 x the 99th
  percentile measured on an MI355X (see DIR_P99).
* segment sums: |err| <= (N + 2) u sum|terms| per ray, bit-identical between calls.
* through render(): relative error per ray <= TAU_RAY for >= 99 % of the rays with a
  nonzero gradient; TAU_RAY = 4 x the measured 99th percentile (RAY_P99; the MLP
  backward's dL/denc carries fp16 gradient storage).
"""
import pytest
import torch

import composite_ref as CR
import hashgrid as HG
import input_grad_ref as R
import synthetic as S
import vren
from losses import NeRFLoss
from models import custom_functions as CF
from models.networks import NGP
from models.rendering import render
from pose_refine import PoseRefiner

pytestmark = pytest.mark.gpu
DEV = "cuda"
POS_C = 20
DIR_P99 = 2.3e-6   # 99th percentile of the per-row relative error measured on an MI355X (worst of the four modes)
TAU_DIR = 4 * DIR_P99
RAY_P99 = 1.37e-3  # the same per ray through render()
TAU_RAY = 4 * RAY_P99


def _model(seed=3):
    m = NGP(0.5, seed=seed)
    with torch.no_grad():  # table values large enough that the field has structure (test_normal_gpu._model)
        g = torch.Generator().manual_seed(seed)
        m.params[HG.MLP_PARAMS:] = (torch.rand(m.params.numel() - HG.MLP_PARAMS, generator=g) * 2 - 1) * 0.5
        m.density_bitfield.copy_(S.packbits_cpu(S.shell_density_grid(128, m.cascades, 0.5), 0.5))
    return m.to(DEV)


@pytest.fixture(scope="module")
def model():
    m = _model()
    return m, R.FieldRef64(m.params.detach().cpu())


def _points(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, 3, generator=g) * 2 - 1) * 0.45
    d = torch.randn(n, 3, generator=g)
    return x, d, g


def _check_position(ref, x, denc, got, rows=None, what=""):
    tot, mag = ref.position_terms(x, denc)
    got = got.cpu().double()
    if rows is not None:
        unlisted = torch.ones(len(x), dtype=torch.bool)
        unlisted[rows] = False
        assert float(got[unlisted].abs().sum()) == 0, "an unlisted row was written"
        got, tot, mag = got[rows], tot[rows], mag[rows]
    bound = POS_C * R.U * mag * R.SLACK + R.TINY
    frac = float(((got - tot).abs() / bound).max())
    print(f"position {what}: n={len(tot)} worst err/bound = {frac:.3f}")
    assert frac <= 1.0
    assert float(tot.abs().max()) > 0
    return frac


# ------------------------------------------------------------- position part
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4113])
def test_position_part(model, n):
    m, ref = model
    x, _, g = _points(n, 100 + n)
    denc = torch.randn(n, 32, generator=g)
    dx, dd = HG.field_input_grad(x.to(DEV), None, m.grid, m._shadow.get(), None, None, denc.to(DEV), want_dirs=False)
    assert dd is None
    _check_position(ref, x, denc, dx, what="all rows")


def test_position_part_listed_rows_and_device_count(model):
    m, ref = model
    n = 300
    x, _, g = _points(n, 7)
    p16 = m._shadow.get()
    # a list with gaps (every third row, shuffled), longer than its device count: entries past it are never read
    rows = torch.arange(0, n, 3)[torch.randperm(100, generator=g)]
    idx = torch.full((128,), -1, dtype=torch.int32)
    idx[:100] = rows.int()
    denc = torch.randn(128, 32, generator=g)
    cnt = torch.tensor([100], dtype=torch.int64)
    dx, _ = HG.field_input_grad(x.to(DEV), None, m.grid, p16, None, None, denc.to(DEV), n_dev=cnt.to(DEV),
                                sample_idx=idx.to(DEV), want_dirs=False)
    got = dx.cpu()
    tot, mag = ref.position_terms(x[rows], denc[:100])
    unlisted = torch.ones(n, dtype=torch.bool)
    unlisted[rows] = False
    assert float(got[unlisted].abs().sum()) == 0, "an unlisted row was written"
    frac = float(((got[rows].double() - tot).abs() / (POS_C * R.U * mag * R.SLACK + R.TINY)).max())
    print(f"position listed rows: worst err/bound = {frac:.3f}")
    assert frac <= 1.0
    # n_dev < n without a list: rows past the count stay zero
    denc2 = torch.randn(n, 32, generator=g)
    cnt2 = torch.tensor([137], dtype=torch.int64)
    dx2, _ = HG.field_input_grad(x.to(DEV), None, m.grid, p16, None, None, denc2.to(DEV), n_dev=cnt2.to(DEV),
                                 want_dirs=False)
    _check_position(ref, x, denc2, dx2, rows=torch.arange(137), what="n_dev < n")


def test_position_part_on_cell_boundaries(model):
    """Points whose grid position p = scale_l x01 + 0.5 is an integer on a dense level (pos = 0, the cell's
    lower face): both one-sided weights are exact there and the derivative is the cell's own."""
    m, ref = model
    g = torch.Generator().manual_seed(9)
    pts, hit = [], 0
    dense = [l for l in range(16) if int(ref.spec.res[l]) ** 3 <= int(ref.spec.sizes[l])]
    assert len(dense) >= 2
    for l in dense:
        sc = float(ref.spec.scales[l])
        k = torch.randint(1, int(sc), (256, 3), generator=g).float()
        x = (k - 0.5) / sc - 0.5
        _, p32, _ = ref.cell(x)
        on = (p32[:, l, :] == torch.floor(p32[:, l, :])).all(1)
        hit += int(on.sum())
        pts.append(x[on])
    x = torch.cat(pts)
    assert hit >= 32, hit
    denc = torch.randn(len(x), 32, generator=g)
    dx, _ = HG.field_input_grad(x.to(DEV), None, m.grid, m._shadow.get(), None, None, denc.to(DEV), want_dirs=False)
    _check_position(ref, x, denc, dx, what=f"{hit} boundary points")


# ------------------------------------------------------------ direction part
def _direction(m, x, d, drgb, act):
    p16 = m._shadow.get()
    _, _, enc, _ = HG.field_forward(x, d, m.grid, p16, save_enc=True, rgb_act=act)
    denc = torch.zeros(x.shape[0], 32, device=DEV)
    _, dd = HG.field_input_grad(x, d, m.grid, p16, enc, drgb, denc, rgb_act=act)
    return dd.cpu().double()


@pytest.mark.parametrize("act", [HG.RGB_SIGMOID, HG.RGB_NONE, HG.RGB_LEAKY_RELU, HG.RGB_RELU])
def test_direction_part(model, act):
    m, ref = model
    n = 4113
    x, d, g = _points(n, 21)
    drgb = torch.randn(n, 3, generator=g)
    got = _direction(m, x.to(DEV), d.to(DEV), drgb.to(DEV), act)
    xg, dg = x.double().requires_grad_(True), d.double().requires_grad_(True)
    _, rgb, det = ref.forward(xg, dg, act, detail=True)
    want, gu = torch.autograd.grad((rgb * drgb.double()).sum(), (dg, det["u"]))
    rel = (got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-300)
    rel = torch.where((want.norm(dim=1) == 0) & (got.norm(dim=1) == 0), torch.zeros_like(rel), rel)
    p99 = float(torch.quantile(rel, 0.99))
    print(f"direction act={act}: median {float(rel.median()):.3e} p99 {p99:.3e} p99.9 "
          f"{float(torch.quantile(rel, 0.999)):.3e} beyond tau {float((rel > TAU_DIR).double().mean()):.2e}")
    assert float((rel <= TAU_DIR).double().mean()) >= 0.99
    assert float(want.norm(dim=1).max()) > 0 and torch.isfinite(got).all()
    # dL/dd is tangent to the sphere: <dL/dd, d> = <gu, u> - dot |u|^2 with dot = fl(<gu, u>): three roundings in
    # the dot product, four in |u|^2, two per component of gu - u dot, one in the division -- 16 u |gu| covers it
    perp = (got * d.double()).sum(1).abs()
    worst = float((perp / (16 * R.U * gu.norm(dim=1) * (1 + TAU_DIR) + R.TINY))[rel <= TAU_DIR].max())
    print(f"direction act={act}: worst <dL/dd, d> / (16 u |dL/du|) = {worst:.3f}")
    assert worst <= 1.0
    # d -> 3 d: dL/dd -> dL/dd / 3 (same unit vector up to rounding, so up to the same rare flips)
    got3 = _direction(m, x.to(DEV), (3 * d).to(DEV), drgb.to(DEV), act) * 3
    rel3 = (got3 - got).norm(dim=1) / got.norm(dim=1).clamp_min(1e-300)
    rel3 = torch.where((got.norm(dim=1) == 0) & (got3.norm(dim=1) == 0), torch.zeros_like(rel3), rel3)
    print(f"direction act={act}: scaling p99 {float(torch.quantile(rel3, 0.99)):.3e}")
    assert float((rel3 <= TAU_DIR).double().mean()) >= 0.99


# -------------------------------------------------------------- segment sums
@pytest.mark.parametrize("with_dirs", [True, False])
def test_ray_segment_sum(with_dirs):
    Ns = [0, 1, 63, 64, 65, 1024, 0, 2]
    g = torch.Generator().manual_seed(4)
    starts = [0]
    for nn in Ns[:-1]:
        starts.append(starts[-1] + nn)
    rays_a = torch.tensor([[r, starts[r], Ns[r]] for r in range(len(Ns))], dtype=torch.int64)
    N = sum(Ns)
    gx, gd, ts = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g), torch.rand(N, generator=g) * 2
    a = vren.ray_segment_sum(gx.to(DEV), gd.to(DEV) if with_dirs else None, ts.to(DEV), rays_a.to(DEV))
    b = vren.ray_segment_sum(gx.to(DEV), gd.to(DEV) if with_dirs else None, ts.to(DEV), rays_a.to(DEV))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "not run-to-run bit-identical"
    do, dd, ao, ad = R.segment_sums64(gx, gd if with_dirs else None, ts, rays_a, len(Ns))
    nn = torch.tensor(Ns, dtype=torch.float64)[:, None]
    fo = (a[0].cpu().double() - do).abs() / ((nn + 2) * R.U * ao * R.SLACK + R.TINY)
    fd = (a[1].cpu().double() - dd).abs() / ((nn + 2) * R.U * ad * R.SLACK + R.TINY)
    print(f"segment sums dirs={with_dirs}: worst err/bound rays_o {float(fo.max()):.3f} rays_d {float(fd.max()):.3f}")
    assert float(fo.max()) <= 1.0 and float(fd.max()) <= 1.0
    for r, n_r in enumerate(Ns):
        if n_r == 0:
            assert float(a[0][r].abs().sum()) == 0 and float(a[1][r].abs().sum()) == 0
    # the comparison helper (index_add_) agrees to rounding
    h = CF._segment_sum(gx.to(DEV), rays_a.to(DEV), len(Ns)).cpu().double()
    assert float(((h - do).abs() / ((nn + 2) * R.U * ao * R.SLACK + R.TINY)).max()) <= 1.0


# ----------------------------------------------------------- through render()
def _scene(n_rays=256, n_images=10, seed=3):
    sc = S.SyntheticScene(W=40, H=40, n_images=n_images, seed=seed)
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, n_images, (n_rays,), generator=g)
    pix = torch.randint(0, 1600, (n_rays,), generator=g)
    gt = torch.rand(n_rays, 3, generator=g)
    noise = torch.rand(n_rays, generator=g)
    return sc, img, pix, gt, noise


@pytest.fixture()
def fixed_noise():
    def use(noise):
        CF.NOISE_HOOK = lambda rays_o: noise.to(rays_o.device)
    yield use
    CF.NOISE_HOOK = None


def _loss(m, o, d, gt):
    res = render(m, o, d, exp_step_factor=0.0)
    ld = NeRFLoss(30, "raw", 0.5, 0.0, lambda_distortion=0.0)(res, {"rgb": gt})
    return sum(v.mean() for v in ld.values()), res


def _ray_grads(m, o, d, gt):
    o, d = o.detach().clone().requires_grad_(True), d.detach().clone().requires_grad_(True)
    seen = []
    hook = m.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach()))
    try:
        loss, res = _loss(m, o, d, gt)
    finally:
        hook.remove()
    res["xyzs"] = seen[0]  # the sample positions the field was evaluated at
    go, gd = torch.autograd.grad(loss, (o, d))
    return go, gd, res


def _ray_grads_ref(ref, o, d, gt, res):
    """The same loss in fp64 on the march's own samples (fixed at their t, as in the reference)."""
    rays_a, ts, deltas = res["rays_a"].cpu(), res["ts"].detach().cpu(), res["deltas"].detach().cpu()
    n_rays = o.shape[0]
    o64, d64 = o.cpu().double().requires_grad_(True), d.cpu().double().requires_grad_(True)
    ray_of = torch.repeat_interleave(rays_a[:, 0], rays_a[:, 2])
    order = torch.cat([torch.arange(s, s + n) for _, s, n in rays_a.tolist()]) if len(ray_of) else ray_of
    x32 = torch.zeros(len(ts), 3)
    # the marcher's fp32 sample positions, carried straight-through: fl(o + t d) per component (fmaf or two roundings:
    # within an ulp either way; the restatement takes the fp32 value the field kernels read)
    xs = (o.cpu()[ray_of] + d.cpu()[ray_of] * ts[order, None])
    x32[order] = xs
    xg = torch.zeros(len(ts), 3, dtype=torch.float64).index_add(0, order, o64[ray_of] + d64[ray_of] * ts.double()[order, None])
    dirs = torch.zeros(len(ts), 3, dtype=torch.float64).index_add(0, order, d64[ray_of])
    x = R.st(x32.double(), xg)
    sig, rgb = ref.forward(x, dirs, HG.RGB_SIGMOID)
    f = CR.composite_ref64(sig, rgb, deltas, ts, rays_a, 1e-4)
    z3, z1 = torch.zeros(n_rays, 3, dtype=torch.float64), torch.zeros(n_rays, dtype=torch.float64)
    Rr, Oo = z3.index_add(0, f.ray, f.R), z1.index_add(0, f.ray, f.O)
    xrgb = Rr + (1 - Oo)[:, None]  # white background (exp_step_factor 0, rendering.py:290-296)
    l_rgb = ((xrgb - gt.cpu().double()) / (xrgb.detach() + CR.C_DEN)) ** 2
    oo = Oo + CR.C_EPS
    loss = l_rgb.mean() + (1e-3 * (-oo * torch.log(oo))).mean()
    go, gd = torch.autograd.grad(loss, (o64, d64))
    return go, gd, x32


def test_render_ray_gradients(model, fixed_noise):
    m, ref = model
    sc, img, pix, gt, noise = _scene()
    fixed_noise(noise)
    o, d = sc.rays(img, pix)
    o, d, gt = o.to(DEV).contiguous(), d.to(DEV).contiguous(), gt.to(DEV)
    go, gd, res = _ray_grads(m, o, d, gt)
    assert torch.isfinite(go).all() and torch.isfinite(gd).all()
    assert float(go.abs().sum()) > 0 and float(gd.abs().sum()) > 0
    ro, rd, x32 = _ray_grads_ref(ref, o, d, gt, res)
    assert torch.equal(x32, res["xyzs"].cpu()), "the restatement's sample positions are not the march's"
    got = torch.cat([go, gd], 1).cpu().double()
    want = torch.cat([ro, rd], 1)
    nz = want.norm(dim=1) > 0
    assert int(nz.sum()) >= 128, int(nz.sum())
    rel = ((got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-300))[nz]
    print(f"render: {int(nz.sum())} rays with gradient, {int(res['rays_a'][:, 2].sum())} samples; per-ray relative error "
          f"median {float(rel.median()):.3e} p99 {float(torch.quantile(rel, 0.99)):.3e} max {float(rel.max()):.3e}")
    assert float((rel <= TAU_RAY).double().mean()) >= 0.99
    assert float(got[~nz].abs().sum()) == 0
    # frozen parameters: the same input gradients, bit for bit
    m.params.requires_grad_(False)
    try:
        fo, fd, _ = _ray_grads(m, o, d, gt)
    finally:
        m.params.requires_grad_(True)
    assert torch.equal(fo, go) and torch.equal(fd, gd)


def test_render_param_gradients_unchanged(model, fixed_noise):
    """Inputs that require no gradient: the backward launches exactly the kernels it launched before (none of
    the two new ones; the per-kernel launch counts of the timing hook), and asking for the input gradients as
    well adds one launch of each and leaves the parameter gradient where it was.

    The parameter gradient cannot be compared bit for bit: the unchanged path is not bit-identical to itself
    from run to run (the MLP backward's dW and the coarse hash levels are fp32 atomic sums over blocks; measured
    on an MI355X on this batch: two runs of the unchanged path differ by up to 4.7e-10 absolute, 5.8e-10 against
    the run with input gradients).  It is held to the project's bar for the same gradient in another atomic
    order (test_trainer_gpu.py: relative L2 < 1e-5), and the launch sequence is compared exactly."""
    import ktimer as KT
    m, _ = model
    sc, img, pix, gt, noise = _scene(seed=5)
    fixed_noise(noise)
    o, d = sc.rays(img, pix)
    o, d, gt = o.to(DEV).contiguous(), d.to(DEV).contiguous(), gt.to(DEV)
    timer = KT.KernelTimer(torch.zeros(1, dtype=torch.int64, device=DEV), rows=4, device=DEV)

    def params_grad(req):
        m.params.grad = None
        oo, dd = o.clone().requires_grad_(req), d.clone().requires_grad_(req)
        loss, _ = _loss(m, oo, dd, gt)
        timer.arm()
        try:
            loss.backward()
        finally:
            counts = dict(zip(KT.NAMES, timer.disarm()))
        gp, m.params.grad = m.params.grad.clone(), None
        return gp, counts

    (a, ca), (b, cb), (c, cc) = params_grad(False), params_grad(False), params_grad(True)
    print(f"params.grad: repeat run equal {torch.equal(a, b)}, max |diff| {float((a - b).abs().max()):.3e}; "
          f"with input gradients equal {torch.equal(a, c)}, max |diff| {float((a - c).abs().max()):.3e}")
    print("backward launches:", {k: v for k, v in ca.items() if v}, "+ with input gradients:",
          {k: cc[k] - ca[k] for k in cc if cc[k] != ca[k]})
    assert ca == cb and ca["input_grad"] == 0 and ca["ray_segment_sum"] == 0
    assert ca["mlp_bwd"] == 1 and ca["hash_bwd_coarse"] >= 1
    assert {k: cc[k] - ca[k] for k in cc if cc[k] != ca[k]} == {"input_grad": 1, "ray_segment_sum": 1}
    assert float(a.abs().sum()) > 0
    assert float((b - a).norm() / a.norm()) < 1e-5
    assert float((c - a).norm() / a.norm()) < 1e-5


# -------------------------------------------------------- PoseRefiner end to end
def test_pose_refiner_end_to_end(model, fixed_noise):
    m, _ = model
    sc, img, pix, gt, noise = _scene(seed=8)
    img = torch.tensor([0, 2, 3, 5, 7])[img % 5]  # images 1, 4, 6, 8, 9 never in the batch
    fixed_noise(noise)
    dirs, poses = sc.directions.to(DEV), sc.poses.to(DEV)
    img, pix, gt = img.to(DEV), pix.to(DEV), gt.to(DEV)
    pr = PoseRefiner(10, device=DEV)
    opt = pr.optimizer(lr=1e-3)
    keep = poses.clone()
    for step in range(2):
        o, d = pr.rays(img, pix, dirs, poses)
        loss, _ = _loss(m, o, d, gt)
        loss.backward()
        if step == 0:
            # ext.grad = the chain rule applied to the per-ray gradients (axisangle_to_R / get_rays by torch autograd)
            go, gd, _ = _ray_grads(m, o, d, gt)
            o2, d2 = pr.rays(img, pix, dirs, poses)
            (want,) = torch.autograd.grad((o2 * go).sum() + (d2 * gd).sum(), pr.ext)
            err = float((pr.ext.grad - want).norm() / want.norm())
            print(f"pose refiner: |ext.grad - chain rule| / |chain rule| = {err:.3e}")
            assert float(want.norm()) > 0 and err <= 1e-6
        opt.step()
        opt.zero_grad()
    assert torch.equal(poses, keep)
    dR, dT = pr.dR.detach().cpu(), pr.dT.detach().cpu()
    assert torch.isfinite(dR).all() and torch.isfinite(dT).all()
    seen = torch.zeros(10, dtype=torch.bool)
    seen[[0, 2, 3, 5, 7]] = True
    assert (dR[seen].abs().sum(1) > 0).all() and (dT[seen].abs().sum(1) > 0).all()
    assert float(dR[~seen].abs().sum()) == 0 and float(dT[~seen].abs().sum()) == 0
    assert float(pr.ext.detach()[60:].abs().sum()) == 0
    moved = pr.refined_poses(poses)
    assert float((moved - poses)[seen].abs().max()) > 0 and torch.equal(moved[~seen], poses[~seen])
