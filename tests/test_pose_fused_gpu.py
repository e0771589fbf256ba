"""Pose refinement inside the fused training step (NGPTrainer(optimize_ext=True);
csrc/pose.hip: ngp_pose_compose, ngp_pose_grad) against the fp64 restatement
tests/pose_ref.py (checked on the CPU by test_pose_chain_cpu.py) and against the
project's own references for the quantities the step already had.

Bars (u = 2^-24; every figure is printed before it is asserted).  Each is
u * sum_t k_t |term_t| with k_t the kernel's own count of roundings on the term's
path, first order (SLACK covers the second); the counts stand next to the code
they count, below.  sinf / cosf are taken at 2 ulp = 4 u (the device library's
documented bound is no worse), a division or a square root at 1.

theta = |v| + 1e-7 carries K_THETA = 5 u: three roundings in v.v (halved by the
square root: 1.5), the root, the addition, and the constant 1e-7f itself (1 u of
1e-7 <= 1 u of theta).  A coefficient f(theta) sees it multiplied by its condition
number kappa_f = |theta f'/f| (pose_ref.condition_numbers: <= 1 for small theta,
21 for A = sin(theta)/theta at theta = 3, where sin(theta) is small and theta cot
theta is not).

compose, rotation entry (a,b) = sum_c Rod[a][c] R[c][b], Rod = (I + A K) + B K2:
  k_I   = 2 (the two sums of Rod) + 3 (product and two sums of the 3-term dot)             = 5
  k_AK  = 4 (sinf) + 1 (/ theta) + K_THETA kappa_A + 1 (A * K) + 5                          = 11 + 5 kappa_A
  k_BK2 = 2 * (4 (sinf) + 1 (/ theta)) + 1 (square) + K_THETA kappa_B
          + 3 (the entry of K2: two products and a sum) + 1 (B * K2) + 5                    = 20 + 5 kappa_B
translation t + dT: one rounding.

pose gradient of image i with n_i rays: every term passes through at most n_i
roundings of its thread's running sum (one fmaf per ray) and
  K_COMMON = 6 (butterfly) + 3 (the four waves' sums) + 3 (a row of M = G R^T) + 16 (the 3x3 algebra: w,
             M v, M^T v, v^T M v, |v|^2 tr M, v_k / |v| with its root and division, and the sums that join
             them: no term passes through more than 16 of them)                              = 28
plus its coefficient's own count + K_THETA kappa:
  A: 5, B: 11 as above;
  A': series (Horner, 6 levels of one product and one difference, alternating terms whose absolute sum is at
      most 1.5 x the value on theta < 1.5) 2 * 6 + theta^2 + the final product, x 1.5 -> 21; closed form
      (theta >= 1.5: the two terms no longer cancel, amplification <= 1.3) (4 + 1 + 4) * 1.3 + 3 -> 15;      21
  B': series (8 levels, absolute sum <= 2.3 x the value on theta < 2.5) (2 * 8 + 2) * 2.3 -> 42; closed
      form (amplification <= 2.4) (4 + 1 + 2 * 4 + 2) * 2.4 + 4 -> 40;                                       42
dL/dT_i = sum of the image's go: (n_i + 9) u sum |go| (held to n_i + K_COMMON).
"""
import pytest
import torch

import hashgrid as HG
import input_grad_ref as R
import ktimer as KT
import pose_ref as PR
import synthetic as S
import test_input_grad_gpu as TIG
import vren
from datasets.ray_utils import get_rays
from trainer import NGPTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAGS = [0.0, 1e-7, 1e-6, 1e-4, 1e-2, 0.3, 1.0, 3.0]
K_THETA = 5.0
K_COMMON = 28.0
SEEN = [0, 2, 3, 5, 7]


def _k_compose(theta):
    kA, kB, _, _ = PR.condition_numbers(theta)
    return torch.full_like(theta, 5.0), 11.0 + K_THETA * kA, 20.0 + K_THETA * kB


def _k_grad(theta):
    kA, kB, kdA, kdB = PR.condition_numbers(theta)
    return [5.0 + K_THETA * kA, 11.0 + K_THETA * kB, 21.0 + K_THETA * kdA, 42.0 + K_THETA * kdB]


def _ext(n_img, gen, shift=0, mags=MAGS):
    """ext with dR rows at the listed magnitudes (row i: mags[(i + shift) % len], a random direction; the
    magnitude 0 row is exactly 0) and dT ~ 0.1 N(0,1); padding 0"""
    n_pad = (6 * n_img + 3) // 4 * 4
    ext = torch.zeros(n_pad)
    d = torch.randn(n_img, 3, generator=gen, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    m = torch.tensor([mags[(i + shift) % len(mags)] for i in range(n_img)], dtype=torch.float64)
    ext[:3 * n_img] = (d * m[:, None]).float().reshape(-1)
    ext[3 * n_img:6 * n_img] = torch.randn(3 * n_img, generator=gen) * 0.1
    return ext


def _p(t):
    return vren.c_void_p(t.data_ptr())


def _compose(poses, ext):
    out = torch.full_like(poses, float("nan"))
    vren._ok(vren.lib().ngp_pose_compose(_p(poses), _p(ext), poses.shape[0], _p(out), vren._stream()), "pose_compose")
    return out


# -------------------------------------------------------------------- compose
@pytest.mark.parametrize("n_img", [1, 3, 10, 65])
def test_compose(n_img):
    gen = torch.Generator().manual_seed(40 + n_img)
    poses = torch.randn(n_img, 3, 4, generator=gen)
    ext = _ext(n_img, gen)
    assert float(ext[:3].abs().sum()) == 0  # row 0: exactly zero
    got = _compose(poses.to(DEV), ext.to(DEV)).cpu()
    want, mag = PR.compose(poses, ext, _k_compose)
    frac = (got.double() - want).abs() / (PR.U * mag * PR.SLACK + PR.TINY)
    print(f"compose n_img={n_img}: worst err/bound rotation {float(frac[:, :, :3].max()):.3f} translation "
          f"{float(frac[:, :, 3].max()):.3f}; zero row bit-equal: {torch.equal(got[0, :, :3], poses[0, :, :3])}")
    assert torch.isfinite(got).all()
    assert float(frac.max()) <= 1.0
    again = _compose(poses.to(DEV), ext.to(DEV)).cpu()
    assert torch.equal(got, again)


# -------------------------------------------------------------- pose gradient
def _assignment(n_rays, gen):
    """image of every ray, 10 images: image 9 never; image 8 exactly once; image 0 more than 64 rays where the
    batch has them (65: all of it; 255 - 257: 100 consecutive rays; beyond: about 30 % of the batch at random
    positions, so that with 8192 rays it holds more than 1024 and a thread of its block about ten of them, in
    every slot of the kernel's four-wide index walk and in all eight trips of its loop)"""
    if n_rays == 65:
        return torch.zeros(65, dtype=torch.int64)
    img = torch.randint(1, 8, (n_rays,), generator=gen)
    if n_rays > 257:
        img[torch.rand(n_rays, generator=gen) < 0.3] = 0
    elif n_rays >= 255:
        img[1:101] = 0
    img[0] = 8
    return img


@pytest.fixture(scope="module")
def scene():
    return S.SyntheticScene(W=40, H=40, n_images=10, seed=3)


def _pose_grad(go, gd, img, pix, directions, poses, ext):
    out = torch.full_like(ext, float("nan"))
    vren._ok(vren.lib().ngp_pose_grad(_p(go), _p(gd), _p(img), _p(pix), img.numel(), _p(directions), _p(poses), _p(ext),
                                      poses.shape[0], _p(out), vren._stream()), "pose_grad")
    return out


# (the kernel: one 256-thread block per image, thread t walks rays t + 256 j four at a time -- sizes around one
# wave, one block (255 / 256 / 257), one four-wide trip (1023 / 1024 / 1025), and the production batch, 8192)
@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8192])
def test_pose_grad(scene, n_rays):
    gen = torch.Generator().manual_seed(70 + n_rays)
    img = _assignment(n_rays, gen)
    pix = torch.randint(0, 1600, (n_rays,), generator=gen)
    go, gd = torch.randn(n_rays, 3, generator=gen), torch.randn(n_rays, 3, generator=gen)
    ext = _ext(10, gen, shift=3)  # image 0: 1e-4, image 5: 0, image 8: 1e-4, images 2-4: 0.3, 1, 3
    dirs, poses = scene.directions.float().contiguous(), scene.poses.float().contiguous()
    cnt = torch.bincount(img, minlength=10)
    if n_rays >= 255:
        assert int(cnt[9]) == 0 and int(cnt[8]) == 1 and int(cnt[0]) > 64
    if n_rays == 8192:
        assert int(cnt[0]) > 1024
    args = [t.to(DEV) for t in (go, gd, img, pix, dirs, poses, ext)]
    got = _pose_grad(*args).cpu()
    again = _pose_grad(*args).cpu()
    assert torch.isfinite(got).all(), "an entry of grad_ext was not written"
    assert torch.equal(got, again), "not run-to-run bit-identical"
    want, bound = PR.pose_grad(go, gd, img, pix, dirs, poses, ext, _k_grad, K_COMMON)
    frac = (got.double() - want).abs() / (PR.U * bound * PR.SLACK + PR.TINY)
    absent = (cnt == 0).nonzero().flatten()
    gR, gT = got[:30].view(10, 3), got[30:60].view(10, 3)
    print(f"pose_grad n_rays={n_rays}: worst err/bound dR {float(frac[:30].max()):.3f} dT {float(frac[30:60].max()):.3f}; "
          f"rays per image {cnt.tolist()}")
    assert float(gR[absent].abs().sum()) == 0 and float(gT[absent].abs().sum()) == 0
    assert float(got[60:].abs().sum()) == 0
    assert float(frac.max()) <= 1.0
    assert float(want.abs().max()) > 0


# ------------------------------------------------------- the coefficients
def test_rod_coefficients_over_the_whole_range():
    """A, B, A', B' as the kernels evaluate them (ngp_pose_rod_coefficients: the same device functions) against the
    fp64 restatement on 20001 values of theta, log-spaced over [1e-7, pi], plus both sides of the two series
    thresholds (1.5, 2.5): each within its own rounding count of the docstring above (5, 11, 21, 42 u; theta is
    given exactly here, so no condition number enters).  This is the check of the series paths that the
    pose-gradient bars cannot give at small theta, where the A' and B' terms of dL/dv sit below the rounding of
    the A term: the small end holds the leading terms -theta/3 and -theta/12, theta around 1 the later ones (the
    theta^3 term of A' is a tenth of the value there)."""
    th = torch.logspace(-7, 0.49714987269413385, 20001, dtype=torch.float64).float()
    edge = torch.tensor([1.5, 2.5])
    th = torch.cat([th, torch.nextafter(edge, torch.zeros(2)), edge, torch.nextafter(edge, torch.full((2,), 4.0))])
    th = th[th <= 3.1415927].contiguous()
    out = torch.full((len(th), 4), float("nan"), device=DEV)
    vren._ok(vren.lib().ngp_pose_rod_coefficients(_p(th.to(DEV)), len(th), _p(out), vren._stream()), "rod_coefficients")
    want = torch.stack(PR.coefficients(th.double()), 1)
    rel = (out.cpu().double() - want).abs() / want.abs() / PR.U
    worst = rel.max(0).values
    print("coefficients, worst relative error in u: A %.2f  B %.2f  A' %.2f  B' %.2f (at theta = %s)"
          % (*worst.tolist(), [round(float(th[i]), 4) for i in rel.argmax(0)]))
    assert torch.isfinite(out).all()
    for j, k in enumerate((5.0, 11.0, 21.0, 42.0)):
        assert float(worst[j]) <= k * PR.SLACK


# ------------------------------------------------ one fused step, three references
@pytest.fixture(scope="module")
def model():
    m = TIG._model()
    return m, R.FieldRef64(m.params.detach().cpu())


def _trainer(m, **kw):
    tr = NGPTrainer(scale=0.5, batch_size=256, device=DEV, seed=3, **kw)
    tr.load_params(m.params.detach())
    tr.density_bitfield.copy_(m.density_bitfield)
    tr.global_step = 1  # no occupancy update inside the step
    return tr


def _batch(seed):
    sc, img, pix, gt, noise = TIG._scene(seed=seed)
    img = torch.tensor(SEEN)[img % 5]  # images 1, 4, 6, 8, 9 never in the batch
    return sc, img, pix, gt, noise


def test_fused_step_against_the_projects_references(model):
    m, ref = model
    sc, img, pix, gt, noise = _batch(8)
    dirs, poses = sc.directions.to(DEV).float().contiguous(), sc.poses.to(DEV).float().contiguous()
    dv = [t.to(DEV) for t in (img, pix, gt)]
    tr = _trainer(m, optimize_ext=True)
    tr._pose_state(poses)
    gen = torch.Generator().manual_seed(5)
    ext0 = _ext(10, gen, mags=MAGS[:5])  # corrections up to 1e-2: the rays still meet the shell
    tr.pose_refiner.load_reference({"dR": ext0[:30].view(10, 3), "dT": 0.1 * ext0[30:60].view(10, 3)})
    ext0 = tr.pose_refiner.ext.detach().cpu().clone()
    tr.step(*dv, dirs, poses, noise=noise.to(DEV), apply_adam=False)
    torch.cuda.synchronize()
    assert torch.equal(tr.pose_refiner.ext.detach().cpu(), ext0), "apply_adam=False stepped the poses"
    ps = tr._ps
    # (a) the per-ray gradients against the fp64 restatement of the field on the march's own samples
    n = int(tr.n_samples.item())
    res = {"rays_a": tr.rays_a, "ts": tr.ts[:n], "deltas": tr.deltas[:n]}
    ro, rd, _ = TIG._ray_grads_ref(ref, tr.rays_o, tr.rays_d, dv[2], res)
    go, gd = ps["d_rays_o"].cpu(), ps["d_rays_d"].cpu()
    got, want = torch.cat([go, gd], 1).double(), torch.cat([ro, rd], 1)
    nz = want.norm(dim=1) > 0
    assert int(nz.sum()) >= 128, int(nz.sum())
    rel = ((got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-300))[nz]
    print(f"fused step: {int(nz.sum())} rays with gradient, {n} samples; per-ray relative error median "
          f"{float(rel.median()):.3e} p99 {float(torch.quantile(rel, 0.99)):.3e} max {float(rel.max()):.3e}")
    assert float((rel <= TIG.TAU_RAY).double().mean()) >= 0.99
    assert float(got[~nz].abs().sum()) == 0
    # (b) ext's gradient = the restatement's chain rule applied to those same per-ray buffers
    wg, bound = PR.pose_grad(go, gd, img, pix, dirs.cpu(), poses.cpu(), ext0, _k_grad, K_COMMON)
    frac = (ps["grad"].cpu().double() - wg).abs() / (PR.U * bound * PR.SLACK + PR.TINY)
    print(f"fused step: ext gradient worst err/bound {float(frac.max()):.3f}, |grad| {float(wg.norm()):.3e}")
    assert float(frac.max()) <= 1.0 and float(wg.abs().max()) > 0
    unseen = [i for i in range(10) if i not in SEEN]
    g = ps["grad"].cpu()
    assert float(g[:30].view(10, 3)[unseen].abs().sum()) == 0 and float(g[30:60].view(10, 3)[unseen].abs().sum()) == 0
    # (c) the parameter gradient is that of a trainer without optimize_ext on the same rays
    eff = ps["poses_eff"].clone()
    plain = _trainer(m)
    plain.step(*dv, dirs, eff, noise=noise.to(DEV), apply_adam=False)
    torch.cuda.synchronize()
    assert torch.equal(plain.rays_o, tr.rays_o) and torch.equal(plain.rays_d, tr.rays_d)
    d = float((tr.grad - plain.grad).norm() / plain.grad.norm())
    print(f"fused step: parameter gradient against a trainer without optimize_ext, relative L2 {d:.3e}")
    assert float(plain.grad.abs().sum()) > 0 and d < 1e-5
    assert plain._ps is None and plain.pose_refiner is None


def test_two_steps_with_adam(model):
    m, _ = model
    sc, img, pix, gt, noise = _batch(8)
    dirs, poses = sc.directions.to(DEV).float().contiguous(), sc.poses.to(DEV).float().contiguous()
    keep = poses.clone()
    dv = [t.to(DEV) for t in (img, pix, gt)]
    tr = _trainer(m, optimize_ext=True, pose_lr=1e-3)
    tr.step(*dv, dirs, poses, noise=noise.to(DEV))
    ext1 = tr.pose_refiner.ext.detach().clone()
    assert torch.equal(tr.rays_o, poses[dv[0], :, 3]), "step 1's rays are not those of ext = 0"
    tr.step(*dv, dirs, poses, noise=noise.to(DEV))
    torch.cuda.synchronize()
    # the second step's rays are those of ext after step 1
    eff1 = _compose(poses, ext1)
    assert torch.equal(tr.rays_o, eff1[dv[0], :, 3])
    _, d1 = get_rays(dirs[dv[1]], eff1[dv[0]])
    assert torch.allclose(tr.rays_d, d1, rtol=0, atol=1e-6)
    assert torch.equal(poses, keep), "the caller's poses were modified"
    pr = tr.pose_refiner
    dR, dT = pr.dR.detach().cpu(), pr.dT.detach().cpu()
    seen = torch.zeros(10, dtype=torch.bool)
    seen[SEEN] = True
    assert torch.isfinite(dR).all() and torch.isfinite(dT).all()
    assert (dR[seen].abs().sum(1) > 0).all() and (dT[seen].abs().sum(1) > 0).all()
    assert float(dR[~seen].abs().sum()) == 0 and float(dT[~seen].abs().sum()) == 0
    assert float(pr.ext.detach()[60:].abs().sum()) == 0
    assert not torch.equal(pr.ext.detach(), ext1)
    moved = tr.refined_poses(poses)
    assert float((moved - poses)[seen].abs().max()) > 0 and torch.equal(moved[~seen], poses[~seen])
    sd = pr.state_dict_reference()
    assert set(sd) == {"dR", "dT"} and torch.equal(sd["dR"].cpu(), dR)


# ------------------------------------------------------------ eager-only
def test_use_graphs_has_no_effect_under_optimize_ext():
    """optimize_ext ships eager-only: train_step past the warm-up captures and replays
    no graph and marches nothing ahead with use_graphs on (the default), the device counters advance once per
    step, and the poses move.  A trainer without optimize_ext on the same schedule does replay."""
    sc = S.AnalyticScene(W=100, H=100, n_images=10)
    dirs, poses = sc.directions.to(DEV), sc.poses.to(DEV)
    gt_img = sc.gt_images(device=DEV)
    out = {}
    for on in (True, False):
        tr = NGPTrainer(scale=0.5, batch_size=4096, device=DEV, seed=3, warmup_steps=16, optimize_ext=on,
                        pose_lr=1e-4, pair_steps=on)
        tr.mark_invisible_cells(sc.K, sc.poses, (sc.W, sc.H))
        for _ in range(36):
            loss = tr.train_step(gt_img, dirs, poses)
        tr.drain()
        torch.cuda.synchronize()
        out[on] = (len(tr._graphs), tr.n_prefetched, tr.global_step, tr.dctr[:2].tolist())
        assert torch.isfinite(loss).all()
        if on:
            assert not tr.pair_steps and not tr.pre_coarse and not any(m["pre_ready"] for m in tr.msets)
            assert float(tr.pose_refiner.ext.detach().abs().max()) > 1e-5
    print("graphs, batches marched ahead, steps, device counters: optimize_ext", out[True], "plain", out[False])
    assert out[True] == (0, 0, 36, [36, 36])
    assert out[False][0] >= 1 and out[False][1] >= 1 and out[False][2:] == (36, [36, 36])


# ------------------------------------------------------------------ off is off
def test_off_is_off(model):
    m, _ = model
    sc, img, pix, gt, noise = _batch(8)
    dirs, poses = sc.directions.to(DEV).float().contiguous(), sc.poses.to(DEV).float().contiguous()
    dv = [t.to(DEV) for t in (img, pix, gt)]
    new = ("input_grad", "ray_segment_sum", "pose_compose", "pose_grad")
    counts = {}
    for on in (False, True):
        tr = _trainer(m, optimize_ext=on) if on else _trainer(m)
        timer = KT.KernelTimer(tr.dctr, rows=4, device=DEV)
        timer.arm()
        try:
            for _ in range(2):
                tr.step(*dv, dirs, poses, noise=noise.to(DEV))
        finally:
            counts[on] = dict(zip(KT.NAMES, timer.disarm()))
        torch.cuda.synchronize()
        if not on:
            assert tr._ps is None and tr.pose_refiner is None and tr.pre_coarse
            assert torch.equal(tr.refined_poses(poses), poses)
    print("launches in two steps, off:", {k: counts[False][k] for k in new}, "on:", {k: counts[True][k] for k in new})
    assert all(counts[False][k] == 0 for k in new)
    assert all(counts[True][k] == 2 for k in new)
    assert counts[True]["adam"] == counts[False]["adam"] + 2  # the pose Adam
    for k in KT.NAMES:
        if k not in new and k != "adam":
            assert counts[True][k] == counts[False][k], k
    with pytest.raises(NotImplementedError):
        NGPTrainer(scale=0.5, batch_size=256, device=DEV, optimize_ext=True, emulate_dp=2)


# ------------------------------------------------------------------- surface
def test_train_scene_optimize_ext_saves_reference_keys(tmp_path):
    """scripts/train_scene.py --optimize_ext --ckpt: trains through the refining step and writes
    dR / dT under the reference's keys beside the parameters."""
    import importlib.util
    import os
    root = tmp_path / "Synthetic_Test" / "Sphere"
    S.write_nsvf_scene(str(root), res=100, n_train=24, n_test=1)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_scene", os.path.join(here, "scripts", "train_scene.py"))
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    ck = str(tmp_path / "ck.pt")
    res = ts.main(["--dataset", "nsvf", "--root", str(root), "--downsample", "0.125", "--steps", "300",
                   "--optimize_ext", "--pose_lr", "1e-5", "--ckpt", ck])
    d = torch.load(ck)
    assert res["optimize_ext"] and res["guard_hits"] == 0
    assert set(d) == {"params", "dR", "dT"} and d["dR"].shape == (24, 3) and d["dT"].shape == (24, 3)
    assert torch.isfinite(d["dR"]).all() and float(d["dR"].abs().max()) > 0 and float(d["dT"].abs().max()) > 0
