"""Pose refinement in the fused step, the parts that need no GPU: the fp64
restatement tests/pose_ref.py (compose and the chain rule to dR / dT) against the
reference function's recorded outputs (tests/golden/axisangle.npz) and against
torch.autograd of an fp64 copy of axisangle_to_R + get_rays, and the C-ABI of the
two new entry points (exports and argument guards, as test_capi_cpu.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pose_ref as PR
import vren

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "axisangle.npz")
MAGS = [0.0, 1e-7, 1e-6, 1e-4, 1e-2, 0.3, 1.0, 3.0]


def test_restatement_matches_reference_golden():
    """The golden file holds the reference function's fp32 outputs: R of 12 axis-angle rows and the gradient
    of sum(R * M).  An fp32 Rod entry is a handful of roundings of values <= 1 + |v| + |v|^2 / 2 <= 9.1 (rows
    up to |v| = 3.14): 1e-5 absolute covers 16 roundings of that; the gradient's entries are sums of 9 such
    products with |M| <= 4."""
    g = np.load(GOLD)
    v, M = torch.from_numpy(g["v"]), torch.from_numpy(g["M"])
    rod, th, nv = PR.rodrigues(v)
    err_R = float((rod - torch.from_numpy(g["R"]).double()).abs().max())
    grad, _ = PR.rod_grad(v, M)
    err_g = float((grad - torch.from_numpy(g["grad"]).double()).abs().max())
    print(f"restatement vs golden: max |dR| {err_R:.2e}, max |dgrad| {err_g:.2e}")
    assert err_R <= 1e-5
    assert err_g <= 16 * 9 * 4 * 9.1 * PR.U
    eye = torch.eye(3, dtype=torch.float64).expand(12, 3, 3)
    assert float((rod @ rod.transpose(1, 2) - eye).abs().max()) <= 1e-6  # (theta = |v| + 1e-7: not exactly orthogonal)


def _vectors(mag, n, gen):
    d = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    return d / d.norm(dim=1, keepdim=True) * mag


@pytest.mark.parametrize("mag", MAGS)
def test_closed_form_gradient_equals_autograd(mag):
    """dL/d(dR, dT) by the restatement's closed form against torch.autograd of an fp64 copy of axisangle_to_R +
    get_rays, 1e-12 relative (|difference| against the gradient's norm, per image) at every magnitude.  The
    copy writes 1 - cos(theta) as 2 sin^2(theta/2) (pose_ref.axisangle_to_R64: the literal form's own fp64
    cancellation reaches 6.4e-11 at |v| = 1e-7, 4.5e-11 at 1e-6 and 5.8e-13 at 1e-4, measured).  The literal copy is run as well
    and held to 1e-12 plus that cancellation, 4 eps64 / theta: 1 - cos is good to eps64 / 2 absolute, autograd
    divides twice that by theta^3 and multiplies by K^2 = O(theta^2)."""
    gen = torch.Generator().manual_seed(int(mag * 1e7) + 3)
    n_img, n_rays, hw = 6, 80, 50
    poses = torch.randn(n_img, 3, 4, generator=gen)
    directions = torch.randn(hw, 3, generator=gen)
    img = torch.randint(n_img - 1, (n_rays,), generator=gen)  # the last image has no ray
    pix = torch.randint(hw, (n_rays,), generator=gen)
    go, gd = torch.randn(n_rays, 3, generator=gen), torch.randn(n_rays, 3, generator=gen)
    ext = torch.zeros(6 * n_img, dtype=torch.float64)
    ext[:3 * n_img] = _vectors(mag, n_img, gen).reshape(-1)
    ext[3 * n_img:] = torch.randn(3 * n_img, generator=gen, dtype=torch.float64) * 0.1
    grad, _ = PR.pose_grad(go, gd, img, pix, directions, poses, ext)
    e = ext.clone().requires_grad_(True)
    o, d = PR.rays64(e, img, pix, directions, poses)
    (want,) = torch.autograd.grad((o * go.double()).sum() + (d * gd.double()).sum(), e)
    gR, wR = grad[:3 * n_img].view(n_img, 3), want[:3 * n_img].view(n_img, 3)
    gT, wT = grad[3 * n_img:6 * n_img].view(n_img, 3), want[3 * n_img:].view(n_img, 3)
    rel_R = float(((gR - wR).norm(dim=1) / wR.norm(dim=1).clamp_min(1e-300))[:-1].max())
    rel_T = float(((gT - wT).norm(dim=1) / wT.norm(dim=1).clamp_min(1e-300))[:-1].max())
    print(f"|v| = {mag:g}: closed form vs autograd, worst relative difference dR {rel_R:.2e} dT {rel_T:.2e}")
    assert float(wR[:-1].norm(dim=1).min()) > 0
    assert float(gR[-1].abs().sum()) == 0 and float(gT[-1].abs().sum()) == 0 and float(grad[6 * n_img:].abs().sum()) == 0
    assert rel_R <= 1e-12 and rel_T <= 1e-12
    o, d = PR.rays64(e, img, pix, directions, poses, literal=True)
    (lit,) = torch.autograd.grad((o * go.double()).sum() + (d * gd.double()).sum(), e)
    lR = lit[:3 * n_img].view(n_img, 3)
    rel_L = float(((gR - lR).norm(dim=1) / lR.norm(dim=1).clamp_min(1e-300))[:-1].max())
    print(f"|v| = {mag:g}: against the literal 1 - cos copy {rel_L:.2e}")
    assert rel_L <= 1e-12 + 4 * 2.0 ** -52 / (mag + PR.GUARD)
    # compose is the same function the rays were formed from
    eff, _ = PR.compose(poses, ext)
    assert float((eff[:, :, :3] - PR.axisangle_to_R64(ext[:3 * n_img].view(n_img, 3)) @ poses.double()[:, :, :3])
                 .abs().max()) <= 1e-12
    assert torch.equal(eff[:, :, 3], poses.double()[:, :, 3] + ext[3 * n_img:].view(n_img, 3))


def test_compose_identity_at_zero():
    gen = torch.Generator().manual_seed(1)
    poses = torch.randn(5, 3, 4, generator=gen)
    eff, mag = PR.compose(poses, torch.zeros(32))
    # theta = 1e-7 at v = 0 and K = 0: Rod = I exactly
    assert torch.equal(eff, poses.double())
    assert torch.equal(mag[:, :, :3], poses.double()[:, :, :3].abs())


def test_coefficient_series_meet_closed_forms():
    """The restatement's own A', B': series below 0.5, closed forms above; both written out at 0.5 agree to
    fp64 rounding times the closed forms' cancellation there (3 / theta^2 = 12)."""
    th = torch.tensor([0.5 - 1e-9, 0.5 + 1e-9], dtype=torch.float64)
    _, _, dA, dB = PR.coefficients(th)
    assert abs(float(dA[0] - dA[1])) <= 1e-9 and abs(float(dB[0] - dB[1])) <= 1e-9
    assert abs(float(dA[0]) - (-0.5 / 3 + 0.125 / 30)) <= 1e-4 and abs(float(dB[0]) - (-0.5 / 12 + 0.125 / 180)) <= 1e-5


# ---------------------------------------------------------------------- C-ABI
def test_pose_entry_points_exported_and_guard_arguments():
    L = ctypes.CDLL(vren.LIB_PATH)
    for name in ("ngp_pose_compose", "ngp_pose_grad", "ngp_pose_rod_coefficients", "ngp_field_input_grad_pm"):
        assert hasattr(L, name), name
    V = vren.lib()
    z, one = None, ctypes.c_void_p(16)  # (never dereferenced: every call below returns before a launch)
    assert V.ngp_pose_compose(z, one, 4, one, z) == -1
    assert V.ngp_pose_compose(one, z, 4, one, z) == -1
    assert V.ngp_pose_compose(one, one, 4, z, z) == -1
    assert V.ngp_pose_compose(one, one, -1, one, z) == -1
    assert V.ngp_pose_compose(one, one, 0, one, z) == 0  # no image: a no-op
    ok = [one, one, one, one, 8, one, one, one, 4, one, z]
    for i in (0, 1, 2, 3, 5, 6, 7, 9):  # every pointer null in turn
        a = list(ok)
        a[i] = z
        assert V.ngp_pose_grad(*a) == -1, i
    a = list(ok); a[4] = -1
    assert V.ngp_pose_grad(*a) == -1
    a = list(ok); a[8] = -1
    assert V.ngp_pose_grad(*a) == -1
    a = list(ok); a[8] = 0
    assert V.ngp_pose_grad(*a) == 0
    assert V.ngp_pose_rod_coefficients(z, 4, one, z) == -1 and V.ngp_pose_rod_coefficients(one, 4, z, z) == -1
    assert V.ngp_pose_rod_coefficients(one, -1, one, z) == -1 and V.ngp_pose_rod_coefficients(one, 0, one, z) == 0
    # the pair-major entry takes a pair-major stride only ((n,32) rows are ngp_field_input_grad's)
    import hashgrid as HG
    H = HG._lib()
    g = ctypes.byref(HG.HashGrid(0.5).desc)
    assert H.ngp_field_input_grad_pm(one, z, 4, z, z, g, one, z, z, 0, z, one, 0, one, z, z) == -1
    assert H.ngp_field_input_grad_pm(one, z, 4, z, z, g, one, z, z, -8, z, one, 0, one, z, z) == -1
    assert H.ngp_field_input_grad_pm(z, z, 0, z, z, g, z, z, z, 8, z, z, 0, z, z, z) == 0  # n = 0: a no-op
    assert H.ngp_field_input_grad_pm(z, z, 4, z, z, g, z, z, z, 8, z, z, 0, z, z, z) == -1  # null pointers


def test_optimize_ext_refuses_a_world_above_one():
    """The pose gradient is not reduced across ranks: the constructor says so before it allocates anything
    (emulate_dp: the trainer's emulated-world knob)."""
    from trainer import NGPTrainer
    with pytest.raises(NotImplementedError):
        NGPTrainer(device="cpu", optimize_ext=True, emulate_dp=2)
