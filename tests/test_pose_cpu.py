"""Pose refinement, the parts that need no GPU: datasets.ray_utils.axisangle_to_R
against the reference function's recorded outputs (tests/golden/axisangle.npz,
tests/golden/make_axisangle_golden.py), pose_refine.PoseRefiner's ray
generation and parameter layout, the argument guards of the two new entry
points, and the soundness of the fp64 restatement the GPU tests hold the
input-gradient kernels to (tests/input_grad_ref.py) against the oracle's
forward."""
import ctypes
import os

import numpy as np
import pytest
import torch

import hashgrid as HG
import input_grad_ref as R
import oracle as O
import vren
from datasets.ray_utils import axisangle_to_R, get_rays
from pose_refine import PoseRefiner

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "axisangle.npz")


# ------------------------------------------------------------ axisangle_to_R
def test_axisangle_matches_reference_golden():
    g = np.load(GOLD)
    v, M = torch.from_numpy(g["v"]), torch.from_numpy(g["M"])
    norms = v.norm(dim=1)
    assert float(norms[8]) == 0 and 0 < float(norms[9]) < 2e-8 and float(norms[10]) > 3.14  # the fixture's edge rows
    vg = v.clone().requires_grad_(True)
    Rb = axisangle_to_R(vg)
    assert Rb.shape == (12, 3, 3) and Rb.dtype == torch.float32
    assert float((Rb.detach() - torch.from_numpy(g["R"])).abs().max()) <= 1e-6
    (grad,) = torch.autograd.grad((Rb * M).sum(), vg)
    assert float((grad - torch.from_numpy(g["grad"])).abs().max()) <= 1e-6
    for i in range(len(v)):  # (3) -> (3,3)
        Ri = axisangle_to_R(v[i])
        assert Ri.shape == (3, 3)
        assert float((Ri - torch.from_numpy(g["R_single"][i])).abs().max()) <= 1e-6
    eye = torch.eye(3).expand(12, 3, 3)
    assert float((Rb.detach() @ Rb.detach().transpose(1, 2) - eye).abs().max()) <= 1e-6


def test_axisangle_zero_gradient_finite_and_fp32_under_autocast():
    v = torch.zeros(3, requires_grad=True)
    Rm = axisangle_to_R(v)
    assert torch.equal(Rm.detach(), torch.eye(3))
    (gr,) = torch.autograd.grad((Rm * torch.arange(9.0).view(3, 3)).sum(), v)
    assert torch.isfinite(gr).all()
    # d R / d v at 0 is the skew generator: sum(R * M) -> (M21 - M12, M02 - M20, M10 - M01)
    assert torch.allclose(gr, torch.tensor([7.0 - 5.0, 2.0 - 6.0, 3.0 - 1.0]), atol=1e-6)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert axisangle_to_R(torch.randn(4, 3).bfloat16()).dtype == torch.float32


def test_get_rays_differentiable_in_c2w():
    g = torch.Generator().manual_seed(0)
    dirs = torch.randn(7, 3, generator=g)
    c2w = torch.randn(7, 3, 4, generator=g, dtype=torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda c: get_rays(dirs.double(), c), (c2w,))
    one = torch.randn(3, 4, generator=g, dtype=torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda c: get_rays(dirs.double(), c), (one,))


# --------------------------------------------------------------- PoseRefiner
@pytest.mark.parametrize("n_img", [1, 3, 10])
def test_pose_refiner_identity_rays_and_layout(n_img):
    g = torch.Generator().manual_seed(n_img)
    poses = torch.randn(n_img, 3, 4, generator=g)
    directions = torch.randn(50, 3, generator=g)
    img = torch.randint(n_img, (64,), generator=g)
    pix = torch.randint(50, (64,), generator=g)
    pr = PoseRefiner(n_img, device="cpu")
    assert pr.ext.numel() % 4 == 0 and pr.ext.numel() >= 6 * n_img
    assert [n for n, _ in pr.named_parameters()] == ["ext"]
    assert pr.dR.shape == (n_img, 3) and pr.dT.shape == (n_img, 3)
    assert float(pr.ext.detach().abs().max()) == 0
    keep = poses.clone()
    o, d = pr.rays(img, pix, directions, poses)
    o0, d0 = get_rays(directions[pix], poses[img])
    assert torch.equal(o, o0) and torch.equal(d, d0)
    assert torch.equal(poses, keep), "poses modified in place"
    # views of the one parameter: a gradient reaches ext through both, in the rows of the batch's images only
    (o.sum() + (d * d).sum()).backward()
    gR = pr.ext.grad[:3 * n_img].view(n_img, 3)
    gT = pr.ext.grad[3 * n_img:6 * n_img].view(n_img, 3)
    seen = torch.zeros(n_img, dtype=torch.bool)
    seen[img] = True
    assert (gT[seen].abs().sum(1) > 0).all() and float(gT[~seen].abs().sum()) == 0
    assert float(gR[~seen].abs().sum()) == 0 and float(pr.ext.grad[6 * n_img:].abs().sum()) == 0
    # the reference's checkpoint keys, and a non-zero correction moves the poses (train.py:92-95)
    sd = pr.state_dict_reference()
    assert set(sd) == {"dR", "dT"}
    sd["dR"] = torch.randn(n_img, 3, generator=g) * 0.1
    sd["dT"] = torch.randn(n_img, 3, generator=g) * 0.1
    pr.load_reference(sd)
    want = torch.cat([axisangle_to_R(sd["dR"]) @ poses[..., :3], (poses[..., 3] + sd["dT"])[..., None]], -1)
    assert torch.allclose(pr.refined_poses(poses), want, atol=1e-6)
    assert torch.equal(poses, keep)


# ------------------------------------------------------------ argument guards
def test_new_entry_points_guard_arguments():
    L = HG._lib()
    grid = HG.HashGrid(0.5)
    g, z = ctypes.byref(grid.desc), None
    one = ctypes.c_void_p(16)  # (never dereferenced: every call below returns before a launch)
    for act in (-1, 4):
        assert L.ngp_field_input_grad(z, z, 0, z, z, g, z, z, z, z, z, act, z, z, z) == -1
    assert L.ngp_field_input_grad(z, z, 0, z, z, g, z, z, z, z, z, 0, z, z, z) == 0  # n = 0: a no-op
    assert L.ngp_field_input_grad(z, z, -1, z, z, g, z, z, z, z, z, 0, z, z, z) == -1
    assert L.ngp_field_input_grad(z, z, 4, z, z, g, z, z, z, z, z, 0, z, z, z) == -1  # null pointers
    assert L.ngp_field_input_grad(z, z, 4, z, z, z, z, z, z, z, z, 0, z, z, z) == -2  # no grid
    # dL_ddirs given: dirs / mlp / enc / dL_drgbs become mandatory
    assert L.ngp_field_input_grad(one, z, 4, z, z, g, one, z, z, z, one, 0, one, one, z) == -1
    V = vren.lib()
    assert V.ngp_ray_segment_sum(z, z, z, 0, z, 0, z, z, z) == 0
    assert V.ngp_ray_segment_sum(z, z, z, 0, z, -1, z, z, z) == -1
    assert V.ngp_ray_segment_sum(z, z, z, 8, z, 4, z, z, z) == -1


# ------------------------------------------------- the fp64 restatement itself
@pytest.fixture(scope="module")
def field():
    f = O.OracleNGPField(scale=0.5, table_init=0.5)
    nd = f.n_dens
    flat = torch.cat([f.xyz_params.detach()[:nd], f.rgb_params.detach(), f.xyz_params.detach()[nd:]])
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(1024, 3, generator=g) * 2 - 1) * 0.45
    d = torch.randn(1024, 3, generator=g)
    return f, R.FieldRef64(flat), x, d


def test_restatement_encoding_matches_oracle(field):
    f, ref, x, _ = field
    enc64 = ref.encode(x.double())
    exact = ref.enc_exact(x)
    # the oracle's fp16 value is the rounding of an fp32 accumulation of the same 8 products: within half
    # an fp16 ulp of the fp64 sum, plus the fp32 sum's own error (8 fmaf: 8 u sum |w t|, and u per weight)
    idx, p32, _ = ref.cell(x)
    pos = p32.double() - torch.floor(p32.double())
    mag = (ref.corner_weights(pos)[..., None] * ref.table[idx].abs()).sum(2).reshape(len(x), -1)
    assert bool(((enc64 - exact).abs() <= 0.5 * R.ulp16(exact) * (1 + 2.0 ** -10) + 12 * R.U * mag).all())
    same = enc64.half() == exact.half()
    assert float(same.double().mean()) >= 0.999


def test_restatement_forward_matches_oracle(field):
    """The restatement's forward against the oracle's, layer by layer, inside oracle.mlp_forward_bound: the
    bound on two implementations with the same fp16 storage points that accumulate each dot product
    differently (here fp64 against the oracle's fp32 GEMM), an fp16 ulp where a sum straddles a rounding."""
    f, ref, x, d = field
    sig, rgb, det = ref.forward(x.double(), d.double(), HG.RGB_SIGMOID, detail=True)
    with torch.no_grad():
        sig_o, rgb_o = f(x, d)
        enc16 = O.hash_encode_fwd(f.spec, x, f.xyz_min, f.xyz_max, f.xyz_params[f.n_dens:])
        Wd, _ = O.mlp_layers(f.xyz_params[:f.n_dens], f.dens_dims)
        h_o, d_h = O.mlp_forward_bound(enc16, Wd)
        sh_o = O.sh4(d).float()
        Wc, _ = O.mlp_layers(f.rgb_params, f.color_dims)
        d_sh = R.ulp16(sh_o.double()).float()  # an fp64 and an fp32 polynomial, each rounded to fp16
        o_o, d_o = O.mlp_forward_bound(torch.cat([sh_o, h_o], 1), Wc, d_in=torch.cat([d_sh, d_h], 1))
    assert bool(((det["h"].float() - h_o).abs() <= d_h).all())
    assert bool(((det["sh"].float() - sh_o).abs() <= d_sh).all())
    assert bool(((det["o"].float() - o_o[:, :3]).abs() <= d_o[:, :3]).all())
    # sigma = exp(h0): h0 within d_h, expf within 2 ulp; rgb = fp16(sigmoid(o)): sigmoid is 1/4-Lipschitz
    assert bool(((sig.float() / sig_o).log().abs() <= d_h[:, 0] + 8 * R.U).all())
    assert bool(((rgb.float() - rgb_o).abs() <= d_o[:, :3] / 4 + 2.0 ** -11).all())
    assert float((rgb.float() == rgb_o).float().mean()) >= 0.9  # (and mostly the same fp16 value)


def test_restatement_gradients_match_central_differences(field):
    """autograd of the restatement against fp64 central differences of its own straight-through-free
    smooth part: the encoding path (position) and the SH path (direction) on a linear readout."""
    _, ref, x, d = field
    x, d = x[:64], d[:64]
    g = torch.Generator().manual_seed(5)
    denc = torch.randn(64, 32, generator=g)
    tot, mag = ref.position_terms(x, denc)
    xg = x.double().requires_grad_(True)
    (ga,) = torch.autograd.grad((ref.encode(xg) * denc.double()).sum(), xg)
    assert bool(((ga - tot).abs() <= 64 * 2.0 ** -53 * mag + 1e-300).all())  # the same 256 terms, fp64 both ways
    u = lambda t: t / t.norm(dim=1, keepdim=True)  # noqa: E731
    w = torch.randn(16, generator=g).double()
    dg = d.double().requires_grad_(True)
    (gd,) = torch.autograd.grad((R.sh4_poly(u(dg)) @ w).sum(), dg)
    eps = 1e-6
    for k in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[k] = eps
        num = ((R.sh4_poly(u(d.double() + e)) - R.sh4_poly(u(d.double() - e))) @ w) / (2 * eps)
        assert float((num - gd[:, k]).abs().max()) <= 1e-7 * (1 + float(gd.abs().max()))
    assert float((gd * d.double()).sum(1).abs().max()) <= 1e-12 * float(gd.abs().max() * d.norm(dim=1).max())


def test_segment_sums_reference():
    g = torch.Generator().manual_seed(2)
    rays_a = torch.tensor([[0, 0, 3], [1, 3, 0], [2, 3, 5]])
    gx, gd, ts = torch.randn(8, 3, generator=g), torch.randn(8, 3, generator=g), torch.rand(8, generator=g)
    do, dd, ao, ad = R.segment_sums64(gx, gd, ts, rays_a, 3)
    assert torch.allclose(do[0], gx[:3].double().sum(0)) and float(do[1].abs().sum()) == 0
    assert torch.allclose(dd[2], (ts[3:, None].double() * gx[3:].double() + gd[3:].double()).sum(0))
    assert bool((ao >= do.abs()).all() and (ad >= dd.abs() - 1e-12).all())
