"""The SG light probes on the device (csrc/sgfit.hip, sg_probe.py,
probes.sg_probe) against the golden fixture of the reference's own
insert/envfit.py and insert/render_utils.py (tests/golden/sg_probe.npz).

The bars are those of test_sg_probe_ref_cpu.py (its docstring states them):
4 x the reference's own fp32 deviation from its fp64 run over three orders of
pixels and lights -- per checkpoint and kind of parameter for the trajectories,
per parameter with the floor 2^-24 A_p for the gradient, per case for the
lookups.  The kernels keep their sums in fp64 in one fixed order and use the
device's expf.
"""
import numpy as np
import pytest
import torch

import probes
import sg_probe
import shading
import sg_probe_ref as PR
import vren
from fixture_model import load
from test_golden_gpu import _product_model
from test_sg_probe_ref_cpu import (CASES, LOOK_RES, assert_gradient, assert_trajectory, case, name_of,
                                   run_checkpoints)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def fx():
    return load("sg_probe")


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _optim(c, n_iter=25, lr=0.1, params=None):
    opt = sg_probe.EnvOptim(len(c["init"]), N_iter=n_iter, lr=lr, device=DEV)
    opt.reset(torch.from_numpy(c["init"] if params is None else params))
    assert opt.lgtSGs.is_cuda and opt.lgtSGs.dtype == torch.float32
    return opt


# ------------------------------------------------------------------ lookups
@pytest.mark.parametrize("res", LOOK_RES)
def test_lookup_against_the_reference_fp64(fx, res):
    cm, d = _d(fx[f"cubemap{res}"]), _d(fx[f"look_dirs_r{res}"])
    out = sg_probe.cubemap_sample(cm, d, res)
    assert out.shape == (300, 3) and out.dtype == torch.float32 and out.is_cuda
    err, bar = np.abs(out.cpu().numpy().astype(np.float64) - fx[f"look64_r{res}"]).max(), 4 * fx[f"look_dev_r{res}"]
    print(f"lookup res {res}: max err {err:.2e}, bar {bar:.2e}")
    assert err <= bar
    none = torch.from_numpy(fx[f"look_face_r{res}"] == -1).to(DEV)
    assert bool((out[none] == 1).all())
    # a list of any length gives the bits of that prefix of the longest list
    for n in (1, 63, 64, 65, 257):
        assert torch.equal(sg_probe.cubemap_sample(cm, d[:n].contiguous(), res), out[:n]), n
    assert sg_probe.cubemap_sample(cm, d[:0], res).shape == (0, 3)


def test_env_maps(fx):
    e = sg_probe.cubemap2env_map(_d(fx["cubemap5"]), 5, 5, 8)
    assert e.shape == (5, 8, 3) and np.abs(e.cpu().numpy() - fx["env64_5x8"]).max() <= 4 * fx["env_dev_5x8"]
    ref = PR.cubemap_sample_ref(fx["cubemap32"], PR.env_dirs(128, 128), 32)[0].reshape(128, 128, 3)
    e = sg_probe.cubemap2env_map(_d(fx["cubemap32"]), 32, 128, 128)
    err = np.abs(e.cpu().numpy() - ref).max()
    print(f"128 x 128 env map: max err {err:.2e}, bar {4 * fx['env_dev_128']:.2e}")
    assert e.shape == (128, 128, 3) and err <= 4 * fx["env_dev_128"]
    H, W, L = CASES[3]
    got = sg_probe.SG2Envmap(_d(case(fx, H, W, L)["init"]), H, W)
    err = np.abs(got.cpu().numpy() - fx["sg_env64"]).max()
    print(f"SG2Envmap: max err {err:.2e}, bar {4 * fx['sg_env_dev']:.2e}")
    assert got.shape == (H, W, 3) and err <= 4 * fx["sg_env_dev"]


# ------------------------------------------------------------------ the fit
@pytest.mark.parametrize("H,W,L", CASES)
def test_gradient_and_loss_at_the_recorded_checkpoints(fx, H, W, L):
    c = case(fx, H, W, L)
    target = _d(c["target"])
    for gi in range(2):
        opt = _optim(c, n_iter=1, lr=0.0, params=c["gparams"][gi])   # lr 0: the gradient, no movement
        res = opt.eval(target)
        assert np.array_equal(res.cpu().numpy(), c["gparams"][gi]) and int(opt.step) == 1
        assert_gradient(c, gi, opt.last_grad.cpu().numpy(), opt.losses[0].item(), f"gpu {name_of(H, W, L)}")
        # the loss of SG2Envmap's own map (the same lights-ascending sum)
        env = sg_probe.SG2Envmap(opt.lgtSGs, H, W)
        mse = ((env - target).double() ** 2).mean().item()
        assert abs(mse - opt.losses[0].item()) <= 2.0 ** -22 * mse


@pytest.mark.parametrize("H,W,L", CASES)
def test_trajectory_at_every_recorded_iteration(fx, H, W, L):
    c = case(fx, H, W, L)
    target = _d(c["target"])
    opt = _optim(c)
    run_checkpoints(opt, target, c, f"gpu {name_of(H, W, L)}")       # 1+1+1+2+5+15 iterations, warm
    assert int(opt.step) == 25
    stepped = opt.lgtSGs.clone()
    # two runs are bit-equal; 25 at once = 10 then 15 = the checkpoint-wise run
    a = _optim(c)
    once = a.eval(target).clone()
    assert a.losses.shape == (25,) and torch.equal(once, stepped)
    b = _optim(c)
    b.N_iter = 10
    b.eval(target)
    first = b.losses.clone()
    b.N_iter = 15
    assert torch.equal(b.eval(target), once) and int(b.step) == 25
    assert torch.equal(torch.cat([first, b.losses]), a.losses)
    assert torch.equal(b.last_grad, a.last_grad) and torch.equal(b.exp_avg, a.exp_avg)
    assert torch.equal(b.exp_avg_sq, a.exp_avg_sq)
    # the fixed parameters stay bit-fixed
    fixed = torch.from_numpy(c["fixed"])
    assert torch.equal(once.cpu()[fixed], torch.from_numpy(c["init"])[fixed])
    assert bool((a.last_grad.cpu()[fixed] == 0).all())


def test_captured_graph_replays_the_iterations(fx):
    H, W, L = CASES[3]
    c = case(fx, H, W, L)
    target = _d(c["target"])
    eager = _optim(c, n_iter=10)
    want = eager.eval(target).clone()
    opt = _optim(c, n_iter=1)
    opt.eval(target)                                                  # warm: code loaded, the directions cached
    opt.reset(torch.from_numpy(c["init"]))                            # back to the start
    opt.N_iter = 10
    g = torch.cuda.CUDAGraph()
    with vren.graph_capture(g):                                       # (records the launches, runs nothing)
        opt.eval(target)
    assert int(opt.step) == 0
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(opt.lgtSGs, want) and int(opt.step) == 10
    assert torch.equal(opt.losses, eager.losses) and torch.equal(opt.last_grad, eager.last_grad)
    g.replay()                                                        # a second replay goes on: iterations 11 .. 20
    torch.cuda.synchronize()
    eager.eval(target)
    assert torch.equal(opt.lgtSGs, eager.lgtSGs) and int(opt.step) == 20 and torch.equal(opt.losses, eager.losses)


# ------------------------------------------------------------------ the probe
def test_sg_probe_is_the_composed_calls():
    ins = load("insert_frame")
    model = _product_model(ins)
    pt = torch.tensor([0.05, -0.1, 0.02])
    sh = torch.randn(9, 3, generator=torch.Generator().manual_seed(3)) * 0.2
    sh[0] += 1.0
    kw = dict(T_threshold=1e-2, max_samples=100)
    init = sg_probe.EnvOptim(generator=torch.Generator().manual_seed(7), device=DEV).lgtSGs.clone()
    opt = sg_probe.EnvOptim(device=DEV)
    opt.reset(init)
    out = probes.sg_probe(model, pt, opt, SH_bkg=sh, **kw)
    assert out["lSGs"].shape == (32, 7) and out["envmap"].shape == (128, 128, 3) and out["cubemap_rgb"].shape == (6144, 3)
    # composed: the cube-map rays through sh_probes, the lookup, the fit, trans_raw_sg
    rays = probes.sh_probes(model, pt.reshape(1, 3), dirs=probes.get_cubemap_rays(1, 32)[0], SH_bkg=sh,
                            probes_per_batch=1, return_rays=True, **kw)
    assert torch.equal(out["cubemap_rgb"], rays["rgb"][0])
    env = sg_probe.cubemap2env_map(rays["rgb"][0].contiguous(), 32, 128, 128)
    assert torch.equal(out["envmap"], env)
    ref = sg_probe.EnvOptim(device=DEV)
    ref.reset(init)
    raw = ref.eval(env)
    assert torch.equal(raw, opt.lgtSGs) and int(opt.step) == 25
    assert torch.equal(out["lSGs"], sg_probe.trans_raw_sg(raw.clone())) and not torch.equal(out["lSGs"], raw)
    l = out["lSGs"]
    assert bool(torch.isfinite(l).all()) and bool((l[:, 3:] >= 0).all())
    assert torch.allclose(l[:, :3].norm(dim=-1), torch.ones(32, device=DEV), atol=1e-5)
    assert float(opt.losses[-1]) < float(opt.losses[0])
    # the next placement starts warm
    probes.sg_probe(model, pt + 0.01, opt, SH_bkg=sh, **kw)
    assert int(opt.step) == 50
    # what it returns is what the object shade takes
    sg = load("sg_shade")
    H, W = int(sg["H"]), int(sg["W"])
    rgb = shading.sg_shade(H, W, _d(sg["directions"]), _d(sg["pose"]), tuple(int(v) for v in sg["bbox"]),
                           _d(sg["normals"]), _d(sg["obj_depth"]), l.contiguous())
    assert rgb.shape == (H, W, 3) and bool(torch.isfinite(rgb).all()) and float(rgb.max()) > 0


def test_argument_checks(fx):
    c = case(fx, 9, 14, 7)
    opt = _optim(c)
    target = _d(c["target"])
    for bad in (target[:, :, :2], target.reshape(-1, 3), target.transpose(0, 1), target.permute(2, 0, 1)):
        with pytest.raises(ValueError):
            opt.eval(bad)
    assert int(opt.step) == 0
    with pytest.raises(ValueError):
        sg_probe.cubemap_sample(_d(fx["cubemap5"]), _d(fx["look_dirs_r5"])[:, :2], 5)
    with pytest.raises(ValueError):
        sg_probe.cubemap_sample(_d(fx["cubemap5"]), _d(fx["look_dirs_r5"]).repeat(1, 2)[:, :3], 5)   # not contiguous
    with pytest.raises(ValueError):
        sg_probe.SG2Envmap(_d(c["init"])[:, :6], 4, 4)
    # an image of another dtype takes the torch formulation, on its device
    res = opt.eval(target.double())
    assert res.dtype == torch.float64 and res.is_cuda
    assert_trajectory(c, len(PR.CHECKPOINTS) - 1, res.cpu().numpy(), what="torch path on the device")
