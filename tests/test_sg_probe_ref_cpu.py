"""tests/sg_probe_ref.py (the per-pair fp64 restatement of the SG light probes),
sg_probe.sg_fit_torch (the torch formulation) and the CPU path of
sg_probe.EnvOptim held to tests/golden/sg_probe.npz, which the reference's own
insert/envfit.py and insert/render_utils.py produced in fp64 and fp32
(tests/golden/make_sg_probe_golden.py); what that fixture's designed inputs
must hold for the GPU tests to mean anything; and the new entry points'
declarations and argument checks.  No GPU.

Bars.  fp64 against fp64: 1e-9, relative to the largest value compared (the
gradient of a zero lobe is of order 1e6).  fp32, all absolute and 4 x the
reference's own fp32 deviation from its fp64 run (the maximum over three orders
of pixels and lights, mathematically one result):
  trajectories  per checkpoint and kind of parameter (params_dev); the loss
                4 max(loss_dev, 2^-24 loss);
  gradient      per parameter, 4 max(grad_dev_p, 2^-24 A_p), A_p the sum of the
                absolute per-pixel contributions (classes by size would hide the
                sharp lights' tiny gradients);
  lookups       4 look_dev / env_dev, per case.
Recorded deviations, 128 x 128 / L = 32 after 25 iterations: lobe 2.6e-3,
sharpness 1.8e-3, amplitude 1.2e-3; 17 x 31 / L = 33: 1.4e-5, 6.2e-5, 5.5e-6.
"""
import ctypes

import numpy as np
import pytest
import torch

import sg_probe_ref as PR
from capi import C as CONSTS, FUNCS
from fixture_model import load

CASES = ((9, 14, 1), (9, 14, 7), (16, 32, 32), (17, 31, 33), (128, 128, 32))
SMALL = CASES[:4]
LOOK_RES = (2, 5, 32)
FP64_BAR = 1e-9
ULP = 2.0 ** -24


def name_of(H, W, L):
    return f"h{H}x{W}_l{L}"


@pytest.fixture(scope="module")
def fx():
    return load("sg_probe")


def case(fx, H, W, L):
    n = name_of(H, W, L)
    return {k[len(n) + 1:]: v for k, v in fx.items() if k.startswith(n + "_")}


def assert_trajectory(c, ci, got, loss=None, what=""):
    """got (L,7) after iteration CHECKPOINTS[ci] against the fp64 run, per kind; the fixed entries bit-fixed"""
    got = np.asarray(got)
    assert np.isfinite(got).all(), what
    fixed = c["fixed"]
    assert np.array_equal(got[fixed], c["init"].astype(got.dtype)[fixed]), (what, "a fixed parameter moved")
    err = np.abs(got.astype(np.float64) - c["params64"][ci])
    for k, kind in enumerate(PR.KINDS):
        m = (PR.KIND_OF_COLUMN[None, :] == k) & ~fixed
        e, bar = err[m].max(), 4 * c["params_dev"][ci, k]
        print(f"{what} it {PR.CHECKPOINTS[ci]} {kind}: max err {e:.2e}, bar {bar:.2e}")
        assert e <= bar, (what, PR.CHECKPOINTS[ci], kind, e, bar)
    if loss is not None:
        e, bar = abs(float(loss) - c["loss64"][ci]), 4 * max(c["loss_dev"][ci], ULP * c["loss64"][ci])
        print(f"{what} it {PR.CHECKPOINTS[ci]} loss: err {e:.2e}, bar {bar:.2e}")
        assert e <= bar, (what, PR.CHECKPOINTS[ci], "loss", e, bar)


def assert_gradient(c, gi, grad, loss, what=""):
    grad = np.asarray(grad, dtype=np.float64)
    assert np.isfinite(grad).all(), what
    bar = 4 * np.maximum(c["grad_dev"][gi], ULP * c["A"][gi])
    err = np.abs(grad - c["grad64"][gi])
    worst = np.unravel_index(np.argmax(err - bar), err.shape)
    print(f"{what} gradient at it {PR.GRAD_CHECKPOINTS[gi]}: worst entry {worst}: err {err[worst]:.2e}, bar {bar[worst]:.2e}; "
          f"max err / bar {np.max(err[bar > 0] / bar[bar > 0]):.3f}")
    assert np.all(err <= bar), (what, worst, err[worst], bar[worst])
    assert np.all(grad[c["fixed"]] == 0)
    e, lbar = abs(float(loss) - c["gloss64"][gi]), 4 * max(c["gloss_dev"][gi], ULP * c["gloss64"][gi])
    print(f"{what} loss: err {e:.2e}, bar {lbar:.2e}")
    assert e <= lbar, (what, "loss", e, lbar)


def run_checkpoints(opt, target, c, what):
    """eval by eval to every checkpoint (the warm state carries over): each inside its bar"""
    done = 0
    for ci, it in enumerate(PR.CHECKPOINTS):
        opt.N_iter = it - done
        res = opt.eval(target)
        done = it
        assert res.shape == c["init"].shape
        assert_trajectory(c, ci, res.detach().cpu().numpy(), opt.losses[-1].item(), what)


# ------------------------------------------------------------------ the fixture
def test_fixture_is_the_designed_one(fx):
    assert [tuple(r) for r in fx["cases"]] == list(CASES)
    assert tuple(fx["checkpoints"]) == PR.CHECKPOINTS and tuple(fx["grad_checkpoints"]) == PR.GRAD_CHECKPOINTS
    for H, W, L in CASES:
        c = case(fx, H, W, L)
        assert c["init"].shape == (L, 7) and c["init"].dtype == np.float32
        assert c["target"].shape == (H, W, 3) and c["target"].dtype == np.float32 and c["target"].min() >= 0
        assert c["params64"].shape == (6, L, 7) and c["grad64"].shape == c["A"].shape == (2, L, 7)
        assert np.array_equal(c["gparams"][0], c["init"])
        assert np.all(c["params_dev"] > 0) and np.all(c["loss64"] > 0) and c["loss64"][-1] < c["loss64"][0]
        assert np.all(c["A"] >= np.abs(c["grad64"]) * (1 - 1e-9))
        assert c["target"].max() >= 40                                # an HDR peak
        if (H, W) == (128, 128):
            assert not c["fixed"].any()
            continue
        t = c["target"]
        assert np.all(t[H // 2] == 0) and np.count_nonzero(t == 40) == 3
        x, fixed = c["init"], c["fixed"]
        if L < 7:
            assert not fixed.any()
            continue
        assert x[1, 3] == 0 and x[2, 3] < 0 and np.all(x[2, 4:] < 0) and x[3, 5] == 0 and np.all(x[3, [4, 6]] != 0)
        assert np.all(x[4, :3] == 0) and 290 < x[5, 3] < 310 and np.all(x[0] != 0) and np.all(x[6] != 0)
        want = np.zeros((L, 7), dtype=bool)
        want[1, :4], want[3, 5] = True, True
        assert np.array_equal(fixed, want)
        # most pairs of the sharp light underflow in fp32, some do not
        a = x[5, :3].astype(np.float64) / np.linalg.norm(x[5, :3].astype(np.float64))
        e = np.exp(np.float32(x[5, 3]) * (PR.env_dirs(H, W).astype(np.float64) @ a - 1)).astype(np.float32)
        assert (e == 0).mean() > 0.5 and (e > 1e-3).sum() >= 1
        # the zero lobe moves (da / eps), the fixed entries do not, in the fp64 run
        assert np.all(c["params64"][0][4, :3] != 0) and np.all(np.abs(c["grad64"][0][4, :3]) > 1e3)
        for ci in range(6):
            assert np.array_equal(c["params64"][ci][fixed], x.astype(np.float64)[fixed])
        assert np.all(c["grad64"][:, fixed] == 0) and np.all(c["A"][:, fixed] == 0)
    assert sum(H * W < CONSTS["NGP_SG_FIT_BLOCK_PIXELS"] * 2 for H, W, _ in CASES) == 2          # less than two blocks
    assert (16 * 32) % CONSTS["NGP_SG_FIT_BLOCK_PIXELS"] == 0 and (17 * 31) % CONSTS["NGP_SG_FIT_BLOCK_PIXELS"] != 0
    assert CONSTS["NGP_SG_LIGHT_TILE"] == 64 and CONSTS["NGP_SSDF_LIGHT_TILE"] + 1 == 33
    for res in LOOK_RES:
        d, face = fx[f"look_dirs_r{res}"], fx[f"look_face_r{res}"]
        assert d.shape == (300, 3) and d.dtype == np.float32 and fx[f"cubemap{res}"].shape == (6 * res * res, 3)
        assert set(face.tolist()) == {-1, 0, 1, 2, 3, 4, 5} and (face == -1).sum() == 2
        a = np.abs(d)
        top = a.max(1)
        ties = (a == top[:, None]).sum(1)
        assert ((ties == 2) & (top > 0)).sum() >= 12 and ((ties == 3) & (top > 0)).sum() >= 5
        # ties go to the lowest axis: +x/-x (faces 2, 3) whenever x is among the largest, else y (4, 5)
        for i in np.nonzero((ties >= 2) & (top > 0))[0]:
            axis = int(np.argmax(a[i] == top[i]))
            assert face[i] == PR.SEL_MAP[axis] + (1 if d[i, axis] < 0 else 0), (i, d[i], face[i])
        assert np.any(np.signbit(d) & (d == 0)) and np.any(~np.signbit(d) & (d == 0))
        q = a / np.where(top > 0, top, 1)[:, None]
        edge = np.sort(q, 1)[:, 1]                                    # the larger of (|u|, |v|)
        assert ((edge > 1 - 1.0 / res) & (edge < 1)).sum() >= 20      # within half a texel of an edge
        assert fx[f"look_dev_r{res}"] > 0
    assert fx["env64_5x8"].shape == (5, 8, 3) and fx["env_dev_5x8"] > 0 and fx["env_dev_128"] > 0


# ------------------------------------------------------------------ fp64 against fp64
@pytest.mark.parametrize("res", LOOK_RES)
def test_lookup_restatement_and_torch_formulation_fp64(fx, res):
    import sg_probe
    cm, d = fx[f"cubemap{res}"], fx[f"look_dirs_r{res}"]
    ref = fx[f"look64_r{res}"]
    scale = np.abs(ref).max()
    mine, face = PR.cubemap_sample_ref(cm, d, res)
    assert np.array_equal(face, fx[f"look_face_r{res}"]) and np.abs(mine - ref).max() <= FP64_BAR * scale
    got = sg_probe.cubemap_sample(torch.from_numpy(cm).double(), torch.from_numpy(d).double(), res)
    assert got.dtype == torch.float64 and np.abs(got.numpy() - ref).max() <= FP64_BAR * scale
    got32 = sg_probe.cubemap_sample(torch.from_numpy(cm), torch.from_numpy(d), res)
    assert got32.dtype == torch.float32 and np.abs(got32.numpy() - ref).max() <= 4 * fx[f"look_dev_r{res}"]
    assert np.all(ref[face == -1] == 1)
    # a swapped (u, v) or a wrong face order is orders above the bar
    bar = 4 * fx[f"look_dev_r{res}"]
    swapped = PR.cubemap_sample_ref(cm, d, res, swap_uv=True)[0]
    order = PR.cubemap_sample_ref(cm, d, res, face_order=(2, 3, 4, 5, 0, 1))[0]
    assert np.abs(swapped - ref).max() > 1e3 * bar and np.abs(order - ref).max() > 1e3 * bar


def test_env_maps_fp64(fx):
    import sg_probe
    e = sg_probe.cubemap2env_map(torch.from_numpy(fx["cubemap5"]).double(), 5, 5, 8)
    assert e.shape == (5, 8, 3) and np.abs(e.numpy() - fx["env64_5x8"]).max() <= FP64_BAR
    e32 = sg_probe.cubemap2env_map(torch.from_numpy(fx["cubemap5"]), 5, 5, 8)
    assert e32.dtype == torch.float32 and np.abs(e32.numpy() - fx["env64_5x8"]).max() <= 4 * fx["env_dev_5x8"]
    assert np.array_equal(sg_probe.env_dirs(5, 8).numpy(), PR.env_dirs(5, 8))
    assert sg_probe.env_dirs(5, 8) is sg_probe.env_dirs(5, 8)          # cached
    # the 128 x 128 map: the fit's target is the reference's fp32 result; the restatement gives the fp64 one
    c = case(fx, 128, 128, 32)
    ref = PR.cubemap_sample_ref(fx["cubemap32"], PR.env_dirs(128, 128), 32)[0].reshape(128, 128, 3)
    assert np.abs(c["target"] - ref).max() <= fx["env_dev_128"]
    mine = sg_probe.cubemap2env_map(torch.from_numpy(fx["cubemap32"]), 32, 128, 128)
    assert np.abs(mine.numpy() - ref).max() <= 4 * fx["env_dev_128"]
    # SG2Envmap
    H, W, L = CASES[3]
    lights = torch.from_numpy(case(fx, H, W, L)["init"])
    scale = np.abs(fx["sg_env64"]).max()
    assert np.abs(PR.sg_envmap_ref(lights.numpy(), PR.env_dirs(H, W)).reshape(H, W, 3) - fx["sg_env64"]).max() <= FP64_BAR * scale
    assert np.abs(sg_probe.SG2Envmap(lights.double(), H, W).numpy() - fx["sg_env64"]).max() <= FP64_BAR * scale
    assert np.abs(sg_probe.SG2Envmap(lights, H, W).numpy() - fx["sg_env64"]).max() <= 4 * fx["sg_env_dev"]


@pytest.mark.parametrize("H,W,L", CASES)
def test_gradient_restatement_fp64(fx, H, W, L):
    c = case(fx, H, W, L)
    for gi in range(2):
        loss, grad, A = PR.sg_grad_ref(c["gparams"][gi], PR.env_dirs(H, W), c["target"])
        scale = np.abs(c["grad64"][gi]).max()
        assert np.abs(grad - c["grad64"][gi]).max() <= FP64_BAR * scale
        assert abs(loss - c["gloss64"][gi]) <= FP64_BAR * c["gloss64"][gi]
        assert np.abs(A - c["A"][gi]).max() <= FP64_BAR * np.abs(c["A"][gi]).max()


@pytest.mark.parametrize("H,W,L", SMALL)
def test_trajectories_fp64(fx, H, W, L):
    """sg_probe_ref's Adam and sg_fit_torch in fp64 against the reference's fp64 run (the 128 x 128 trajectory
    is left to the fp32 tests: seconds of numpy loops)"""
    import sg_probe
    c = case(fx, H, W, L)
    dirs = PR.env_dirs(H, W)
    mine = PR.sg_fit_ref(c["init"], dirs, c["target"])
    p = torch.from_numpy(c["init"]).double().requires_grad_(True)
    opt, done, losses = None, 0, []
    for ci, it in enumerate(PR.CHECKPOINTS):
        _, opt = sg_probe.sg_fit_torch(p, torch.from_numpy(c["target"]).double(), torch.from_numpy(dirs).double(),
                                       it - done, optimizer=opt, losses=losses)
        done = it
        scale = np.abs(c["params64"][ci]).max()
        assert np.abs(mine["params"][it] - c["params64"][ci]).max() <= FP64_BAR * scale, it
        assert np.abs(p.detach().numpy() - c["params64"][ci]).max() <= FP64_BAR * scale, it
        assert abs(mine["loss"][it] - c["loss64"][ci]) <= FP64_BAR * c["loss64"][ci]
        assert abs(float(losses[-1]) - c["loss64"][ci]) <= FP64_BAR * c["loss64"][ci]


# ------------------------------------------------------------------ fp32 within the bars
@pytest.mark.parametrize("H,W,L", CASES)
def test_torch_formulation_and_cpu_path_fp32(fx, H, W, L):
    import sg_probe
    c = case(fx, H, W, L)
    target = torch.from_numpy(c["target"])
    opt = sg_probe.EnvOptim(L, N_iter=25)
    assert opt.lgtSGs.shape == (L, 7) and opt.N_iter == 25 and opt.device.type == "cpu"
    for gi in range(2):                                               # the gradient where it is recorded: lr 0
        opt.reset(torch.from_numpy(c["gparams"][gi]))
        opt.N_iter, opt.lr = 1, 0.0
        res = opt.eval(target)
        assert np.array_equal(res.numpy(), c["gparams"][gi])
        assert_gradient(c, gi, opt.last_grad.numpy(), opt.losses[0].item(), f"cpu {name_of(H, W, L)}")
    opt.reset(torch.from_numpy(c["init"]))
    opt.lr = 0.1
    run_checkpoints(opt, target, c, f"cpu {name_of(H, W, L)}")
    assert opt.lgtSGs.dtype == torch.float32
    if (H, W) != (128, 128):                                          # sg_fit_torch alone, in one call
        p = torch.from_numpy(c["init"]).clone().requires_grad_(True)
        res, _ = sg_probe.sg_fit_torch(p, target, torch.from_numpy(PR.env_dirs(H, W)), 25)
        assert torch.equal(res, opt.lgtSGs)


def test_envoptim_surface():
    import sg_probe
    g = torch.Generator().manual_seed(5)
    a = sg_probe.EnvOptim(generator=g)
    want = torch.randn(32, 7, generator=torch.Generator().manual_seed(5))
    want[..., 3:4] *= 100.
    assert a.numLgtSGs == 32 and a.N_iter == 25 and a.lr == 0.1 and torch.equal(a.lgtSGs, want)
    im = torch.rand(6, 9, 3, generator=g)
    a.N_iter = 3
    r1 = a.eval(im).clone()
    assert a.losses.shape == (3,) and a.last_grad.shape == (32, 7) and int(a._torch[1].state_dict()["state"][0]["step"]) == 3
    a.N_iter = 0
    assert torch.equal(a.eval(im), r1) and a.losses.shape == (0,)
    # trans_raw_sg works in place and returns its argument; parse_raw_sg does not touch it
    raw = r1.clone()
    lobes, lam, mu = sg_probe.parse_raw_sg(raw)
    assert torch.equal(raw, r1) and lobes.shape == (32, 3) and lam.shape == (32, 1) and mu.shape == (32, 3)
    out = sg_probe.trans_raw_sg(raw)
    assert out is raw and torch.equal(raw[:, :3], lobes) and torch.equal(raw[:, 3:4], lam) and torch.equal(raw[:, 4:], mu)
    assert torch.allclose(raw[:, :3].norm(dim=-1), torch.ones(32), atol=1e-6) and bool((raw[:, 3:] >= 0).all())
    for bad in (dict(numLgtSGs=0), dict(numLgtSGs=129)):
        with pytest.raises(ValueError):
            sg_probe.EnvOptim(**bad)
    for bad in (torch.rand(6, 9), torch.rand(6, 9, 4), torch.zeros(6, 9, 3, dtype=torch.int32), None):
        with pytest.raises(ValueError):
            a.eval(bad)
    a.N_iter = -1
    with pytest.raises(ValueError):
        a.eval(im)
    cm = torch.rand(24, 3)
    with pytest.raises(ValueError):
        sg_probe.cubemap_sample(cm, torch.rand(4, 3), 2, rough=torch.rand(4, 1))
    with pytest.raises(ValueError):
        sg_probe.cubemap_sample(cm, torch.rand(4, 3), 2, blur_cm=True)
    with pytest.raises(ValueError):
        sg_probe.cubemap_sample(cm, torch.rand(4, 3), 3)
    with pytest.raises(ValueError):
        sg_probe.cubemap_sample(cm, torch.rand(4, 2), 2)
    with pytest.raises(ValueError):
        sg_probe.SG2Envmap(torch.rand(3, 6), 4, 4)
    with pytest.raises(ValueError):
        sg_probe.SG2Envmap(torch.rand(3, 7), 4, 4, upper_hemi=True)


# ------------------------------------------------------------------ the C ABI
def test_header_declares_the_entry_points():
    want = {"ngp_cubemap_sample": 6, "ngp_sg_envmap": 6, "ngp_sg_fit_workspace_bytes": 2, "ngp_sg_fit": 14}
    for name, n in want.items():
        assert name in FUNCS and len(FUNCS[name][1]) == n, name
        assert FUNCS[name][0] is (ctypes.c_int64 if name.endswith("bytes") else ctypes.c_int)
    assert CONSTS["NGP_SG_FIT_MAX_LIGHTS"] == 128 and CONSTS["NGP_SG_FIT_BLOCK_PIXELS"] == 64


def test_argument_errors_return_before_any_launch():
    """Host-side checks of the entry points (no GPU needed): NGP_EINVAL (-1); the workspace size: 0."""
    import vren
    lib = vren.lib()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails its checks first
    assert lib.ngp_sg_fit_workspace_bytes(128 * 128, 32) == 256 * 32 * 8 * 8
    assert lib.ngp_sg_fit_workspace_bytes(65, 1) == 2 * 8 * 8
    for P, L in ((0, 32), (-1, 32), (100, 0), (100, 129), ((1 << 24) + 1, 4)):
        assert lib.ngp_sg_fit_workspace_bytes(P, L) == 0, (P, L)

    def look(cm=p, res=4, dirs=p, n=5, out=p):
        return lib.ngp_cubemap_sample(cm, res, dirs, n, out, None)
    for over in (dict(cm=None), dict(dirs=None), dict(out=None), dict(res=0), dict(res=-2), dict(n=-1)):
        assert look(**over) == -1, over
    assert look(n=0, dirs=None, out=None) == 0                        # no directions: a no-op

    def env(lights=p, L=3, dirs=p, P=10, out=p):
        return lib.ngp_sg_envmap(lights, L, dirs, P, out, None)
    for over in (dict(lights=None), dict(dirs=None), dict(out=None), dict(L=0), dict(L=129), dict(P=0)):
        assert env(**over) == -1, over

    names = ("lights", "dirs", "target", "m", "v", "step", "ws", "grad", "losses")

    def fit(L=3, P=10, n_iter=2, **ptr):
        a = {k: ptr.get(k, p) for k in names}
        return lib.ngp_sg_fit(a["lights"], L, a["dirs"], a["target"], P, n_iter, ctypes.c_float(0.1), a["m"], a["v"],
                              a["step"], a["ws"], a["grad"], a["losses"], None)
    for k in names:
        assert fit(**{k: None}) == -1, k
    for over in (dict(L=0), dict(L=129), dict(P=0), dict(n_iter=-1), dict(ws=ctypes.c_void_p(260))):
        assert fit(**over) == -1, over
    assert fit(n_iter=0) == 0                                         # no iterations: a no-op
