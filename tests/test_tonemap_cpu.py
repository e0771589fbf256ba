"""Exposure-conditioned models (NGP(use_exposure=True)), the parts
that need no GPU: the soundness of the reference the GPU tests use
(tests/tonemap_ref.py) against torch autograd on the reference project's own
expression, the size of the ReLU-ambiguous set on every GPU case, the model's
constructor surface, the tonemapper_net_i.params checkpoint mapping, the
HDR-NeRF branch of the COLMAP loader, and the entry points' argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import hashgrid as HG
import tonemap_ref as T
import vren


# ------------------------------------------------------------ 1. the reference
def test_split_views_the_flat_layout():
    w = np.arange(T.PARAMS, dtype=np.float64)
    A, B = T.split(w)
    assert np.shares_memory(A, w) and np.shares_memory(B, w)
    assert A[1, 2, 3] == T.NET + 2 * 16 + 3 and B[2, 0, 5] == 2 * T.NET + 1024 + 5


@pytest.mark.parametrize("n", [1, 65, 257])
def test_reference_backward_equals_autograd_on_the_padded_mlps(n):
    """Three 16 -> 64 -> 16 bias-free MLPs fed (u, 1, ..., 1), output row 0, sigmoid -- what the
    reference project builds, under the padding this build assumes -- in fp64 torch autograd against
    tonemap_ref.backward.  (The reference adds the padding columns in fp32, autograd's sum is fp64:
    that is the 1e-6.)"""
    c = T.case(n)
    w = torch.tensor(c["w"], dtype=torch.float64, requires_grad=True)
    x = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
    u = x + torch.log(torch.tensor(c["e"], dtype=torch.float64))[:, None]
    ys = []
    for ch in range(3):
        A = w[ch * T.NET:ch * T.NET + 1024].view(64, 16)
        B = w[ch * T.NET + 1024:(ch + 1) * T.NET].view(16, 64)
        inp = torch.cat([u[:, ch:ch + 1], torch.ones(n, 15, dtype=torch.float64)], 1)
        ys.append(torch.sigmoid((torch.relu(inp @ A.t()) @ B.t())[:, 0]))
    y = torch.stack(ys, 1)
    (y * torch.tensor(c["dy"], dtype=torch.float64)).sum().backward()
    ref = T.backward(c["w"], c["x"], c["e"], c["dy"])
    assert np.abs(y.detach().numpy() - T.forward(c["w"], c["x"], c["e"])).max() < 1e-7
    gw, gx = w.grad.numpy(), x.grad.numpy()
    assert np.abs(gw - ref["grad"]).max() <= 1e-6 * max(np.abs(gw).max(), 1e-30)
    assert np.abs(gx - ref["dx"]).max() <= 1e-6 * max(np.abs(gx).max(), 1e-30)
    A, B = T.split(ref["grad"])
    assert np.all(B[:, 1:] == 0) and np.all(A[:, :, 1:] == A[:, :, 1:2])
    assert np.all(ref["dx"][(c["dy"] == 0)] == 0)


@pytest.mark.parametrize("n", T.SIZES)
def test_the_relu_ambiguous_set_is_small_on_every_gpu_case(n):
    """At most 0.1 % of the (row, unit) pairs sit within 2^-18 (|A_j0 u| + sum_k |A_jk|) of the ReLU's
    kink, where a device fp32 a_j may take the other branch (test_tonemap_gpu.py adds their
    contribution to its bars)."""
    c = T.case(n)
    for e in (None, c["e"]):
        amb = T.ambiguous(c["w"], c["x"], e)
        share = float(amb.mean())
        print(f"n = {n}, exposure {'per row' if e is not None else 'absent'}: {int(amb.sum())} of {amb.size} pairs")
        assert share <= T.AMBIGUOUS_CAP


def test_radiance_reference_clamps():
    y = T.radiance(np.array([-3.0, 0.0, 1.0, 20.0, 25.0]))
    assert y[0] == y[1] == 1.0 and y[3] == y[4] == np.exp(20.0) and abs(y[2] - np.e) < 1e-15


# ------------------------------------------------------------ 2. the model's surface
def test_ngp_use_exposure_constructor_surface():
    from models.networks import NGP
    with pytest.raises(NotImplementedError, match="tonemapper"):
        NGP(0.5, 'None', False)
    with pytest.raises(NotImplementedError, match="use_exposure"):
        NGP(0.5, 'None', False)
    for bad in (dict(rgb_act='Sigmoid'), dict(rgb_act='None', use_raw_HDR=True), dict(rgb_act='Sigmoid', use_raw_HDR=True)):
        with pytest.raises(ValueError, match="use_exposure"):
            NGP(0.5, use_exposure=True, **bad)
    m, ldr = NGP(0.5, 'None', False, use_exposure=True), NGP(0.5)
    assert m.tone_params.shape == (HG.TONE_PARAMS,) == (6144,) and m.tone_params.dtype == torch.float32
    assert m.tone_params._ngp_shadow is m._tone_shadow and m._tone_shadow.master is m.tone_params
    assert [k for k in m.state_dict() if k not in ldr.state_dict()] == ['tone_params']
    assert torch.equal(m.params, ldr.params)  # the field's parameters are what every other mode draws from the seed
    assert 'tone_params' not in NGP(0.5, 'None', True).state_dict()
    assert m.rgb_mode() == m.rgb_mode(True) == HG.RGB_NONE
    assert (m.tone_mode(), m.tone_mode(True), ldr.tone_mode()) == (HG.TONE_LDR, HG.TONE_RADIANCE, None)
    # Xavier-uniform per matrix: within the bound, and not degenerate
    t = m.tone_params.detach().view(3, 2048)
    a = (6.0 / 80) ** 0.5
    assert float(t.abs().max()) <= a and float(t.abs().max()) > 0.9 * a and abs(float(t.mean())) < 0.01
    assert not torch.equal(m.tone_params, NGP(0.5, 'None', False, seed=5, use_exposure=True).tone_params)
    with pytest.raises(RuntimeError, match="use_exposure"):
        ldr.log_radiance_to_rgb(torch.zeros(1, 3))


def test_exposure_argument_forms():
    dev = torch.device("cpu")
    assert HG.tone_exposure(None, 5, dev) == (None, 0)
    for one in (torch.tensor(2.0), torch.tensor([2.0]), torch.tensor([[2.0]]), 2.0):
        e, k = HG.tone_exposure(one, 5, dev)
        assert k == 1 and e.shape == (1,) and float(e) == 2.0
    for per_row in (torch.arange(1., 6.), torch.arange(1., 6.)[:, None]):
        e, k = HG.tone_exposure(per_row, 5, dev)
        assert k == 5 and e.shape == (5,) and e.is_contiguous()
    assert HG.tone_exposure(torch.ones(1, 1), 1, dev)[1] == 1
    for bad in (torch.ones(4), torch.ones(5, 2), torch.ones(1, 5), "1.0"):
        with pytest.raises(ValueError, match="exposure"):
            HG.tone_exposure(bad, 5, dev)


# ------------------------------------------------------------ 3. checkpoints
def test_tonemapper_checkpoint_round_trip_and_its_errors(tmp_path):
    from models.networks import NGP
    from utils import load_ckpt, tcnn_state_dict
    src = NGP(0.5, 'None', False, seed=9, use_exposure=True)
    sd = tcnn_state_dict(src)
    keys = [f"tonemapper_net_{i}.params" for i in range(3)]
    assert all(sd[k].shape == (2048,) for k in keys) and 'tone_params' not in sd and 'params' not in sd
    for i, k in enumerate(keys):
        assert torch.equal(sd[k], src.tone_params.detach()[2048 * i:2048 * (i + 1)])
    path = str(tmp_path / "exposure.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}}, path)
    dst = NGP(0.5, 'None', False, seed=4, use_exposure=True)
    assert not torch.equal(dst.tone_params, src.tone_params)
    load_ckpt(dst, path)
    assert torch.equal(dst.tone_params, src.tone_params) and torch.equal(dst.params, src.params)
    # a checkpoint with the tonemappers, a model without them
    with pytest.raises(RuntimeError, match=r"tonemapper_net_0\.params.*use_exposure"):
        load_ckpt(NGP(0.5, 'None', True), path)
    # a model with them, a checkpoint without (one or all missing)
    for drop in (keys[1:2], keys):
        part = {"model." + k: v for k, v in sd.items() if k not in drop}
        with pytest.raises(RuntimeError, match=r"tonemapper_net_1\.params"):
            load_ckpt(NGP(0.5, 'None', False, use_exposure=True), {"state_dict": part})
    # the model's own state_dict (tone_params as one entry) loads too
    own = NGP(0.5, 'None', False, use_exposure=True)
    load_ckpt(own, {"model." + k: v for k, v in src.state_dict().items()})
    assert torch.equal(own.tone_params, src.tone_params)


# ------------------------------------------------------------ 4. the HDR-NeRF loader
def _write_colmap(root, n_poses, rng):
    from datasets import colmap_utils as CU
    (root / "sparse" / "0").mkdir(parents=True)
    cams = {1: CU.Camera(1, "PINHOLE", 16, 12, np.array([20.0, 21.0, 8.0, 6.0]))}
    ims = {}
    for i in range(n_poses):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        ims[i + 1] = CU.Image(i + 1, q, rng.normal(size=3) * 3, 1, f"view_{i:03d}.png", np.zeros((0, 2)),
                              np.zeros(0, np.int64))
    pts = {k: CU.Point3D(k, rng.normal(size=3), np.array([1, 2, 3]), 0.5, np.zeros(0), np.zeros(0)) for k in range(20)}
    CU.write_model_binary(str(root / "sparse" / "0"), cams, ims, pts)
    return ims, pts


def _centred(ims, pts):
    from datasets import colmap_utils as CU
    from datasets.ray_utils import center_poses
    c2w = []
    for k in sorted(ims, key=lambda k: ims[k].name):
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = CU.qvec2rotmat(ims[k].qvec), ims[k].tvec
        c2w.append(np.linalg.inv(w2c)[:3])
    pc, _, _ = center_poses(np.stack(c2w), np.stack([p.xyz for p in pts.values()]))
    pc[..., 3] /= np.linalg.norm(pc[..., 3], axis=-1).min()
    return pc.astype(np.float32)


def test_hdr_nerf_synthetic_scene_loader(tmp_path):
    """.../HDR-NeRF/syndata/<scene>: 35 poses, the first 17 test (exposures 1, 3), the last 18 train
    (exposures 0, 2, 4), each pose repeated per exposure; the grey level of every written image is its
    (view, exposure) so the pairing with the poses shows."""
    from datasets import dataset_dict
    from datasets.png import write_png
    root = tmp_path / "HDR-NeRF" / "syndata" / "sponza"
    rng = np.random.default_rng(5)
    ims, pts = _write_colmap(root, 35, rng)
    for split, views in (("train", range(18)), ("test", range(17))):
        (root / split).mkdir()
        for v in views:
            for e in range(5):
                write_png(str(root / split / f"{v:03d}_{e}.png"), np.full((12, 16, 3), 10 * v + e, np.uint8))
    pc = _centred(ims, pts)
    table = {0: 0.5, 1: 2, 2: 4, 3: 8, 4: 32}  # sponza
    for split, picks, pose_rows in (("train", (0, 2, 4), range(17, 35)), ("test", (1, 3), range(17))):
        ds = dataset_dict['colmap'](str(root), split=split)
        k = len(picks)
        assert ds.unit_exposure_rgb == 0.73
        assert ds.rays.shape == (len(pose_rows) * k, 192, 4) and ds.poses.shape == (len(pose_rows) * k, 3, 4)
        np.testing.assert_allclose(ds.poses.numpy(), np.repeat(pc[list(pose_rows)], k, 0), rtol=1e-5, atol=1e-5)
        for i in range(len(ds.poses)):
            v, e = i // k, picks[i % k]
            assert torch.all(ds.rays[i, :, :3] == np.float32(10 * v + e) / np.float32(255))
            assert torch.all(ds.rays[i, :, 3] == table[e])
    train = dataset_dict['colmap'](str(root), split='train')
    train.batch_size, train.ray_sampling_strategy = 64, 'all_images'
    batch = train[0]
    assert batch['rgb'].shape == (64, 3) and batch['exposure'].shape == (64, 1)
    assert set(batch['exposure'].flatten().tolist()) <= {0.5, 4.0, 32.0}
    frame = dataset_dict['colmap'](str(root), split='test')[1]
    assert frame['exposure'].dim() == 0 and float(frame['exposure']) == 8.0  # one exposure per test frame
    with pytest.raises(ValueError, match="invalid for HDR-NeRF"):
        dataset_dict['colmap'](str(root), split='trainval')
    assert dataset_dict['colmap'](str(root), split='test_traj').poses.shape[1:] == (3, 4)


def test_hdr_nerf_real_scene_loader(tmp_path):
    """A real-style folder: input_images/*N.jpg, even views train at exposures 0, 2, 4, odd views
    test at 1, 3, the poses tiled per exposure."""
    from PIL import Image as PILImage

    from datasets import dataset_dict
    root = tmp_path / "HDR-NeRF" / "real" / "flower"
    rng = np.random.default_rng(6)
    ims, pts = _write_colmap(root, 6, rng)
    (root / "input_images").mkdir()
    for v in range(6):
        for e in range(5):
            PILImage.fromarray(np.full((12, 16, 3), 40 * v + 8 * e, np.uint8)).save(
                root / "input_images" / f"{v:02d}_{e}.jpg", quality=100)
    pc = _centred(ims, pts)
    table = {0: 1 / 3, 1: 1 / 6, 2: 0.1, 3: 0.05, 4: 1 / 45}  # flower
    for split, picks, views in (("train", (0, 2, 4), (0, 2, 4)), ("test", (1, 3), (1, 3, 5))):
        ds = dataset_dict['colmap'](str(root), split=split)
        assert ds.unit_exposure_rgb == 0.5
        assert ds.rays.shape == (len(views) * len(picks), 192, 4)
        np.testing.assert_allclose(ds.poses.numpy(), np.tile(pc[list(views)], (len(picks), 1, 1)), rtol=1e-5, atol=1e-5)
        for i in range(len(ds.poses)):
            e, v = picks[i // len(views)], views[i % len(views)]
            assert abs(float(ds.rays[i, 0, 0]) * 255 - (40 * v + 8 * e)) <= 2, (split, i)  # (JPEG)
            assert torch.all(ds.rays[i, :, 3] == np.float32(table[e]))
    bad = tmp_path / "HDR-NeRF" / "real" / "garden"
    _write_colmap(bad, 2, rng)
    (bad / "input_images").mkdir()
    PILImage.fromarray(np.zeros((12, 16, 3), np.uint8)).save(bad / "input_images" / "00_0.jpg")
    with pytest.raises(ValueError, match="garden"):
        dataset_dict['colmap'](str(bad), split='train')


# ------------------------------------------------------------ 5. the entry points' argument checks
def test_tonemap_entry_points_refuse_bad_arguments_without_launching():
    L = vren.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # (host memory: a launch would fault, a refusal never reads it)
    z = None
    LDR, RAD = HG.TONE_LDR, HG.TONE_RADIANCE
    assert (LDR, RAD, HG.TONE_PARAMS) == (0, 1, 6144)
    fwd, bwd = L.ngp_tonemap_forward, L.ngp_tonemap_backward
    # empty calls are no-ops, also with null pointers
    assert fwd(z, z, 0, 0, z, z, z, LDR, z, z) == 0 and fwd(z, z, 1, 0, z, z, z, RAD, z, z) == 0
    assert bwd(z, z, 0, 0, z, z, z, z, z, z, z) == 0
    for mode in (-1, 2):
        assert fwd(p, z, 0, 4, z, z, p, mode, p, z) == -1 and fwd(z, z, 0, 0, z, z, z, mode, z, z) == -1
    assert fwd(p, z, 0, -1, z, z, p, LDR, p, z) == -1
    for n_exposure in (-1, 2, 3, 5):  # not in {0, 1, n = 4}
        assert fwd(p, p, n_exposure, 4, z, z, p, LDR, p, z) == -1
        assert bwd(p, p, n_exposure, 4, z, p, p, p, p, p, z) == -1
    assert fwd(p, z, 1, 4, z, z, p, LDR, p, z) == -1 and fwd(p, z, 4, 4, z, z, p, LDR, p, z) == -1  # exposure missing
    assert fwd(z, z, 0, 4, z, z, p, LDR, p, z) == -1 and fwd(p, z, 0, 4, z, z, p, LDR, z, z) == -1
    assert fwd(p, z, 0, 4, z, z, z, LDR, p, z) == -1  # the weights, in LDR mode
    assert fwd(p, z, 0, 4, z, p, p, LDR, p, z) == -1  # sample_idx without its count
    for hole in range(6):  # log_rad, tone, dL_drgbs, dL_dlog_rad, grad_tone, workspace
        a = [p] * 6
        a[hole] = z
        assert bwd(a[0], z, 0, 4, z, a[1], a[2], a[3], a[4], a[5], z) == -1
    assert bwd(p, z, 1, 4, z, p, p, p, p, p, z) == -1
    ws = L.ngp_tonemap_backward_workspace
    assert ws(0) == 0 and ws(-3) == 0 and ws(1) == ws(256) == 384 * 4 and ws(257) == 2 * 384 * 4
    assert ws(512 * 256) == ws(1 << 24) == 512 * 384 * 4  # the grid, and so the workspace, stop growing
    with pytest.raises(vren.NGPError):
        vren.kernels().ngp_tonemap_forward(z, z, 0, 4, z, z, z, 7, z, z)
