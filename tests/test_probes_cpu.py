"""probes.py's torch helpers against the reference's own outputs
(tests/golden/sh_probe.npz, written by tests/golden/make_sh_golden.py from
insert/insert_utils.py), and the argument checks of the three light-probe
entry points (no launch, no GPU)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import probes
import vren

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(HERE, "golden", "sh_probe.npz")) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def _close(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    err = float((a - b).abs().max())
    print("max abs error", err)
    assert err <= 1e-6


def test_sh9_basis_is_the_documented_table(fx):
    d = fx["dirs"].reshape(-1, 3).double()
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    ref = torch.stack([0.2820947918 * torch.ones_like(x), 0.4886025119 * y, 0.4886025119 * z, 0.4886025119 * x,
                       1.0925484306 * x * y, 1.0925484306 * y * z, 0.3153915653 * (3 * z * z - 1),
                       1.0925484306 * x * z, 0.5462742153 * (x * x - y * y)], -1)
    Y = probes.sh9_basis(fx["dirs"].reshape(-1, 3))
    assert Y.shape == (130, 9) and Y.dtype == torch.float32
    assert float((Y.double() - ref).abs().max()) <= 1e-6


def test_get_SH_coeff_matches_reference(fx):
    _close(probes.get_SH_coeff(fx["dirs"], fx["rgb"]), fx["coeff"])
    _close(probes.get_SH_coeff(fx["dirs"], fx["trans"]), fx["coeff_trans"])


@pytest.mark.parametrize("clamp", [False, True])
def test_get_SH_val_matches_reference(fx, clamp):
    ref = fx["val_clamp"] if clamp else fx["val"]
    flat = fx["dirs"].reshape(-1, 3)
    _close(probes.get_SH_val(fx["shec"], flat, clamp_postive=clamp), ref)
    # any leading shape, like the reference's
    _close(probes.get_SH_val(fx["shec"], fx["dirs"], clamp_postive=clamp), ref.reshape(2, 65, 3))
    if clamp:
        assert (fx["val"] < 0).any() and float(probes.get_SH_val(fx["shec"], flat, clamp_postive=True).min()) == 0


def test_get_cubemap_rays_matches_reference(fx):
    _close(probes.get_cubemap_rays(1, 4), fx["cube"])
    _close(probes.get_cubemap_rays(1, 4, keep_raw_dim=True), fx["cube_raw"])
    many = probes.get_cubemap_rays(3, 4)
    assert many.shape == (3, 96, 3) and torch.equal(many[2], fx["cube"][0])


def test_get_sphere_rays_unit_shape_reproducible(fx):
    g = torch.Generator().manual_seed(7)
    d = probes.get_sphere_rays(3, 65, generator=g)
    assert d.shape == (3, 65, 3) and d.dtype == torch.float32
    assert float((d.norm(dim=-1) - 1).abs().max()) <= 1e-6
    assert torch.equal(d, probes.get_sphere_rays(3, 65, generator=torch.Generator().manual_seed(7)))
    assert not torch.equal(d, probes.get_sphere_rays(3, 65, generator=torch.Generator().manual_seed(8)))
    # without a generator: the global stream, the reference's own draw
    torch.manual_seed(int(fx["seed"]))
    _close(probes.get_sphere_rays(2, 65), fx["dirs"])


def test_probe_entry_points_reject_bad_arguments_without_launching():
    """NGP_EINVAL (-1) on null pointers, negative counts and R = 0 with P > 0;
    nothing to do (P = 0 / n_rays = 0) is NGP_OK.  No launch either way."""
    L = vren.lib()
    p = C.c_void_p(256)  # never dereferenced: every call below fails its checks first or has nothing to do
    near = C.c_float(0.01)
    # ngp_probe_rays(pts, dirs, dirs_per_probe, P, R, center, half_size, near, rays_o, rays_d, hits_t, stream)
    assert L.ngp_probe_rays(None, None, 0, 2, 4, None, None, near, None, None, None, None) == -1
    assert L.ngp_probe_rays(p, p, 0, 2, 4, p, p, near, p, p, None, None) == -1
    assert L.ngp_probe_rays(p, None, 1, 2, 4, p, p, near, p, p, p, None) == -1
    assert L.ngp_probe_rays(p, p, 0, -1, 4, p, p, near, p, p, p, None) == -1
    assert L.ngp_probe_rays(p, p, 0, 2, -4, p, p, near, p, p, p, None) == -1
    assert L.ngp_probe_rays(p, p, 0, 2, 0, p, p, near, p, p, p, None) == -1
    assert L.ngp_probe_rays(p, p, 2, 2, 4, p, p, near, p, p, p, None) == -1
    assert L.ngp_probe_rays(p, p, 0, 1 << 16, 1 << 15, p, p, near, p, p, p, None) == -1  # P*R = 2^31
    assert L.ngp_probe_rays(None, None, 0, 0, 4, None, None, near, None, None, None, None) == 0
    # ngp_render_test_finish_sh(opacity, rays_d, n_rays, shec, rgb, stream)
    assert L.ngp_render_test_finish_sh(None, None, 4, None, None, None) == -1
    assert L.ngp_render_test_finish_sh(p, p, 4, None, p, None) == -1
    assert L.ngp_render_test_finish_sh(p, None, 4, p, p, None) == -1
    assert L.ngp_render_test_finish_sh(p, p, -1, p, p, None) == -1
    assert L.ngp_render_test_finish_sh(None, None, 0, p, None, None) == 0
    # ngp_probe_sh9_project(rays_d, rgb, opacity, P, R, rgb_sh, trans_sh, stream)
    assert L.ngp_probe_sh9_project(None, None, None, 2, 4, None, None, None) == -1
    assert L.ngp_probe_sh9_project(p, p, p, 2, 4, None, p, None) == -1
    assert L.ngp_probe_sh9_project(p, p, None, 2, 4, p, p, None) == -1  # trans_sh needs opacity
    assert L.ngp_probe_sh9_project(p, p, p, -2, 4, p, p, None) == -1
    assert L.ngp_probe_sh9_project(p, p, p, 2, -4, p, p, None) == -1
    assert L.ngp_probe_sh9_project(p, p, p, 2, 0, p, p, None) == -1
    assert L.ngp_probe_sh9_project(p, p, p, 1 << 16, 1 << 15, p, p, None) == -1
    assert L.ngp_probe_sh9_project(None, None, None, 0, 4, None, None, None) == 0


def test_wrappers_reject_cpu_tensors_like_check_input():
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="pts must be a CUDA tensor"):
        vren.probe_rays(x, x, torch.zeros(1, 3), torch.ones(1, 3), 0.01)
    with pytest.raises(RuntimeError, match="opacity must be a CUDA tensor"):
        vren.render_test_finish_sh(torch.zeros(4), x, torch.zeros(9, 3), x.clone())
    with pytest.raises(RuntimeError, match="rays_d must be a CUDA tensor"):
        vren.probe_sh9_project(x[None], x[None])
