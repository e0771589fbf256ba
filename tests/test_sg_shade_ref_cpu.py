"""tests/sg_shade_ref.py (the per-pixel fp64 restatement of the object shade,
lights in the kernel's order) and shading.sg_shade_torch (the torch
formulation, CPU fp32) held to tests/golden/sg_shade.npz, which the reference's
own SG_render_core produced in fp64 and fp32 (tests/golden/make_sg_golden.py);
and what that fixture's designed inputs must hold for the GPU tests to mean
anything.  No GPU.

sg_shade_ref against the fixture's fp64 output: both are fp64, only the order
of operations differs.  Measured per class, max |a - b| / (1e-3 + |b|) over
the five configurations (the bars in REF64_BAR are 10x these, rounded up):
    uncovered 0 (exact)   facing 9.5e-12   middle 3.4e-11   grazing 6.0e-10   back 8.4e-12
(the grazing class carries the distribution lobe's sharpness 2 / m^2 / (4 n.v)
of up to 6e3 into exp(lm (|um| - 1)), which multiplies the rounding of |um|).
"""
import numpy as np
import pytest
import torch

import sg_shade_ref as SR
from capi import C, FUNCS
from fixture_model import load

REF64_BAR = {"uncovered": 0.0, "facing": 1e-10, "middle": 4e-10, "grazing": 6e-9, "back": 1e-10}


@pytest.fixture(scope="module")
def fx():
    return load("sg_shade")


def fp32_bound(fx, k, cls_index, ref64):
    """The fp32 bar of a class: 4x the reference's own fp32 deviation from its fp64 run, absolute or relative
    (to 1e-3 + |ref64|), whichever is looser at the value"""
    return 4 * np.maximum(fx["ref32_abs"][k, cls_index], fx["ref32_rel"][k, cls_index] * (1e-3 + np.abs(ref64)))


def test_fixture_frame_is_the_designed_one(fx):
    H, W = int(fx["H"]), int(fx["W"])
    hs, ws, hl, wl = (int(v) for v in fx["bbox"])
    assert (H, W) == (13, 11) and (H * W) % 64 != 0
    assert 0 < hs < hl < H and 0 < ws < wl < W                     # the box strictly inside the frame
    assert [str(s) for s in fx["config_names"]] == list(SR.CONFIGS)
    assert [str(s) for s in fx["class_names"]] == list(SR.CLASSES)
    K = len(SR.CONFIGS)
    assert fx["out64"].shape == (K, H, W, 3) and fx["out64"].dtype == np.float64
    assert fx["out32"].shape == (K, H, W, 3) and fx["out32"].dtype == np.float32
    assert fx["ref32_abs"].shape == fx["ref32_rel"].shape == (K, len(SR.CLASSES))
    for k in ("directions", "normals", "obj_depth", "lSGs", "decay", "metal_map", "rough_map", "albedo_map", "pose"):
        assert fx[k].dtype == np.float32, k
    assert np.isfinite(fx["out64"]).all() and np.isfinite(fx["out32"]).all()
    # the recorded deviations are those of the recorded outputs
    err = np.abs(fx["out32"].astype(np.float64) - fx["out64"]).reshape(K, -1, 3)
    for i in range(len(SR.CLASSES)):
        m = fx["class_of"] == i
        assert np.array_equal(err[:, m].max((1, 2)), fx["ref32_abs"][:, i])


def test_designed_inputs_hold_every_class(fx):
    """Conditions on the fixture's inputs (not measurements)."""
    H, W = int(fx["H"]), int(fx["W"])
    bbox = tuple(int(v) for v in fx["bbox"])
    depth = fx["obj_depth"]
    inbox = np.zeros((H, W), dtype=bool)
    inbox[bbox[0]:bbox[2], bbox[1]:bbox[3]] = True
    inbox = inbox.reshape(-1)
    eps = np.float32(1e-6)
    assert np.float64(eps) != 1e-6                                   # the compare is on the fp32 value
    below, above = np.nextafter(eps, np.float32(0)), np.nextafter(eps, np.float32(1))
    mask = SR.cover_mask(H, W, bbox, depth)
    for val, cov in ((np.float32(0), False), (np.float32(5e-7), False), (eps, False), (below, False), (above, True)):
        m = inbox & (depth == val)
        assert m.sum() >= 1 and np.all(mask[m] == cov), val
    assert np.any(inbox & (depth > 0.1)) and np.any(~inbox & (depth > 0.1)) and np.any(~inbox & (depth == 0))
    assert not mask[~inbox].any()
    # classes: every pixel in exactly one; each present
    cls = SR.pixel_classes(H, W, fx["directions"], fx["pose"], bbox, fx["normals"], depth)
    assert np.array_equal(sum(cls[c].astype(int) for c in SR.CLASSES), np.ones(H * W, dtype=int))
    for i, c in enumerate(SR.CLASSES):
        assert cls[c].sum() >= 3 and np.array_equal(fx["class_of"] == i, cls[c]), c
    # normals of non-unit length, none zero
    ln = np.linalg.norm(fx["normals"].astype(np.float64), axis=-1)
    assert ln.min() > 0.2 and np.any(ln < 0.7) and np.any(ln > 1.5)
    # lights: sharpness over 1e-1 .. 1e4, one dark, L = 33 and L = 1 recorded
    lam = fx["lSGs"][:, 3]
    assert fx["lSGs"].shape == (33, 7) and lam.min() <= 0.11 and lam.max() >= 9e3
    assert np.sum(np.all(fx["lSGs"][:, 4:] == 0, axis=1)) == 1
    assert sorted({c["L"] for c in SR.CONFIGS.values()}) == [1, 33]
    ax = np.linalg.norm(fx["lSGs"][:, :3].astype(np.float64), axis=1)
    assert np.all(np.abs(ax - 1) < 1e-6)
    # materials: rough as 0.2, as 0.1 (below the map's clip: a scalar is used as given) and as a map with values
    # on both sides of [0.2, 1]; metal as a number and a map; albedo absent, one row, a map; decay both ways
    cfgs = SR.CONFIGS.values()
    assert {0.2, 0.1, "map"} <= {c["rough"] for c in cfgs}
    assert np.any(fx["rough_map"][mask] < 0.2) and np.any(fx["rough_map"][mask] > 1.0)
    assert "map" in {c["metal"] for c in cfgs} and any(isinstance(c["metal"], float) for c in cfgs)
    assert {None, "row", "map"} == {c["albedo"] for c in cfgs}
    assert {True, False} == {c["decay"] for c in cfgs} == {c["clamp01"] for c in cfgs}
    assert fx["albedo_row"].shape == (1, 3) and fx["decay"].shape == (H * W, 33)
    assert np.any(fx["decay"] == 0) and np.all(fx["decay"] <= 1)
    # outputs above 1 where the radiance is kept, clamped ones where it is not
    for k, (name, c) in enumerate(SR.CONFIGS.items()):
        if c["clamp01"]:
            assert fx["out64"][k].max() <= 1.0
    assert any(not c["clamp01"] and (fx["out64"][k] > 1).sum() >= 3 for k, c in enumerate(SR.CONFIGS.values()))
    assert any(c["clamp01"] and (fx["out64"][k] == 1).sum() >= 3 for k, c in enumerate(SR.CONFIGS.values()))
    # back-facing pixels are lit (the diffuse term) and finite
    back = fx["class_of"] == SR.CLASSES.index("back")
    assert np.any(fx["out64"][0].reshape(-1, 3)[back] > 0)


@pytest.mark.parametrize("name", list(SR.CONFIGS))
def test_restatement_matches_the_reference_fp64(fx, name):
    k = list(SR.CONFIGS).index(name)
    out = SR.sg_shade_ref(**SR.config_args(fx, name)).reshape(-1, 3)
    ref = fx["out64"][k].reshape(-1, 3)
    assert out.dtype == np.float64 and np.isfinite(out).all()
    for i, c in enumerate(SR.CLASSES):
        m = fx["class_of"] == i
        rel = float((np.abs(out[m] - ref[m]) / (1e-3 + np.abs(ref[m]))).max())
        print(f"{name} {c}: {rel:.2e} (bar {REF64_BAR[c]:.0e})")
        assert rel <= REF64_BAR[c], (name, c, rel)


def _torch_args(a):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v for k, v in a.items()}


@pytest.mark.parametrize("name", list(SR.CONFIGS))
def test_torch_formulation_cpu_fp32_within_the_fp32_bar(fx, name):
    import shading
    k = list(SR.CONFIGS).index(name)
    a = _torch_args(SR.config_args(fx, name))
    out = shading.sg_shade_torch(**a)
    assert out.dtype == torch.float32 and out.shape == (a["H"], a["W"], 3)
    assert torch.equal(shading.sg_shade(**a), out)                   # CPU tensors take the torch path
    out = out.numpy().reshape(-1, 3).astype(np.float64)
    ref = fx["out64"][k].reshape(-1, 3)
    assert np.isfinite(out).all()
    for i, c in enumerate(SR.CLASSES):
        m = fx["class_of"] == i
        err = np.abs(out[m] - ref[m])
        print(f"{name} {c}: max err {err.max():.2e}, worst share of the bar "
              f"{(err / np.maximum(fp32_bound(fx, k, i, ref[m]), 1e-300)).max():.2f}")
        assert np.all(err <= fp32_bound(fx, k, i, ref[m])), (name, c)
    assert np.all(out[fx["class_of"] == 0] == 0)


def test_torch_formulation_fp64_and_rectangles(fx):
    import shading
    a = _torch_args(SR.config_args(fx, "maps_decay_ldr"))
    a64 = {k: v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v for k, v in a.items()}
    out = shading.sg_shade_torch(**a64).numpy()
    assert float(np.abs(out - fx["out64"][list(SR.CONFIGS).index("maps_decay_ldr")]).max()) <= 1e-9
    H, W = a["H"], a["W"]
    assert float(shading.sg_shade_torch(**dict(a, bbox=(5, 5, 5, 9))).abs().max()) == 0      # empty
    assert float(shading.sg_shade_torch(**dict(a, bbox=(9, 5, 5, 9))).abs().max()) == 0      # inverted
    whole = shading.sg_shade_torch(**dict(a, bbox=(0, 0, H, W)))
    past = shading.sg_shade_torch(**dict(a, bbox=torch.tensor([-4, -1, H + 7, W + 2], dtype=torch.int32)))
    assert torch.equal(whole, past)                                   # a box reaching past the frame is clamped
    ref = SR.sg_shade_ref(**dict(SR.config_args(fx, "maps_decay_ldr"), bbox=(0, 0, H, W)))
    assert np.isfinite(ref).all() and (whole.numpy().reshape(-1, 3)[fx["obj_depth"] > np.float32(1e-6)] > 0).any()
    assert SR.clamp_bbox((-3, 2, 50, 43), 13, 11) == ((0, 2, 13, 11), 13 * 9)
    assert SR.clamp_bbox((9, 7, 5, 9), 13, 11)[1] == 0


def test_header_declares_the_shade_entry_point():
    assert "ngp_sg_shade" in FUNCS
    restype, args = FUNCS["ngp_sg_shade"]
    assert len(args) == 19
    assert C["NGP_SG_LIGHT_TILE"] == 64


def test_argument_errors_return_before_any_launch():
    """Host-side checks of the entry point (no GPU needed): NGP_EINVAL (-1)."""
    import ctypes

    import vren
    L = vren.lib()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails its checks first
    f = ctypes.c_float(0.5)

    def shade(H=13, W=11, ptrs=(p,) * 7, n_lights=3, albedo=None, rows=0):
        bbox, dirs, pose, nrm, dep, lsg, out = ptrs
        return L.ngp_sg_shade(bbox, H, W, dirs, pose, nrm, dep, lsg, n_lights, None, albedo, rows, None, f, None, f,
                              1, out, None)
    assert shade(H=0) == -1 and shade(W=0) == -1 and shade(H=-1) == -1
    assert shade(H=1 << 16, W=1 << 15) == -1                         # H*W = 2^31
    for k in range(7):                                               # every pointer is needed
        assert shade(ptrs=(p,) * k + (None,) + (p,) * (6 - k)) == -1, k
    assert shade(n_lights=0) == -1 and shade(n_lights=-2) == -1
    assert shade(albedo=None, rows=1) == -1 and shade(albedo=p, rows=0) == -1 and shade(albedo=p, rows=2) == -1
