"""The object shade on the device (csrc/shade.hip, shading.sg_shade,
InsertRenderer.shade_sg, models.rendering.render_insert_sg) against the golden
fixture of the reference's own SG_render_core (tests/golden/sg_shade.npz) and
the per-pixel fp64 restatement (tests/sg_shade_ref.py).

The bar against the fixture's fp64 output, per configuration and pixel class:
|kernel - ref64| <= 4 * ref32_abs, or 4 * ref32_rel * (1e-3 + |ref64|) where
that is looser -- ref32_* being the reference's own fp32 deviation from its
fp64 run on the same inputs.  4x: the kernel may use another exp and sums the
lights in another order than torch's reduction; beyond that it has no licence
to be worse than the reference's own fp32.  Every pixel of the frame is in
exactly one class, so none is left out.
"""
import numpy as np
import pytest
import torch

import renderer as R
import sg_shade_ref as SR
import shading
from capi import C
from fixture_model import load
from models.rendering import render_insert, render_insert_sg
from test_golden_gpu import _product_model
from test_sg_shade_ref_cpu import fp32_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = C["NGP_SG_LIGHT_TILE"]
APP = dict(T_threshold=1e-2, max_samples=100)


@pytest.fixture(scope="module")
def fx():
    return load("sg_shade")


def _dev(a):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if isinstance(v, np.ndarray) else v
            for k, v in a.items()}


def _args(fx, name, **over):
    return _dev(dict(SR.config_args(fx, name), **over))


def _assert_classes(fx, k, out, ref64, scale=1.0, what=""):
    out = out.detach().cpu().numpy().reshape(-1, 3).astype(np.float64)
    ref64 = ref64.reshape(-1, 3)
    assert np.isfinite(out).all(), what
    seen = np.zeros(out.shape[0], dtype=bool)
    for i, c in enumerate(SR.CLASSES):
        m = fx["class_of"] == i
        seen |= m
        err = np.abs(out[m] - ref64[m])
        bound = scale * fp32_bound(fx, k, i, ref64[m])
        print(f"{what} {c}: max err {err.max():.2e}, worst share of the bar "
              f"{(err / np.maximum(bound, 1e-300)).max():.2f}")
        assert np.all(err <= bound), (what, c, float(err.max()))
    assert seen.all()                                   # no pixel left out
    assert np.all(out[fx["class_of"] == 0] == 0)         # uncovered: exactly 0


@pytest.mark.parametrize("name", list(SR.CONFIGS))
def test_kernel_against_the_reference_fp64(fx, name):
    k = list(SR.CONFIGS).index(name)
    out = shading.sg_shade(**_args(fx, name))
    assert out.dtype == torch.float32 and out.shape == (13, 11, 3)
    _assert_classes(fx, k, out, fx["out64"][k], what=name)
    if not SR.CONFIGS[name]["clamp01"]:
        assert float(out.max()) > 1.0
    else:
        assert float(out.max()) <= 1.0


def test_cover_follows_the_fp32_compare_exactly(fx):
    a = _args(fx, "maps_hdr")
    out = shading.sg_shade(**a).reshape(-1, 3).cpu().numpy()
    mask = SR.cover_mask(13, 11, a["bbox"], fx["obj_depth"])
    assert np.all(out[~mask] == 0)
    assert np.all(out[mask].max(-1) > 0)                 # every covered pixel is lit under these lights
    eps = np.float32(1e-6)
    d = fx["obj_depth"]
    assert np.all(out[d == eps] == 0) and np.all(out[d == np.nextafter(eps, np.float32(0))] == 0)
    inbox = SR.cover_mask(13, 11, a["bbox"], np.ones_like(d))
    above = inbox & (d == np.nextafter(eps, np.float32(1)))
    assert above.any() and np.all(out[above].max(-1) > 0)
    # a pre-filled out buffer: uncovered pixels are written, not skipped
    buf = torch.full((13, 11, 3), 7.0, device=DEV)
    res = shading.sg_shade(**a, out=buf)
    assert res.data_ptr() == buf.data_ptr() and np.array_equal(buf.reshape(-1, 3).cpu().numpy(), out)


def _more_lights(fx, n_total, seed):
    """the fixture's 33 lights and seeded ones after them, at a tenth of the fixture's amplitudes"""
    g = np.random.default_rng(seed)
    extra = n_total - 33
    ax = g.normal(size=(extra, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    lam = 10 ** g.uniform(-1, 4, size=extra)
    amp = 0.1 * g.uniform(0.1, 1.3, size=(extra, 3)) * (lam / (2 * np.pi * (1 - np.exp(-2 * lam))))[:, None]
    return np.concatenate([fx["lSGs"], np.concatenate([ax, lam[:, None], amp], 1).astype(np.float32)])


@pytest.mark.parametrize("n_lights", [TILE + 1, 2 * TILE + 3])
def test_more_lights_than_one_tile(fx, n_lights):
    """L past the kernel's light tile: the reference is sg_shade_ref.  The bar is the fixture's for the same
    materials (maps_hdr), scaled by the growth of the summed light energy sum_j |amp_j| 2 pi / lambda_j
    (1 - exp(-2 lambda_j)): every term of the light sum carries a rounding error in proportion to its size."""
    lights = _more_lights(fx, n_lights, seed=n_lights)
    energy = lambda l: float((np.abs(l[:, 4:]).sum(1) * 2 * np.pi / l[:, 3] * (1 - np.exp(-2 * l[:, 3]))).sum())  # noqa: E731
    scale = energy(lights.astype(np.float64)) / energy(fx["lSGs"].astype(np.float64))
    assert 1.0 < scale < 1.5
    a = dict(SR.config_args(fx, "maps_hdr"), lSGs=lights)
    ref = SR.sg_shade_ref(**a)
    assert float(np.abs(ref - fx["out64"][list(SR.CONFIGS).index("maps_hdr")]).max()) > 1e-3   # the new lights show
    out = shading.sg_shade(**_dev(a))
    _assert_classes(fx, list(SR.CONFIGS).index("maps_hdr"), out, ref, scale=scale, what=f"L={n_lights}")
    # the tiles are summed in order: the first 33 lights alone give the fixture's frame bit for bit whether or not
    # dark lights follow in later tiles
    dark = lights.copy()
    dark[33:, 4:] = 0
    assert torch.equal(shading.sg_shade(**_dev(dict(a, lSGs=dark))), shading.sg_shade(**_args(fx, "maps_hdr")))


def test_decay_of_ones_is_no_decay(fx):
    a = _args(fx, "maps_hdr")
    ones = torch.ones(13 * 11, 33, device=DEV)
    assert torch.equal(shading.sg_shade(**dict(a, decay=ones)), shading.sg_shade(**a))
    b = _args(fx, "maps_decay_ldr")
    assert not torch.equal(shading.sg_shade(**b), shading.sg_shade(**dict(b, decay=None)))


def test_value_does_not_depend_on_the_launch_shape(fx):
    """The 13 x 11 frame's pixels inside a 64 x 5 frame (another grid, other lanes and blocks): the same bits."""
    a = _args(fx, "maps_decay_ldr")
    small = shading.sg_shade(**a).reshape(-1, 3)
    H2, W2, n = 64, 5, 13 * 11
    # the frame's pixels, row-major, become the first 143 pixels of the padded frame, each keeping its inputs;
    # the box covers the padded frame and the cover is carried by the depth alone
    mask = torch.from_numpy(SR.cover_mask(13, 11, a["bbox"], fx["obj_depth"])).to(DEV)

    def pad(t, fill=0.0):
        t = t.reshape(n, -1)
        out = torch.full((H2 * W2, t.shape[1]), fill, device=DEV)
        out[:n] = t
        return out.reshape(-1) if t.shape[1] == 1 else out
    depth = torch.where(mask, a["obj_depth"], torch.zeros_like(a["obj_depth"]))
    b = dict(a, H=H2, W=W2, bbox=(0, 0, H2, W2), directions=pad(a["directions"], 1.0), normals=pad(a["normals"], 1.0),
             obj_depth=pad(depth), metal=pad(a["metal"]), rough=pad(a["rough"]), albedo=pad(a["albedo"]),
             decay=pad(a["decay"]))
    big = shading.sg_shade(**b).reshape(-1, 3)
    assert torch.equal(big[:n], small) and not bool(big[n:].any())


def test_rectangles(fx):
    a = _args(fx, "scalars_ldr")
    H, W = 13, 11
    whole_ref = SR.sg_shade_ref(**dict(SR.config_args(fx, "scalars_ldr"), bbox=(0, 0, H, W)))
    assert not bool(shading.sg_shade(**dict(a, bbox=(5, 5, 5, 9))).any())                     # empty
    assert not bool(shading.sg_shade(**dict(a, bbox=torch.tensor([9, 7, 5, 9], dtype=torch.int32, device=DEV))).any())
    whole = shading.sg_shade(**dict(a, bbox=(0, 0, H, W)))
    covered = torch.from_numpy(fx["obj_depth"] > np.float32(1e-6)).to(DEV)
    assert bool((whole.reshape(-1, 3)[covered].max(-1).values > 0).all()) and not bool(whole.reshape(-1, 3)[~covered].any())
    assert torch.isfinite(whole).all() and np.isfinite(whole_ref).all()
    # a device box reaching past the frame is clamped like insert_frame_begin's rect
    past = shading.sg_shade(**dict(a, bbox=torch.tensor([-4, -1, H + 7, W + 2], dtype=torch.int32, device=DEV)))
    assert torch.equal(past, whole)
    part = shading.sg_shade(**dict(a, bbox=torch.tensor([-4, 3, 6, W + 2], dtype=torch.int32, device=DEV)))
    assert torch.equal(part, shading.sg_shade(**dict(a, bbox=(0, 3, 6, W))))
    # the same box as ints and as a device tensor
    box = tuple(int(v) for v in fx["bbox"])
    assert torch.equal(shading.sg_shade(**dict(a, bbox=torch.tensor(box, dtype=torch.int32, device=DEV))),
                       shading.sg_shade(**dict(a, bbox=box)))
    for bad in [(-1, 0, 4, 4), (0, 0, H + 1, 4), (5, 0, 4, 4), (0, 9, 4, 8)]:                 # ints are checked
        with pytest.raises(ValueError):
            shading.sg_shade(**dict(a, bbox=bad))


def _frame_inputs(seed, L, h=16, w=16):
    g = torch.Generator().manual_seed(seed)
    normals = (torch.randn(h, w, 3, generator=g) + torch.tensor([0.0, 0.0, -1.5])).to(DEV)
    ax = torch.nn.functional.normalize(torch.randn(L, 3, generator=g), dim=-1)
    lam = 10 ** (torch.rand(L, 1, generator=g) * 3 - 1)
    amp = torch.rand(L, 3, generator=g) * lam / 6.0
    return normals.contiguous(), torch.cat([ax, lam, amp], 1).to(DEV).contiguous()


def test_renderer_shades_into_its_own_buffer_without_recapture():
    ins = load("insert_frame")
    model = _product_model(ins)
    h, w = int(ins["H"]), int(ins["W"])
    dirs, pose = torch.from_numpy(ins["directions"]).to(DEV), torch.from_numpy(ins["pose"]).to(DEV)
    obj_depth = torch.from_numpy(ins["obj_depth"]).to(DEV)
    rr = R.insert_for_model(model, h, w, dirs, **APP)     # shades, then renders from its own buffers
    r2 = R.insert_for_model(model, h, w, dirs, **APP)     # is handed the shaded image
    frames = [((5, 0, 16, 13), (3, 1, 15, 12), 7), ((0, 0, 16, 16), (0, 0, 16, 16), 33),
              ((2, 2, 9, 14), torch.tensor([-3, 4, 12, 40], dtype=torch.int32, device=DEV), 3)]
    for i, (rect, bbox, L) in enumerate(frames):
        normals, lights = _frame_inputs(i, L)
        depth = obj_depth * (1.0 + 0.1 * i)
        kw = dict(metal=0.5, rough=0.3, clamp01=(i != 1))
        ptr = rr.obj_rgb.data_ptr()
        shaded = rr.shade_sg(pose, bbox, normals, depth, lights, **kw)
        assert shaded.data_ptr() == ptr == rr.obj_rgb.data_ptr() and torch.equal(rr.obj_depth.view(h, w), depth)
        out = rr.render_rect(pose, rect)
        obj_rgb = shading.sg_shade(h, w, dirs, pose, bbox, normals, depth, lights, **kw)
        assert torch.equal(obj_rgb, shaded) and bool(obj_rgb.any())
        ref = r2.render_rect(pose, rect, obj_rgb=obj_rgb, obj_depth=depth)
        for k in ("rgb", "depth", "pts"):
            assert torch.equal(out[k], ref[k]), (i, k)
        assert int(out["total_samples"]) == int(ref["total_samples"])
        assert rr.n_captures == 2, i
    # render_insert_sg is the composed calls on render_insert's cached renderer
    rect, bbox, L = frames[0]
    normals, lights = _frame_inputs(0, L)
    out = render_insert_sg(model, pose, dirs, h, w, rect, bbox, normals, obj_depth, lights, metal=0.5, rough=0.3, **APP)
    assert len(model._insert_renderers) == 1
    cached = next(iter(model._insert_renderers.values()))
    obj_rgb = shading.sg_shade(h, w, dirs, pose, bbox, normals, obj_depth, lights, metal=0.5, rough=0.3, clamp01=True)
    assert torch.equal(cached.obj_rgb.view(h, w, 3), obj_rgb)
    got = {k: out[k].clone() for k in ("rgb", "depth", "pts")}
    ref = render_insert(model, pose, dirs, h, w, rect, obj_rgb, obj_depth, **APP)
    assert len(model._insert_renderers) == 1 and cached.n_captures == 2
    for k in ("rgb", "depth", "pts"):
        assert torch.equal(got[k], ref[k]), k
    # clamp01 defaults to not output_radiance
    bright = lights.clone()
    bright[:, 4:] *= 50
    render_insert_sg(model, pose, dirs, h, w, rect, bbox, normals, obj_depth, bright, metal=0.5, rough=0.3, **APP)
    assert float(cached.obj_rgb.max()) == 1.0
    render_insert_sg(model, pose, dirs, h, w, rect, bbox, normals, obj_depth, bright, metal=0.5, rough=0.3,
                     clamp01=False, **APP)
    assert float(cached.obj_rgb.max()) > 1.0


def test_argument_checks(fx):
    a = _args(fx, "maps_decay_ldr")
    n = 13 * 11
    bad = [dict(normals=a["normals"].double()), dict(obj_depth=a["obj_depth"].half()), dict(lSGs=a["lSGs"].double()),
           dict(directions=a["directions"].double()), dict(c2w=a["c2w"].double()),
           dict(lSGs=a["lSGs"][:, :6].contiguous()), dict(lSGs=a["lSGs"].reshape(-1)),
           dict(decay=a["decay"][:, :32].contiguous()), dict(decay=a["decay"][:n - 1].contiguous()),
           dict(decay=a["decay"].double()), dict(metal=a["metal"][:n - 1].contiguous()),
           dict(rough=a["rough"][:5].contiguous()), dict(rough=a["rough"].double()),
           dict(albedo=a["albedo"][:2].contiguous()), dict(albedo=a["albedo"].half()),
           dict(normals=a["normals"][:n - 1].contiguous()), dict(obj_depth=a["obj_depth"][:n - 1].contiguous()),
           dict(out=torch.zeros(13, 11, 3, dtype=torch.float64, device=DEV)),
           dict(out=torch.zeros(13, 10, 3, device=DEV)), dict(normals=a["normals"].t()),
           dict(bbox=torch.tensor([0, 0, 4, 4], device=DEV)), dict(H=0)]
    for over in bad:
        with pytest.raises(ValueError):
            shading.sg_shade(**dict(a, **over))
    assert torch.isfinite(shading.sg_shade(**a)).all()
