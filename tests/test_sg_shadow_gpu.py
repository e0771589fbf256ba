"""The SSDF soft shadows on the device (csrc/shadow.hip, sg_shadow.SGShadow,
InsertRenderer.self_shadow_decay / cast_shadow,
models.rendering.render_insert_sg_shadow) against the golden fixture of the
reference's own insert/sg_shadow.py (tests/golden/sg_shadow.npz).

The bar, per class of point (factor) and of pair (decay): |kernel - ref64| <=
4 x the reference's own fp32 deviation from its fp64 run, the maximum over
three orders of the C axis (test_sg_shadow_ref_cpu.py states it; the kernel
sums the components in its own fixed order and uses the device's acos, atan2,
asin, log10, exp and pow).  Every point and every pair is in exactly one
class.  The factor is recorded, with its own deviations, at L = 1, 32 (one
light tile, NGP_SSDF_LIGHT_TILE) and 33; for L = 32 the decay's reference is
the first 32 columns of the L = 33 record (a pair's decay is its own).
"""
import numpy as np
import pytest
import torch

import sg_shadow
import shading
from capi import C as CONSTS
from fixture_model import load
from models.rendering import render_insert_sg, render_insert_sg_shadow
from test_golden_gpu import _product_model
from test_sg_shadow_ref_cpu import CS, assert_decay, assert_factor, case, rotated

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = CONSTS["NGP_SSDF_LIGHT_TILE"]
APP = dict(T_threshold=1e-2, max_samples=100)


@pytest.fixture(scope="module")
def fx():
    return load("sg_shadow")


def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _shadow(fx, C, **kw):
    a = case(fx, C, 0)
    return sg_shadow.SGShadow(_d(a["coeff"]), _d(a["components"]), _d(a["mean"]), _d(a["fh_tab"]), a["vol_range"],
                              a["angle_decay_fac"], a["shadow_pow_fac"], a["self_shadow_pow_fac"], **kw)


@pytest.fixture(scope="module")
def sh128(fx):
    return _shadow(fx, 128)


def _run(sh, fx, k, L=33, idx=None):
    """(factor, decay) of the fixture's points (idx: a selection) under the first L lights, rotation k"""
    pts = fx["pts"] if idx is None else np.ascontiguousarray(fx["pts"][idx])
    pts, pos, rot = _d(pts), _d(fx["model_pos"]), _d(fx["rot_inv"]) if k else None
    scale = float(fx["scale"])
    fac = sh.calc_shadow_factor(scale, pts, pos, _d(rotated(fx, k, L)), rot)
    dec = sh.self_shadow_decay(scale, pts, pos, _d(fx["lSGs"][:L]), rot)
    return fac, dec


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("k", (0, 1))
def test_kernels_against_the_reference_fp64(fx, C, k):
    sh = _shadow(fx, C)
    fac, dec = _run(sh, fx, k)
    assert fac.dtype == dec.dtype == torch.float32 and fac.shape == (70,) and dec.shape == (70, 33)
    assert_factor(fx, f"c{C}", k, fac.cpu().numpy(), fx[f"factor64_c{C}"][k], what=f"C={C} k={k}")
    assert_decay(fx, f"c{C}", k, dec.cpu().numpy(), fx[f"decay64_c{C}"][k], what=f"C={C} k={k}")
    assert float(dec.min()) == 0.0 and float(dec.max()) == 1.0        # the exact classes are exact


@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("L", [1, TILE, TILE + 1])
def test_shapes_across_block_and_tile_edges(fx, sh128, P, L):
    """P points drawn from the fixture's 70 (a seeded order, repeats past 70): the class bars hold, and every
    point has the bits it has in the fixture's own list, whatever P and its place in the list."""
    assert TILE + 1 == 33
    idx = np.random.default_rng(P).permutation(70)
    idx = np.concatenate([idx] * 4)[:P]
    for k in (0, 1):
        fac, dec = _run(sh128, fx, k, L, idx)
        assert fac.shape == (P,) and dec.shape == (P, L)
        # (the fixture records the factor at L = 1, 32 and 33; a pair's decay does not depend on the other lights,
        # so L = 32 is judged on the first 32 columns of the L = 33 record)
        fs, ds = {1: ("l1", "l1"), TILE: ("l32", "c128"), 33: ("c128", "c128")}[L]
        assert_factor(fx, fs, k, fac.cpu().numpy(), fx[f"factor64_{fs}"][k][idx], idx=idx, what=f"P={P} L={L} k={k}")
        assert_decay(fx, ds, k, dec.cpu().numpy(), fx[f"decay64_{ds}"][k][idx][:, :L], idx=idx,
                     lights=None if L != TILE else np.arange(L), what=f"P={P} L={L} k={k}")
        base_f, base_d = _run(sh128, fx, k, L)
        sel = torch.from_numpy(idx).to(DEV)
        assert torch.equal(fac, base_f[sel]) and torch.equal(dec, base_d[sel])


def test_runs_are_bit_equal_and_outputs_do_not_depend_on_each_other(fx, sh128):
    for k in (0, 1):
        pts, pos, rot = _d(fx["pts"]), _d(fx["model_pos"]), _d(fx["rot_inv"]) if k else None
        lights = _d(fx["lSGs"])
        scale = float(fx["scale"])
        f1, d1 = sh128.factor_and_decay(scale, pts, pos, lights, rot, rotate_lights=True)
        f2, d2 = sh128.factor_and_decay(scale, pts, pos, lights, rot, rotate_lights=True)
        assert torch.equal(f1, f2) and torch.equal(d1, d2)
        assert torch.equal(sh128.self_shadow_decay(scale, pts, pos, lights, rot), d1)             # decay alone
        f3, d3 = sh128.factor_and_decay(scale, pts, pos, lights, rot, rotate_lights=False)
        assert torch.equal(sh128.calc_shadow_factor(scale, pts, pos, lights, rot), f3)            # factor alone
        assert torch.equal(f3, f1) == (k == 0)
        # the (P,L,7) call of the reference's spelling: the lights times the decay
        full = sh128.calc_self_shadow_light_dacay(scale, pts, pos, lights, rot)
        assert full.shape == (70, 33, 7) and torch.equal(full[:, :, 4:], lights[None, :, 4:] * d1[:, :, None])
        assert torch.equal(full[:, :, :4], lights[None, :, :4].expand(70, 33, 4))
    # out buffers are written in place; no points is a no-op
    buf = torch.full((70,), 7.0, device=DEV)
    res = sh128.calc_shadow_factor(scale, pts, pos, lights, rot, out=buf)
    assert res.data_ptr() == buf.data_ptr() and torch.equal(buf, f3)
    assert sh128.calc_shadow_factor(scale, pts[:0], pos, lights).shape == (0,)
    assert sh128.self_shadow_decay(scale, pts[:0], pos, lights).shape == (0, 33)


def test_the_sliders_change_the_next_result(fx):
    sh = _shadow(fx, 67)
    f0, d0 = _run(sh, fx, 1)
    sh.delta_shadow_fac = 1
    f1, d1 = _run(sh, fx, 1)
    assert not torch.equal(f0, f1) and torch.equal(d0, d1)
    assert torch.allclose(f1 * f1, f0, atol=2e-6)
    sh.delta_self_shadow_fac = 0.5
    f2, d2 = _run(sh, fx, 1)
    assert torch.equal(f2, f1) and not torch.equal(d2, d1)
    sh.delta_angle_decay_fac = 1.0
    f3, d3 = _run(sh, fx, 1)
    dis = fx["dis64_c67"][1]
    outside, inside = torch.from_numpy(dis > 1.001).to(DEV), torch.from_numpy(dis < 0.999).to(DEV)
    assert not torch.equal(f3[outside], f2[outside]) and torch.equal(f3[inside], f2[inside])       # delta = 0 inside


# ------------------------------------------------------------------ the frame front end
def _host_points(dirs, pose, depth):
    """pose[:,3] + depth * normalize(ray direction) in the kernel's order of fp32 operations (IEEE +, *, /, sqrt)
    -> pts (n,3), the directions (n,3) and their lengths (n)"""
    d = np.stack([(dirs[:, 0] * pose[i, 0] + dirs[:, 1] * pose[i, 1]) + dirs[:, 2] * pose[i, 2] for i in range(3)], 1)
    dl = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    pts = pose[None, :, 3] + depth[:, None] * (d / dl[:, None])
    assert d.dtype == dl.dtype == pts.dtype == np.float32
    return np.ascontiguousarray(pts), d, dl


def _frame(fx):
    """a 13 x 11 frame (the object shade's fixture: its designed depths) seen from its pose, the model of the
    shadow fixture placed in front of the camera; and the points of the covered pixels, formed on the host in
    the kernel's order of fp32 operations (IEEE +, *, /, sqrt)"""
    sg = load("sg_shade")
    H, W = int(sg["H"]), int(sg["W"])
    dirs, pose, depth = sg["directions"], sg["pose"], sg["obj_depth"]
    f = np.float32
    pts, d, dl = _host_points(dirs, pose, depth)
    # the model 1.5 along the central ray, so that the points spread over the volume and beyond it
    centre = (pose[:, 3] + f(1.5) * (d[(H // 2) * W + W // 2] / dl[(H // 2) * W + W // 2])).astype(f)
    return dict(H=H, W=W, dirs=dirs, pose=pose, depth=depth, pts=np.ascontiguousarray(pts), model_pos=centre,
                bbox=tuple(int(v) for v in sg["bbox"]))


@pytest.mark.parametrize("k", (0, 1))
def test_frame_decay_is_the_point_entry_on_the_covered_pixels(fx, sh128, k):
    fr = _frame(fx)
    H, W, n = fr["H"], fr["W"], fr["H"] * fr["W"]
    hs, ws, hl, wl = fr["bbox"]
    rot, lights, pos = _d(fx["rot_inv"]) if k else None, _d(fx["lSGs"]), _d(fr["model_pos"])
    inbox = np.zeros((H, W), dtype=bool)
    inbox[hs:hl, ws:wl] = True
    eps = np.float32(1e-6)
    covered = inbox.reshape(-1) & (fr["depth"] > eps)
    # depths of exactly float32(1e-6) and its two neighbours: only the one above is covered, as in shade.hip
    below, above = np.nextafter(eps, np.float32(0)), np.nextafter(eps, np.float32(1))
    for val, cov in ((eps, False), (below, False), (above, True)):
        m = inbox.reshape(-1) & (fr["depth"] == val)
        assert m.any() and np.all(covered[m] == cov)
    out = torch.full((n, 33), -7.0, device=DEV)
    res = sh128.frame_decay(H, W, _d(fr["dirs"]), _d(fr["pose"]), fr["bbox"], _d(fr["depth"]), 0.5, pos, lights, out,
                            rot)
    assert res.data_ptr() == out.data_ptr()
    cov = torch.from_numpy(covered).to(DEV)
    assert bool((out[~cov] == -7.0).all())                            # uncovered rows, rows outside bbox: untouched
    want = sh128.self_shadow_decay(0.5, _d(fr["pts"][covered]), pos, lights, rot)
    assert torch.equal(out[cov], want)
    assert float(want.min()) >= 0 and float(want.max()) <= 1 and float(want.max() - want.min()) > 0.5
    # a device box reaching past the frame is clamped; an empty one writes nothing
    out2 = torch.full((n, 33), -7.0, device=DEV)
    sh128.frame_decay(H, W, _d(fr["dirs"]), _d(fr["pose"]), torch.tensor([-3, -1, H + 4, W + 9], dtype=torch.int32,
                      device=DEV), _d(fr["depth"]), 0.5, pos, lights, out2, rot)
    cov_all = torch.from_numpy(fr["depth"] > eps).to(DEV)
    assert bool((out2[~cov_all] == -7.0).all()) and bool((out2[cov_all] >= 0).all())
    assert torch.equal(out2[cov], out[cov])
    out3 = torch.full((n, 33), -7.0, device=DEV)
    sh128.frame_decay(H, W, _d(fr["dirs"]), _d(fr["pose"]), (5, 5, 5, 9), _d(fr["depth"]), 0.5, pos, lights, out3, rot)
    assert bool((out3 == -7.0).all())


# ------------------------------------------------------------------ blur and apply
@pytest.mark.parametrize("name,h,w", [("apply", 6, 5), ("apply2", 2, 2)])
def test_apply_against_the_fp64_case(fx, name, h, w):
    """a 9-term sum of products, each of magnitude at most 1, times the colour: within 4 fp32 ulps of the value"""
    rgb, fac = _d(fx[f"{name}_rgb"]), _d(fx[f"{name}_factor"])
    keep = rgb.clone()
    out = sg_shadow.shadow_apply(rgb, fac, h, w)
    assert out.shape == (h, w, 3) and out.dtype == torch.float32 and out.data_ptr() != rgb.data_ptr()
    assert torch.equal(rgb, keep)                                      # frame_rgb is left untouched
    ref = fx[f"{name}_out64"]
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print(f"{name}: worst {float((err / ulp).max()):.2f} ulp")
    assert np.all(err <= 4 * ulp)
    buf = torch.zeros(h, w, 3, device=DEV)
    assert sg_shadow.shadow_apply(rgb, fac, h, w, out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf, out)
    with pytest.raises(ValueError):
        sg_shadow.shadow_apply(rgb, fac, h, w, out=rgb)


# ------------------------------------------------------------------ the renderer
def _frame_inputs(seed, L, h, w):
    g = torch.Generator().manual_seed(seed)
    normals = (torch.randn(h, w, 3, generator=g) + torch.tensor([0.0, 0.0, -1.5])).to(DEV)
    ax = torch.nn.functional.normalize(torch.randn(L, 3, generator=g), dim=-1)
    lam = 10 ** (torch.rand(L, 1, generator=g) * 3 - 1)
    amp = torch.rand(L, 3, generator=g) * lam / 6.0
    return normals.contiguous(), torch.cat([ax, lam, amp], 1).to(DEV).contiguous()


def test_render_insert_sg_shadow_is_the_composed_calls(fx):
    ins = load("insert_frame")
    model = _product_model(ins)
    h, w = int(ins["H"]), int(ins["W"])
    dirs, pose = torch.from_numpy(ins["directions"]).to(DEV), torch.from_numpy(ins["pose"]).to(DEV)
    obj_depth = torch.from_numpy(ins["obj_depth"]).to(DEV)
    sh = _shadow(fx, 67)
    rot = _d(fx["rot_inv"])
    # the model where the object's surface is: the mean of the covered pixels' points, a radius of their spread
    host_pts = _d(_host_points(ins["directions"].reshape(-1, 3), ins["pose"], ins["obj_depth"].reshape(-1))[0])
    on = obj_depth.reshape(-1) > 1e-6
    pos = host_pts[on].mean(0).contiguous()
    scale = float((host_pts[on] - pos).norm(dim=-1).max()) * 0.5
    frames = [((5, 0, 16, 13), (3, 1, 15, 12), 7, None), ((0, 0, h, w), (0, 0, h, w), 33, rot),
              ((2, 2, 9, 14), torch.tensor([-3, 4, 12, 40], dtype=torch.int32, device=DEV), 3, rot)]
    kw = dict(metal=0.5, rough=0.3)
    for i, (rect, bbox, L, r) in enumerate(frames):
        normals, lights = _frame_inputs(i, L, h, w)
        out = render_insert_sg_shadow(model, pose, dirs, h, w, rect, bbox, normals, obj_depth, lights, sh, scale, pos,
                                      rot_inv=r, **kw, **APP)
        assert len(model._insert_renderers) == 1
        rr = next(iter(model._insert_renderers.values()))
        assert rr.n_captures == 2, i
        got = {k: out[k].clone() for k in ("rgb", "depth", "pts", "shadowed")}
        # composed: point-list decay of every pixel's point (uncovered rows are never read), render_insert_sg,
        # point-list factor on frame_pts, apply
        boxt = shading._bbox_tensor(bbox, h, w, DEV)
        hs, ws, hl, wl = (min(max(int(v), 0), lim) for v, lim in zip(boxt.tolist(), (h, w, h, w)))
        inbox = torch.zeros(h, w, dtype=torch.bool, device=DEV)
        inbox[hs:hl, ws:wl] = True
        cov = inbox.reshape(-1) & on
        assert bool(cov.any())
        decay = torch.ones(h * w, L, device=DEV)
        decay[cov] = sh.self_shadow_decay(scale, host_pts[cov].contiguous(), pos, lights, r)
        assert torch.equal(decay, rr.decay)
        ref = render_insert_sg(model, pose, dirs, h, w, rect, bbox, normals, obj_depth, lights, decay=decay, **kw, **APP)
        for k in ("rgb", "depth", "pts"):
            assert torch.equal(got[k], ref[k]), (i, k)                # the canvases: unshadowed, as with this decay
        lrot = lights
        if r is not None:
            lrot = lights.clone()
            lrot[:, :3] = (r @ lrot[:, :3].T).T
        factor = sh.calc_shadow_factor(scale, ref["pts"].reshape(-1, 3), pos, lrot, r)
        assert torch.equal(factor, rr.frame_factor)
        want = sg_shadow.shadow_apply(ref["rgb"], factor, h, w)
        assert torch.equal(got["shadowed"], want) and not torch.equal(want, ref["rgb"])
        assert rr.n_captures == 2 and len(model._insert_renderers) == 1
    # both passes off: render_insert_sg
    rect, bbox, L, r = frames[0]
    normals, lights = _frame_inputs(0, L, h, w)
    off = render_insert_sg_shadow(model, pose, dirs, h, w, rect, bbox, normals, obj_depth, lights, sh, scale, pos,
                                  self_shadow=False, gen_shadow=False, **kw, **APP)
    assert "shadowed" not in off
    got = {k: off[k].clone() for k in ("rgb", "depth", "pts")}
    ref = render_insert_sg(model, pose, dirs, h, w, rect, bbox, normals, obj_depth, lights, **kw, **APP)
    for k in ("rgb", "depth", "pts"):
        assert torch.equal(got[k], ref[k]), k
    # the slider: the next frame's shadow follows delta_shadow_fac
    a = render_insert_sg_shadow(model, pose, dirs, h, w, rect, bbox, normals, obj_depth, lights, sh, scale, pos,
                                **kw, **APP)["shadowed"].clone()
    sh.delta_shadow_fac = 4
    b = render_insert_sg_shadow(model, pose, dirs, h, w, rect, bbox, normals, obj_depth, lights, sh, scale, pos,
                                **kw, **APP)["shadowed"]
    assert not torch.equal(a, b) and bool((b <= a).all())
    assert next(iter(model._insert_renderers.values())).n_captures == 2


def test_argument_checks(fx, sh128):
    pts, pos, lights = _d(fx["pts"]), _d(fx["model_pos"]), _d(fx["lSGs"])
    rot = _d(fx["rot_inv"])
    bad = [dict(pts=pts.double()), dict(pts=pts[:, :2].contiguous()), dict(pts=pts.t()), dict(pts=pts.cpu()),
           dict(model_pos=pos.double()), dict(model_pos=pos[:2].contiguous()), dict(lSGs=lights[:, :6].contiguous()),
           dict(lSGs=lights.double()), dict(lSGs=lights[:0]), dict(rot_inv=rot[:2].contiguous()),
           dict(rot_inv=rot.double()), dict(scale=0.0), dict(out=torch.zeros(69, device=DEV)),
           dict(out=torch.zeros(70, dtype=torch.float64, device=DEV))]
    for over in bad:
        a = dict(scale=0.5, pts=pts, model_pos=pos, lSGs=lights, rot_inv=rot)
        a.update(over)
        with pytest.raises(ValueError):
            sh128.calc_shadow_factor(**a)
    with pytest.raises(ValueError):
        sh128.self_shadow_decay(0.5, pts, pos, lights, out=torch.zeros(70, 32, device=DEV))
    with pytest.raises(ValueError):
        sg_shadow.SGShadow(sh128.coeff, sh128.components[:5].contiguous(), sh128.mean, sh128.fh_tab, 2.0)
    with pytest.raises(ValueError):
        sg_shadow.SGShadow(sh128.coeff.double(), sh128.components, sh128.mean, sh128.fh_tab, 2.0)
    with pytest.raises(ValueError):
        sg_shadow.shadow_apply(torch.zeros(1, 5, 3, device=DEV), torch.zeros(1, 5, device=DEV), 1, 5)
    with pytest.raises(ValueError):
        sg_shadow.shadow_apply(torch.zeros(4, 5, 3, device=DEV), torch.zeros(4, 4, device=DEV), 4, 5)
