"""tests/insert_ref.py (the numpy restatement of an insertion frame's glue:
rectangle -> pixels, mesh clip, IM_bkg blend, canvas scatter) held to
tests/golden/insert_frame.npz, which the reference's own render() and app
slices produced (tests/golden/make_insert_golden.py); and what that fixture's
designed inputs must contain for the GPU tests to mean anything.  No GPU."""
import numpy as np
import pytest

import insert_ref as IR
from capi import C, FUNCS
from fixture_model import load


@pytest.fixture(scope="module")
def fx():
    return load("insert_frame")


def _n(fx):
    hs, ws, hl, wl = (int(v) for v in fx["rect"])
    return (hl - hs) * (wl - ws)


def test_fixture_frame_is_the_designed_one(fx):
    H, W = int(fx["H"]), int(fx["W"])
    hs, ws, hl, wl = (int(v) for v in fx["rect"])
    assert (H, W) == (16, 16)
    assert 0 <= hs < hl <= H and 0 <= ws < wl <= W
    assert hl - hs != wl - ws and _n(fx) < H * W          # neither square nor full
    assert float(fx["T_threshold"]) == 1e-2 and int(fx["max_samples"]) == 100  # the app's settings
    for k in ("rays_o", "rays_d", "rgb", "rgb_pre", "pts"):
        assert fx[k].shape == (_n(fx), 3) and fx[k].dtype == np.float32, k
    for k in ("hits_raw", "hits_clip"):
        assert fx[k].shape == (_n(fx), 2) and fx[k].dtype == np.float32, k


def test_rectangle_to_pixel_index_is_exact(fx):
    H, W = int(fx["H"]), int(fx["W"])
    pix = IR.rect_pixels(fx["rect"], H, W)
    assert pix.dtype == np.int64 and np.array_equal(pix, fx["pix"])
    # the app's slice of the camera (main.py:639) is the gather through these indices
    hs, ws, hl, wl = (int(v) for v in fx["rect"])
    sl = fx["directions"].reshape(H, W, 3)[hs:hl, ws:wl].reshape(-1, 3)
    assert np.array_equal(fx["directions"][pix], sl)
    assert np.array_equal(fx["obj_depth"].reshape(-1)[pix], fx["obj_depth"][hs:hl, ws:wl].reshape(-1))


def test_rect_clamp_and_empty_rectangles():
    assert IR.rect_clamp((-3, 2, 50, 43), 48, 40) == ((0, 2, 48, 40), 48 * 38)
    assert IR.rect_clamp((5, 7, 5, 9), 48, 40)[1] == 0        # no rows
    assert IR.rect_clamp((9, 7, 5, 9), 48, 40)[1] == 0        # inverted
    assert IR.rect_clamp((60, 0, 70, 10), 48, 40) == ((48, 0, 48, 10), 0)  # wholly outside
    assert IR.rect_pixels((9, 7, 5, 9), 48, 40).size == 0
    assert np.array_equal(IR.rect_pixels((47, 39, 48, 40), 48, 40), [48 * 40 - 1])
    # H != W: a row/column swap gives other indices
    assert np.array_equal(IR.rect_pixels((1, 2, 3, 4), 48, 40), [42, 43, 82, 83])


def test_mesh_clip_is_exact(fx):
    pix = fx["pix"]
    clip = IR.mesh_clip(fx["hits_raw"], fx["obj_depth"].reshape(-1)[pix])
    assert clip.dtype == np.float32
    assert np.array_equal(clip.view(np.int32), fx["hits_clip"].view(np.int32))
    assert np.array_equal(clip[:, 0], fx["hits_raw"][:, 0])  # only t2 moves


def test_designed_inputs_hold_every_class(fx):
    """Conditions on the fixture's inputs (not measurements): at least one ray of the rectangle per class."""
    depth = fx["obj_depth"].reshape(-1)[fx["pix"]]
    cls = IR.ray_classes(fx["hits_raw"], depth)
    for name, m in cls.items():
        assert int(m.sum()) >= 1, name
    clip, raw = fx["hits_clip"], fx["hits_raw"]
    # a miss keeps -1 whether or not the object covers it
    assert np.all(clip[cls["miss"]] == -1) and np.any(depth[cls["miss"]] >= IR.DEPTH_EPS)
    # depth 0, (0, 1e-6) and the fp32 number below 1e-6: no object, the ray keeps its length
    for name in ("depth_zero", "depth_tiny", "depth_eps_below"):
        m = cls[name] & ~cls["miss"]
        assert m.any() and np.array_equal(clip[m], raw[m]), name
    # float32(1e-6) and the number above it: an object in front of the near plane, zero length
    for name in ("depth_eps", "depth_eps_above"):
        m = cls[name] & ~cls["miss"]
        assert m.any() and np.array_equal(clip[m, 1], raw[m, 0]), name
    assert np.float32(1e-6) == IR.DEPTH_EPS and np.float64(IR.DEPTH_EPS) != 1e-6  # the comparison is in fp32
    # depth <= t1: zero length, no sample, the colour is the object's exactly
    z = cls["zero_length"]
    assert np.array_equal(clip[z, 1], clip[z, 0])
    assert np.all(fx["opacity"][z] == 0) and np.all(fx["depth"][z] == 0)
    assert np.array_equal(fx["rgb"][z], fx["obj_rgb"].reshape(-1, 3)[fx["pix"]][z])
    # t1 < depth < t2: the ray ends at the object
    i = cls["inside"]
    assert np.array_equal(clip[i, 1], depth[i]) and np.all(clip[i, 1] < raw[i, 1])
    # depth >= t2: untouched
    b = cls["beyond"]
    assert np.array_equal(clip[b], raw[b])


def test_the_sample_budget_cuts_rays_short_and_n_rays_shows(fx):
    """At least one ray is alive when the max_samples=100 budget ends, so the N_samples schedule -- and with it the
    N_rays of the iteration rule -- shows in the pixels; total_samples differs from the same rays at N_rays = H*W."""
    ns, alive = fx["n_samples"], fx["alive_after"]
    n = _n(fx)
    assert len(ns) == len(alive) and int(alive[-1]) >= 1           # the last iteration composited and left rays
    assert int(ns.sum()) >= 100 > int(ns[:-1].sum())               # it was the budget that ended the loop
    # the schedule is the rule of rendering.py:196 at N_rays = n (min_samples 1)
    prev = np.concatenate([[n], alive[:-1]])
    assert np.array_equal(ns, np.maximum(np.minimum(n // prev, 64), 1))
    full = np.maximum(np.minimum(int(fx["H"]) * int(fx["W"]) // prev, 64), 1)
    assert not np.array_equal(full, ns)
    assert int(fx["total_samples"]) != int(fx["total_samples_full_n"])
    assert not np.array_equal(fx["opacity"], fx["opacity_full_n"])
    # no transmittance the composites saw is within 2 % of T_threshold: the fp16 product (sigma ~1e-3 from the
    # oracle's) ends every ray at the same sample, so the schedule above is the product's too
    assert float(fx["t_margin"]) >= 0.02
    # both endings are present: rays that ended on T <= T_threshold and rays that never did
    assert np.any(fx["opacity"] >= 0.99) and np.any((fx["opacity"] > 0) & (fx["opacity"] < 0.99))


def test_blend_scatter_and_points(fx):
    pix = fx["pix"]
    bkg = fx["obj_rgb"].reshape(-1, 3)[pix]
    rgb = IR.blend(fx["rgb_pre"], fx["opacity"], bkg)
    assert rgb.dtype == np.float32
    assert float(np.abs(rgb - fx["rgb"]).max()) <= 1e-6
    assert np.any(fx["rgb"] != fx["rgb_pre"])
    canvas_rgb = IR.scatter(fx["canvas0_rgb"], pix, rgb)
    canvas_depth = IR.scatter(fx["canvas0_depth"], pix, fx["depth"])
    assert float(np.abs(canvas_rgb - fx["canvas_rgb"]).max()) <= 1e-6
    assert np.array_equal(canvas_depth, fx["canvas_depth"])
    # outside the rectangle the canvases keep their bits; inside, nothing of the junk is left
    outside = np.ones(int(fx["H"]) * int(fx["W"]), dtype=bool)
    outside[pix] = False
    assert np.array_equal(canvas_rgb.reshape(-1, 3)[outside], fx["canvas0_rgb"].reshape(-1, 3)[outside])
    assert np.array_equal(fx["canvas_rgb"].reshape(-1, 3)[outside], fx["canvas0_rgb"].reshape(-1, 3)[outside])
    assert np.all(fx["canvas0_rgb"] >= 2.0) and np.all(fx["canvas_rgb"].reshape(-1, 3)[pix] < 2.0)
    pts = IR.surface_pts(fx["rays_o"], fx["rays_d"], fx["depth"])
    assert float(np.abs(pts - fx["pts"]).max()) <= 1e-6


def test_header_declares_the_insertion_entry_points():
    for name in ("ngp_insert_frame_begin", "ngp_render_test_march_n", "ngp_insert_frame_finish"):
        assert name in FUNCS, name
    assert C["NGP_INSERT_HEADER_WORDS"] == 8 and C["NGP_RENDER_STATE_WORDS"] == 8
    # the `_n` march is the plain one with the count from the device and a capacity
    a, b = FUNCS["ngp_render_test_march"][1], FUNCS["ngp_render_test_march_n"][1]
    assert len(b) == len(a) + 1 and b[:3] == a[:3] and b[5:] == a[4:]


def test_argument_errors_return_before_any_launch():
    """Host-side checks of the new entry points (no GPU needed): NGP_EINVAL (-1)."""
    import ctypes

    import vren
    L = vren.lib()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails its checks first
    f = ctypes.c_float(0.01)
    begin = lambda H, W, ptrs: L.ngp_insert_frame_begin(ptrs[0], H, W, *ptrs[1:5], f, *ptrs[5:], None)  # noqa: E731
    ok = [p] * 15
    assert begin(0, 16, ok) == -1 and begin(16, 0, ok) == -1 and begin(-1, 16, ok) == -1
    assert begin(1 << 16, 1 << 15, ok) == -1                      # H*W = 2^31
    assert begin(1 << 31, 1, ok) == -1
    for k in range(15):                                           # every pointer is needed
        assert begin(16, 16, ok[:k] + [None] + ok[k + 1:]) == -1, k
    finish = lambda H, W, ptrs: L.ngp_insert_frame_finish(ptrs[0], H, W, *ptrs[1:], None)  # noqa: E731
    ok = [p] * 10
    assert finish(0, 16, ok) == -1 and finish(1 << 16, 1 << 15, ok) == -1
    for k in range(9):                                            # (frame_pts, the last one, may be null)
        assert finish(16, 16, ok[:k] + [None] + ok[k + 1:]) == -1, k
    bf = ctypes.c_void_p(256)

    def march(n_dev=p, cap=64, bitfield=bf, min_samples=1, parity=0, state=p, bufs=p):
        return L.ngp_render_test_march_n(bufs, bufs, bufs, n_dev, cap, bitfield, 1, 128, ctypes.c_float(0.5),
                                         ctypes.c_float(0.0), 1024, min_samples, 100, parity, state, bufs, None, bufs,
                                         bufs, bufs, bufs, bufs, bufs, None)
    assert march(n_dev=None) == -1 and march(cap=-1) == -1 and march(cap=(1 << 31) - 1) == -1
    assert march(parity=2) == -1 and march(parity=-1) == -1 and march(min_samples=0) == -1
    assert march(state=None) == -1 and march(bufs=None) == -1 and march(bitfield=None) == -1
    assert march(bitfield=ctypes.c_void_p(260)) == -1             # (the bitfield's 8-byte alignment)
    assert march(cap=1 << 29, min_samples=4) == -1                # slots past 2^31
