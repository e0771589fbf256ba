"""A numpy restatement of what surrounds the render loop in an insertion frame
(csrc/insert.hip; the reference's insert/main.py:632-660 and models/rendering.py
:38-44, 245-250).  A helper module (not a conftest), like render_ref.py:
test_insert_ref_cpu.py holds it to the reference glue's fixture
(tests/golden/insert_frame.npz), test_insert_gpu.py uses its index rule.

  rect_clamp    the rectangle clamped to the frame, n = 0 when inverted or empty
  rect_pixels   ray i of the rectangle -> pixel index, row-major as the app slices
  mesh_clip     hits_t[:,1] = max(min(t2, depth), t1) where depth >= 1e-6
  blend         rgb + IM_bkg * (1 - opacity), fp32 like the reference's torch expression
  scatter       last_rgb[hs:hl, ws:wl] = rgb etc. through the pixel indices
  surface_pts   rays_o + rays_d * depth
"""
import numpy as np

F32 = np.float32
DEPTH_EPS = F32(1e-6)   # models/rendering.py:40  valid_depth = mesh_depth_map >= 1e-6


def rect_clamp(rect, H, W):
    """(hs, ws, hl, wl) -> the clamped rectangle and its ray count"""
    hs, ws, hl, wl = (int(v) for v in rect)
    hs, hl = min(max(hs, 0), H), min(max(hl, 0), H)
    ws, wl = min(max(ws, 0), W), min(max(wl, 0), W)
    h, w = hl - hs, wl - ws
    return (hs, ws, hl, wl), (h * w if h > 0 and w > 0 else 0)


def rect_pixels(rect, H, W):
    """pixel index p = (hs + i // w) * W + ws + i % w of ray i = 0..n-1 (int64)"""
    (hs, ws, hl, wl), n = rect_clamp(rect, H, W)
    i = np.arange(n, dtype=np.int64)
    w = max(wl - ws, 1)
    return (hs + i // w) * W + ws + i % w


def mesh_clip(hits, depth):
    """hits (n,2) fp32 = (t1, t2), depth (n) fp32 -> the clipped copy"""
    hits = np.array(hits, dtype=F32, copy=True)
    depth = np.asarray(depth, dtype=F32)
    valid = depth >= DEPTH_EPS
    hits[valid, 1] = np.maximum(np.minimum(hits[valid, 1], depth[valid]), hits[valid, 0])
    return hits


def blend(rgb, opacity, bkg):
    """fp32: m = fl(1 - opacity), fl(rgb + fl(bkg m))"""
    m = (F32(1) - np.asarray(opacity, dtype=F32))[:, None]
    return np.asarray(rgb, dtype=F32) + np.asarray(bkg, dtype=F32) * m


def scatter(canvas, pix, values):
    """canvas (H,W,c) or (H,W) -> a copy with the rectangle's pixels replaced"""
    out = np.array(canvas, copy=True)
    flat = out.reshape(canvas.shape[0] * canvas.shape[1], -1)
    flat[pix] = np.asarray(values).reshape(len(pix), -1)
    return out


def surface_pts(rays_o, rays_d, depth):
    return np.asarray(rays_o, dtype=F32) + np.asarray(rays_d, dtype=F32) * np.asarray(depth, dtype=F32)[:, None]


def ray_classes(hits_raw, depth):
    """the classes of test_insert_ref_cpu.py's conditions -> dict of boolean masks over the rays"""
    t1, t2 = hits_raw[:, 0], hits_raw[:, 1]
    depth = np.asarray(depth, dtype=F32)
    hit = t1 >= 0
    below, above = np.nextafter(DEPTH_EPS, F32(0)), np.nextafter(DEPTH_EPS, F32(1))
    return {
        "miss": ~hit,
        "depth_zero": depth == 0,
        "depth_tiny": (depth > 0) & (depth < DEPTH_EPS),
        "depth_eps": depth == DEPTH_EPS,
        "depth_eps_below": depth == below,
        "depth_eps_above": depth == above,
        "zero_length": hit & (depth >= DEPTH_EPS) & (depth <= t1),
        "inside": hit & (depth > t1) & (depth < t2),
        "beyond": hit & (depth >= t2),
    }
