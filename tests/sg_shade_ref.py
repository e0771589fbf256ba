"""Per-pixel fp64 restatement of the object shade (csrc/shade.hip,
ngp_sg_shade): the SG branch of the reference app's render_object and its
SG_render_core, written from the formulas -- numpy, a loop over the lights in
the kernel's own order (lights ascending, the rectifier after the sum).

Inputs may be fp32; everything is computed in float64.  Scalars (metal, rough,
the constants) are Python floats, as the reference takes them.
"""
import math

import numpy as np

EPS = 1e-6
DEPTH_EPS = np.float32(1e-6)  # the cover test is an fp32 compare (main.py:526)
COS_LAMBDA, COS_AMP, COS_OFF = 0.0315, 32.7080, 31.7003


def clamp_bbox(bbox, H, W):
    """-> (hs, ws, hl, wl) clamped to the frame, and the pixel count (0 for an empty or inverted box)"""
    hs, ws, hl, wl = (int(v) for v in bbox)
    hs, hl = min(max(hs, 0), H), min(max(hl, 0), H)
    ws, wl = min(max(ws, 0), W), min(max(wl, 0), W)
    h, w = hl - hs, wl - ws
    return (hs, ws, hl, wl), (h * w if h > 0 and w > 0 else 0)


def cover_mask(H, W, bbox, obj_depth):
    """(H*W) bool: in the clamped box and obj_depth > float32(1e-6), compared in fp32"""
    (hs, ws, hl, wl), n = clamp_bbox(bbox, H, W)
    m = np.zeros((H, W), dtype=bool)
    if n:
        m[hs:hl, ws:wl] = True
    return m.reshape(-1) & (np.asarray(obj_depth, dtype=np.float32).reshape(-1) > DEPTH_EPS)


def view_dirs(directions, c2w):
    """-(normalize(directions @ R^T)) in fp64: the unit direction from the surface to the camera"""
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3) @ np.asarray(c2w, dtype=np.float64)[:, :3].T
    return -(d / np.sqrt((d * d).sum(-1, keepdims=True)))


def _hemi_consts(lam):
    lv = np.maximum(lam, EPS)
    il = 1.0 / lv
    t = np.sqrt(lv) * (1.6988 + 10.8438 * il) / (1.0 + 6.2201 * il + 10.2415 * il * il)
    inv_a = np.exp(-t)
    k = 2.0 * math.pi / lv
    e1 = np.exp(-lv)
    return t, inv_a, k * (e1 - np.exp(-2.0 * lv)), k * (1.0 - e1)


def _hemi_integral(consts, cos_beta):
    t, inv_a, Ab, Au = consts
    e = np.exp(-(t * np.abs(cos_beta)))
    up = cos_beta >= 0
    ie = inv_a * e
    num = np.where(up, 1.0 - ie, e - inv_a)
    den = np.where(up, 1.0 - inv_a + e - ie, (1.0 - inv_a) * (e + 1.0))
    s = num / den
    return Ab * (1.0 - s) + Au * s


def _product(ax1, l1, ax2, l2):
    """axes (P,3), sharpnesses (P,) or scalars -> the product lobe's axis, sharpness and amplitude gain"""
    lm = l1 + l2
    um = (np.reshape(l1, (-1, 1)) * ax1 + np.reshape(l2, (-1, 1)) * ax2) / np.reshape(lm, (-1, 1))
    ln = np.sqrt((um * um).sum(-1))
    return um * (1.0 / ln)[:, None], lm * ln, np.exp(lm * (ln - 1.0))


def _irradiance(ax, lam, amp, n):
    """one lobe per pixel (ax (P,3), lam (P,), amp (P,3)) against the clamped cosine about n (P,3), before the sum"""
    axc, lc, gain = _product(ax, lam, n, COS_LAMBDA)
    w_cos = _hemi_integral(_hemi_consts(lc), (axc * n).sum(-1))
    w_own = _hemi_integral(_hemi_consts(lam), (ax * n).sum(-1))
    return w_cos[:, None] * (amp * COS_AMP * gain[:, None]) - COS_OFF * (w_own[:, None] * amp)


def sg_shade_ref(H, W, directions, c2w, bbox, normals, obj_depth, lSGs, metal=0.9, rough=0.2, albedo=None,
                 decay=None, clamp01=True):
    """-> obj_rgb (H,W,3) float64.  metal / rough: a Python float or an (H*W) map (the rough map is clipped to
    [0.2, 1], the scalar is not); albedo: None, (1,3) or (H*W,3); decay: None or (H*W, L)."""
    n_pix = H * W
    mask = cover_mask(H, W, bbox, obj_depth)
    idx = np.nonzero(mask)[0]
    out = np.zeros((n_pix, 3))
    if idx.size == 0:
        return out.reshape(H, W, 3)
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    nrm = f64(normals).reshape(-1, 3)[idx]
    nrm = nrm / np.sqrt((nrm * nrm).sum(-1, keepdims=True))
    v = view_dirs(f64(directions).reshape(-1, 3)[idx], c2w)
    P = idx.size
    if albedo is None:
        alb = np.ones((P, 3))
    else:
        alb = f64(albedo).reshape(-1, 3)
        alb = np.broadcast_to(alb, (P, 3)) if alb.shape[0] == 1 else alb[idx]
    met = np.full(P, float(metal)) if np.ndim(metal) == 0 else f64(metal).reshape(-1)[idx]
    rgh = np.full(P, float(rough)) if np.ndim(rough) == 0 else np.clip(f64(rough).reshape(-1)[idx], 0.2, 1.0)
    lights = f64(lSGs).reshape(-1, 7)
    dec = None if decay is None else f64(decay).reshape(n_pix, -1)[idx]

    ndv = (nrm * v).sum(-1)
    dax = ndv[:, None] * nrm * 2.0 - v
    m2 = rgh * rgh
    dlam = 2.0 / m2 / (4.0 * np.maximum(ndv, EPS))
    damp = 1.0 / (math.pi * m2)
    spec, diff = np.zeros((P, 3)), np.zeros((P, 3))
    for j in range(lights.shape[0]):
        lax = np.broadcast_to(lights[j, :3], (P, 3))
        llam = np.full(P, lights[j, 3])
        amp = np.broadcast_to(lights[j, 4:], (P, 3))
        if dec is not None:
            amp = amp * dec[:, j:j + 1]
        pax, plam, pgain = _product(dax, dlam, lax, llam)
        spec += _irradiance(pax, plam, damp[:, None] * amp * pgain[:, None], nrm)
        diff += _irradiance(lax, llam, amp, nrm)
    spec, diff = np.maximum(spec, 0.0), np.maximum(diff, 0.0)

    ndv_pos = np.maximum(ndv, 0.0)
    om5 = (1.0 - ndv_pos) ** 5
    with np.errstate(divide="ignore"):
        tan2 = m2 * np.maximum(1.0 / (ndv_pos * ndv_pos) - 1.0, 0.0)
    G = 1.0 / (0.5 * (np.sqrt(1.0 + tan2) - 1.0) * 2.0 + 1.0)
    F0 = 0.04 * (1.0 - met)[:, None] + alb * met[:, None]
    F = F0 + (1.0 - F0) * om5[:, None]
    Moi = F * G[:, None] / (4.0 * ndv_pos * ndv_pos + EPS)[:, None]
    kS = F0 + (np.maximum((1.0 - rgh)[:, None], F0) - F0) * om5[:, None]
    kD = (1.0 - kS) * (1.0 - met)[:, None]
    rad = kD * (alb / math.pi * diff) + Moi * spec
    out[idx] = np.clip(rad, 0.0, 1.0) if clamp01 else np.maximum(rad, 0.0)
    return out.reshape(H, W, 3)


def pixel_classes(H, W, directions, c2w, bbox, normals, obj_depth):
    """Every pixel of the frame in exactly one class (bool (H*W) each): uncovered; of the covered ones facing
    (n.v >= 0.3), middle (0.05 <= n.v < 0.3), grazing (0 < n.v < 0.05), back (n.v <= 0), n.v in fp64."""
    mask = cover_mask(H, W, bbox, obj_depth)
    nrm = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = nrm / np.sqrt((nrm * nrm).sum(-1, keepdims=True))
    ndv = (nrm * view_dirs(directions, c2w)).sum(-1)
    return {"uncovered": ~mask, "facing": mask & (ndv >= 0.3), "middle": mask & (ndv >= 0.05) & (ndv < 0.3),
            "grazing": mask & (ndv > 0) & (ndv < 0.05), "back": mask & (ndv <= 0)}


CLASSES = ("uncovered", "facing", "middle", "grazing", "back")

# The recorded configurations of tests/golden/sg_shade.npz (tests/golden/make_sg_golden.py):
# name: lights (the first L of the fixture's), rough / metal (a number or "map"), albedo (None, "row", "map"),
# decay (present or not), clamp01
CONFIGS = {
    "scalars_ldr": dict(L=33, rough=0.2, metal=0.9, albedo=None, decay=False, clamp01=True),
    "rough01_hdr": dict(L=33, rough=0.1, metal="map", albedo="row", decay=True, clamp01=False),
    "maps_hdr": dict(L=33, rough="map", metal=0.3, albedo="map", decay=False, clamp01=False),
    "one_light": dict(L=1, rough=0.2, metal=0.9, albedo=None, decay=False, clamp01=True),
    "maps_decay_ldr": dict(L=33, rough="map", metal="map", albedo="map", decay=True, clamp01=True),
}


def config_args(fx, name):
    """The fixture's arrays as sg_shade's arguments for configuration `name` (numpy; scalars stay Python floats)"""
    cfg = CONFIGS[name]
    L = cfg["L"]
    return dict(H=int(fx["H"]), W=int(fx["W"]), directions=fx["directions"], c2w=fx["pose"],
                bbox=tuple(int(v) for v in fx["bbox"]), normals=fx["normals"], obj_depth=fx["obj_depth"],
                lSGs=np.ascontiguousarray(fx["lSGs"][:L]),
                metal=fx["metal_map"] if cfg["metal"] == "map" else cfg["metal"],
                rough=fx["rough_map"] if cfg["rough"] == "map" else cfg["rough"],
                albedo={None: None, "row": fx["albedo_row"], "map": fx["albedo_map"]}[cfg["albedo"]],
                decay=np.ascontiguousarray(fx["decay"][:, :L]) if cfg["decay"] else None, clamp01=cfg["clamp01"])
