"""Per-pair fp64 restatement of the SSDF soft shadows (insert/sg_shadow.py of
the reference; csrc/shadow.hip, sg_shadow.py here) in numpy loops: no
grid_sample, no matrix product -- every sample is written out from the
definition of bilinear interpolation, so a transposed axis, a wrong corner
convention or a wrong padding rule in the kernels or in the torch formulation
shows against it.  Also the blur-and-apply step and the classes the fp32 bars
are recorded per.
"""
import numpy as np

HALF_PI = np.pi / 2
LUMA = (0.2989, 0.5870, 0.1140)
POINT_CLASSES = ("inside", "outside")
# every pair in exactly one, tested in this order
PAIR_CLASSES = ("low", "saturated", "deep", "high", "mid")
DEEP, SATURATED = 1e-3, 1.05


def _axis_false(x, n):
    """pixel-centre coordinates (align_corners False), border padding -> (i0, i1, w0, w1)"""
    g = min(max(((x + 1.0) * n - 1.0) / 2.0, 0.0), n - 1.0)
    i0 = int(np.floor(g))
    return i0, min(i0 + 1, n - 1), (i0 + 1.0) - g, g - i0


def _axis_true(x, n):
    """corner coordinates (align_corners True), border padding"""
    g = min(max((x + 1.0) / 2.0 * (n - 1), 0.0), n - 1.0)
    i0 = int(np.floor(g))
    return i0, min(i0 + 1, n - 1), (i0 + 1.0) - g, g - i0


def sample2d(img, x, y):
    """img (..., h, w) at (x along w, y along h)"""
    h, w = img.shape[-2:]
    x0, x1, wx0, wx1 = _axis_false(x, w)
    y0, y1, wy0, wy1 = _axis_false(y, h)
    return (img[..., y0, x0] * wx0 * wy0 + img[..., y0, x1] * wx1 * wy0 + img[..., y1, x0] * wx0 * wy1
            + img[..., y1, x1] * wx1 * wy1)


def sample_volume(coeff, q):
    """coeff (G,G,G,C) as stored, at q = (x, y, z) in [-1,1]^3: x indexes the first axis -> (C)"""
    G = coeff.shape[0]
    ax = [_axis_true(float(v), G) for v in q]
    out = np.zeros(coeff.shape[-1])
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                w = ax[0][2 + dx] * ax[1][2 + dy] * ax[2][2 + dz]
                out += w * coeff[ax[0][dx], ax[1][dy], ax[2][dz]]
    return out


def lights_pre(lSGs, components, mean, rot=None):
    """-> comp_s (L,C), mean_s (L), row (L), fh_n (L), inte_L (3)"""
    lSGs = np.asarray(lSGs, dtype=np.float64)
    components, mean = np.asarray(components, dtype=np.float64), np.asarray(mean, dtype=np.float64)
    mean = mean.reshape(mean.shape[-2:])
    L = lSGs.shape[0]
    comp_s, mean_s = np.zeros((L, components.shape[0])), np.zeros(L)
    for l in range(L):
        a = lSGs[l, :3]
        if rot is not None:
            a = np.asarray(rot, dtype=np.float64) @ a
        phi, theta = np.arccos(a[1]), np.arctan2(a[2], a[0])
        x, y = theta / np.pi, phi / np.pi * 2 - 1
        comp_s[l] = sample2d(components, x, y)
        mean_s[l] = sample2d(mean, x, y)
    lam = lSGs[:, 3]
    row = (np.log10(np.abs(lam + 1e-6)) - 1.5) / 2.5
    fh_n = 2 * np.pi / lam * (1 - np.exp(-lam))
    inte = (fh_n[:, None] * lSGs[:, 4:]).sum(0)
    return comp_s, mean_s, row, fh_n, inte


def points_pre(pts, model_pos, rot, scale, vol_range, angle_decay_fac):
    """-> q (P,3) normalised, dis (P) (the norm BEFORE the clip at 1), delta (P)"""
    m = np.asarray(pts, dtype=np.float64) - np.asarray(model_pos, dtype=np.float64)[None]
    if rot is not None:
        m = m @ np.asarray(rot, dtype=np.float64).T
    q = m / scale / vol_range
    dis = np.linalg.norm(q, axis=-1)
    d1 = np.maximum(dis, 1.0)
    delta = (np.arcsin(1 / vol_range) - np.arcsin(1 / (d1 * vol_range))) * angle_decay_fac
    return q / d1[:, None], dis, delta


def sg_shadow_ref(coeff, components, mean, fh_tab, vol_range, scale, pts, model_pos, lSGs, rot_inv=None,
                  rotate_lights=False, angle_decay_fac=0.4, shadow_pow_fac=2, self_shadow_pow_fac=0.1):
    """-> dict: factor (P), decay (P,L), ssdf (P,L) before the clip, ratio (P,L) = |fh / fh_n| before the clip,
    dis (P)"""
    coeff, fh_tab = np.asarray(coeff, dtype=np.float64), np.asarray(fh_tab, dtype=np.float64)
    lSGs = np.asarray(lSGs, dtype=np.float64)
    comp_s, mean_s, row, fh_n, inte = lights_pre(lSGs, components, mean, rot_inv if rotate_lights else None)
    q, dis, delta = points_pre(pts, model_pos, rot_inv, scale, vol_range, angle_decay_fac)
    P, L = q.shape[0], lSGs.shape[0]
    ssdf, fh = np.zeros((P, L)), np.zeros((P, L))
    for p in range(P):
        pca = sample_volume(coeff, q[p])
        for l in range(L):
            s = 0.0
            for c in range(pca.shape[0]):
                s += pca[c] * comp_s[l, c]
            ssdf[p, l] = s + mean_s[l] + delta[p]
            fh[p, l] = sample2d(fh_tab, min(max(ssdf[p, l], -HALF_PI), HALF_PI) / HALF_PI, row[l])
    ratio = np.abs(fh / fh_n[None])
    decay = np.clip(ratio, 0, 1) ** self_shadow_pow_fac
    f = np.clip(np.abs((fh[:, :, None] * lSGs[None, :, 4:]).sum(1) / inte[None]), 0, 1)
    factor = (LUMA[0] * f[:, 0] + LUMA[1] * f[:, 1] + LUMA[2] * f[:, 2]) ** shadow_pow_fac
    return dict(factor=factor, decay=decay, ssdf=ssdf, ratio=ratio, dis=dis)


def point_class(dis):
    """0 inside the unit range (|q| <= 1), 1 outside"""
    return (np.asarray(dis) > 1.0).astype(np.int32)


def pair_class(ssdf, ratio):
    """The class index (PAIR_CLASSES) of every pair from the fp64 ssdf before the clip and |fh / fh_n|:
    low (ssdf clipped at -pi/2: fh = 0 exactly), saturated (ratio >= 1.05: the decay is 1 exactly), deep
    (ratio < 1e-3: pow(x, 0.1) amplifies rounding without bound towards 0), high (clipped at pi/2), mid."""
    ssdf, ratio = np.asarray(ssdf), np.asarray(ratio)
    out = np.full(ssdf.shape, PAIR_CLASSES.index("mid"), dtype=np.int32)
    out[ssdf >= HALF_PI] = PAIR_CLASSES.index("high")
    out[ratio < DEEP] = PAIR_CLASSES.index("deep")
    out[ratio >= SATURATED] = PAIR_CLASSES.index("saturated")
    out[ssdf <= -HALF_PI] = PAIR_CLASSES.index("low")
    return out


def blur_weights():
    """torchvision's gaussian_blur(kernel 3): sigma 0.8, exp(-0.5 (x/0.8)^2) over x = -1, 0, 1, normalised"""
    w = np.exp(-0.5 * (np.array([-1.0, 0.0, 1.0]) / 0.8) ** 2)
    return w / w.sum()


def shadow_apply_ref(frame_rgb, factor):
    """frame_rgb (H,W,3) * blur3x3(factor (H,W)): reflect padding, the 2-D kernel the outer product, fp64"""
    rgb, f = np.asarray(frame_rgb, dtype=np.float64), np.asarray(factor, dtype=np.float64)
    H, W = f.shape
    w = blur_weights()
    refl = lambda i, n: -i if i < 0 else (2 * n - 2 - i if i >= n else i)  # noqa: E731
    out = np.zeros_like(rgb)
    for y in range(H):
        for x in range(W):
            b = 0.0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    b += w[dy + 1] * w[dx + 1] * f[refl(y + dy, H), refl(x + dx, W)]
            out[y, x] = rgb[y, x] * b
    return out
