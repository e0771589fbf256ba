"""Per-pair fp64 restatement of the SG light probes (insert/render_utils.py
cubemap_sample / cubemap2env_map and insert/envfit.py SG2Envmap / EnvOptim of
the reference; csrc/sgfit.hip, sg_probe.py here) in numpy loops: no
grid_sample, no autograd -- the bilinear lookup is written out from its
definition and the gradient from the chain rule, a light at a time, so a
swapped (u, v), a wrong face order or a wrong derivative in the kernels or in
the torch formulation shows against it.  Also A_p, the sum over the pixels of
the absolute contributions to each parameter's gradient, which the gradient
bars are stated in, and the parameter kinds the trajectory bars are recorded
per.
"""
import numpy as np

TINY = 1e-8
SEL_MAP = (2, 4, 0)
KINDS = ("lobe", "sharpness", "amplitude")
KIND_OF_COLUMN = np.array([0, 0, 0, 1, 2, 2, 2])
CHECKPOINTS = (1, 2, 3, 5, 10, 25)
GRAD_CHECKPOINTS = (1, 10)
BETAS, ADAM_EPS, LR = (0.9, 0.999), 1e-8, 0.1


def env_dirs(H, W):
    """the directions of the equirectangular map from fp32 angles as the reference forms them (float32 in, float32 out)"""
    import torch
    phi, theta = torch.meshgrid([torch.linspace(0., np.pi, H, dtype=torch.float32),
                                 torch.linspace(-0.5 * np.pi, 1.5 * np.pi, W, dtype=torch.float32)], indexing="ij")
    d = torch.stack([torch.cos(theta) * torch.sin(phi), torch.cos(phi), torch.sin(theta) * torch.sin(phi)], -1)
    return d.reshape(-1, 3).numpy()


def _axis(x, n):
    """pixel-centre coordinates (align_corners False), border padding -> (i0, i1, w0, w1)"""
    g = min(max(((x + 1.0) * n - 1.0) / 2.0, 0.0), n - 1.0)
    i0 = int(np.floor(g))
    return i0, min(i0 + 1, n - 1), (i0 + 1.0) - g, g - i0


def cubemap_sample_ref(cubemap, dirs, res, swap_uv=False, face_order=None):
    """cubemap (6*res*res,3), dirs (n,3) -> rgb (n,3) float64, face (n) (-1: none).  swap_uv / face_order: the
    two mistakes the tests show to be visible."""
    cm = np.asarray(cubemap, dtype=np.float64).reshape(6, res, res, 3)
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    rgb, faces = np.ones((len(d), 3)), -np.ones(len(d), dtype=np.int64)
    for i, v in enumerate(d):
        a = np.abs(v)
        axis = 0
        for k in (1, 2):
            if a[k] > a[axis]:
                axis = k
        if not a[axis] > 0 or not np.isfinite(a[axis]):
            continue
        q = v / a[axis]
        face = SEL_MAP[axis] + (1 if q[axis] < 0 else 0)
        faces[i] = face
        if face_order is not None:
            face = face_order[face]
        u, w = [q[k] for k in range(3) if k != axis]
        if swap_uv:
            u, w = w, u
        i0, i1, a0, a1 = _axis(u, res)      # u: the face's first index
        j0, j1, b0, b1 = _axis(w, res)      # v: its second
        rgb[i] = cm[face, i0, j0] * a0 * b0 + cm[face, i0, j1] * a0 * b1 + cm[face, i1, j0] * a1 * b0 \
            + cm[face, i1, j1] * a1 * b1
    return rgb, faces


def parse(lights):
    x = np.asarray(lights, dtype=np.float64)
    n = np.sqrt((x[:, :3] ** 2).sum(1))
    return x[:, :3] / (n + TINY)[:, None], np.abs(x[:, 3]), np.abs(x[:, 4:]), n


def sg_envmap_ref(lights, dirs):
    """(P,3) float64, a light at a time"""
    a, lam, mu, _ = parse(lights)
    v = np.asarray(dirs, dtype=np.float64)
    out = np.zeros((len(v), 3))
    for l in range(len(a)):
        out += mu[l][None, :] * np.exp(lam[l] * (v @ a[l] - 1.0))[:, None]
    return out


def sg_grad_ref(lights, dirs, target):
    """loss, grad (L,7) and A (L,7) = the sum over pixels of the absolute values of the terms that pixel adds to
    the gradient entry: what one rounding per term can cost is 2^-24 A.  A lobe entry is the difference of two
    sums -- dx_k = sum_p da_pk / (n+eps) - x_k sum_p (da_p . x) / (n (n+eps)^2), nearly equal for a sharp light,
    whose pixels all lie along its axis -- and any fp32 evaluation rounds the terms of both before they cancel,
    so both enter A in absolute value: A_k = sum_p |da_pk| / (n+eps) + |x_k| sum_p sum_j |da_pj x_j| / (n (n+eps)^2)."""
    x = np.asarray(lights, dtype=np.float64)
    a, lam, mu, n = parse(x)
    v = np.asarray(dirs, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    P, L = len(v), len(x)
    r = sg_envmap_ref(x, v) - t
    g = 2.0 * r / (3.0 * P)
    grad, A = np.zeros((L, 7)), np.zeros((L, 7))
    sign = np.sign(x)
    for l in range(L):
        dm = v @ a[l] - 1.0
        e = np.exp(lam[l] * dm)
        for c in range(3):
            term = e * g[:, c] * sign[l, 4 + c]
            grad[l, 4 + c], A[l, 4 + c] = term.sum(), np.abs(term).sum()
        s = g @ mu[l]
        term = s * e * dm * sign[l, 3]
        grad[l, 3], A[l, 3] = term.sum(), np.abs(term).sum()
        da = (s * e * lam[l])[:, None] * v                                            # P,3: per-pixel d loss / d axis
        ne = n[l] + TINY
        dx, adx = da / ne, np.abs(da) / ne
        if n[l] > 0:                                                                  # (the norm's derivative at 0 is 0)
            dx = dx - (da @ x[l, :3])[:, None] * x[l, :3][None, :] / (n[l] * ne * ne)
            adx = adx + (np.abs(da) @ np.abs(x[l, :3]))[:, None] * np.abs(x[l, :3])[None, :] / (n[l] * ne * ne)
        grad[l, :3], A[l, :3] = dx.sum(0), adx.sum(0)
    return float((r * r).sum() / (3.0 * P)), grad, A


def sg_fit_ref(lights, dirs, target, n_iter=25, lr=LR, checkpoints=CHECKPOINTS):
    """torch.optim.Adam's steps in fp64 -> {'params': {it: (L,7)}, 'loss': {it: float}} (loss before step `it`)"""
    x = np.array(lights, dtype=np.float64)
    m, v2 = np.zeros_like(x), np.zeros_like(x)
    b1, b2 = BETAS
    params, losses = {}, {}
    for it in range(1, n_iter + 1):
        loss, grad, _ = sg_grad_ref(x, dirs, target)
        m = m + (1 - b1) * (grad - m)
        v2 = v2 * b2 + (1 - b2) * grad * grad
        denom = np.sqrt(v2) / np.sqrt(1 - b2 ** it) + ADAM_EPS
        x = x - (lr / (1 - b1 ** it)) * (m / denom)
        if it in checkpoints:
            params[it], losses[it] = x.copy(), loss
    return dict(params=params, loss=losses)
