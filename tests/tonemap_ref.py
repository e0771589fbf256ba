"""The exposure tonemappers (ngp_tonemap_* of include/ngp_amd.h)
restated in fp64 NumPy -- forward, backward, radiance mode -- with the error
budgets the GPU tests hold the kernels to, and the case generator both test
files share.

One channel c has T_c = [A (64x16, row-major [out][in]) | B (16x64)]; the
network's one real input is column 0 of A, the fifteen padded inputs are 1, the
output is row 0 of B:
    beta_j = A[j,1] + ... + A[j,15]   (ascending, fp32: the spec's definition)
    a_j = A[j,0] u + beta_j,  r_j = max(a_j, 0),  z = sum_j B[0,j] r_j,  y = 1 / (1 + exp(-z))
with u = x + log(e).
"""
import functools

import numpy as np

NET, PARAMS = 2048, 6144
# wave, block and grid edges of the kernels; the last: 512 workgroups x 256 rows and more, so that a
# workgroup of the backward walks a second tile and the fold adds more than one partial sum
SIZES = (1, 63, 64, 65, 257, 4099, 512 * 256 + 4099)
EXPOSURES = (1 / 8, 1 / 2, 2.0, 8.0, 32.0)
TAIL = 21  # device buffers hold n + TAIL rows, NaN past n
AMBIGUOUS_SLACK = 2.0 ** -18
AMBIGUOUS_CAP = 1e-3  # at most 0.1 % of the (row, unit) pairs


def xavier_fp16(seed):
    """(PARAMS) f32 holding fp16 values: Xavier-uniform per matrix, padding rows and columns included."""
    g = np.random.default_rng(seed)
    parts = []
    for _ in range(3):
        for out_d, in_d in ((64, 16), (16, 64)):
            a = np.sqrt(6.0 / (in_d + out_d))
            parts.append(g.uniform(-a, a, out_d * in_d))
    return np.concatenate(parts).astype(np.float16).astype(np.float32)


def split(w):
    """-> A (3,64,16), B (3,16,64), views of w (PARAMS)"""
    w = w.reshape(3, NET)
    return w[:, :1024].reshape(3, 64, 16), w[:, 1024:].reshape(3, 16, 64)


def beta_of(A):
    """(3,64) f64: the fifteen padding columns added in ascending order in fp32"""
    b = A[..., 1].astype(np.float32)
    for k in range(2, 16):
        b = (b + A[..., k].astype(np.float32)).astype(np.float32)
    return b.astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(n, seed=None):
    """Inputs of one size: weights (fp16 values), x (n,3) uniform in [-8, 4] rounded to fp16, per-row
    exposures from EXPOSURES, upstream gradients g (n,3) (about a tenth of the rows exactly zero)."""
    seed = n if seed is None else seed
    g = np.random.default_rng(1000 + seed)
    x = g.uniform(-8, 4, (n, 3)).astype(np.float16).astype(np.float32)
    e = np.asarray(EXPOSURES, np.float32)[g.integers(0, len(EXPOSURES), n)]
    dy = g.standard_normal((n, 3)).astype(np.float32)
    dy[(g.random(n) < 0.1) & (np.arange(n) > 0)] = 0.0  # (row 0 always carries gradient: n = 1)
    return {"n": n, "w": xavier_fp16(seed), "x": x, "e": e, "dy": dy}


def _u(x, e):
    x = np.asarray(x, np.float64)
    if e is None:
        return x
    return x + np.log(np.asarray(e, np.float64)).reshape(-1, 1)


def forward(w, x, e=None, with_bound=False):
    """y (n,3) f64 [, the forward's error bar (n,3)]: 0.25 2^-23 66 sum_j |B_0j| (|A_j0 u| + |beta_j|) + 2^-22 --
    a 64-term fp32 dot product (and u's two roundings) in the worst case through a slope <= 1/4, plus the
    sigmoid's own rounding."""
    A, B = split(np.asarray(w, np.float64))
    beta = beta_of(A)
    u = _u(x, e)
    y = np.empty_like(u)
    bar = np.empty_like(u)
    for c in range(3):
        au = u[:, c:c + 1] * A[c, :, 0][None]
        z = (np.maximum(au + beta[c][None], 0.0) * B[c, 0][None]).sum(1)
        y[:, c] = 1.0 / (1.0 + np.exp(-z))
        bar[:, c] = 0.25 * 2.0 ** -23 * 66 * (np.abs(B[c, 0])[None] * (np.abs(au) + np.abs(beta[c])[None])).sum(1) \
            + 2.0 ** -22
    return (y, bar) if with_bound else y


def radiance(x):
    """output_radiance: exp(min(max(x, 0), 20)), f64"""
    return np.exp(np.clip(np.asarray(x, np.float64), 0.0, 20.0))


def _ambiguous(A, beta, u, c):
    au = u[:, c:c + 1] * A[c, :, 0][None]
    return np.abs(au + beta[c][None]) <= AMBIGUOUS_SLACK * (np.abs(au) + np.abs(A[c, :, 1:]).sum(-1)[None])


def ambiguous(w, x, e=None):
    """(n,3,64) bool: |a_j| <= 2^-18 (|A_j0 u| + sum_k |A_jk|) -- the (row, unit) pairs where an fp32
    evaluation of a_j may legitimately land on the other side of the ReLU."""
    A, _ = split(np.asarray(w, np.float64))
    beta, u = beta_of(A), _u(x, e)
    return np.stack([_ambiguous(A, beta, u, c) for c in range(3)], 1)


def backward(w, x, e, dy):
    """fp64 backward of the spec over all rows, with its error bars.  Returns a dict:
    dx (n,3), grad (PARAMS), and per output the bar 2^-23 (n_terms + 64) S + Bamb (dx_bar, grad_bar), where S
    sums the absolute values of the terms in the split form (|A_j0 u delta| and |beta_j delta| separately)
    and Bamb the absolute contribution of the ambiguous pairs; n_amb their number."""
    w64 = np.asarray(w, np.float64)
    A, B = split(w64)
    beta = beta_of(A)
    u = _u(x, e)
    dy = np.asarray(dy, np.float64)
    n = u.shape[0]
    n_amb = 0
    grad, S, Bamb = np.zeros(PARAMS), np.zeros(PARAMS), np.zeros(PARAMS)
    gA, gB = split(grad)
    sA, sB = split(S)
    bA, bB = split(Bamb)
    dx, dx_S, dx_amb = (np.empty((n, 3)) for _ in range(3))
    for c in range(3):
        a0, b0 = A[c, :, 0][None], B[c, 0][None]
        uc = u[:, c:c + 1]
        au = uc * a0
        a = au + beta[c][None]
        m = a > 0
        y = 1.0 / (1.0 + np.exp(-(np.where(m, a, 0.0) * b0).sum(1)))
        delta = (dy[:, c] * y * (1.0 - y))[:, None]
        q = m * b0 * delta
        gB[c, 0] = (delta * np.where(m, a, 0.0)).sum(0)
        gA[c, :, 0] = (q * uc).sum(0)
        gA[c, :, 1:] = q.sum(0)[:, None]
        dx[:, c] = (q * a0).sum(1)
        # the terms' absolute values, masked (S) and on the ambiguous pairs whatever the mask (Bamb)
        tB = np.abs(au * delta) + np.abs(beta[c][None] * delta)
        tA0, tAk, tx = np.abs(b0 * delta * uc), np.abs(b0 * delta) + 0 * uc, np.abs(b0 * delta * a0)
        am = _ambiguous(A, beta, u, c)
        n_amb += int(am.sum())
        sB[c, 0], bB[c, 0] = (m * tB).sum(0), (am * tB).sum(0)
        sA[c, :, 0], bA[c, :, 0] = (m * tA0).sum(0), (am * tA0).sum(0)
        sA[c, :, 1:], bA[c, :, 1:] = (m * tAk).sum(0)[:, None], (am * tAk).sum(0)[:, None]
        dx_S[:, c], dx_amb[:, c] = (m * tx).sum(1), (am * tx).sum(1)
    ulp = 2.0 ** -23
    return {"dx": dx, "grad": grad, "dx_bar": ulp * (1 + 64) * dx_S + dx_amb, "grad_bar": ulp * (n + 64) * S + Bamb,
            "n_amb": n_amb}
