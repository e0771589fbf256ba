"""fp64 per-sample references, rounding bounds and designed input sets for the
compositing kernels and the fused NeRF loss: ngp_composite_loss (loss.hip),
ngp_composite_train_fw / _bw and ngp_composite_test_fw (composite.hip) and
ngp_nerf_loss_fw / _bw.  A plain helper module (not a conftest), like
hash_ref.py: test_composite_ref_cpu.py shows on the CPU that the references
agree with each other and that a correct fp32 implementation lies inside the
bounds, test_composite_ref_gpu.py holds the kernels to them.

Everything is evaluated in fp64 from the fp32 inputs, rows padded to the
longest row.  u = 2^-24; every bound is scaled by SLACK = 1 + 2^-20 and gains
TINY = 2^-126 (as in hash_ref.py); `dq` below is the absolute error bound of
the fp32 quantity q against its fp64 value.

Forward (volumerendering.cu:5-44)
---------------------------------
x = sigma delta, e = exp(-x), a = 1 - e, Tb_k = prod_{j<k} (1 - a_j) (the
transmittance in front of sample k), Ta_k = Tb_k (1 - a_k), w_k = a_k Tb_k.
K = the first k with Ta_k <= T_thr, else N.  Samples 0..K are composited (the
break follows the sums), the composited COUNT is K (the break precedes the
count), n_active = min(K + 1, N): the samples that carry gradient.

* e: the kernels form fl(sigma delta) (relative u, so x u e in e) and
  __expf(-x) = exp2(fl(log2e x)) (__clang_hip_math.h): the rounded constant and
  the product move the argument by 2u |x log2e|, i.e. e by 2 |x| u e, and
  v_exp_f32 is good to 1 ulp = 2u: (2x + 2) u e for the intrinsic.  ROCm does
  not document a figure, so the intrinsic alone was measured once on an MI355X
  against fp64 exp over 2^22 arguments in [0, 104) (the tests' range): the
  worst err / ((2x + 2) u e) is 0.60 (EXPF below: 1.2, that with a 2x margin);
  from x = 87 on the result is flushed to 0, absolute error <= 2^-126 = TINY.
  de = (EXPF (2x + 2) + x) u e + TINY.  x == 0 gives e = 1, a = 0, w = 0
  exactly: all errors 0.
* a = fl(1 - e): da = de + u a.  om = fl(1 - a): dom = da + u / 2.  Relative
  error of one factor: eps = dom / e.  (For an opaque sample, x = 12, eps is
  1.5 u e^12 = 1.4e-2: om = 6e-6 is a difference of numbers near 1.  It is the
  terminating sample, so this reaches only its own Ta.)
* Tb_j: j factors and j multiplications in any association (a serial chain,
  a Hillis-Steele scan and a chunk carry are all product trees with j inner
  nodes), + 2u for the carry in: rb_j = sum_{k<j} (eps_k + u) + 2u relative;
  ra_j = rb_j + eps_j + u for Ta_j.  composite_test's T starts at fl(1 -
  opacity): + u.
* w_j = fl(a_j Tb_j): dw_j = Tb_j da_j + w_j (rb_j + u).
* per-ray sums R_c = sum w_k c_k (D with t, O with 1): the terms are off by
  |c_k| dw_k + u |w_k c_k|, and a sum of n terms by depth(n) u sum |terms|:
  dR_c = sum |c_k| dw_k + (depth + 1) u sum |w_k c_k|.  depth is the number
  of additions a term can pass through -- the only thing that differs
  between the paths:
    serial  (composite.hip, readlane left folds)         depth = n
    tree    (loss.hip: wave.h's 6-level wave sums / Hillis-Steele
             scans per 64-sample chunk + one carry per chunk) depth = 6 + ceil(n / 64)
    test    (composite_test_kernel, a serial loop onto a
             non-zero base: the base counts as a term)    depth = n + 1
* The analysis above is first order.  One constant C = 2 per path (C_PATH)
  covers what it leaves out: products of two error terms (eps reaches 1.4e-2),
  the difference between |q| and |fl(q)| inside the magnitudes, and the
  roundings of intermediate sums counted once where a worst case would count
  them per operand.  It is the same for the three paths because their
  difference is already in depth.  A dropped, doubled or misplaced term moves
  an output by its whole magnitude, 10^2..10^5 bounds.

Loss (models/rendering.py:287-296, losses.py:63-82)
---------------------------------------------------
x_c = R_c + bg_c (1 - O); rgb term l(x_c, gt_c) by type (0 raw, 1 mse, 2 log,
3 tanh), mean over 3 n_rays; o = O + 1e-10, lambda_op (-o log o), mean over
n_rays; v = D / scale + 1e-10, -lambda_depth log(min(v, 1)), whose gradient
follows torch's clip: it passes where the fp32 value of v is <= 1 (at equality
too).  The constants 1e-3, 1e-10, 0.2935, 0.7607 are the fp32 ones.  The input
sets keep |v - 1| >= 1e-3 except on rows built to give fl(v) == 1 exactly.
  dx_c = dR_c + |bg_c| (dO + u) + 2u (|R_c| + |bg_c| (1 - O))
  dg_c = (h_c dx_c + rg_c + 3u |l'_c|) / 3n, h = |d2l/dx2| (below), rg the
  rounding of l' itself: raw 6u |l'|, mse 2u |l'|; log: lg = log(A / B) is off
  by 3u + 4u |lg| (three roundings in the ratio, logf <= 2 ulp), l' = 2 lg k^2 /
  A by 2 k^2 / A of that + 10u |l'| (autograd's sequence: two products, a division
  by the ratio a / b as the forward rounded it, 3u, a division by b, 1u: 9u; the
  kernels divide by a once: 4u); tanh: tanhf <= 2 ulp = 4u absolute each.
  dgop = sum (|bg_c| dg_c + 2u |g_c bg_c|) + lambda_op / n (do / o + 4u |log o|
         + 3u |log o + 1|) + 3u (sum |g_c bg_c| + |op term|)
  gs = gop (1 - O): dgs = dgop (1 - O) + |gop| (dO + 2u)
  dgdep = |gdep| (dv / v + 5u), dv = dD / scale + 2u |v|
  d(loss) = sum_c (sl_c dx_c + rl_c + 3u l_c) / 3n + the same for the other
  terms + 8u sum |terms|; sl = |dl/dx| of the VALUE (for the raw type the
  denominator moves it too: 2 |d| (1 / den + |x - y| / den^2)), rl the rounding
  of l itself.
Distortion (losses.cu:8-140, the scan form of sum_ij w_i w_j |t_i - t_j| + 1/3
sum w_i^2 delta_i for sorted t): gw_j = 2 lam / n (AB_j + w_j delta_j / 3), AB_j =
sum_k w_k |t_j - t_k| formed from prefix sums as (t we - wte) + ((D - b) - t (O -
a)): d(AB_j) = sum_k |t_j - t_k| dw_k (first order in the weights) + (3 depth +
7) u (|t_j| O + D) (the prefix sums and differences, absolute in their operands).
  dgw_j = 2 lam / n (d(AB_j) + delta_j / 3 (dw_j + 3u w_j)) + 4u |gw_j|
  S = sum gw_k w_k: dS = sum (|gw_k| dw_k + w_k dgw_k) + (depth + 1) u sum |gw_k w_k|
  The loss itself, ld = sum_i 2 (b_i we_i - a_i wte_i) + w_i^2 delta_i / 3 with a, b the inclusive prefix sums of w
  and w t: first order in the weights, sum |dld/dw_k| dw_k, + the prefix sums' roundings, absolute in the products
  the differences are formed from, (8 depth + 12) u sum_i a_i b_i, + 4u sum w^2 delta / 3 + depth u sum |l_i|.

Backward (volumerendering.cu:86-150)
------------------------------------
dL/dsigma_j = delta_j (sum_c g_c (c_j Ta_j - (R_c - pr_j)) + gs + gdep (t_j Ta_j -
(D - pd_j)) + Ta_j gw_j - (S - pw_j)), j < n_active; dL/drgbs_j = g w_j; exactly 0
past n_active.  This is the exact derivative of the forward truncated at the
fixed K (1 - O = Ta_K telescopes), so fp64 autograd through that forward checks
it independently.  The suffix sums are formed as R - prefix, in the analytic
reference too, so their error is absolute in R, not relative to the suffix:
d(R_c - pr_j) = 2 dR_c + 2u sum |w_k c_k|.
  d(dL/dsigma_j) = delta_j (sum_c [dg_c (|c_j| Ta_j + suf_c) + |g_c| (|c_j| dTa_j +
      2 dR_c + 3u (|c_j| Ta_j + sum |w c|))] + dgs + [the same with gdep, t, D]
      + |gw_j| dTa_j + Ta_j dgw_j + 2u Ta_j |gw_j| + 2 dS + 2u sum |gw w|
      + 10u sum |terms|) + u |dL/dsigma_j|
  d(dL/drgbs_jc) = dg_c w_j + |g_c| dw_j + u |g_c w_j|
Where a bound is 0 (w_j == 0 from sigma == 0, an all-zero upstream gradient,
past the termination where the contract has the element written) the output
must be exactly 0.

Termination precondition (enforce_margin)
-----------------------------------------
For every row and every sample k up to the fp64 termination, |ln Ta_k - ln
T_thr| >= 4 (k + 2) 2^-20 (four times the flip bound test_composite_train_fw_bw
documents) and |Ta_k - T_thr| >= 2 dTa_k (the bound above).  The offending
sigma is nudged at generation time until both hold, so no fp32 evaluation
within the bounds can terminate elsewhere: n_active, counts and alive are
compared exactly.
"""
import functools
import math
import types

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -20
# __expf(-x) against fp64 exp, measured once on an MI355X (2^22 arguments in
# [0, 104)): max relative error 0.65 u for x < 0.02, 2.8 u for x < 2, 16.3 u
# for x < 20, 59 u for x < 64, 65 u for x < 87, flushed to 0 from there (absolute
# error <= 2^-126); max err / ((2x + 2) u e) = 0.60.  EXPF is that with a 2x margin.
EXPF = 1.2
C_PATH = {"serial": 2.0, "tree": 2.0, "test": 2.0}
LOGF = 4.0   # logf <= 2 ulp, in units of u
TANHF = 4.0  # tanhf <= 2 ulp of a value <= 1, absolute, in units of u
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
C_DEN, C_EPS, C_B, C_K = F32(1e-3), F32(1e-10), F32(0.2935), F32(0.7607)
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300, 500)
TERM_POS = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192)


def depth(path, n):
    n = n.double()
    if path == "serial":
        return n
    if path == "tree":
        return 6 + torch.ceil(n / 64)
    if path == "test":
        return n + 1
    raise KeyError(path)


# ------------------------------------------------------------------ padding
def pad_index(rays_a, n_samples):
    """-> (idx (R, L) flat sample index, valid (R, L)) of the rows of rays_a"""
    start, N = rays_a[:, 1], rays_a[:, 2]
    L = max(int(N.max()) if N.numel() else 0, 1)
    k = torch.arange(L)[None, :]
    valid = k < N[:, None]
    idx = (start[:, None] + k).clamp(max=max(n_samples - 1, 0))
    return idx, valid


def pad(t, idx, valid):
    v = t.double()[idx]
    return v * (valid if v.dim() == 2 else valid[..., None])


def unpad(p, idx, valid, n_samples, fill=0.0):
    """the padded per-sample values p back in the flat layout (other samples: fill)"""
    out = torch.full((n_samples,) + tuple(p.shape[2:]), fill, dtype=p.dtype)
    out[idx[valid]] = p[valid]
    return out


# ------------------------------------------------------------------ forward
def _forward(S, C, Dl, Ts, valid, T_thr, T0=None, m=None):
    """padded forward; m: a fixed active mask (the truncated forward autograd runs through)"""
    x = S * Dl
    cs = torch.cumsum(x, 1)
    t0 = 1.0 if T0 is None else T0[:, None]
    Ta, Tb = torch.exp(-cs) * t0, torch.exp(-(cs - x)) * t0
    a = -torch.expm1(-x)
    N = valid.sum(1)
    if m is None:
        hit = valid & (Ta <= T_thr)
        K = torch.minimum((torch.cumsum(hit, 1) == 0).sum(1), N)
        n_active = torch.minimum(K + 1, N)
        m = torch.arange(valid.shape[1])[None, :] < n_active[:, None]
    else:
        K = n_active = None
    w = a * Tb * m
    return types.SimpleNamespace(x=x, e=torch.exp(-x), a=a, Ta=Ta, Tb=Tb, w=w, m=m, K=K, n_active=n_active, N=N,
                                 R=(w[..., None] * C).sum(1), O=w.sum(1), D=(w * Ts).sum(1))


def forward_bounds(f, C, Ts, path, T0=False):
    """absolute error bounds of the forward (module docstring) -> namespace(dTa, dTb, dw (R, L), dR (R, 3), dO, dD,
    Rabs, Dabs, dep)"""
    nz = f.x != 0
    de = torch.where(nz, (EXPF * (2 * f.x + 2) + f.x) * U * f.e + TINY, torch.zeros_like(f.x))
    da = torch.where(nz, de + U * f.a, torch.zeros_like(f.x))
    eps = torch.where(nz, (da + U / 2) / f.e, torch.zeros_like(f.x))
    ce = torch.cumsum(eps + U, 1)
    rb = torch.cat([torch.zeros_like(ce[:, :1]), ce[:, :-1]], 1) + 2 * U + (U if T0 else 0.0)  # (exclusive: no ce - eps)
    ra = rb + eps + U
    dTb, dTa = f.Tb * rb, f.Ta * ra
    dw = (f.Tb * da + f.w * (rb + U)) * f.m * nz
    dep = depth(path, f.m.sum(1))
    Rabs, Dabs = (f.w[..., None] * C.abs()).sum(1), (f.w * Ts.abs()).sum(1)
    dR = (dw[..., None] * C.abs()).sum(1) + (dep[:, None] + 1) * U * Rabs
    dD = (dw * Ts.abs()).sum(1) + (dep + 1) * U * Dabs
    dO = dw.sum(1) + dep * U * f.O
    return types.SimpleNamespace(dTa=dTa, dTb=dTb, dw=dw, dR=dR, dO=dO, dD=dD, Rabs=Rabs, Dabs=Dabs, dep=dep)


def composite_ref64(sig, rgbs, deltas, ts, rays_a, T_thr, T0=None):
    """fp64 composite_train_fw of the rows of rays_a -> namespace: per row (in row order, `ray` says where the
    kernels store it) R (rgb), O (opacity), D (depth), K, count (composited samples: K), n_active, N; per sample
    (padded (rows, L), `idx` / `valid` map to the flat layout) w (ws), Ta, Tb, a, x, m (the active mask)."""
    n = sig.shape[0]
    idx, valid = pad_index(rays_a, n)
    S, C, Dl, Ts = pad(sig, idx, valid), pad(rgbs.reshape(-1, 3), idx, valid), pad(deltas, idx, valid), \
        pad(ts, idx, valid)
    f = _forward(S, C, Dl, Ts, valid, T_thr, T0)
    f.count = f.K
    f.ray, f.start = rays_a[:, 0], rays_a[:, 1]
    f.idx, f.valid, f.n = idx, valid, n
    f.S, f.C, f.Dl, f.Ts, f.T_thr, f.T0 = S, C, Dl, Ts, T_thr, T0
    return f


def flat(f, p, fill=0.0):
    return unpad(p, f.idx, f.valid, f.n, fill)


# --------------------------------------------------------------------- loss
def rgb_term64(loss_type, x, y):
    """-> l, l' = dl/dx, h >= |d2l/dx2| (for the raw type: of the gradient the loss defines, denominator detached),
    rl, rg: the absolute rounding errors of an fp32 evaluation of l and l' (module docstring), sl >= |dl/dx| as the
    VALUE of l moves with x (= |l'| except for the raw type, whose detached denominator moves the value too)"""
    sl = None
    if loss_type == 0:
        den = x.detach() + C_DEN
        d = (x - y) / den
        l, g = d * d, 2 * d / den
        h = 2 / den ** 2 + 4 * (x - y).abs() / den ** 3
        rl, rg = 8 * U * l, 6 * U * g.abs()
        sl = 2 * d.abs() * (1 / den + (x - y).abs() / den ** 2)  # (the VALUE moves with the denominator too)
    elif loss_type == 1:
        d = x - y
        l, g = d * d, 2 * d
        h = torch.full_like(x, 2.0)
        rl, rg = 4 * U * l, 2 * U * g.abs()
    elif loss_type == 2:
        A, B = C_B + x, C_B + y
        lg = torch.log(A / B)
        v = lg * C_K
        l, g = v * v, 2 * v * C_K / A
        h = 2 * C_K ** 2 / A ** 2 + 2 * v.abs() * C_K / A ** 2
        dv = C_K * (3 * U + LOGF * U * lg.abs()) + U * v.abs()
        rl, rg = 2 * v.abs() * dv + U * l, 2 * C_K / A * dv + 10 * U * g.abs()
    elif loss_type == 3:
        tx, ty = torch.tanh(x), torch.tanh(y)
        d, s = tx - ty, 1 - tx * tx
        l, g = d * d, 2 * d * s
        h = 2 * s * s + 4 * d.abs() * tx.abs() * s
        dd, ds = 2 * TANHF * U + U * d.abs(), 2 * tx.abs() * TANHF * U + 2 * U
        rl, rg = 2 * d.abs() * dd + U * l, 2 * s * dd + 2 * d.abs() * ds + 2 * U * g.abs()
    else:
        raise KeyError(loss_type)
    return l, g, h, rl, rg, (g.abs() if sl is None else sl)


def clip_pass(v):
    """torch's clip(max=1) passes the gradient where the fp32 value of v is <= 1"""
    return v.detach().float() <= 1.0


def _dist_scan(w, Ts, Dl):
    """per sample: the distortion loss's terms and AB_j = sum_k w_k |t_j - t_k| (sorted t), by prefix sums"""
    wt = w * Ts
    a, b = torch.cumsum(w, 1), torch.cumsum(wt, 1)
    we, wte = a - w, b - wt
    l = 2 * w * (Ts * we - wte) + w * w * Dl / 3
    AB = (Ts * we - wte) + ((b[:, -1:] - b) - Ts * (a[:, -1:] - a))
    return l, AB, a, b


def _loss_terms(f, C, Ts, Dl, gt, bg, cfg, n_rays):
    """per-row loss contributions of a forward f (autograd-friendly)"""
    xc = f.R + bg[None, :] * (1 - f.O)[:, None]
    l = rgb_term64(cfg.loss_type, xc, gt)[0]
    loss = l.sum(1) / (3 * n_rays)
    o = f.O + C_EPS
    loss = loss + cfg.lambda_opacity * (-o * torch.log(o)) / n_rays
    if cfg.lambda_depth != 0:
        v = f.D / cfg.depth_scale + C_EPS
        vc = torch.where(clip_pass(v), v, torch.ones_like(v))
        loss = loss + (-cfg.lambda_depth) * torch.log(vc) / n_rays
    if cfg.lambda_distortion != 0:
        ld, _, _, _ = _dist_scan(f.w, Ts, Dl)
        loss = loss + cfg.lambda_distortion * ld.sum(1) / n_rays
    return xc, loss


def config(loss_type=0, lambda_opacity=1e-3, lambda_depth=0.0, depth_scale=1.0, lambda_distortion=0.0):
    return types.SimpleNamespace(loss_type=loss_type, lambda_opacity=F32(lambda_opacity), lambda_depth=F32(lambda_depth),
                                 depth_scale=F32(depth_scale), lambda_distortion=F32(lambda_distortion))


def backward64(f, g, gs, gdep, gw):
    """The analytic compositing backward in fp64 (padded): g (R, 3) = dL/drgb, gs (R,) = dL/dopacity (1 - O),
    gdep (R,), gw (R, L) = dL/dws (or None) -> dL/dsigma (R, L), dL/drgbs (R, L, 3)"""
    w, Ta = f.w, f.Ta
    pr = torch.cumsum(w[..., None] * f.C, 1)
    pd = torch.cumsum(w * f.Ts, 1)
    inner = (g[:, None, :] * (f.C * Ta[..., None] - (f.R[:, None, :] - pr))).sum(2) + gs[:, None] \
        + gdep[:, None] * (f.Ts * Ta - (f.D[:, None] - pd))
    if gw is not None:
        gww = gw * w
        inner = inner + Ta * gw - (gww.sum(1, keepdim=True) - torch.cumsum(gww, 1))
    return f.Dl * inner * f.m, g[:, None, :] * w[..., None]


def backward_bound(f, fb, path, g, dg, gs, dgs, gdep, dgdep, gw=None, dgw=None):
    """per-element bounds of |dL/dsigma|, |dL/drgbs| errors (module docstring), padded"""
    w, Ta, C, Ts = f.w, f.Ta, f.C.abs(), f.Ts.abs()
    sufR = (fb.Rabs[:, None, :] - torch.cumsum(w[..., None] * C, 1)).clamp(min=0)
    sufD = (fb.Dabs[:, None] - torch.cumsum(w * Ts, 1)).clamp(min=0)
    ga, gda = g.abs()[:, None, :], gdep.abs()[:, None]
    err = (dg[:, None, :] * (C * Ta[..., None] + sufR)
           + ga * (C * fb.dTa[..., None] + 2 * fb.dR[:, None, :]
                   + 3 * U * (C * Ta[..., None] + fb.Rabs[:, None, :]))).sum(2)
    terms = (ga * (C * Ta[..., None] + sufR)).sum(2) + gs.abs()[:, None] + gda * (Ts * Ta + sufD)
    err = err + dgs[:, None] + dgdep[:, None] * (Ts * Ta + sufD) \
        + gda * (Ts * fb.dTa + 2 * fb.dD[:, None] + 3 * U * (Ts * Ta + fb.Dabs[:, None]))
    if gw is not None:
        gwa = gw.abs() * f.m
        Sabs = (gwa * w).sum(1, keepdim=True)
        dS = (gwa * fb.dw + w * dgw).sum(1, keepdim=True) + (fb.dep[:, None] + 1) * U * Sabs
        err = err + gwa * fb.dTa + Ta * dgw + 2 * U * Ta * gwa + 2 * dS + 2 * U * Sabs
        terms = terms + Ta * gwa + Sabs
    val = f.Dl * terms
    b_sig = (f.Dl * (err + 10 * U * terms) + U * val) * f.m
    b_rgb = (dg[:, None, :] * w[..., None] + ga * fb.dw[..., None] + U * ga * w[..., None]) * f.m[..., None]
    c = C_PATH[path] * SLACK
    return b_sig * c + TINY * (b_sig > 0), b_rgb * c + TINY * (b_rgb > 0)


def loss_ref64(inp, cfg, bg, n_rays=None, path="tree"):
    """The fused step of the first n_rays rows of an input set in fp64 -> namespace:
      f            the forward (composite_ref64) of those rows, fb its bounds
      xc (R, 3)    rgb after the background, loss (R,) per-row contributions; b_R / b_xc / b_O / b_D / b_loss bounds
      dsig, drgbs  (R, L), (R, L, 3): fp64 autograd through the forward truncated at the fixed K
      dsig_an, drgbs_an: the analytic backward; b_dsig, b_drgbs: bounds
    (rows in row order; f.ray says where the kernels store per-ray outputs)."""
    ra = inp.rays_a if n_rays is None else inp.rays_a[:n_rays]
    nr = ra.shape[0]
    f = composite_ref64(inp.sig, inp.rgbs, inp.deltas, inp.ts, ra, inp.T_thr)
    fb = forward_bounds(f, f.C, f.Ts, path)
    gt = inp.gt.double()[f.ray]
    bg = bg.double()
    # autograd through the truncated forward
    S = f.S.clone().requires_grad_(True)
    C = f.C.clone().requires_grad_(True)
    ft = _forward(S, C, f.Dl, f.Ts, f.valid, inp.T_thr, None, f.m)
    xc_t, loss_t = _loss_terms(ft, C, f.Ts, f.Dl, gt, bg, cfg, nr)
    dsig, drgbs = torch.autograd.grad(loss_t.sum(), (S, C))
    xc, loss = xc_t.detach(), loss_t.detach()
    # analytic chain and its bounds
    inv_n = 1.0 / nr
    l, lp, h, rl, rg, sl = rgb_term64(cfg.loss_type, xc, gt)
    g = lp * inv_n / 3
    bga = bg.abs()[None, :]
    dx = fb.dR + bga * (fb.dO[:, None] + U) + 2 * U * (f.R.abs() + bga * (1 - f.O).abs()[:, None])
    dg = (h * dx + rg + 3 * U * lp.abs()) * inv_n / 3
    o = f.O + C_EPS
    lo = torch.log(o)
    do = fb.dO + U * o
    t_op = cfg.lambda_opacity * (-(lo + 1)) * inv_n
    gop = -(g * bg[None, :]).sum(1) + t_op
    gbg = (g.abs() * bga).sum(1)
    dgop = (bga * dg).sum(1) + 2 * U * gbg + 3 * U * (gbg + t_op.abs()) \
        + cfg.lambda_opacity * inv_n * (do / o + LOGF * U * lo.abs() + 3 * U * (lo + 1).abs())
    gs = gop * (1 - f.O)
    dgs = dgop * (1 - f.O).abs() + gop.abs() * (fb.dO + 2 * U)
    gdep, dgdep = torch.zeros(nr, dtype=torch.float64), torch.zeros(nr, dtype=torch.float64)
    b_loss = ((sl * dx + rl + 3 * U * l).sum(1) * inv_n / 3
              + cfg.lambda_opacity * inv_n * ((lo + 1).abs() * do + (LOGF + 3) * U * (o * lo).abs()))
    parts = l.sum(1) * inv_n / 3 + cfg.lambda_opacity * inv_n * (o * lo).abs()
    v = pass_ = None
    if cfg.lambda_depth != 0:
        v = f.D / cfg.depth_scale + C_EPS
        pass_ = clip_pass(v)
        dv = fb.dD / cfg.depth_scale + 2 * U * v.abs()
        gdep = torch.where(pass_, -cfg.lambda_depth / v / cfg.depth_scale * inv_n, gdep)
        dgdep = gdep.abs() * (dv / v + 5 * U)
        lv = torch.log(torch.where(pass_, v, torch.ones_like(v))).abs()
        b_loss = b_loss + torch.where(pass_, cfg.lambda_depth * inv_n * (dv / v + LOGF * U * lv + 3 * U * lv), gdep * 0)
        parts = parts + cfg.lambda_depth * inv_n * lv
    gw = dgw = None
    if cfg.lambda_distortion != 0:
        lam_n = cfg.lambda_distortion * inv_n
        ld, AB, a, b = _dist_scan(f.w, f.Ts, f.Dl)
        gw = 2 * lam_n * (AB + f.w * f.Dl / 3) * f.m
        # sum_k |t_j - t_k| dw_k by prefix sums of dw (t sorted along the row)
        _, dAB, _, _ = _dist_scan(fb.dw, f.Ts, f.Dl)
        dAB = dAB.abs() + ((3 * fb.dep + 7) * U)[:, None] * (f.Ts.abs() * f.O[:, None] + fb.Dabs[:, None])
        dgw = (2 * lam_n * (dAB + f.Dl / 3 * (fb.dw + 3 * U * f.w)) + 4 * U * gw.abs()) * f.m
        # the loss: first order in the weights + the prefix sums' roundings, absolute in a_i b_i
        unscaled = 2 * (AB + f.w * f.Dl / 3)
        d_ld = (unscaled.abs() * fb.dw).sum(1) + ((8 * fb.dep + 12) * U) * (a * b * f.m).sum(1) \
            + (f.w * f.w * f.Dl / 3 * 4 * U).sum(1) + fb.dep * U * ld.abs().sum(1)
        b_loss = b_loss + cfg.lambda_distortion * inv_n * (d_ld + 3 * U * ld.abs().sum(1))
        parts = parts + cfg.lambda_distortion * inv_n * ld.abs().sum(1)
    dsig_an, drgbs_an = backward64(f, g, gs, gdep, gw)
    b_dsig, b_drgbs = backward_bound(f, fb, path, g, dg, gs, dgs, gdep, dgdep, gw, dgw)
    c = C_PATH[path] * SLACK
    return types.SimpleNamespace(
        f=f, fb=fb, n_rays=nr, xc=xc, loss=loss, gt=gt, v=v, clip_pass=pass_, g=g, gs=gs, gdep=gdep, gw=gw,
        b_R=fb.dR * c + TINY, b_xc=dx * c + TINY, b_O=fb.dO * c + TINY * (fb.dO > 0), b_D=fb.dD * c + TINY * (fb.dD > 0),
        b_loss=(b_loss + 8 * U * parts) * c + TINY, dsig=dsig * f.m, drgbs=drgbs * f.m[..., None],
        dsig_an=dsig_an, drgbs_an=drgbs_an, b_dsig=b_dsig, b_drgbs=b_drgbs)


def train_bw_ref64(f, path, gop, gdep, grgb, gws):
    """composite_train_bw of the forward f with fp32 upstream gradients per ray (indexed by ray) and dL/dws per sample
    (flat) -> dsig, drgbs (padded, analytic fp64) and their bounds.  The upstream gradients are exact inputs; the
    kernel is fed its own forward outputs, whose errors fb already carries."""
    fb = forward_bounds(f, f.C, f.Ts, path)
    g, go, gd = grgb.double()[f.ray], gop.double()[f.ray], gdep.double()[f.ray]
    gw = pad(gws, f.idx, f.valid) * f.m
    z = torch.zeros_like(go)
    gs = go * (1 - f.O)
    dgs = go.abs() * (fb.dO + 2 * U)
    dsig, drgbs = backward64(f, g, gs, gd, gw)
    b_sig, b_rgb = backward_bound(f, fb, path, g, torch.zeros_like(g), gs, dgs, gd, z, gw, torch.zeros_like(gw))
    return dsig, drgbs, b_sig, b_rgb, fb


def ratio(err, bound):
    """worst err / bound (inf where something moved that must not)"""
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------- NeRFLoss, one element at a time
def nerf_loss_ref64(loss_type, rgb, gt, op, dep, lam_op, lam_depth, scale, up_rgb=None, up_op=None, up_dep=None):
    """ngp_nerf_loss_fw / _bw per element in fp64 (the reference's expressions, losses.py:63-76) -> namespace of
    (value, bound) pairs l_rgb, l_op, l_dep, d_rgb, d_op, d_dep; up_*: the upstream gradient of each term (None: no
    gradient flows into it, the gradient is exactly 0).  A handful of roundings each, counted as in the module
    docstring: the bounds hold for autograd's sequence of the log type's backward (/ (a / b), / b) and for the kernel's
    (/ a) alike."""
    x, y, o, dp = rgb.double(), gt.double(), op.double() + C_EPS, dep.double()
    lam_op, lam_depth, scale = F32(lam_op), F32(lam_depth), F32(scale)
    l, lp, _, rl, rg, _ = rgb_term64(loss_type, x, y)
    lo = torch.log(o)
    v = dp / scale + C_EPS
    ps = clip_pass(v)
    lv = torch.log(torch.where(ps, v, torch.ones_like(v)))
    z = lambda t: torch.zeros_like(t)  # noqa: E731
    out = types.SimpleNamespace(
        l_rgb=(l, (rl + U * l) * SLACK + TINY),
        l_op=(lam_op * (-o * lo), lam_op * (U * o * (lo + 1).abs() + (LOGF + 3) * U * (o * lo).abs()) * SLACK + TINY),
        l_dep=(-lam_depth * lv, lam_depth * (4 * U + (LOGF + 2) * U * lv.abs()) * ps * SLACK + TINY * ps))
    ur = z(x) if up_rgb is None else up_rgb.double()
    uo = z(o) if up_op is None else up_op.double()
    ud = z(v) if up_dep is None else up_dep.double()
    d_rgb = ur * lp
    d_op = uo * lam_op * (-(lo + 1))
    d_dep = torch.where(ps, ud * (-lam_depth) / v / scale, z(v))
    out.d_rgb = (d_rgb, (ur.abs() * (rg + 2 * U * lp.abs())) * SLACK + TINY * (ur != 0))
    out.d_op = (d_op, (uo.abs() * lam_op * ((LOGF + 3) * U * lo.abs() + 6 * U)) * SLACK + TINY * (uo != 0))
    out.d_dep = (d_dep, d_dep.abs() * 8 * U * SLACK + TINY * (d_dep != 0))
    out.clip_pass = ps
    return out


# ------------------------------------------------------- termination margin
def margin_violations(sig, deltas, rays_a, T_thr, T0=None):
    """-> (bad (R, L) bool: samples up to the fp64 termination that break the precondition, f)"""
    n = sig.shape[0]
    z3 = torch.zeros(n, 3)
    f = composite_ref64(sig, z3, deltas, torch.zeros(n), rays_a, T_thr, T0)
    fb = forward_bounds(f, f.C, f.Ts, "serial", T0 is not None)
    k = torch.arange(f.valid.shape[1])[None, :].double()
    upto = f.m  # samples 0..K (the terminating one included)
    lnT = torch.log(f.Ta.clamp(min=1e-300))
    bad = (lnT - math.log(T_thr)).abs() < 4 * (k + 2) * 2.0 ** -20
    bad |= (f.Ta - T_thr).abs() < 2 * fb.dTa
    return bad & upto, f


def enforce_margin(sig, deltas, rays_a, T_thr, T0=None):
    """nudges the offending sigmas (in place, x 1.02 or to a small value) until the precondition holds"""
    for _ in range(200):
        bad, f = margin_violations(sig, deltas, rays_a, T_thr, T0)
        if not bool(bad.any()):
            return sig
        i = f.idx[bad]
        sig[i] = torch.where(sig[i] > 0, sig[i] * 1.02, torch.full_like(sig[i], 0.5))
    raise AssertionError("termination margin not reached")


# --------------------------------------------------------------- input sets
T_THR = {"thr1e-4": 1e-4, "thr1e-2": 1e-2}
DEPTH_SCALE = 0.5  # the scale the v == 1 rows and the two sides of the clip are built for


@functools.lru_cache(maxsize=None)
def rows(name, seed):
    """A designed input set -> namespace(sig, rgbs, deltas, ts (flat fp32), rays_a (R, 3) i64 in shuffled row
    order with a non-identity ray permutation, gt (R, 3) by ray, T_thr, kind: per row a (family, N, term position
    or None) tuple, v1_rows: the rows whose depth term sits at fl(v) == 1).  Families:
      never     transparent to the end, every length of LENGTHS
      term      transparent, then one sample with sigma delta ~ 12 at a position of TERM_POS or the row's last sample,
                then arbitrary samples the kernels must ignore
      opaque    the same with sigma delta ~ 100 (alpha == 1 in fp32, Ta == 0)
      gradual   T drifts through the threshold
      v1        sigma == 0, then one sigma delta = 100 sample at ts == DEPTH_SCALE: D == DEPTH_SCALE exactly
    The termination precondition (module docstring) is enforced here."""
    T_thr = T_THR[name]
    g = torch.Generator().manual_seed(1000 * seed + int(-math.log10(T_thr)))
    lnT = -math.log(T_thr)
    R = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    specs = []
    for N in LENGTHS:
        specs.append(("never", N, None))
    for p in TERM_POS:
        for N in sorted({p + 1, p + 2, p + 40} | {n for n in LENGTHS if n > p + 2 and n - p < 140}):
            specs.append(("term", N, p))
    specs += [("term", 300, 299), ("term", 500, 499), ("term", 500, 130), ("term", 300, 192)]
    specs += [("opaque", 9, 0), ("opaque", 20, 5), ("opaque", 100, 70), ("opaque", 200, 130), ("opaque", 131, 130)]
    for N in (30, 70, 100, 140, 200, 260, 400):
        specs += [("gradual", N, None)] * 3
    specs += [("v1", 1, 0), ("v1", 7, 3), ("v1", 70, 66)]
    # the first five rows (n_rays = 1 and 5 use them)
    head = [("term", 193, 129), ("never", 300, None), ("never", 0, None), ("v1", 7, 3), ("gradual", 140, None)]
    perm = torch.randperm(len(specs), generator=g).tolist()
    specs = head + [specs[i] for i in perm]
    nrows = len(specs)
    sig_l, dl_l, ts_l = [], [], []
    for fam, N, p in specs:
        dl = R(N) * 1e-2 + 1e-3
        t = 0.05 + R(1) * 0.3 + torch.cumsum(dl, 0) - dl
        if fam == "never":
            x = R(N) + 0.1
            x = x / x.sum().clamp(min=1e-9) * lnT * (0.3 + 0.3 * float(R(1)))
        elif fam in ("term", "opaque"):
            x = R(N) * 0.05
            pre = R(p) + 0.1
            x[:p] = pre / pre.sum().clamp(min=1e-9) * lnT * (0.1 + 0.3 * float(R(1))) * min(1.0, p / 8)
            x[p] = 100.0 if fam == "opaque" else 11.5 + float(R(1))
        elif fam == "gradual":
            x = (R(N) * 0.9 + 0.1) * (2.6 / N) * lnT
        else:  # v1
            x = R(N) * 0.05
            x[:p] = 0.0
            x[p] = 100.0
            dl = torch.full((N,), 2.0 ** -7)
            t = DEPTH_SCALE + (torch.arange(N) - p).float() * 2.0 ** -7
        sig_l.append(x / dl); dl_l.append(dl); ts_l.append(t)
    Ns = torch.tensor([s[1] for s in specs])
    # storage order differs from row order, ray ids are a non-identity permutation
    order = torch.randperm(nrows, generator=g)
    start = torch.zeros(nrows, dtype=torch.int64)
    start[order] = torch.cumsum(Ns[order], 0) - Ns[order]
    ray = torch.randperm(nrows, generator=g)
    rays_a = torch.stack([ray, start, Ns], 1).contiguous()
    n = int(Ns.sum())
    sig, deltas, ts = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    for r in range(nrows):
        s, N = int(start[r]), int(Ns[r])
        sig[s:s + N], deltas[s:s + N], ts[s:s + N] = sig_l[r].float(), dl_l[r].float(), ts_l[r].float()
    rgbs = R(n, 3).float()
    gt = R(nrows, 3).float()
    enforce_margin(sig, deltas, rays_a, T_thr)
    v1_rows = torch.tensor([r for r, s in enumerate(specs) if s[0] == "v1"])
    # keep the depth term a margin away from the clip except on the v1 rows
    for _ in range(50):
        f = composite_ref64(sig, rgbs, deltas, ts, rays_a, T_thr)
        near = ((f.D / F32(DEPTH_SCALE) + C_EPS) - 1).abs() < 1e-3
        near[v1_rows] = False
        if not bool(near.any()):
            break
        for r in torch.nonzero(near)[:, 0].tolist():
            s, N = int(start[r]), int(Ns[r])
            ts[s:s + N] += 0.01
    else:
        raise AssertionError("depth margin not reached")
    assert not bool((ray == torch.arange(nrows)).all()) and n <= 60000 and nrows <= 700
    return types.SimpleNamespace(name=name, sig=sig, rgbs=rgbs, deltas=deltas, ts=ts, rays_a=rays_a, gt=gt, T_thr=T_thr,
                                 kind=specs, v1_rows=v1_rows, n=n, n_rows=nrows)


BG = {"zero": (0.0, 0.0, 0.0), "colour": (0.9, 0.25, 0.6)}


def bg_tensor(name):
    return torch.tensor(BG[name], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def reference(name, seed, loss_type, bg, lambda_depth, depth_scale, lambda_distortion, n_rays, path="tree"):
    """loss_ref64 of an input set (computed once per process; read-only)"""
    inp = rows(name, seed)
    cfg = config(loss_type, 1e-3, lambda_depth, depth_scale, lambda_distortion)
    return loss_ref64(inp, cfg, bg_tensor(bg), n_rays, path)


# ------------------------------------------------------- composite_test_fw
@functools.lru_cache(maxsize=None)
def alive_rows(Ns, seed, n_alive=300, n_rays=1000, T_thr=1e-4):
    """Inputs of ngp_composite_test_fw: (n_alive, Ns) samples, alive (a shuffled subset of the rays), n_eff in
    0..Ns (zeros and values below Ns forced), non-zero opacity / depth / rgb to start from."""
    g = torch.Generator().manual_seed(77 * seed + Ns)
    R = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    alive = torch.randperm(n_rays, generator=g)[:n_alive].contiguous()
    n_eff = torch.randint(0, Ns + 1, (n_alive,), generator=g).to(torch.int32)
    n_eff[:8] = torch.tensor([0, Ns, 0, max(Ns - 1, 0), Ns, 1, Ns, 0], dtype=torch.int32).clamp(max=Ns)
    deltas = R(n_alive, Ns) * 1e-2 + 1e-3
    x = R(n_alive, Ns) * 2.5 * (R(n_alive, 1) < 0.7) + 12.0 * (R(n_alive, Ns) < 0.1)
    sig = (x / deltas).float()
    deltas = deltas.float()
    ts = (0.05 + torch.cumsum(deltas, 1)).float()
    rgbs = R(n_alive, Ns, 3).float()
    op0 = (R(n_rays) * 0.9).float()
    dep0, rgb0 = R(n_rays).float(), R(n_rays, 3).float()
    rays_a = torch.stack([alive, torch.arange(n_alive) * Ns, n_eff.long()], 1)
    T0 = 1 - op0.double()[alive]
    flat_sig = sig.reshape(-1)
    enforce_margin(flat_sig, deltas.reshape(-1), rays_a, T_thr, T0)
    return types.SimpleNamespace(sig=flat_sig.reshape(n_alive, Ns), rgbs=rgbs, deltas=deltas, ts=ts, alive=alive,
                                 n_eff=n_eff, op0=op0, dep0=dep0, rgb0=rgb0, rays_a=rays_a, T0=T0, T_thr=T_thr, Ns=Ns)


def alive_ref64(t):
    """fp64 composite_test_fw of alive_rows -> namespace(alive (n_alive,), op / dep (n_rays,), rgb (n_rays, 3) and
    their bounds b_op / b_dep / b_rgb; rays not listed keep their values, bound 0)"""
    f = composite_ref64(t.sig.reshape(-1), t.rgbs.reshape(-1, 3), t.deltas.reshape(-1), t.ts.reshape(-1), t.rays_a,
                        t.T_thr, t.T0)
    fb = forward_bounds(f, f.C, f.Ts, "test", T0=True)
    r = t.alive
    op, dep, rgb = t.op0.double().clone(), t.dep0.double().clone(), t.rgb0.double().clone()
    b_op, b_dep, b_rgb = torch.zeros_like(op), torch.zeros_like(dep), torch.zeros_like(rgb)
    live = t.n_eff.long() > 0
    c = C_PATH["test"] * SLACK
    dT0 = U * f.O  # T starts at fl(1 - opacity): relative u of every weight
    op[r] += f.O; dep[r] += f.D; rgb[r] += f.R
    b_op[r] = (fb.dO + dT0 + fb.dep * U * t.op0.double()[r]) * c * live
    b_dep[r] = (fb.dD + U * fb.Dabs + fb.dep * U * t.dep0.double()[r]) * c * live
    b_rgb[r] = (fb.dR + U * fb.Rabs + (fb.dep * U)[:, None] * t.rgb0.double()[r]) * c * live[:, None]
    terminated = f.K < f.N
    alive = torch.where(terminated | ~live, torch.full_like(r, -1), r)
    return types.SimpleNamespace(alive=alive, op=op, dep=dep, rgb=rgb, b_op=b_op, b_dep=b_dep, b_rgb=b_rgb, f=f)
