"""Exact input sets and a plain fp64 reference for the MLP backward
(field_bwd.hip field_bwd_mlp_coop_kernel, C ABI ngp_field_backward_mlp_act).  CPU
only, numpy fp64.

The kernel stores the forward in fp16, the gradient chain in fp16 times a
power of two per sample, re-scales the weight-gradient operands to one power of
two per layer and 128-row block, sums in fp32 MFMA tiles and adds the tiles to
global memory with fp32 atomics.  On a `lattice_case` every one of those values
is exactly representable where it is stored and every fp32 partial sum is exact
(`check_exact` asserts the conditions), so the result does not depend on the
summation order, the tiling, the order of the atomics or the exponents chosen:
it equals `mlp_bwd_ref64` bit for bit.

Network (hashgrid.OW, row-major [out][in] fp16):
    h1 = relu(W1 e)          e: 32 encoding features         W1 64x32
    h  = W2 h1               h[0] -> sigma = TruncExp(h[0])  W2 16x64
    h3 = relu(W3 [SH16(d), h])                               W3 64x32
    h4 = relu(W4 h3)                                         W4 64x64
    o  = W5 h4               rgb = act(o[0..2])              W5 16x64
"""
import functools
from types import SimpleNamespace

import numpy as np

from capi import C

RGB_NONE, RGB_RELU = C["NGP_RGB_NONE"], C["NGP_RGB_RELU"]
OW = {"W1": (0, 64, 32), "W2": (2048, 16, 64), "W3": (3072, 64, 32), "W4": (5120, 64, 64), "W5": (9216, 16, 64)}
MLP_PARAMS = C["NGP_MLP_PARAMS"]
BLOCK_ROWS = 128       # rows per block iteration (CW * 16)
E_SPREAD = 4           # per-row gradient exponents e_s in 0..E_SPREAD
ZERO_SHARE = 8         # one row in ZERO_SHARE has an all-zero upstream gradient
BASE_MAX = 4           # grad_mlp starts from integers in [-BASE_MAX, BASE_MAX] x q_w


def _sparse_rows(rng, n_out, n_in, lo=0, one_plus=False):
    """n_out rows of n_in columns, 3 nonzeros in {-1, +1} per row at columns >= lo; one_plus: at least
    one +1 per row (a row of -1 only over a ReLU's non-negative output is a dead unit)"""
    W = np.zeros((n_out, n_in))
    for o in range(n_out):
        cols = lo + rng.choice(n_in - lo, 3, replace=False)
        W[o, cols] = rng.choice([-1.0, 1.0], 3)
        if one_plus:
            W[o, cols[0]] = 1.0
    return W


def lattice_weights(seed):
    """The weight set shared by every lattice case: 3 nonzeros in {-1, +1} per
    row; row 0 of W2 zero (h0 = 0: TruncExp's backward factor is expf(0) = 1);
    W3's 16 SH columns zero (the forward never sees the inexact SH values);
    W5 rows 3..15 zero; the nonzeros of W5 rows 0..2 spread over the four
    16-unit tiles of the hidden layer so that every tile carries gradient, two
    +1 and one -1 each so that the ReLU colour mode passes part of the rows."""
    rng = np.random.default_rng(1000 + seed)
    W = {"W1": _sparse_rows(rng, 64, 32), "W2": _sparse_rows(rng, 16, 64), "W3": _sparse_rows(rng, 64, 32, lo=16),
         "W4": _sparse_rows(rng, 64, 64, one_plus=True), "W5": np.zeros((16, 64))}
    W["W2"][0] = 0.0
    for r in range(3):
        for j, sign in enumerate(rng.permutation([1.0, 1.0, -1.0])):  # (mixed signs: o > 0 on part of the rows)
            W["W5"][r, 16 * ((3 * r + j) % 4) + int(rng.integers(16))] = sign
    return W


def flat_weights(W):
    flat = np.zeros(MLP_PARAMS)
    for name, (o, od, idim) in OW.items():
        flat[o:o + od * idim] = W[name].reshape(-1)
    return flat


@functools.lru_cache(maxsize=None)
def lattice_case(n, seed=0, shift=0, act=RGB_NONE):
    """n rows of exact inputs.  enc: integers in [-2, 2]; dirs: random,
    unnormalised; dL_drgb in {-1, 0, 1} x 2^(shift - 10 - e_s) with at least one
    nonzero per live row, dL_dsig likewise, e_s in 0..E_SPREAD per row; one row
    in ZERO_SHARE has an all-zero upstream gradient.  base: the integer lattice
    grad_mlp starts from, in units of q_w = 2^(shift - 10 - E_SPREAD) (the
    smallest quantum of any gradient x integer activation product).  The random
    draws do not depend on shift or act: a shift scales dL and base by 2^shift."""
    rng = np.random.default_rng(seed * 7919 + n)
    enc = rng.integers(-2, 3, size=(n, 32)).astype(np.float64)
    dirs = rng.standard_normal((n, 3))
    dirs[np.abs(dirs).sum(1) < 1e-3] = (0.0, 0.0, 1.0)
    es = rng.integers(0, E_SPREAD + 1, size=n)
    q = np.ldexp(1.0, shift - 10 - es)  # per-row quantum
    drgb = rng.integers(-1, 2, size=(n, 3)).astype(np.float64)
    none = ~drgb.any(1)
    drgb[none, rng.integers(0, 3, size=n)[none]] = 1.0
    dsig = rng.integers(-1, 2, size=n).astype(np.float64)
    zero = rng.integers(0, ZERO_SHARE, size=n) == 0
    if n >= 2 * ZERO_SHARE:
        zero[n // 2] = True  # (every set of more than a few rows holds one)
    drgb[zero] = 0.0
    dsig[zero] = 0.0
    q_w = np.ldexp(1.0, shift - 10 - E_SPREAD)
    base = rng.integers(-BASE_MAX, BASE_MAX + 1, size=MLP_PARAMS).astype(np.float64) * q_w
    return SimpleNamespace(n=n, seed=seed, shift=shift, act=act, W=lattice_weights(seed), enc=enc,
                           dirs=dirs.astype(np.float32), es=es, q=q, q_w=q_w, zero=zero,
                           dsig=dsig * q, drgb=drgb * q[:, None], base=base)


def to_pair_major(enc, stride, fill=0.0):
    """(n, 32) -> (8, stride, 4): pair p holds features 4p..4p+3 of every row (ngp_hash_encode's layout)"""
    n = enc.shape[0]
    out = np.full((8, stride, 4), fill, dtype=enc.dtype)
    out[:, :n, :] = enc.reshape(n, 8, 4).transpose(1, 0, 2)
    return out


def mlp_bwd_ref64(enc, sh, W, dsig, drgb, act, rows=None, count=None, pm_stride=0):
    """The MLP backward in fp64, row by row semantics, no tiles and no exponents.

    enc: (n, 32), or pair-major (8, pm_stride, 4) when pm_stride > 0; sh: (n, 16)
    SH values the colour net sees (fp16 values in fp64).  rows: the sample list
    (default: 0..n-1); count: how many of its entries are processed (default:
    all).  Compact row j of every per-row result belongs to sample rows[j].
    -> namespace: denc (count, 32); dW[name] weight gradients; absW3 = sum_n |G| |c|
    and termsW3 = the number of nonzero terms per element of W3 (for the SH
    columns' bound); the forward / gradient storage points (for check_exact)."""
    enc = np.asarray(enc, dtype=np.float64)
    if pm_stride > 0:
        assert enc.shape == (8, pm_stride, 4)
        enc = enc.transpose(1, 0, 2).reshape(pm_stride, 32)
    rows = np.arange(enc.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    rows = rows[:len(rows) if count is None else count]
    e = enc[rows]
    s = np.asarray(sh, dtype=np.float64)[rows]
    gs = np.asarray(dsig, dtype=np.float64)[rows]
    gr = np.asarray(drgb, dtype=np.float64)[rows]
    relu = lambda v: np.maximum(v, 0.0)
    # forward
    h1 = relu(e @ W["W1"].T)
    h = h1 @ W["W2"].T
    c = np.concatenate([s, h], axis=1)
    h3 = relu(c @ W["W3"].T)
    h4 = relu(h3 @ W["W4"].T)
    o = h4 @ W["W5"].T
    # backward
    dout = np.zeros_like(o)
    dout[:, :3] = gr if act == RGB_NONE else gr * (o[:, :3] > 0)
    da4 = (dout @ W["W5"]) * (h4 > 0)
    da3 = (da4 @ W["W4"]) * (h3 > 0)
    dh = (da3 @ W["W3"])[:, 16:].copy()
    dh[:, 0] += gs * np.exp(np.clip(h[:, 0], -15.0, 15.0))
    da1 = (dh @ W["W2"]) * (h1 > 0)
    denc = da1 @ W["W1"]
    G = {"W5": dout, "W4": da4, "W3": da3, "W2": dh, "W1": da1}
    H = {"W5": h4, "W4": h3, "W3": c, "W2": h1, "W1": e}
    dW = {k: G[k].T @ H[k] for k in G}
    absW = {k: np.abs(G[k]).T @ np.abs(H[k]) for k in G}
    termsW3 = (G["W3"] != 0).astype(np.float64).T @ (H["W3"] != 0).astype(np.float64)
    return SimpleNamespace(rows=rows, denc=denc, dW=dW, absW=absW, termsW3=termsW3, G=G, H=H, h=h, o=o)


def flat_grad(dW, base=None):
    g = np.zeros(MLP_PARAMS) if base is None else np.array(base, dtype=np.float64)
    for name, (o, od, idim) in OW.items():
        g[o:o + od * idim] += dW[name].reshape(-1)
    return g


def sh_columns_mask():
    """True at W3's 16 SH columns of the flat buffer (the only inexact elements of a lattice case)"""
    m = np.zeros(MLP_PARAMS, dtype=bool)
    o, od, idim = OW["W3"]
    m[o:o + od * idim].reshape(od, idim)[:, :16] = True
    return m


def _colsum_exp(W):
    """ceil(log2(max_i sum_o |W[o][i]|)): how far one W^T can lift a gradient's largest entry"""
    a = np.abs(W).sum(0).max()
    return int(np.ceil(np.log2(a))) if a > 0 else 0


def check_exact(case, rows=None, count=None):
    """The conditions under which ANY evaluation that stores the forward in
    fp16, the gradient chain in fp16 x a power of two per row (>= 11 bits below
    the row's largest entry), a block's weight-gradient operands in fp16 x one
    power of two per aligned 128-row block, and sums in fp32 is exact:

    1. every forward storage point (h1, h, h3, h4, o) round-trips through fp16;
    2. per row and gradient storage point (dout, da4, da3, dh, da1) the entries
       are multiples of the row's quantum q with max / q < 2^11;
    3. per weight element every G x H term is a multiple of q_w, and
       (sum_n |G H| + |base|) / q_w <= 2^24: any order of fp32 adds is exact,
       across blocks and through the atomics too;
    4. within any aligned 128-row block of the processing order, the block's
       largest chain input (dout, resp. dh) over the smallest row quantum, times
       the lift 2^k of the inner layers' W^T (k5 + k4, resp. k2), stays <= 2^27:
       with the largest entry scaled into [2^13, 2^14) the smallest quantum then
       sits at >= 2^-14, ten bits above fp16's subnormal floor 2^-24.
    Conditions, not measurements.  -> the reference of that row list."""
    sh = np.zeros((case.n, 16))  # (W3's SH columns are zero: the chain does not depend on SH)
    r = mlp_bwd_ref64(case.enc, sh, case.W, case.dsig, case.drgb, case.act, rows, count)
    assert not case.W["W3"][:, :16].any() and not case.W["W2"][0].any() and not case.W["W5"][3:].any()
    assert not r.h[:, 0].any()
    # 1
    for name, v in (("h1", r.H["W2"]), ("h", r.h), ("h3", r.H["W4"]), ("h4", r.H["W5"]), ("o", r.o)):
        assert np.array_equal(v.astype(np.float16).astype(np.float64), v), name
        assert np.array_equal(v, np.round(v)), name
    # 2
    q = case.q[r.rows][:, None]
    for name, g in r.G.items():
        u = g / q
        assert np.array_equal(u, np.round(u)), name
        assert np.abs(u).max(initial=0.0) < 2 ** 11, name
    # 3
    budget = 0.0
    for name, (o, od, idim) in OW.items():
        a = r.absW[name] + np.abs(case.base[o:o + od * idim]).reshape(od, idim)
        if name == "W3":
            a = a[:, 16:]
        u = r.dW[name] / case.q_w
        if name == "W3":
            u = u[:, 16:]
        assert np.array_equal(u, np.round(u)), name
        budget = max(budget, float(a.max() / case.q_w))
    assert budget <= 2 ** 24, budget
    # 4
    k5, k4, k2 = _colsum_exp(case.W["W5"]), _colsum_exp(case.W["W4"]), _colsum_exp(case.W["W2"])
    spread = 0.0
    for name, lift in (("W5", k5 + k4), ("W2", k2)):
        g = np.abs(r.G[name]).max(1)
        for b in range(0, len(g), BLOCK_ROWS):
            gb, qb = g[b:b + BLOCK_ROWS], q[b:b + BLOCK_ROWS, 0]
            if gb.any():
                spread = max(spread, float(gb.max() / qb[gb > 0].min()) * 2.0 ** lift)
    assert spread <= 2 ** 27, spread
    r.budget_bits = float(np.log2(max(budget, 1.0)))
    r.spread_bits = float(np.log2(max(spread, 1.0)))
    return r


def tiles_with_gradient(dW):
    """how many of the 40 16x16 weight-gradient tiles (W5: its first 16 rows x 4) hold a nonzero entry"""
    cnt = 0
    for name, (_, od, idim) in OW.items():
        d = dW[name]
        for o0 in range(0, od, 16):
            for i0 in range(0, idim, 16):
                cnt += bool(d[o0:o0 + 16, i0:i0 + 16].any())
    return cnt


def list_rows(n, seed=0):
    """a shuffled list of about a third of n rows (at least one)"""
    rng = np.random.default_rng(31 * seed + n)
    return rng.permutation(n)[:max(1, n // 3)].astype(np.int32)


def perm_rows(n, seed=0):
    """every row once, shuffled"""
    return np.random.default_rng(57 * seed + n).permutation(n).astype(np.int32)


def multipass_n(cus=256):
    """two passes of one resident block per CU and a partial block: 2 or 3 passes of the persistent loop
    for 2 or 1 resident blocks per CU"""
    return 2 * BLOCK_ROWS * cus + 165
