"""Exact input sets and a plain fp64 reference for the field forward (field.hip:
field_fwd_kernel, field_encode_mlp_reg_kernel, field_first_chunk_kernel,
hash_encode_kernel, encode_coarse_first_kernel).  CPU only, numpy fp64; the
forward's counterpart of mlp_bwd_ref.py.

The kernels store the encoding and every layer output in fp16 and sum in fp32
MFMA tiles over a permuted K order (field_net.h P64 / P32).  On the sets below
every storage point is an integer that fp16 holds exactly and every partial
sum is an integer below 2^24 (`check_exact_fwd` asserts the conditions), so the
tiling and the K permutation cannot change a bit: h, the encoding and the
colour row o equal `mlp_fwd_ref64` bit for bit.  The SH probes feed the
inexact SH values through sums of a single term, which are exact whatever the
value.

Network (hashgrid.OW, row-major [out][in] fp16):
    h1 = relu(W1 e)          e: 32 encoding features         W1 64x32
    h  = W2 h1               h[0] -> sigma = exp(h[0])       W2 16x64
    h3 = relu(W3 [SH16(d), h])                               W3 64x32
    h4 = relu(W4 h3)                                         W4 64x64
    o  = W5 h4               rgb = act(o[0..2])              W5 16x64
"""
import functools
import os
import re
from types import SimpleNamespace

import numpy as np

from mlp_bwd_ref import OW, _sparse_rows, flat_weights, list_rows, perm_rows, to_pair_major  # noqa: F401
from capi import C

RGB_SIGMOID, RGB_NONE, RGB_LEAKY_RELU, RGB_RELU = (C["NGP_RGB_" + m] for m in ("SIGMOID", "NONE", "LEAKY_RELU", "RELU"))
ACTS = {"sigmoid": RGB_SIGMOID, "none": RGB_NONE, "leaky": RGB_LEAKY_RELU, "relu": RGB_RELU}
MLP_PARAMS = C["NGP_MLP_PARAMS"]
N_LEVELS = 16
T_THR = 1e-4

# below, at and past a column block (16), a wave's chunk (64), field_fwd_kernel's block (4 x 64) and
# field_encode_mlp_reg_kernel's block (8 x 64), and one row
SIZES = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513]
# round 1: rows per launch (below, at, past a block's 8 waves; test_field_gpu's 400) and samples per row
# (none, one, around a column block, around the chunk, several chunks)
ROUND1_R = [1, 7, 8, 9, 400]
ROUND1_N = [65, 200, 0, 64, 1, 17, 63, 16, 15]

# what bounds the resident blocks of the persistent forward kernels from above (DESIGN.md "The field
# forward, value for value"): the CU's LDS over the block's weight image, and the CU's wave slots
LDS_PER_CU = 160 * 1024
WAVES_PER_CU = 4 * 8  # 4 SIMDs x 8 waves


def _csrc(name):
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ar-nerf_amd", "csrc", name)


@functools.lru_cache(maxsize=None)
def source_constants():
    """R32, R64 (field_net.h), FEM2_WAVES (field.hip) and the forward kernels' block sizes, parsed from the
    sources -> namespace; image_bytes = the forward weight image sw[SWF] in bytes"""
    net, fld = open(_csrc("field_net.h")).read(), open(_csrc("field.hip")).read()
    m = re.search(r"constexpr int R32 = (\d+), R64 = (\d+);", net)
    r32, r64 = int(m.group(1)), int(m.group(2))
    waves = int(re.search(r"constexpr int FEM2_WAVES = (\d+)", fld).group(1))
    swf = 64 * r32 + 16 * r64 + 64 * r32 + 64 * r64 + 16 * r64
    assert re.search(r"SWF = SW5 \+ 16 \* R64;", net) and "SW5 = SW4 + 64 * R64" in net
    bounds = {k: re.search(r"__launch_bounds__\(([^)]*)\)\s*" + k + r"\(", fld).group(1)
              for k in ("field_fwd_kernel", "field_encode_mlp_reg_kernel", "field_first_chunk_kernel")}
    return SimpleNamespace(R32=r32, R64=r64, FEM2_WAVES=waves, image_bytes=2 * swf, launch_bounds=bounds)


def resident_block_bounds():
    """upper bounds on resident blocks per CU: (256-thread field_fwd_kernel, 512-thread reg / first-chunk)"""
    k = source_constants()
    by_lds = LDS_PER_CU // k.image_bytes
    return min(by_lds, WAVES_PER_CU // 4), min(by_lds, WAVES_PER_CU // k.FEM2_WAVES)


def multipass_sizes(cus=256):
    """One size per kernel family at which the persistent loop takes a second iteration whatever the true
    resident-block count is (it is at most the bound, so one iteration covers at most bound x CUs blocks):
    fwd:   field_fwd_kernel, 64 rows per block iteration, <= 6 blocks per CU: 2 * 64 * 6 * CUs + 37 rows
           (every wave of a full grid takes a second 16-row block; the last block is partial);
    reg:   field_encode_mlp_reg_kernel, 512 rows per block iteration, <= 4 blocks per CU:
           512 * 4 * CUs + 64 * 37 + 5 rows (37 full chunks and a 5-row one past any first iteration);
    first: field_first_chunk_kernel, 8 rows per block iteration, <= 4 blocks per CU: 8 * 4 * CUs + 133 rows."""
    b256, b512 = resident_block_bounds()
    w = source_constants().FEM2_WAVES
    return SimpleNamespace(fwd=2 * 64 * b256 * cus + 37, reg=64 * w * b512 * cus + 64 * 37 + 5,
                           first=w * b512 * cus + 133, fwd_first_pass=64 * b256 * cus,
                           reg_first_pass=64 * w * b512 * cus, first_first_pass=w * b512 * cus)


# ---------------------------------------------------------------------------------------------- weight families
def lattice_fwd_weights(seed):
    """3 nonzeros in {-1, +1} per row in every matrix; row 0 of W2 non-zero (h0 varies in sign and size over the
    rows); W3's 16 SH columns zero; W4 rows with at least one +1; W5 rows 0..2 with two +1 and one -1, rows 3..15
    non-zero too (the forward computes them and must not let them leak)."""
    rng = np.random.default_rng(2000 + seed)
    W = {"W1": _sparse_rows(rng, 64, 32), "W2": _sparse_rows(rng, 16, 64), "W3": _sparse_rows(rng, 64, 32, lo=16),
         "W4": _sparse_rows(rng, 64, 64, one_plus=True), "W5": _sparse_rows(rng, 16, 64)}
    for r in range(3):
        W["W5"][r, np.nonzero(W["W5"][r])[0]] = rng.permutation([1.0, 1.0, -1.0])
    W["W2"][0, np.nonzero(W["W2"][0])[0]] = rng.permutation([1.0, 1.0, -1.0])  # (h0 of both signs)
    return W


def cyclic_weights(k):
    """One nonzero per row: W1[o, (o+k) % 32], W2[o, (o+k) % 64], W3[o, 16 + (o+k) % 16], W4[o, (o+k) % 64],
    W5[o, (o+k) % 64], of sign (-1)^(o+k) -- but +1 where a -1 would feed only ReLU zeros downstream.  The rule:
    a weight that reads a ReLU's output (>= 0) and writes into a ReLU must be positive, or its unit is dead and the
    weight unseen.  That is every W4 element; and W3's element reads h[j] = s2(j) h1[.] with h1 >= 0, so it takes
    W2 row j's sign s2(j).  W1 reads signed encodings, W2 and W5 write unclipped outputs: they keep (-1)^(o+k).
    Over k = 0..63 every element of W1, W2, W4, W5 and of W3's h columns is non-zero in at least one set."""
    W = {name: np.zeros((od, idim)) for name, (_, od, idim) in OW.items()}
    sign = lambda o: 1.0 if (o + k) % 2 == 0 else -1.0  # noqa: E731
    for o in range(64):
        W["W1"][o, (o + k) % 32] = sign(o)
        W["W4"][o, (o + k) % 64] = 1.0
    for o in range(16):
        W["W2"][o, (o + k) % 64] = sign(o)
        W["W5"][o, (o + k) % 64] = sign(o)
    for o in range(64):
        j = (o + k) % 16
        W["W3"][o, 16 + j] = sign(j)  # (= W2 row j's sign)
    return W


def sh_probe_weights(k, sign):
    """W3 row o has the single nonzero sign * (-1)^o in SH column (o + k) % 16 and no h columns; W4 is the selection
    h4[o] = h3[(o + 7k) % 64]; W5 row r is the selection o[r] = h4[(21 r + k) % 64] (rows 3..15 too: computed, never
    to leak).  Every sum has one term of weight +-1, so it is exact whatever the SH value: under colour mode none
    rgb[r] = relu(+-SH component probe_column(k, r)) of the sample's own direction, rounded to fp16 -- it differs
    from sample to sample, which pins the routing of samples and lane groups.  W1, W2: lattice_fwd_weights(0)'s."""
    lat = lattice_fwd_weights(0)
    W = {"W1": lat["W1"], "W2": lat["W2"], "W3": np.zeros((64, 32)), "W4": np.zeros((64, 64)), "W5": np.zeros((16, 64))}
    for o in range(64):
        W["W3"][o, (o + k) % 16] = sign * (1.0 if o % 2 == 0 else -1.0)
        W["W4"][o, (o + 7 * k) % 64] = 1.0
    for r in range(16):
        W["W5"][r, (21 * r + k) % 64] = 1.0
    return W


def probe_column(k, r, sign=1):
    """-> (SH column, sign) that colour channel r of sh_probe_weights(k, sign) shows"""
    u = ((21 * r + k) % 64 + 7 * k) % 64  # the h3 unit
    return (u + k) % 16, sign * (1 if u % 2 == 0 else -1)


PROBES = [(k, s) for k in range(16) for s in (1, -1)]


def weights(family, key):
    """family 'lattice' (key: seed), 'cyclic' (key: k) or 'probe' (key: (k, sign))"""
    if family == "lattice":
        return lattice_fwd_weights(key)
    if family == "cyclic":
        return cyclic_weights(key)
    return sh_probe_weights(*key)


# ------------------------------------------------------------------------------------------------------ inputs
def enc_rows(n, seed=0):
    """(n, 32) integers in [-2, 2], as mlp_bwd_ref.lattice_case's encodings"""
    return np.random.default_rng(seed * 7919 + n + 5).integers(-2, 3, size=(n, 32)).astype(np.float64)


def dir_rows(n, seed=0):
    """(n, 3) f32 random, unnormalised directions"""
    d = np.random.default_rng(seed * 104729 + n + 11).standard_normal((n, 3))
    d[np.abs(d).sum(1) < 1e-3] = (0.0, 0.0, 1.0)
    return d.astype(np.float32)


def point_rows(n, scale, seed=0):
    """(n, 3) f32: the box corners and face centres first, then points up to 3x outside the box (every octant),
    a third of them inside it"""
    rng = np.random.default_rng(seed * 15485863 + n + 17)
    x = (rng.random((n, 3)) * 2 - 1) * scale * 3.0
    inside = rng.random(n) < 1 / 3
    x[inside] /= 3.0
    fixed = [[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    fixed += [[s if a == b else 0.0 for b in range(3)] for a in range(3) for s in (-1, 1)]
    fixed = np.array(fixed) * scale
    k = min(n, len(fixed))
    x[n - k:] = fixed[:k]  # (at the end: the last, partial blocks hold them)
    return x.astype(np.float32)


def sh16(dirs):
    """oracle.sh4 of the directions: the fp16-rounded SH values held as fp64"""
    import torch
    import oracle as O
    return O.sh4(torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float32))).double().numpy()


def level_codes(seed):
    """(16, 2) integers in [-2, 2]: the feature pair of every entry of level l"""
    return np.random.default_rng(4000 + seed).integers(-2, 3, size=(N_LEVELS, 2)).astype(np.float64)


def const_level_table(spec, c):
    """The hash table (n_entries, 2) fp16 with every entry of level l set to the pair c[l].  Each corner product
    w c is exact, the fp32 fmaf chain sums the eight weights to 1 within about 2^-20, and the single fp16 rounding
    returns c exactly, whatever the point: with this table the gathering kernels see exact inputs too.
    spec: oracle.HashGridSpec (or anything with offsets[17] and n_entries)."""
    off = [int(v) for v in spec.offsets]
    tab = np.empty((int(spec.n_entries), 2), dtype=np.float16)
    for l in range(N_LEVELS):
        tab[off[l]:off[l + 1]] = np.asarray(c[l], dtype=np.float16)
    return tab


# --------------------------------------------------------------------------------------------------- reference
def mlp_fwd_ref64(enc, sh, W):
    """The two nets in plain fp64 matmuls: no tiles, no permutations.  enc (n, 32); sh (n, 16): the fp16-rounded
    oracle.sh4 values held as fp64 -> h1, h, h3, h4, o (zeros are +0, as an accumulator that starts at +0 gives)."""
    enc, sh = np.asarray(enc, dtype=np.float64), np.asarray(sh, dtype=np.float64)
    relu = lambda v: np.maximum(v, 0.0) + 0.0  # noqa: E731
    h1 = relu(enc @ W["W1"].T)
    h = h1 @ W["W2"].T + 0.0
    h3 = relu(np.concatenate([sh, h], axis=1) @ W["W3"].T)
    h4 = relu(h3 @ W["W4"].T)
    o = h4 @ W["W5"].T + 0.0
    return h1, h, h3, h4, o


def rgb_ref(o, act):
    """The colour output of the row o (n, >= 3; fp16 values in fp64) in mode act.  none / relu / leaky: the exact
    fp32 value the kernel must give (leaky: fp16(fp32(o) * 0.01f) below or at zero); sigmoid: fp64."""
    o = np.asarray(o, dtype=np.float64)[:, :3]
    if act == RGB_SIGMOID:
        return 1.0 / (1.0 + np.exp(-o))
    if act == RGB_NONE:
        return o.astype(np.float32)
    if act == RGB_RELU:
        return (np.maximum(o, 0.0) + 0.0).astype(np.float32)
    slope = (o.astype(np.float32) * np.float32(0.01)).astype(np.float16).astype(np.float32)
    return np.where(o > 0, o.astype(np.float32), slope)


def check_exact_fwd(enc, sh, W):
    """The conditions under which ANY evaluation that stores the encoding and every layer output in fp16 and sums
    in fp32, in any order and over any K permutation, is exact:

    1. every storage point (enc, h1, h, h3, h4, o) is an integer with |v| <= 2048: it round-trips through fp16;
    2. every partial sum is an integer below 2^24: sum_k |W[o][k]| |x[k]| < 2^24 per output;
    or, for a layer that sees the (inexact) SH values -- W3's SH columns non-zero -- and every layer after it:
    3. each row of the matrix has exactly one nonzero, of magnitude 1: every sum has a single term, so each
       storage point holds an fp16 value (or its negation, or zero) unchanged.
    Conditions, not measurements.  -> (h1, h, h3, h4, o)."""
    h1, h, h3, h4, o = r = mlp_fwd_ref64(enc, sh, W)
    probe = bool(W["W3"][:, :16].any())
    cin = np.concatenate([sh if probe else np.zeros_like(sh), h], axis=1)  # (zero SH columns: the values are unseen)
    for name, x, y in (("W1", enc, h1), ("W2", h1, h), ("W3", cin, h3), ("W4", h3, h4), ("W5", h4, o)):
        if probe and name in ("W3", "W4", "W5"):
            assert ((W[name] != 0).sum(1) == 1).all() and set(np.unique(W[name])) <= {-1.0, 0.0, 1.0}, name
            if name == "W3":
                assert not W[name][:, 16:].any()
            assert np.array_equal(y.astype(np.float16).astype(np.float64), y), name
            continue
        for v in (x, y):
            assert np.array_equal(v, np.round(v)) and np.abs(v).max(initial=0.0) <= 2048, name
            assert np.array_equal(v.astype(np.float16).astype(np.float64), v), name
        assert np.array_equal(W[name].astype(np.float16).astype(np.float64), W[name]), name
        assert (np.abs(x) @ np.abs(W[name]).T).max(initial=0.0) < 2 ** 24, name
    return r


def row_position(j):
    """where launch row j runs -> text: field_fwd_kernel deals 16-row column blocks to waves, 4 waves per block;
    the register kernels deal 64-row chunks to waves, each chunk in 4 column blocks"""
    return (f"row {j} (field_fwd_kernel: column block {j // 16}, wave {(j // 16) % 4} of block {j // 64}, lane "
            f"{j % 16}; chunk kernels: chunk {j // 64}, column block {(j % 64) // 16}, lane {j % 64})")


# ----------------------------------------------------------------------------------------------------- round 1
def round1_rows(R, sigma, kind="all", seed=0):
    """R rows of round 1 (ngp_field_forward_first_pre_act) for a field of constant density sigma.

    Row r has N = ROUND1_N[r % 9] samples at start[r] (a gap of r % 3 unused samples before it), and is
    `clear` (sigma x sum of its first chunk's deltas = 2) or `opaque` (= 30), alternating over the rows of each N.
    The deltas of the first min(N, 64) samples are random in a 3 : 1 range and scaled to that sum; the later ones
    are 1.  kind: 'all' (rows NULL) or 'list' (a shuffled list: every row when R > 400, so that the multi-pass
    size stays multi-pass, else four fifths of them with the count on the device).
    -> namespace: rays_a (R, 3) i64, deltas (n_samples) f32, n_samples, rows (the list or None), count,
    and what fp64 says the kernel must give: rest (R; -9 = not written), total2, evaluated (first chunks),
    list2 (sorted), first (the first-chunk samples of the processed rows), lnT (R)."""
    rng = np.random.default_rng(977 * seed + R)
    r = np.arange(R)
    N = np.asarray(ROUND1_N)[r % 9]
    gap = r % 3
    start = np.cumsum(N + gap) - N
    n_samples = int((N + gap).sum()) + 5
    clear = ((r // 9) + (r % 9)) % 2 == 0
    deltas = np.ones(n_samples, dtype=np.float32)
    lnT = np.zeros(R)
    for i in range(R):
        cnt = min(int(N[i]), 64)
        if cnt:
            u = rng.uniform(0.5, 1.5, cnt)
            d = ((2.0 if clear[i] else 30.0) * u / (sigma * u.sum())).astype(np.float32)
            deltas[start[i]:start[i] + cnt] = d
            lnT[i] = -sigma * d.astype(np.float64).sum()
    rows, count = None, R
    if kind == "list":
        rows = np.random.default_rng(13 * seed + R).permutation(R).astype(np.int32)
        count = R if R > 400 else max(1, R - R // 5)
    done = r if rows is None else rows[:count].astype(np.int64)
    # the condition the expected outputs rest on: a factor 2 from T_thr on the log scale, for every row with samples
    ratio = lnT[N > 0] / np.log(T_THR)
    assert ((ratio <= 0.5) | (ratio >= 2.0)).all()
    goes_on = (N > 64) & (lnT > np.log(T_THR))
    rest = np.full(R, -9, dtype=np.int64)
    rest[done] = np.where(goes_on[done], N[done] - 64, 0)
    first = np.concatenate([np.arange(start[i], start[i] + min(int(N[i]), 64)) for i in done] + [np.zeros(0, np.int64)])
    list2 = np.concatenate([np.arange(start[i] + 64, start[i] + N[i]) for i in done if goes_on[i]]
                           + [np.zeros(0, np.int64)])
    rays_a = np.stack([r, start, N], 1).astype(np.int64)
    return SimpleNamespace(R=R, N=N, start=start, rays_a=rays_a, deltas=deltas, n_samples=n_samples, rows=rows,
                           count=count, done=done, rest=rest, total2=int(list2.size), evaluated=int(first.size),
                           list2=np.sort(list2), first=first.astype(np.int64), lnT=lnT, goes_on=goes_on)
