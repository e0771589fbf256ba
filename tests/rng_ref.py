"""Host model of every random draw of the device (numpy only): Philox-4x32-10
written from its definition (Salmon, Moraes, Dror, Shaw: "Parallel random
numbers: as easy as 1, 2, 3", SC'11, section 3.3 / Random123 philox.h), and
one function per consumer that restates the consumer's (key, counter) layout.
The draws are pure functions of (key, counter), so the device has to equal
this model bit for bit (tests/test_rng_gpu.py).

Stream map.  key = (low, high 32 bits of a 64-bit seed); counter words 0..3:

  consumer                      key             w0     w1     w2        w3
  batch (sample_batch_kernel)   sample_seed     q lo   q hi   step lo   step hi
      q = ray_offset + ray, step = the batch counter (+ add);
      x -> image, y -> pixel, z -> march noise (w unused)
  background (random_bg_kernel) sample_seed     0x62   0x67   c lo      c hi
                                 ^ 0x6267
      c = the batch counter (+ add); x, y, z -> r, g, b
  jitter (occ_sample_kernel,    occ_seed        i lo   i hi   ctr lo    cascade
      occ_sample_sorted_kernel)
      i = the sample's position in the 2M list; x, y, z -> jitter;
      unsorted, i >= M: w -> the pick from the occupied list
  uniform cell (occ_sample_     occ_seed        i lo   i hi   ctr lo    0x9E3779B9 ^ cascade
      kernel, i < M)
      x, y, z -> cell coordinates
  exponentials (occ_exp)        occ_seed        k lo   k hi   ctr lo    0x7F4A7C15 ^ cascade << 1 ^ half
      k = 0..M, half 0 = uniform cells, 1 = occupied list; x, y -> a 42-bit uniform

Why no two consumers of one trainer share a (key, counter): the three keys of
a trainer differ pairwise (trainer.rng_keys: base, base ^ 0x6267, base ^
0x5DEECE66D), which separates batch, background and the occupancy draws.  The
three occupancy consumers share occ_seed and are separated by word 3: with
cascade in 0..7 it lies in [0, 8) for the jitter, in 0x9E3779B8..0x9E3779BF for
the uniform cell and in 0x7F4A7C10..0x7F4A7C1F for the exponentials (cascade
<< 1 ^ half in 0..15, injective in (cascade, half)).  Within one consumer the
counter is injective in its arguments (ctr below 2^32).  stream_domains /
domains_disjoint check this mechanically (tests/test_rng_ref_cpu.py).

The sorted draw (occupancy_samples_sorted).  U_(k) = S_{k+1} / S_{M+1}, S_j
the sum of the first j of M + 1 exponentials formed in fp64 as occ_exp forms
them; the cell is floor(U_(k) * n).  The model takes the prefix sums and the
quotient EXACTLY (the fp64 exponentials as scaled Python integers), so its
own error in U_(k) * n is zero given the exponentials; frac_dist is the
distance of U_(k) * n from the nearest integer.  The device sums in fp64: a
prefix passes through at most D additions,

  block sum (occ_exp_sums_kernel)    16 serial + 6 xor-shuffle + 2 (the four waves)   = 24
  scan of the block sums             6 (wave scan) + (nb - 1) // 64 (waves before)
    (occ_exp_scan_kernel)            + 2 (before + incl - v)                          = 8 + (nb - 1) // 64
  in the block                       16 serial (the thread's own sum) + 6 (wave scan)
    (occ_sample_sorted_kernel)       + 3 (waves before) + 2 (run += incl - loc)
                                     + 16 serial (run += e[j])                        = 43

  D = 75 + (nb - 1) // 64   (nb = ceil((M + 1) / 4096) blocks; nb <= 1024: one scan round)

each of relative error <= 2^-53 of a partial sum that never exceeds the
total; S_{M+1} passes through fewer.  With two ulps for the two logs (device
and host libm may differ in the last place of an exponential, which moves a
sum by at most that much relatively), one for the reciprocal and one for the
products, device and model differ in U_(k) * n by less than

  tau = (D + 4) * 2^-52 * n        (sorted_tau)

so a sample whose frac_dist is >= 64 tau falls into the same cell on both.
"""
from itertools import accumulate

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)  # multipliers (philox.h PHILOX_M4x32_0/1)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)  # Weyl key increments (golden ratio, sqrt 3 - 1)

BG_KEY_XOR = 0x6267
TAG_UNIFORM, TAG_EXP = 0x9E3779B9, 0x7F4A7C15
OSC_CH = 4096  # exponentials per block of the sorted sampler


def _u64(x):
    return np.asarray(x, dtype=np.uint64) & M32


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox-4x32-R: R rounds of  (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0,
    lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  the key bumped by the Weyl
    constants between rounds.  Arrays of uint64 holding 32-bit words."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(a) for a in (c0, c1, c2, c3, k0, k1)))
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2  # 32 x 32 -> 64 bits
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32)
    return c0, c1, c2, c3


def uniform_index(u, n):
    """(u * n) >> 32: an index in [0, n) from a 32-bit word (n <= 2^32)"""
    return ((_u64(u) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def unit24(u):
    """float32(u >> 8) * 2^-24: in [0, 1), exact"""
    return (_u64(u) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _split(x):
    """low, high words of 64-bit values (Python ints or arrays; negative ones as two's complement)"""
    if isinstance(x, (int, np.integer)):
        x = int(x) & 0xFFFFFFFFFFFFFFFF
        return np.uint64(x & 0xFFFFFFFF), np.uint64(x >> 32)
    x = np.asarray(x).astype(np.uint64)
    return x & M32, x >> np.uint64(32)


def sample_batch(seed, step, ray_offset, n_rays, n_img, hw):
    """-> img (n_rays) i64, pix i64, noise f32 of ngp_sample_batch(seed, step, ray_offset, ...)"""
    q = np.array([(ray_offset + r) & 0xFFFFFFFFFFFFFFFF for r in range(n_rays)], dtype=np.uint64)
    k0, k1 = _split(seed)
    s0, s1 = _split(step)
    x, y, z, _ = philox4x32(q & M32, q >> np.uint64(32), s0, s1, k0, k1)
    return uniform_index(x, n_img), uniform_index(y, hw), unit24(z)


def random_bg(seed, counter):
    """-> (3) f32 of ngp_random_bg(seed, counter_dev, add) at counter = *counter_dev + add"""
    k0, k1 = _split(seed)
    c0, c1 = _split(counter)
    x, y, z, _ = philox4x32(0x62, 0x67, c0, c1, k0, k1)
    return np.array([unit24(x), unit24(y), unit24(z)], dtype=np.float32).reshape(3)


def _spread3(v):
    v = np.asarray(v, dtype=np.uint64)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton3(x, y, z):
    """bit b of x at bit 3b, of y at 3b + 1, of z at 3b + 2 (10 bits per axis)"""
    return _spread3(x) | (_spread3(y) << np.uint64(1)) | (_spread3(z) << np.uint64(2))


def compact3(m):
    m = np.asarray(m, dtype=np.uint64)
    out = np.zeros_like(m)
    for b in range(11):
        out |= ((m >> np.uint64(3 * b)) & np.uint64(1)) << np.uint64(b)
    return out


def _xyz(idx, jit, G, s_minus_hgs, hgs):
    """(coords / (G - 1) * 2 - 1) * (s - hgs) + (U * 2 - 1) * hgs, one fp32 rounding per operation
    (the library is built without FP contraction)"""
    f = np.float32
    idx = np.asarray(idx).astype(np.int64).astype(np.uint64) & M32  # (uint32_t)idx
    cc = np.stack([compact3(idx), compact3(idx >> np.uint64(1)), compact3(idx >> np.uint64(2))], -1).astype(np.float32)
    a = cc / f(G - 1)
    a = a * f(2.0)
    a = a - f(1.0)
    a = a * f(s_minus_hgs)
    b = jit * f(2.0)
    b = b - f(1.0)
    b = b * f(hgs)
    return (a + b).astype(np.float32)


def _jitter(seed, ctr, cascade, i):
    k0, k1 = _split(seed)
    i0, i1 = _split(i)
    x, y, z, w = philox4x32(i0, i1, _split(ctr)[0], cascade, k0, k1)
    return np.stack([unit24(x), unit24(y), unit24(z)], -1), w


def _count(occ_list, count, G):
    return min(len(occ_list) if count is None else int(count), G ** 3)


def occupancy_samples(seed, ctr, cascade, G, M, s_minus_hgs, hgs, occ_list, lo, hi, count=None):
    """-> flat (hi - lo) i64, xyz (hi - lo, 3) f32 of ngp_occupancy_samples; count: *occ_count
    (default: the whole list), clamped to G^3 as the kernel clamps it."""
    occ_list = np.asarray(occ_list, dtype=np.int64)
    cnt = _count(occ_list, count, G)
    i = np.arange(lo, hi, dtype=np.int64)
    jit, w = _jitter(seed, ctr, cascade, i)
    k0, k1 = _split(seed)
    i0, i1 = _split(i)
    vx, vy, vz, _ = philox4x32(i0, i1, _split(ctr)[0], TAG_UNIFORM ^ cascade, k0, k1)
    idx = morton3(uniform_index(vx, G), uniform_index(vy, G), uniform_index(vz, G)).astype(np.int64)
    occ = i >= M
    if cnt > 0:
        idx[occ] = occ_list[uniform_index(w[occ], cnt)]
    xyz = _xyz(idx, jit, G, s_minus_hgs, hgs)
    flat = cascade * G ** 3 + idx
    if cnt == 0:
        flat[occ] = -1
        xyz[occ] = 0
    return flat, xyz


def occ_exponentials(seed, ctr, cascade, half, M):
    """the M + 1 Exp(1) variates of one half, fp64, as occ_exp forms them"""
    k0, k1 = _split(seed)
    k = np.arange(M + 1, dtype=np.int64)
    i0, i1 = _split(k)
    x, y, _, _ = philox4x32(i0, i1, _split(ctr)[0], TAG_EXP ^ (cascade << 1) ^ half, k0, k1)
    u = ((x >> np.uint64(11)).astype(np.float64) + 1.0) * (1.0 / 2097152.0)  # (0, 1], 21 bits
    u2 = u + (y >> np.uint64(11)).astype(np.float64) * (1.0 / 2097152.0 / 2097152.0)  # 42 bits, exact in fp64
    return -np.log(np.minimum(u2, 1.0))


_FIX = 160  # fixed-point scale 2^-160: every exponential (0 or >= 2^-43, 53-bit mantissa) is an integer in it


def _order_statistics(e, n):
    """floor(S_{k+1} n / S_{M+1}) and the distance of S_{k+1} n / S_{M+1} from the nearest
    integer, k < M, exactly: e (M + 1) fp64 -> Python integers"""
    m, ex = np.frexp(e)
    mant = (m * 2.0 ** 53).astype(np.int64)
    assert np.array_equal(mant.astype(np.float64) * 2.0 ** -53, m) and int(ex.min()) - 53 + _FIX >= 0
    ints = [int(a) << (int(b) - 53 + _FIX) for a, b in zip(mant.tolist(), ex.tolist())]
    pre = list(accumulate(ints))
    tot = pre[-1]
    cell, dist = [], []
    for s in pre[:-1]:
        q, r = divmod(s * n, tot)
        cell.append(q)
        dist.append(min(r, tot - r) / tot)
    return np.array(cell, dtype=np.int64), np.array(dist, dtype=np.float64)


def occupancy_samples_sorted(seed, ctr, cascade, G, M, s_minus_hgs, hgs, occ_list, lo, hi, count=None):
    """-> flat, xyz of ngp_occupancy_samples_sorted over [lo, hi), and frac_dist (hi - lo) f64
    (inf where no cell is drawn: the occupied half of an empty list)"""
    occ_list = np.asarray(occ_list, dtype=np.int64)
    cnt = _count(occ_list, count, G)
    n_cells = G ** 3
    idx = np.full(2 * M, -1, dtype=np.int64)
    dist = np.full(2 * M, np.inf)
    c, d = _order_statistics(occ_exponentials(seed, ctr, cascade, 0, M), n_cells)
    idx[:M], dist[:M] = np.minimum(c, n_cells - 1), d
    if cnt > 0:
        c, d = _order_statistics(occ_exponentials(seed, ctr, cascade, 1, M), cnt)
        idx[M:], dist[M:] = occ_list[np.minimum(c, cnt - 1)], d
    i = np.arange(lo, hi, dtype=np.int64)
    jit, _ = _jitter(seed, ctr, cascade, i)
    idx, dist = idx[lo:hi], dist[lo:hi]
    xyz = _xyz(np.maximum(idx, 0), jit, G, s_minus_hgs, hgs)
    flat = cascade * n_cells + idx
    if cnt == 0:
        flat[i >= M] = -1
        xyz[i >= M] = 0
    return flat, xyz, dist


def sorted_scan_depth(M):
    """D of the module docstring for a list of M samples per half"""
    nb = (M + 1 + OSC_CH - 1) // OSC_CH
    assert nb <= 1024  # (one round of occ_exp_scan_kernel; more needs M > 4.19 M)
    return 75 + (nb - 1) // 64


def sorted_tau(M, n):
    return (sorted_scan_depth(M) + 4) * 2.0 ** -52 * n


# ---- the sorted draw's test inputs (tests/test_rng_gpu.py draws them on the device;
# tests/test_rng_ref_cpu.py shows that none of their samples lies within 64 tau of a cell boundary)
SORTED_G, SORTED_LIST_N = 16, 1234
# (seed, ctr, cascade, M): M = 4095 / 4096 / 4097 put the (M + 1)-th exponential at the end of a
# block, alone in the next one, and there with one neighbour; M = 12293: four blocks
SORTED_CASES = [(99, 7, 0, 1), (99, 7, 0, 4095), (99, 7, 0, 4096), (99, 7, 0, 4097), (99, 7, 0, 12293),
                (0x1234567800000063, 7, 3, 4097)]


def sorted_occ_list(G=SORTED_G, n=SORTED_LIST_N):
    """n distinct cells of G^3 in ascending order (a fixed pseudo-random subset: the n smallest
    Philox words of the cells)"""
    x, _, _, _ = philox4x32(np.arange(G ** 3), 0, 0, 0, 0x0CC, 0)
    return np.sort(np.argsort(x, kind="stable")[:n]).astype(np.int32)


# ---- the stream map, mechanically
def stream_domains(sample_key, bg_key, occ_key, cascades=range(8)):
    """[(name, key, {counter word: set of the values it can take})] of every consumer; a word
    not listed takes any value"""
    out = [("batch", sample_key, {}), ("background", bg_key, {0: {0x62}, 1: {0x67}})]
    for c in cascades:
        out.append((f"jitter c{c}", occ_key, {3: {c}}))
        out.append((f"uniform cell c{c}", occ_key, {3: {TAG_UNIFORM ^ c}}))
        for half in (0, 1):
            out.append((f"exponentials c{c} half {half}", occ_key, {3: {TAG_EXP ^ (c << 1) ^ half}}))
    return out


def domains_disjoint(a, b):
    """no (key, counter) in both: the keys differ, or some counter word is pinned to disjoint sets"""
    (_, ka, wa), (_, kb, wb) = a, b
    return ka != kb or any(not (wa[w] & wb[w]) for w in set(wa) & set(wb))
