"""fp64 references, rounding bounds and input sets for the hash-table backward
(ngp_hash_backward*, hashbin.hip) and the FusedAdam folded into its
accumulation.  A plain helper module (not a conftest): test_hashbin_ref_cpu.py
shows on the CPU that the references and bounds are sound,
test_hashbin_gpu.py holds the kernels to them.

Scatter
-------
dL/dtable[e][f] = sum over (sample, corner) of w_c * dL/denc[2l + f].
``scatter_ref64`` forms that sum in fp64 from the oracle's corner indices and
fp32 corner weights (oracle.hash_corners), with mag = sum |w g| and cnt = the
number of terms per entry.  u = 2^-24 (fp32 unit roundoff).

* fp32 summation of cnt terms in any order (per-sample atomics, the oracle's C
  loop): |err| <= (cnt + 16) u mag -- (cnt - 1) u mag for the sum, the
  remaining 17 u for the terms themselves (below).
* binned levels: |err| <= 10 u mag, independent of cnt.  The oracle's weight
  is fl(fl(Wx Wy) Wz) and the kernel's term fl(Wx fl(fl(Wy Wz) g)), where the
  W are the SAME fp32 numbers on both sides (pos or fl(1 - pos), from the same
  fmaf / floorf): 2 + 3 product roundings apart, 5 u.  A merged run's register
  sum is at most 4 fp32 additions deep (4 u); the sums are then formed in fp64
  (36 000 terms x 2^-53: nothing) and the fp64 LDS image is cast to fp32 once
  (1 u of |sum| <= mag).  5 + 4 + 1 = 10, below the 16 the terms are allowed;
  one lost or doubled term among thousands moves an entry by far more.
* an entry that also receives n32 fp32 terms through memory-side atomics
  (the x+1 corner of a pair split by a bucket boundary: one per such pair plus
  the bucket's flushed image; every entry of a bucket of several chunks: one
  per chunk): (n32 + 10) u mag.
* onto a non-zero base (+= contract): the sole read-add-store of an owned
  range rounds once, u |base + ref|; each further fp32 add into memory rounds
  a partial sum of magnitude <= |base| + mag, so k adds cost
  u |base + ref| + (k - 1) u (|base| + mag).  (The per-atomic rounding at the
  base's magnitude is the term a bound of u |base + ref| alone misses.)
* every bound is scaled by 1 + 2^-20 (second-order terms) and gains
  (cnt + 1) 2^-126 (a term or partial sum that underflows).
* mag == 0: nothing may be added -- the entry keeps its bits.

Adam
----
adam_elem (common.h): m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g;
p -= lr (m / bc1) / (sqrt(v / bc2) + eps), all fp32; adam_bias: bc = 1 -
powf(b, step_dev + 1) with the fp32 betas.  ``adam_ref64`` evaluates the same
formula in fp64 with the bias corrections formed that way, and bounds, with
the gradient known to dg:
  dm   = 3u (|b1 m0| + |(1-b1) g|) + (1-b1) dg
  dv   = 4u (b2 v0 + (1-b2) g^2) + 2 (1-b2) |g| dg
  dupd = lr / (bc1 den) dm + |upd| / den s (dv / 2v + 2u / bc2 + 2u)
         + |upd| (4u / bc1 + 4u),   s = sqrt(v / bc2), den = s + eps
  dp   = u (|p| + |upd|) + dupd
(one rounding per operation; the u / bc terms are one ulp of powf; the final
subtraction rounds at the new p's magnitude <= |p| + |upd|).  The state is
chosen so that dupd <= 0.1 |upd| wherever the update is not itself a
cancellation (|m| >= 1e-2 (|b1 m0| + |(1-b1) g|)): a skipped, doubled or
unscaled update fails there.
"""
import functools
import types

import torch

import oracle as O

U = 2.0 ** -24
TINY = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -20
BSHIFT, BENT, CH, TILE = 13, 1 << 13, 32768, 256  # hashbin.hip's bucket / chunk / tile sizes
C_TERM = 16   # fp32-summed paths: (cnt + 16) u mag
C_BIN = 10    # binned levels (derivation above)
N_LEVELS = 16


def box(scale):
    return -scale * torch.ones(3), scale * torch.ones(3)


@functools.lru_cache(maxsize=None)
def spec(scale):
    return O.HashGridSpec(scale=scale)


# ------------------------------------------------------------------ scatter
def scatter_ref64(sp, x, xyz_min, xyz_max, denc, levels=None):
    """-> (ref, mag, cnt), 2 * n_entries each: the fp64 table gradient of the
    samples x (m, 3) with dL/denc (m, 32), sum |w g|, and terms per entry."""
    idx, w = O.hash_corners(sp, x, xyz_min, xyz_max)
    n2 = 2 * sp.n_entries
    ref = torch.zeros(n2, dtype=torch.float64)
    mag = torch.zeros(n2, dtype=torch.float64)
    cnt = torch.zeros(n2, dtype=torch.float64)
    if x.shape[0] == 0:
        return ref, mag, cnt
    d = denc.double()
    one = torch.ones(x.shape[0] * 8, dtype=torch.float64)
    for l in (range(sp.L) if levels is None else levels):
        e = idx[:, l, :].long()
        wl = w[:, l, :].double()
        for f in range(2):
            k = (2 * e + f).reshape(-1)
            t = (wl * d[:, 2 * l + f, None]).reshape(-1)
            ref.index_add_(0, k, t)
            mag.index_add_(0, k, t.abs())
            cnt.index_add_(0, k, one)
    return ref, mag, cnt


def bucket_info(sp, x, xyz_min, xyz_max, level_lo=0, merge_hi=0):
    """What the binned path does with the samples x (in the order the kernel
    sees them), from the oracle's corner indices:
      recs   (L, 64)  records per (level, bucket): bucket = local entry >> 13,
                      a pair record keyed by its first (x) corner; on a merged
                      level (l < merge_hi) the run decisions of a wave -- 16
                      consecutive samples, equal (x, x+1) pairs per y/z corner:
                      a run of >= 2 puts one record into each corner's bucket
      nch    (L, 64)  chunks of <= 32768 records
      pairs  (m, L)   the sample has an x pair whose corners lie in different
                      buckets (any y/z corner)
      nstr   (2E,)    direct fp32 adds per element: the x+1 corner of a split
                      pair that is written as a pair record
      n32    (2E,)    fp32 terms added through memory per element: nstr + the
                      bucket's chunk images when there are several or nstr > 0
      touched (L, 64) the bucket receives a record or a direct add
    """
    L = sp.L
    m = x.shape[0]
    n2 = 2 * sp.n_entries
    recs = torch.zeros(L, 64, dtype=torch.int64)
    touched = torch.zeros(L, 64, dtype=torch.bool)
    pairs = torch.zeros(m, L, dtype=torch.bool)
    nstr = torch.zeros(n2, dtype=torch.int64)
    n32 = torch.zeros(n2, dtype=torch.int64)
    if m:
        idx, _ = O.hash_corners(sp, x, xyz_min, xyz_max)
        j = torch.arange(m)
        for l in range(L):
            off = int(sp.offsets[l])
            loc = idx[:, l, :].long() - off
            e0, e1 = loc[:, 0::2], loc[:, 1::2]          # (m, 4): pairs (0,1) (2,3) (4,5) (6,7)
            b0, b1 = e0 >> BSHIFT, e1 >> BSHIFT
            pairs[:, l] = (b0 != b1).any(1)
            if l < level_lo:
                continue
            head = torch.ones(m, 4, dtype=torch.bool)
            longrun = torch.zeros(m, 4, dtype=torch.bool)
            if l < merge_hi and m > 1:
                same = torch.zeros(m, 4, dtype=torch.bool)
                same[1:] = (e0[1:] == e0[:-1]) & (e1[1:] == e1[:-1]) & ((j[1:] % 16) != 0)[:, None]
                head = ~same
                longrun[:-1] = head[:-1] & same[1:]
            recs[l] += torch.bincount(b0[head], minlength=64)
            recs[l] += torch.bincount(b1[longrun], minlength=64)
            split = head & ~longrun & (b0 != b1)
            es = 2 * (e1[split] + off)
            one = torch.ones_like(es)
            nstr.index_add_(0, es, one)
            nstr.index_add_(0, es + 1, one)
            touched[l] = recs[l] > 0
            touched[l, b1[split].unique()] = True
    nch = (recs + CH - 1) // CH
    for l in range(level_lo, L):
        a, b = int(sp.offsets[l]), int(sp.offsets[l + 1])
        ent = torch.arange(b - a)
        c = nch[l][ent >> BSHIFT].repeat_interleave(2)
        s = nstr[2 * a:2 * b]
        n32[2 * a:2 * b] = s + c * ((c > 1) | (s > 0))
    return types.SimpleNamespace(recs=recs, nch=nch, pairs=pairs, nstr=nstr, n32=n32, touched=touched)


def scatter_bound(sp, ref, mag, cnt, n32=None, level_lo=N_LEVELS, base=None):
    """Per-element bound of |out - (base + ref)| (module docstring).  Levels
    below level_lo sum their cnt terms in fp32; the levels from level_lo on are
    binned, with n32 terms through memory (n32 None: every level fp32-summed,
    the atomic kernel or a spilled workspace)."""
    split = 2 * int(sp.offsets[level_lo]) if n32 is not None else ref.numel()
    const = cnt + C_TERM
    adds = cnt.clamp(min=1.0)
    if n32 is not None:
        const = const.clone()
        adds = adds.clone()
        const[split:] = n32[split:].to(ref.dtype) + C_BIN
        adds[split:] = n32[split:].to(ref.dtype).clamp(min=1.0)
    b = const * U * mag * SLACK + (cnt + 1) * TINY
    if base is not None:
        bd = base.to(ref.dtype)
        b = b + (U * (bd + ref).abs() + (adds - 1) * U * (bd.abs() + mag)) * SLACK
    return b


def level_ratios(sp, err, bound):
    """worst err / bound per level (0 where nothing is expected to move)"""
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")),
                                                       torch.zeros_like(err)))
    return [float(r[2 * int(sp.offsets[l]):2 * int(sp.offsets[l + 1])].max()) for l in range(sp.L)]


# --------------------------------------------------------------------- Adam
def adam_bias32(b1, b2, step):
    """adam_bias: fp32 betas, 1 - powf(b, step) in fp32 (step = step_dev + 1)"""
    st = torch.tensor(float(step), dtype=torch.float32)
    b1f, b2f = torch.tensor(b1, dtype=torch.float32), torch.tensor(b2, dtype=torch.float32)
    bc1 = torch.tensor(1.0, dtype=torch.float32) - torch.pow(b1f, st)
    bc2 = torch.tensor(1.0, dtype=torch.float32) - torch.pow(b2f, st)
    return float(b1f), float(b2f), float(bc1), float(bc2)


def adam_ref64(p, m, v, g, lr, step, b1=0.9, b2=0.999, eps=1e-15, grad_scale=1.0, dg=None):
    """Adam in fp64 from the fp32 state (p, m, v), the fp64 gradient g (before
    grad_scale, known to within dg) -> namespace(p, m, v, dp, dm, dv, upd,
    dupd, cancel): new values, their bounds, the update and its bound, and
    where the new m is a cancellation of its two terms.  Runs on g's device."""
    b1f, b2f, bc1, bc2 = adam_bias32(b1, b2, step)
    lr = float(torch.tensor(lr, dtype=torch.float32))
    eps = float(torch.tensor(eps, dtype=torch.float32))
    gs = float(torch.tensor(grad_scale, dtype=torch.float32))
    p0, m0, v0 = p.double(), m.double(), v.double()
    g = g.double() * gs
    dg = (torch.zeros_like(g) if dg is None else dg.double() * gs) + U * g.abs()  # the fp32 product g x grad_scale
    a, b = b1f * m0, (1 - b1f) * g
    mn = a + b
    dm = 3 * U * (a.abs() + b.abs()) + (1 - b1f) * dg
    vn = b2f * v0 + (1 - b2f) * g * g
    dv = 4 * U * vn + 2 * (1 - b2f) * g.abs() * dg
    s = torch.sqrt(vn / bc2)
    den = s + eps
    upd = lr * (mn / bc1) / den
    rel_s = torch.where(vn > 0, dv / (2 * vn).clamp(min=TINY), torch.zeros_like(vn)) + 2 * U / bc2 + 2 * U
    dupd = lr / (bc1 * den) * dm + upd.abs() / den * s * rel_s + upd.abs() * (4 * U / bc1 + 4 * U)
    pn = p0 - upd
    dp = U * (p0.abs() + upd.abs()) + dupd
    cancel = mn.abs() < 1e-2 * (a.abs() + b.abs())
    return types.SimpleNamespace(p=pn, m=mn, v=vn, dp=dp * SLACK, dm=dm * SLACK + TINY, dv=dv * SLACK + TINY,
                                 upd=upd, dupd=dupd, cancel=cancel, b1f=b1f, b2f=b2f, bc1=bc1, bc2=bc2)


def adam_state(n, seed, device="cpu"):
    """The state the Adam checks start from: p U(-1,1) x {1e-4, 1}, m N(0, 1e-3),
    v U(1e-8, 1e-4) -- non-zero moments, so that an entry without gradient
    still moves."""
    g = torch.Generator(device=device).manual_seed(seed)
    f = dict(generator=g, device=device)
    p = (torch.rand(n, **f) * 2 - 1) * torch.where(torch.rand(n, **f) < 0.5, 1e-4, 1.0)
    m = torch.randn(n, **f) * 1e-3
    v = torch.rand(n, **f) * (1e-4 - 1e-8) + 1e-8
    return p.float(), m.float(), v.float()


# --------------------------------------------------------------- input sets
def _uniform_points(n, scale, g):
    """n points uniform in the box; the first 8 are its corners, the next 12
    have one coordinate exactly +-scale"""
    x = (torch.rand(n, 3, generator=g) * 2 - 1) * scale
    x[:8] = torch.tensor([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * scale
    for k in range(12):
        x[8 + k, k % 3] = scale if k % 2 else -scale
    return x


def ray_points(n_rays, per_ray, scale, seed):
    """samples along rays, consecutive per ray (a march's layout): runs of
    equal corner pairs on the coarse levels (test_field_gpu._ray_points)"""
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(n_rays, 3, generator=g) * 2 - 1) * scale * 0.9
    d = torch.randn(n_rays, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    t = torch.arange(per_ray).float() * (3 ** 0.5 / 1024) * scale * 2
    return (o[:, None] + t[None, :, None] * d[:, None]).clamp(-scale, scale).reshape(-1, 3).contiguous()


def hashed_levels(sp):
    return [l for l in range(sp.L) if int(sp.res[l]) ** 3 > int(sp.sizes[l])]


@functools.lru_cache(maxsize=None)
def input_set(name, scale):
    """-> namespace(name, scale, x (n, 3): the xyzs buffer, sidx (n,) int32 or
    None, m: the device count, denc (n, 32), xc (m, 3) / dc (m, 32): the
    samples and dL/denc rows the kernels are to scatter, in order).  Each
    set's precondition is asserted here, from the oracle's corner indices."""
    sp = spec(scale)
    mn, mx = box(scale)
    g = torch.Generator().manual_seed({"scattered": 21, "rays": 22, "pile": 23, "sparse": 24, "straddle": 25,
                                       "none": 26}[name] + int(scale))
    sidx = None
    if name == "scattered":
        x = _uniform_points(6007, scale, g)
        n = x.shape[0]
        sub = torch.randperm(n, generator=g)[: n * 3 // 4].sort().values.to(torch.int32)
        m = sub.numel()
        sidx = torch.zeros(n, dtype=torch.int32)
        sidx[:m] = sub
        denc = torch.full((n, 32), float("nan"))
        denc[:m] = torch.randn(m, 32, generator=g) * 1e-2
        assert m < n and m % TILE != 0 and m % 64 != 0 and m % 16 != 0  # partial last tile and wave
        assert bool((sub[1:] > sub[:-1]).all()) and int(sub.max()) > m   # a real subset, sorted
    elif name == "rays":
        x = ray_points(96, 50, scale, seed=31)
        m = x.shape[0]
        denc = torch.randn(m, 32, generator=g) * 1e-2
        info = bucket_info(sp, x, mn, mx, 0, 16)
        unmerged = bucket_info(sp, x, mn, mx, 0, 0)
        hl = hashed_levels(sp)
        # runs exist (records are saved by merging), on a hashed level too
        assert int(info.recs[:8].sum()) < int(unmerged.recs[:8].sum()) * 3 // 4
        assert any(int(info.recs[l].sum()) < int(unmerged.recs[l].sum()) for l in hl)
    elif name == "pile":
        head = _uniform_points(4007, scale, g)
        one = torch.tensor([[0.2371, -0.3113, 0.1279]]) * (scale / 0.5)
        x = torch.cat([head, one.expand(36000, 3)]).contiguous()
        m = x.shape[0]
        decade = 10.0 ** (-torch.randint(0, 7, (m, 1), generator=g).float())
        denc = torch.randn(m, 32, generator=g) * 1e-2 * decade
        info = bucket_info(sp, x, mn, mx, 0, 0)
        assert bool((info.recs.max(1).values > CH).all()), info.recs.max(1).values  # a multi-chunk bucket per level
        for l in hashed_levels(sp):  # the pile's four y/z records: 4 distinct buckets of 36 000 each
            assert int((info.recs[l] >= 36000).sum()) == 4, (l, info.recs[l])
        merged = bucket_info(sp, x, mn, mx, 0, 16)
        # whole-wave runs: two records per 16 copies, a single chunk again on the hashed levels
        assert int(merged.nch[hashed_levels(sp)].max()) == 1
    elif name == "sparse":
        x = _uniform_points(28, scale, g)[20:].contiguous()  # 8 interior points
        m = x.shape[0]
        denc = torch.randn(m, 32, generator=g) * 1e-2
        info = bucket_info(sp, x, mn, mx, 0, 0)
        for l in hashed_levels(sp):
            assert int((~info.touched[l]).sum()) >= 30, (l, int(info.touched[l].sum()))
    elif name == "straddle":
        cand = (torch.rand(400000, 3, generator=g) * 2 - 1) * scale
        pairs = bucket_info(sp, cand, mn, mx, sp.L, 0).pairs  # (level_lo = L: the split pairs only)
        keep = pairs.any(1)
        pad = _uniform_points(100, scale, g)
        x = torch.cat([cand[keep], pad])
        x = x[torch.randperm(x.shape[0], generator=g)].contiguous()
        m = x.shape[0]
        denc = torch.randn(m, 32, generator=g) * 1e-2
        per_level = pairs[keep].sum(0)
        hl = hashed_levels(sp)
        if scale == 0.5:
            assert all(int(per_level[l]) >= 100 for l in range(1, 6)), per_level
        else:
            assert all(int(per_level[l]) >= 100 for l in range(1, 4)), per_level
            assert all(l in hl and int(per_level[l]) >= 20 for l in (13, 14, 15)), per_level
        assert m <= 40000
    elif name == "none":
        x = _uniform_points(300, scale, g)
        m = 0
        denc = torch.full((300, 32), float("nan"))
    else:
        raise KeyError(name)
    x = x.contiguous()
    xc = (x[sidx[:m].long()] if sidx is not None else x[:m]).contiguous()
    dc = denc[:m].contiguous()
    assert bool(torch.isfinite(dc).all())
    return types.SimpleNamespace(name=name, scale=scale, x=x, sidx=sidx, m=m, denc=denc.contiguous(), xc=xc, dc=dc)


@functools.lru_cache(maxsize=None)
def reference(name, scale):
    """scatter_ref64 of an input set (computed once per process; read-only)"""
    s = input_set(name, scale)
    mn, mx = box(scale)
    return scatter_ref64(spec(scale), s.xc, mn, mx, s.dc)


@functools.lru_cache(maxsize=None)
def info(name, scale, level_lo, merge_hi):
    s = input_set(name, scale)
    mn, mx = box(scale)
    return bucket_info(spec(scale), s.xc, mn, mx, level_lo, merge_hi)
