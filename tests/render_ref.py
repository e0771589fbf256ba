"""A plain CPU reference of the device-resident test-time render loop
(csrc/render.hip): one iteration and the whole loop, per ray.  A helper module
(not a conftest), like composite_ref.py: test_render_ref_cpu.py states what the
designed inputs contain, test_render_kernels_gpu.py holds the kernels to it.

No kernel logic lives here: no lattice, no sample lists, no waves.
  * the iteration rule is models/rendering.py:186-195;
  * the march of an alive ray is oracle.raymarching_test (the serial walk of
    raymarching.cu:335-404), rearranged into the kernels' contract: the sample s
    of the ray at alive-list position n sits in slot s * n_alive + n;
  * the composite of an alive ray is composite_ref.py's fp64 composite_test_fw
    reference with its bound, started from the ray's prior opacity / depth / rgb;
  * a host loop chains them with a caller-supplied field.

The kernels' launch constants are mirrored below (each with its source line)
only to DERIVE the sizes at which a launch takes another path; the tests take
every threshold from these functions, never as a literal.
"""
import functools
import math
import types

import numpy as np
import torch

import composite_ref as CR
import oracle as O
from capi import C

# ------------------------------------------------- mirrored kernel constants
STATE_WORDS = C["NGP_RENDER_STATE_WORDS"]
RS_ALIVE0, RS_ALIVE1, RS_SAMPLES, RS_NS, RS_ACTIVE, RS_VALID, RS_TOTAL, RS_ITERS = range(8)  # march.h:535-536
NS_MAX = 64                # render.hip:58   N_samples = min(N_rays // N_alive, 64)
BLOCK = 256                # render.hip:224  __launch_bounds__(256) of every loop kernel
WAVE_RAYS = 4              # render.hip:170  rays per block per trip of the wave-per-ray mode (one per wave)
CRPT = 4                   # render.hip:90   rays per thread per composite pass
WAVE_NS = 16               # render.hip:136  N_samples from which a SIMPLE march runs wave-per-ray
STAGE = 2048               # render.hip:137  staged sample indices per block
FLUSH_SLACK = 4 * 64       # render.hip:218  flush when nst > STAGE - 4 * 64
MARCH_BLOCKS = 2048        # render.hip:372  grid cap of the march
COMPOSITE_BLOCKS = 1024    # render.hip:429  grid cap of the composite
LSEG = 32                  # march.h:286    lattice segments per ray
NEAR = 0.01                # models/rendering.py NEAR_DISTANCE


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------- derived thresholds
def march_grid(n_rays):
    return min(_cdiv(n_rays, BLOCK), MARCH_BLOCKS)


def composite_grid(n_rays):
    return min(_cdiv(n_rays, BLOCK * CRPT), COMPOSITE_BLOCKS)


def flush_trips(Ns):
    """trips of a block, every ray emitting Ns samples, after which its stage exceeds the flush level"""
    return (STAGE - FLUSH_SLACK) // (WAVE_RAYS * Ns) + 1


def flush_n_alive(Ns):
    """the smallest n_alive at which block 0 of the capped march grid reaches the mid-loop flush"""
    return (flush_trips(Ns) - 1) * MARCH_BLOCKS * WAVE_RAYS + 1


def lane_second_trip_n_alive():
    """the smallest n_alive at which the lane-per-ray march takes a second grid-stride trip"""
    return MARCH_BLOCKS * BLOCK + 1


def composite_rpt(n_alive, n_rays):
    return CRPT if n_alive > composite_grid(n_rays) * BLOCK else 1


def composite_second_pass_n_alive():
    """the smallest n_alive at which the capped composite grid takes a second pass"""
    return CRPT * COMPOSITE_BLOCKS * BLOCK + 1


def staged_peak(n_eff, n_rays):
    """per block of the wave-mode launch: the most sample indices it has staged when it tests the flush level,
    up to its first flush (running sums over its trips; the first crossing is the same with or without flushes)"""
    return staged_running(n_eff, n_rays).max(0).values


def staged_running(n_eff, n_rays):
    """(trips, blocks): the samples a block of the wave-mode launch has taken after each of its trips"""
    grid = march_grid(n_rays)
    n = n_eff.numel()
    trips = _cdiv(n, grid * WAVE_RAYS)
    pad = torch.zeros(trips * grid * WAVE_RAYS, dtype=torch.int64)
    pad[:n] = n_eff.long()
    return pad.view(trips, grid, WAVE_RAYS).sum(2).cumsum(0)


# ------------------------------------------------------------ iteration rule
def iteration_rule(n_rays, n_alive, samples, budget, min_samples):
    """rendering.py:186-195 -> N_samples, or None when the loop stops"""
    if n_alive == 0 or samples >= budget:
        return None
    return max(min(n_rays // n_alive, NS_MAX), min_samples)


# --------------------------------------------------------------------- march
@functools.lru_cache(maxsize=None)
def bitfield(kind, cascades=1, grid=128, seed=7):
    """dense | rand<frac> | blocks (1 % of the Morton-aligned 4^3 blocks) | centre (one cell)"""
    n = cascades * grid ** 3
    g = torch.Generator().manual_seed(seed)
    if kind == "dense":
        return torch.full((n // 8,), 255, dtype=torch.uint8)
    if kind == "blocks":
        return (torch.rand(n // 64, generator=g) < 0.01).repeat_interleave(8).to(torch.uint8) * 255
    if kind == "centre":
        bf = torch.zeros(n // 8, dtype=torch.uint8)
        c = int(O.morton3D(torch.tensor([[grid // 2] * 3], dtype=torch.int32))[0])
        bf[c // 8] = 1 << (c % 8)
        return bf
    bits = (torch.rand(n, generator=g) < float(kind[4:])).to(torch.uint8)
    return (bits.view(-1, 8) << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8)


def box_rays(n, seed, scale=0.5, inside=False):
    """n unit-direction rays through a point of the inner half of the box [-scale, scale]^3, from outside it (or from
    a point of the inner half: t1 < 0 < t2) -> o, d, hits_t (n, 2) near-clamped as the product's callers do"""
    g = torch.Generator().manual_seed(seed)
    tgt = (torch.rand(n, 3, generator=g) - 0.5) * scale
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    o = (torch.rand(n, 3, generator=g) - 0.5) * scale if inside else tgt - d * (3 * scale + torch.rand(n, 1, generator=g))
    o, d = o.contiguous(), d.contiguous()
    ht = box_hits(o, d, scale)
    if inside:
        ht[:, 0] = NEAR
    return o, d, ht


def box_hits(o, d, scale):
    _, ht, _ = O.ray_aabb_intersect(o, d, torch.zeros(1, 3), torch.ones(1, 3) * scale, 1)
    ht = ht[:, 0].clone()
    ht[(ht[:, 0] >= 0) & (ht[:, 0] < NEAR), 0] = NEAR
    return ht.contiguous()


def shuffled_alive(n_alive, n_buf, seed):
    """a shuffled subset of the ray ids 0..n_buf-1 (ray id != list position)"""
    g = torch.Generator().manual_seed(seed)
    al = torch.randperm(n_buf, generator=g)[:n_alive].to(torch.int32).contiguous()
    assert n_alive < 2 or not torch.equal(al.long(), torch.arange(n_alive))
    return al


def march_ref(o, d, ht, alive, bf, cascades, scale, esf, grid, max_samples, Ns, skip=()):
    """One march of the alive rays: the oracle's serial walk per ray, in the kernels' slots.  ht is NOT modified.
    skip: alive-list positions of rays the oracle cannot walk (t + dt == t: its loop never ends); the kernels end
    such a ray with no sample.  -> namespace: n_eff (n_alive) i32, hits_t (updated copy), valid (Ns * n_alive) bool,
    xyzs / dirs (Ns * n_alive, 3), deltas / ts (Ns * n_alive): the value of every valid slot (others: 0)."""
    n = alive.numel()
    keep = torch.ones(n, dtype=torch.bool)
    keep[list(skip)] = False
    ht2 = ht.clone().contiguous()
    out = O.raymarching_test(o, d, ht2, alive[keep].long(), bf, cascades, scale, esf, grid, max_samples, Ns)
    full = []
    for a in out:
        z = torch.zeros((n,) + tuple(a.shape[1:]), dtype=a.dtype)
        z[keep] = a
        full.append(z)
    xyzs, dirs, deltas, ts, n_eff = full
    valid = (torch.arange(Ns)[:, None] < n_eff[None, :].long()).reshape(-1)
    sm = lambda a: a.transpose(0, 1).reshape((Ns * n,) + tuple(a.shape[2:])).contiguous()  # noqa: E731
    return types.SimpleNamespace(n_eff=n_eff, hits_t=ht2, valid=valid, xyzs=sm(xyzs), dirs=sm(dirs), deltas=sm(deltas),
                                 ts=sm(ts), Ns=Ns, n_alive=n)


def ray_major(a, n_alive, Ns):
    """slot-major (Ns * n_alive, ...) -> (n_alive, Ns, ...)"""
    return a.reshape((Ns, n_alive) + tuple(a.shape[1:])).transpose(0, 1).contiguous()


def slot_major(a):
    """(n_alive, Ns, ...) -> (Ns * n_alive, ...)"""
    return a.transpose(0, 1).reshape((a.shape[0] * a.shape[1],) + tuple(a.shape[2:])).contiguous()


# ----------------------------------------------------------------- composite
def composite_step(sig, rgbs, deltas, ts, n_eff, alive, op0, dep0, rgb0, T_thr):
    """One composite of the alive rays: composite_ref.alive_ref64 (fp64 composite_test_fw, its bounds, survivor
    flags) on slot-major inputs.  op0 / dep0 / rgb0: the rays' prior values, by ray id (fp32).  -> alive_ref64's
    namespace (alive: the ray id of a survivor or -1, per list position) + n_eff_sum."""
    n, Ns = alive.numel(), sig.numel() // max(alive.numel(), 1)
    t = types.SimpleNamespace(
        sig=ray_major(sig, n, Ns), rgbs=ray_major(rgbs, n, Ns), deltas=ray_major(deltas, n, Ns), ts=ray_major(ts, n, Ns),
        alive=alive.long(), n_eff=n_eff, op0=op0, dep0=dep0, rgb0=rgb0, T_thr=T_thr, Ns=Ns,
        rays_a=torch.stack([alive.long(), torch.arange(n) * Ns, n_eff.long()], 1), T0=1 - op0.double()[alive.long()])
    ref = CR.alive_ref64(t)
    ref.n_eff_sum = int(n_eff.sum())
    ref.t = t
    return ref


@functools.lru_cache(maxsize=None)
def composite_set(n_alive, Ns, n_rays, seed, T_thr=1e-4):
    """Designed composite inputs in the kernels' slot-major layout, in the style of composite_ref.alive_rows: n_eff in
    0..Ns with zeros and full rays forced, rows that terminate at their first and at their last sample, rows that
    never do, a non-zero prior opacity / depth / rgb, a shuffled alive list over n_rays + 37 ray ids (so some rays
    are not listed), every transmittance held a margin from T_thr (enforce_margin)."""
    g = torch.Generator().manual_seed(91 * seed + Ns)
    R = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    n_buf = n_rays + 37
    alive = shuffled_alive(n_alive, n_buf, seed + 1)
    n_eff = torch.randint(0, Ns + 1, (n_alive,), generator=g).to(torch.int32)
    n_eff[:8] = torch.tensor([0, Ns, 0, max(Ns - 1, 0), Ns, 1, Ns, 0], dtype=torch.int32).clamp(max=Ns)[:n_alive]
    deltas = R(n_alive, Ns) * 1e-2 + 1e-3
    fam = torch.randint(0, 4, (n_alive, 1), generator=g)  # 0 never, 1 first sample, 2 last sample, 3 anywhere
    x = R(n_alive, Ns) * (2.5 / Ns)
    k = torch.arange(Ns)[None, :]
    last = (n_eff.long() - 1).clamp(min=0)[:, None]
    x = torch.where((fam == 1) & (k == 0), torch.full_like(x, 12.0), x)
    x = torch.where((fam == 2) & (k == last), torch.full_like(x, 12.0), x)
    x = torch.where((fam == 3) & (R(n_alive, Ns) < 0.15), torch.full_like(x, 12.0), x)
    sig = (x / deltas).float()
    deltas = deltas.float()
    ts = (0.05 + torch.cumsum(deltas, 1)).float()
    rgbs = R(n_alive, Ns, 3).float()
    op0, dep0, rgb0 = (R(n_buf) * 0.9).float(), R(n_buf).float(), R(n_buf, 3).float()
    rays_a = torch.stack([alive.long(), torch.arange(n_alive) * Ns, n_eff.long()], 1)
    T0 = 1 - op0.double()[alive.long()]
    flat = sig.reshape(-1)
    CR.enforce_margin(flat, deltas.reshape(-1), rays_a, T_thr, T0)
    sig = flat.reshape(n_alive, Ns)
    return types.SimpleNamespace(sig=slot_major(sig), rgbs=slot_major(rgbs), deltas=slot_major(deltas), ts=slot_major(ts),
                                 alive=alive, n_eff=n_eff, op0=op0, dep0=dep0, rgb0=rgb0, T_thr=T_thr, Ns=Ns,
                                 n_alive=n_alive, n_rays=n_rays, n_buf=n_buf, fam=fam[:, 0], rays_a=rays_a, T0=T0)


@functools.lru_cache(maxsize=None)
def composite_set_ref(n_alive, Ns, n_rays, seed):
    s = composite_set(n_alive, Ns, n_rays, seed)
    return composite_step(s.sig, s.rgbs, s.deltas, s.ts, s.n_eff, s.alive, s.op0, s.dep0, s.rgb0, s.T_thr)


# (n_alive, Ns, n_rays): one ray per thread | CRPT rays per thread, no multiple of 256 or 1024 | a second pass
COMPOSITE_SHAPES = {"thread": (1100, 8, 5000), "crpt": (3001, 8, 5000),
                    "pass2": (composite_second_pass_n_alive() + 999, 2, composite_second_pass_n_alive() + 999)}


def finish_ref(opacity, rgb, bg):
    """rendering.py:240-251 in fp64 and the bound of its three fp32 roundings: m = fl(1 - op), p = fl(bg m),
    fl(rgb + p): |err| <= 2u |bg m| + u |rgb + p| (+ second order: 3u, SLACK)"""
    b = torch.tensor([CR.F32(v) for v in bg], dtype=torch.float64)
    p = b[None, :] * (1 - opacity.double())[:, None]
    r = rgb.double() + p
    return r, (3 * CR.U * p.abs() + CR.U * r.abs()) * CR.SLACK + CR.TINY


# ---------------------------------------------------------------------- loop
def field_bits(xyzs):
    """A field made of integer operations on the sample positions' bit patterns (the same values on any device, in
    any slot order): sigma in {0, 1e4} -- one sample in eight opaque -- and rgb in k / 256.  With sigma delta >= 16.9
    the transmittance behind an opaque sample is at most 2^-24 < T_thr whatever the rounding of exp, and sigma == 0
    gives alpha == 0 exactly: termination is exact with no margin."""
    v = xyzs.contiguous().view(torch.int32).long() & 0xffffffff  # (int64: no product overflows)
    h = (v[:, 0] * 73856093 ^ v[:, 1] * 19349663 ^ v[:, 2] * 83492791) & 0xffffffff
    h = h ^ (h >> 13)
    sig = torch.where((h & 7) == 0, torch.full_like(xyzs[:, 0], 1e4), torch.zeros_like(xyzs[:, 0]))
    rgb = torch.stack([(h >> 3) & 255, (h >> 11) & 255, (h >> 19) & 255], 1).float() / 256
    return sig, rgb


def render_loop_ref(o, d, ht, bf, cascades, scale, esf, grid, max_samples, min_samples, budget, T_thr, field=field_bits,
                    max_iters=1000):
    """The loop of rendering.py:183-236 from begin to the stop -> namespace(iters: per iteration a namespace(n_alive,
    Ns, alive (sorted ray ids), n_eff (by list position of `alive`), total_samples (running, after it)), n_iters,
    total_samples, opacity / depth / rgb (fp64) and their bounds b_op / b_dep / b_rgb, hits_t).
    The alive list is kept sorted: per-ray results depend on it only through its length.  The bounds of successive
    iterations add up, which is valid while a ray's prior state is exact when it receives a non-zero contribution
    (asserted: true for field_bits, where one sample per ray contributes)."""
    n_rays = o.shape[0]
    alive = torch.arange(n_rays, dtype=torch.int32)
    ht = ht.clone()
    op, dep, rgb = torch.zeros(n_rays, dtype=torch.float64), torch.zeros(n_rays, dtype=torch.float64), \
        torch.zeros(n_rays, 3, dtype=torch.float64)
    b_op, b_dep, b_rgb = torch.zeros_like(op), torch.zeros_like(dep), torch.zeros_like(rgb)
    samples = total = 0
    iters = []
    while len(iters) < max_iters:
        Ns = iteration_rule(n_rays, alive.numel(), samples, budget, min_samples)
        if Ns is None:
            break
        samples += Ns
        m = march_ref(o, d, ht, alive, bf, cascades, scale, esf, grid, max_samples, Ns)
        ht = m.hits_t
        sig, c = field(m.xyzs)
        sig, c = sig * m.valid, c * m.valid[:, None]
        al = alive.long()
        assert bool((op.float().double()[al] == op[al]).all())  # the alive rays' prior state is exact in fp32
        st = composite_step(sig, c, m.deltas, m.ts, m.n_eff, alive, op.float(), dep.float(), rgb.float(), T_thr)
        assert not bool((b_op[st.b_op > 0] > 0).any())
        op[al], dep[al], rgb[al] = st.op[al], st.dep[al], st.rgb[al]  # (dead rays keep their fp64 values)
        b_op[al] += st.b_op[al]
        b_dep[al] += st.b_dep[al]
        b_rgb[al] += st.b_rgb[al]
        total += int(m.n_eff.sum())
        iters.append(types.SimpleNamespace(n_alive=alive.numel(), Ns=Ns, alive=alive.clone(), n_eff=m.n_eff,
                                           total_samples=total))
        alive = st.alive[st.alive >= 0].to(torch.int32)
    return types.SimpleNamespace(iters=iters, n_iters=len(iters), total_samples=total, opacity=op, depth=dep, rgb=rgb,
                                 b_op=b_op, b_dep=b_dep, b_rgb=b_rgb, hits_t=ht)


# ------------------------------------------------------- designed march sets
SIMPLE = dict(cascades=1, scale=0.5, esf=0.0, grid=128, max_samples=1024)
CASCADED = dict(cascades=3, scale=2.0, esf=1 / 256, grid=128, max_samples=1024)
DT = math.sqrt(3) / 1024
FAR_T2 = 2.0 ** 23           # the fallback ray's t2: more than LSEG binades above the first step
DEGENERATE_O = 4.0e4         # camera distance of the degenerate ray: ulp(t0) > 2 dt


@functools.lru_cache(maxsize=None)
def march_set(name):
    """A designed march launch -> namespace(o, d, ht (by ray id, n_buf rays), alive, n_alive, n_rays, min_samples, Ns,
    bf_kind, cfg, skip, tags: dict of alive-list positions by purpose).  n_rays is only the number the kernels
    derive N_samples and their grid from; the ray buffers cover the ids of the alive list (n_buf).
      lane1 / lane15    SIMPLE, N_samples 1 / 15 (lane-per-ray), random occupancy, misses, t0 >= t2
      cascaded          3 cascades, exp step: the plain rule gives N_samples 20 >= WAVE_NS, still lane-per-ray
      wave16 / wave64   wave-per-ray at exactly WAVE_NS / NS_MAX, random occupancy, misses, t0 >= t2
      blocks16          sparse 4^3 blocks: most rays' neighbourhood is empty (the dilation early-out)
      dense16 / dense64 every lattice point occupied: the room truncation
      fallback16        dense; one ray with t0 = 1e-12 and t2 = 2^23 (more than LSEG binades)
      degenerate16      one occupied cell; ray 0 of the list has dt below half an ulp of t0 (skip: the oracle spins)
      zero16 / zero64   rays starting inside the box with t0 == 0.0 or the smallest subnormal, dense / random
      flush / noflush   dense, N_samples 64, n_alive just over / at the mid-loop flush threshold
      flush2            one trip more: block 0 crosses the flush level by 1-2 samples, then stages a full trip
      lane2trips        N_samples 1, n_alive just over the lane mode's first grid-stride trip"""
    cfg, bf_kind, min_samples, skip, tags, inside = SIMPLE, "rand0.2", 1, (), {}, False
    if name in ("lane1", "lane15", "wave16", "wave64"):
        Ns, n_alive = {"lane1": 1, "lane15": 15, "wave16": WAVE_NS, "wave64": NS_MAX}[name], 1003
    elif name == "cascaded":
        cfg, bf_kind, Ns, n_alive, min_samples = CASCADED, "rand0.3", 20, 1003, 4
    elif name == "blocks16":
        bf_kind, Ns, n_alive = "blocks", WAVE_NS, 1003
    elif name in ("dense16", "dense64", "fallback16"):
        bf_kind, Ns, n_alive = "dense", WAVE_NS if name != "dense64" else NS_MAX, 301
    elif name == "degenerate16":
        bf_kind, Ns, n_alive, skip = "centre", WAVE_NS, 301, (0,)
    elif name in ("zero16", "zero64"):
        bf_kind, Ns, n_alive, inside = ("dense" if name == "zero16" else "rand0.2"), \
            (WAVE_NS if name == "zero16" else NS_MAX), 301, True
    elif name in ("flush", "noflush", "flush2"):
        bf_kind, Ns = "dense", NS_MAX
        n_alive = {"flush": flush_n_alive(Ns) + 4, "noflush": flush_n_alive(Ns) - 1,
                   "flush2": flush_trips(Ns) * MARCH_BLOCKS * WAVE_RAYS + 5}[name]
    elif name == "lane2trips":
        bf_kind, Ns, n_alive = "dense", 1, lane_second_trip_n_alive() + 299
    else:
        raise KeyError(name)
    n_rays = Ns * n_alive + (n_alive - 1 if Ns < NS_MAX and n_alive < 5000 else 0)  # the largest n_rays of that quotient
    n_buf = n_alive + 41
    o, d, ht = box_rays(n_buf, len(name) + 13 * Ns, cfg["scale"], inside)
    alive = shuffled_alive(n_alive, n_buf, Ns + len(name))
    pos = lambda i: int(alive[i])  # noqa: E731
    if name in ("lane1", "lane15", "wave16", "wave64", "cascaded", "blocks16"):
        tags["miss"] = list(range(3, 11))
        for i in tags["miss"]:
            ht[pos(i)] = -1.0
        tags["t0_ge_t2"] = [20, 21, 22, 23]
        for i in (20, 21):
            ht[pos(i), 0] = ht[pos(i), 1]
        for i in (22, 23):
            ht[pos(i), 0] = ht[pos(i), 1] + 0.125
        tags["short"] = list(range(30, 46))  # a few steps before the far face: fewer than N_samples points left
        for j, i in enumerate(tags["short"]):
            ht[pos(i), 0] = ht[pos(i), 1] - (2 * j + 1.5) * DT
    if name == "flush2":
        # block 0's trip that crosses the flush level brings 1-2 samples (one short ray, three misses) and its next
        # trip a full 4 * Ns: a flush that came any later would overrun the stage
        base = (flush_trips(Ns) - 1) * MARCH_BLOCKS * WAVE_RAYS
        tags["short"], tags["miss"] = [base], [base + 1, base + 2, base + 3]
        ht[pos(base), 0] = ht[pos(base), 1] - 1.5 * DT
        for i in tags["miss"]:
            ht[pos(i)] = -1.0
    if name == "fallback16":
        tags["far"] = [5]
        oi, di, hi = box_rays(1, 3, cfg["scale"], True)
        o[pos(5)], d[pos(5)] = oi[0], di[0]
        ht[pos(5)] = torch.tensor([1e-12, FAR_T2])
    if name == "degenerate16":
        # (as test_march_ends_a_degenerate_ray_instead_of_spinning: the ray passes within a block of the one occupied
        # cell, so no early out, and its first probe at the box's face is empty -- the jump that never advances)
        o[pos(0)] = torch.tensor([DEGENERATE_O, 0.0, 0.0])
        d[pos(0)] = torch.tensor([-1.0, 0.0, 0.0])
        tags["degenerate"] = [0]
        tags["through"] = list(range(1, 41))  # rays through the occupied cell
        for i in tags["through"]:
            o[pos(i)] = torch.full((3,), 0.5 * cfg["scale"] / cfg["grid"]) - 2 * d[pos(i)]
        ht = box_hits(o, d, cfg["scale"])
    if name in ("zero16", "zero64"):
        tags["zero"] = list(range(0, n_alive, 2))
        tags["subnormal"] = list(range(1, n_alive, 4))
        for i in tags["zero"]:
            ht[pos(i), 0] = 0.0
        for i in tags["subnormal"]:
            ht[pos(i), 0] = 2.0 ** -149
    assert iteration_rule(n_rays, n_alive, 0, 1 << 40, min_samples) == Ns
    return types.SimpleNamespace(name=name, o=o, d=d, ht=ht, alive=alive, n_alive=n_alive, n_rays=n_rays, n_buf=n_buf,
                                 min_samples=min_samples, Ns=Ns, bf_kind=bf_kind, cfg=cfg, skip=skip, tags=tags)


@functools.lru_cache(maxsize=None)
def march_set_ref(name, iteration=0):
    """march_ref of a designed set (computed once per process; read-only); iteration 1: a second march from the
    first one's updated hits_t"""
    s = march_set(name)
    c = s.cfg
    ht = s.ht if iteration == 0 else march_set_ref(name, iteration - 1).hits_t
    return march_ref(s.o, s.d, ht, s.alive, bitfield(s.bf_kind, c["cascades"], c["grid"]), c["cascades"], c["scale"],
                     c["esf"], c["grid"], c["max_samples"], s.Ns, s.skip)


def segment_crossings(rays_ts, dt):
    """What a set gives the lattice walk's register-held segment (a segment is the lattice inside one binade
    [2^e, 2^(e+1)); e = floor(log2 t) over t > 0).  rays_ts: per ray, its emitted ts in walk order.  Returns the
    numbers of rays (a) whose emitted ts span a power of two -- a window that straddles a segment -- and (b) with two
    consecutive emitted ts more than 1.5 dt apart in different binades -- a jump that leaves its segment."""
    a = b = 0
    for ts in rays_ts:
        ts = np.asarray(ts, dtype=np.float32)
        ts = ts[ts > 0]
        if len(ts) < 2:
            continue
        e = np.frexp(ts)[1]
        a += int(e.min() != e.max())
        b += int(((np.diff(ts.astype(np.float64)) > 1.5 * dt) & (np.diff(e) != 0)).any())
    return a, b


LOOP = dict(n_rays=20011, seed=5, budget=1 << 40, T_thr=1e-4)


@functools.lru_cache(maxsize=None)
def loop_inputs():
    o, d, ht = box_rays(LOOP["n_rays"], LOOP["seed"])
    ht[::97] = -1.0  # some rays miss the box
    return o, d, ht


@functools.lru_cache(maxsize=None)
def loop_ref():
    o, d, ht = loop_inputs()
    c = SIMPLE
    return render_loop_ref(o, d, ht, bitfield("dense"), c["cascades"], c["scale"], c["esf"], c["grid"], c["max_samples"],
                           1, LOOP["budget"], LOOP["T_thr"])
