"""A plain CPU reference of the training march's own machinery (csrc/march.hip):
the bitfield summary with its one-block dilation, the wave march's conservative
early out, and the designed ray sets the training-march tests run.  A helper
module (not a conftest), like render_ref.py: test_march_ref_cpu.py states what
the designed sets contain, test_march_train_gpu.py holds the kernels to them.

  * summary_ref is written from the definition in ngp_bitfield_summary's
    comment: a 3-d array of blocks per cascade, OR-ed with its 26 shifts.  It
    shares no code with the kernel (no 27-load loop, no ballot).
  * early_out_model restates the early out of march_slots_wave_kernel in fp32
    numpy, the same expressions in the same order.  It is a model of the
    kernel, used to CLASSIFY rays; what a ray must emit is the oracle's walk.
  * every expected sample comes from oracle.raymarching_train.
"""
import functools
import types

import numpy as np
import torch

import oracle as O
import render_ref as RR

F = np.float32
NEAR = RR.NEAR


# ------------------------------------------------------------ Morton order
def compact3(v):
    """every third bit of v, packed (the inverse of the Morton spread)"""
    v = np.asarray(v, dtype=np.uint64)
    out = np.zeros_like(v)
    for b in range(11):
        out |= ((v >> np.uint64(3 * b)) & np.uint64(1)) << np.uint64(b)
    return out.astype(np.int64)


def morton3(x, y, z):
    x, y, z = (np.asarray(a, dtype=np.uint64) for a in (x, y, z))
    out = np.zeros_like(x)
    for b in range(11):
        s = np.uint64(b)
        out |= (((x >> s) & np.uint64(1)) << np.uint64(3 * b)) | (((y >> s) & np.uint64(1)) << np.uint64(3 * b + 1)) \
            | (((z >> s) & np.uint64(1)) << np.uint64(3 * b + 2))
    return out.astype(np.int64)


def cells_bitfield(cells, grid, cascades=1):
    """(n, 4) int rows (cascade, x, y, z) of occupied cells -> uint8 bitfield (cascades * grid^3 / 8)"""
    bits = np.zeros(cascades * grid ** 3, dtype=np.uint8)
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 4)
    bits[c[:, 0] * grid ** 3 + morton3(c[:, 1], c[:, 2], c[:, 3])] = 1
    return torch.from_numpy(np.packbits(bits, bitorder="little"))


# ------------------------------------------------------------------ summary
def summary_dilates(n_words, grid):
    """ngp_bitfield_summary's `dil` condition: whole cascades of a power-of-two grid, whole waves of blocks"""
    bpc = grid ** 3 // 64
    return grid >= 4 and grid & (grid - 1) == 0 and bpc > 0 and n_words % bpc == 0 and n_words % 64 == 0


def summary_ref(bf, grid, cascades):
    """-> (summary_bits, dilated_bits), bool (n_words): bit w of the summary is (64-bit bitfield word w != 0), i.e.
    whether the Morton-aligned 4^3 block w holds an occupied cell; bit w of the dilation is the OR of the summary over
    block w and its up to 26 neighbours of the same cascade, block (bx, by, bz) being the de-interleaved index of w
    inside its cascade.  Where the kernel has no block geometry (summary_dilates false) every dilated bit is set."""
    words = np.ascontiguousarray(bf.numpy() if isinstance(bf, torch.Tensor) else bf).view(np.uint64)
    n_words = words.size
    assert n_words * 64 == cascades * grid ** 3
    s = words != 0
    if not summary_dilates(n_words, grid):
        return s, np.ones(n_words, dtype=bool)
    bpc, side = grid ** 3 // 64, grid // 4
    local = np.arange(bpc)
    bx, by, bz = compact3(local), compact3(local >> 1), compact3(local >> 2)
    d = np.zeros(n_words, dtype=bool)
    for c in range(cascades):
        vol = np.zeros((side + 2,) * 3, dtype=bool)  # one block of empty margin: neighbours out of range are no blocks
        vol[bx + 1, by + 1, bz + 1] = s[c * bpc:(c + 1) * bpc]
        acc = np.zeros((side,) * 3, dtype=bool)
        for dx in range(3):
            for dy in range(3):
                for dz in range(3):
                    acc |= vol[dx:dx + side, dy:dy + side, dz:dz + side]
        d[c * bpc:(c + 1) * bpc] = acc[bx, by, bz]
    return s, d


def pack_summary(summary_bits, dilated_bits):
    """the kernel's layout: 2 x ((n_words + 31) // 32) uint32 words (as int32, the project's convention for unsigned
    words in tensors), summary half first; bits past n_words in each half's last word are 0"""
    halves = []
    for bits in (summary_bits, dilated_bits):
        n32 = (bits.size + 31) // 32
        pad = np.zeros(n32 * 32, dtype=np.uint8)
        pad[:bits.size] = bits
        halves.append(np.packbits(pad, bitorder="little").view(np.uint32))
    return torch.from_numpy(np.concatenate(halves).view(np.int32).copy())


def summary_words(bf, grid, cascades):
    return pack_summary(*summary_ref(bf, grid, cascades))


# ---------------------------------------------------------------- early out
def start_t(ht, noise, cfg):
    """start_t of march.h in fp32: t1 + calc_dt(t1) * noise for t1 >= 0 (calc_dt: the oracle's)"""
    t1 = ht[:, 0].numpy().astype(F)
    L = O.lib()
    dt = np.array([L.or_calc_dt(float(t), cfg["esf"], cfg["max_samples"], cfg["grid"], cfg["scale"]) for t in t1], dtype=F)
    return np.where(t1 >= 0, t1 + dt * noise.numpy().astype(F), t1).astype(F)


def early_out_model(o, d, t0, t2, dilated_bits, scale, grid):
    """march_slots_wave_kernel's early out, expression for expression in fp32 (one cascade, esf 0).  o, d (n, 3),
    t0 (start_t), t2 (n) -> namespace: valid (0 <= t0 < t2: the early out is reached), marched (valid and some point's
    block has its dilated bit), npts (n), blocks (list of int arrays: the block index of every early-out point),
    clamped (n: some point lies outside the grid before the clamp, so its cell is a clamped face cell)."""
    o, d = np.asarray(o, dtype=F), np.asarray(d, dtype=F)
    t0, t2 = np.asarray(t0, dtype=F), np.asarray(t2, dtype=F)
    n = o.shape[0]
    G, gm1 = F(grid), F(grid) - F(1)
    mb = np.minimum(F(0.5), F(scale))
    mbi = F(1) / mb
    dn = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    step = F(0.45) * (F(8) * mb / G) / dn
    valid = (t0 >= 0) & (t0 < t2)
    with np.errstate(invalid="ignore"):
        npts = np.where(valid, np.ceil((t2 - t0) / step).astype(np.int64) + 1, 0)
    j = np.arange(max(int(npts.max()), 1))
    live = j[None, :] < npts[:, None]
    t = np.minimum(t0[:, None] + j[None, :].astype(F) * step[:, None], t2[:, None])
    cell, out = [], np.zeros((n, j.size), dtype=bool)
    for i in range(3):
        x = o[:, i:i + 1] + t * d[:, i:i + 1]
        v = F(0.5) * (x * mbi + F(1)) * G
        out |= (v < 0) | (v >= G)
        cell.append(np.maximum(F(0), np.minimum(v, gm1)).astype(np.int64))
    wi = morton3(cell[0] >> 2, cell[1] >> 2, cell[2] >> 2)
    near = np.asarray(dilated_bits)[wi] & live
    return types.SimpleNamespace(valid=valid, marched=valid & near.any(1), npts=npts,
                                 blocks=[wi[r, :npts[r]] for r in range(n)], clamped=(out & live).any(1))


# ------------------------------------------------------------ designed sets
SPARSE = dict(cascades=1, scale=0.5, esf=0.0, grid=128, max_samples=1024)
D_CLASSES = (0.1, 1.0, 10.0)
ROOM_MAX_SAMPLES = (1, 63, 64, 65, 100)
ROOM_N_RAYS = (1, 3, 4, 5)
SCAN_N_RAYS = (1025, 2500)
SCAN_TILE_N_RAYS = 8193  # 1024 x 8 + 1: the smallest launch with a second tile of the 1024-thread block scan
CASCADED_N_RAYS = (1, 15, 16, 17, 63, 65, 300)
SEEDS = {"sparse": 1, "sparse_quarter": 1, "sparse_wide": 2}  # chosen so that test_march_ref_cpu.py's conditions hold


def sparse_cells(grid, seed):
    """about 40 isolated occupied cells: every second one on a corner of its 4^3 block, cells with index 0 and
    grid - 1 on each axis (the box's faces), and one pair of Morton neighbours across a block boundary (the last cell
    of one block, the first of the next) -> (n, 3) int"""
    g = np.random.default_rng(seed)
    G = grid
    fixed = [(0, 50, 70), (G - 1, 61, 33), (41, 0, 90), (77, G - 1, 58), (66, 21, 0), (30, 99, G - 1), (0, 0, 0),
             (G - 1, G - 1, G - 1)]
    m = 64 * int(morton3(10, 17, 13)) + 63  # block (10, 17, 13): an even index, so its Morton successor is its +x block
    pair = [tuple(int(compact3(c >> k)) for k in range(3)) for c in (m, m + 1)]
    assert pair[1][0] == pair[0][0] + 1 and (pair[0][0] + 1) % 4 == 0
    cells = fixed + pair
    while len(cells) < 40:
        c = g.integers(8, G - 8, 3)
        if len(cells) % 2:
            c = (c // 4) * 4 + g.choice([0, 3], 3)  # a corner cell of its block
        if np.abs(np.array(cells) - c).max(1).min() >= 9:  # isolated: no other occupied cell within two blocks
            cells.append(tuple(int(v) for v in c))
    return np.array(cells)


def _aimed_rays(cells, n, scale, grid, seed, box=None):
    """n rays from a camera two units out (every fourth from a point inside the box: t0 = near): the even ones aimed
    within +-1.6 cells of an occupied cell's centre, the odd ones at uniform points of the box; unit directions, then
    |d| scaled by 0.1, 1 or 10 -> o, d, hits_t, noise, dclass (index into D_CLASSES)"""
    g = np.random.default_rng(seed)
    mb = min(0.5, scale)
    box = scale if box is None else box
    cell = 2 * mb / grid
    pick = cells[g.integers(0, len(cells), n)]
    aimed = ((pick + 0.5) * cell - mb) + 1.6 * g.uniform(-1, 1, (n, 3)) ** 3 * cell  # (denser towards the cell)
    tgt = np.where((np.arange(n) % 2 == 0)[:, None], aimed, g.uniform(-box, box, (n, 3)))
    v = g.normal(size=(n, 3))
    cam = 2.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
    inside = (np.arange(n) // 2) % 4 == 3  # (aimed and uniform ones alike)
    cam = np.where(inside[:, None], g.uniform(-0.8 * box, 0.8 * box, (n, 3)), cam)
    u = tgt - cam
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dclass = g.integers(0, 3, n)
    o = torch.from_numpy(cam.astype(F)).contiguous()
    d = torch.from_numpy((u * np.array(D_CLASSES)[dclass][:, None]).astype(F)).contiguous()
    ht = RR.box_hits(o, d, box)
    noise = torch.from_numpy(g.uniform(0, 1, n).astype(F))
    return o, d, ht, noise, dclass, inside


def _set(name, o, d, ht, noise, bf, cfg, **more):
    ht = ht.contiguous()
    # inside what the box test produces: finite hits, and dt 2^24 above every t (no ray takes the degenerate-ray guard)
    assert bool(torch.isfinite(ht).all()) and bool(torch.isfinite(o).all()) and bool((d != 0).all())
    assert float(ht.max()) < np.sqrt(3) / cfg["max_samples"] * 2 ** 24 / 4
    return types.SimpleNamespace(name=name, o=o, d=d, ht=ht, noise=noise, bf=bf, cfg=cfg, n_rays=o.shape[0], **more)


@functools.lru_cache(maxsize=None)
def march_set(name, *arg):
    """A designed training-march launch -> namespace(o, d, ht, noise, bf, cfg, n_rays, ...).
      sparse          grid 128, scale 0.5: 40 isolated cells (sparse_cells), 2048 rays (_aimed_rays)
      sparse_quarter  the same at scale 0.25: a mip bound below 0.5
      sparse_wide     scale 1.0 with one cascade: the box is larger than the grid, positions clamp onto the face
                      cells; 512 rays
      room, ms, n     dense bitfield, max_samples ms in ROOM_MAX_SAMPLES, the first n in ROOM_N_RAYS of five rays
                      with |d| = 0.25: rays 0, 2, 3 cross more than ms lattice points, rays 1 and 4 fewer (with
                      unit directions no chord of the box holds more than ms steps of sqrt3 / ms: no cut at all)
      scan, n         n in SCAN_N_RAYS (or SCAN_TILE_N_RAYS) rays on rand0.2, every third one missing the box (ray 1024,
                      the first past a lane-per-ray scan, hits)
      cascaded, n     render_ref.CASCADED (3 cascades, scale 2, exp step): sparse whole blocks in cascades 1 and 2, a
                      few single cells in cascade 0; the first n in CASCADED_N_RAYS of 300 rays"""
    if name in ("sparse", "sparse_quarter", "sparse_wide"):
        scale, n = {"sparse": (0.5, 2048), "sparse_quarter": (0.25, 2048), "sparse_wide": (1.0, 512)}[name]
        cfg = dict(SPARSE, scale=scale)
        cells = sparse_cells(cfg["grid"], 3)
        o, d, ht, noise, dclass, inside = _aimed_rays(cells, n, scale, cfg["grid"], SEEDS[name])
        bf = cells_bitfield(np.concatenate([np.zeros((len(cells), 1), dtype=np.int64), cells], 1), cfg["grid"])
        return _set(name, o, d, ht, noise, bf, cfg, cells=cells, dclass=dclass, inside=inside)
    if name == "room":
        ms, n = arg
        cfg = dict(SPARSE, max_samples=ms)
        # long chords through the centre (t length 4 / 0.25 ... > 4: more than 100 steps of sqrt3 / ms for every ms,
        # and more than one of sqrt3 / 1), short ones across a corner (t length about 0.4: under 63 steps of
        # sqrt3 / 63, and with noise > 0.3 no lattice point at all at max_samples 1)
        tgt = torch.tensor([[0.01, 0.02, -0.03], [0.44, 0.43, 0.0], [-0.1, 0.05, 0.1], [0.0, 0.1, -0.05], [-0.43, 0.0, 0.44]])
        u = torch.nn.functional.normalize(torch.tensor([[1.0, 0.2, 0.1], [1.0, -1.0, 0.03], [0.1, 1.0, 0.3],
                                                        [-0.2, 0.1, 1.0], [1.0, 0.02, 1.0]]), dim=1)
        o, d = (tgt - 2 * u)[:n].contiguous(), (0.25 * u)[:n].contiguous()
        noise = torch.tensor([0.25, 0.6, 0.0, 0.99, 0.5])[:n].contiguous()
        return _set(name, o, d, RR.box_hits(o, d, 0.5), noise, RR.bitfield("dense"), cfg)
    if name == "scan":
        (n,) = arg
        o, d, ht = RR.box_rays(n, 100 + n)
        g = torch.Generator().manual_seed(n)
        off = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
        miss = torch.arange(n) % 3 == 2
        perp = torch.nn.functional.normalize(off - (d * off).sum(1, keepdim=True) * d, dim=1)
        o = torch.where(miss[:, None], o + 3.0 * perp, o).contiguous()  # the whole line moved 3 units sideways
        noise = torch.rand(n, generator=g)
        return _set(name, o, d, RR.box_hits(o, d, 0.5), noise, RR.bitfield("rand0.2"), dict(SPARSE), miss=miss)
    if name == "cascaded":
        (n,) = arg
        cfg = dict(RR.CASCADED)
        G, C = cfg["grid"], cfg["cascades"]
        g = torch.Generator().manual_seed(11)
        words = torch.rand(C * G ** 3 // 64, generator=g) < 0.02
        words[:G ** 3 // 64] = False  # cascade 0: single cells only
        bf = (words.repeat_interleave(8).to(torch.uint8) * 255)
        single = torch.randint(40, 88, (12, 3), generator=g).numpy()
        bf = bf | cells_bitfield(np.concatenate([np.zeros((12, 1), dtype=np.int64), single], 1), G, C)
        o, d, ht = RR.box_rays(CASCADED_N_RAYS[-1], 23, cfg["scale"])
        # rays 0-39 through single cells of cascade 0, from 1.5 units away: the exp step there is still below a cell of
        # cascade 0 (t / 256 * grid < 1 for t < 2), so the walk probes cascade 0 and the smallest launches emit too
        cell = 2 * 0.5 / G
        for i in range(40):
            o[i] = torch.from_numpy(((single[i % 12] + 0.5) * cell - 0.5).astype(F)) - 1.5 * d[i]
        noise = torch.rand(o.shape[0], generator=g)
        ht = RR.box_hits(o, d, cfg["scale"])
        return _set(name, o[:n].contiguous(), d[:n].contiguous(), ht[:n], noise[:n].contiguous(), bf, cfg)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def march_set_ref(name, *arg):
    """the oracle's raymarching_train of a designed set (computed once per process; read-only) -> namespace(rays_a,
    xyzs, dirs, deltas, ts, counts, total)"""
    s = march_set(name, *arg)
    c = s.cfg
    rays_a, xyzs, dirs, deltas, ts, counter = O.raymarching_train(s.o, s.d, s.ht, s.bf, c["cascades"], c["scale"], c["esf"],
                                                                 s.noise, c["grid"], c["max_samples"])
    return types.SimpleNamespace(rays_a=rays_a, xyzs=xyzs, dirs=dirs, deltas=deltas, ts=ts,
                                 counts=rays_a[:, 2].to(torch.int32), total=int(counter[0]))


@functools.lru_cache(maxsize=None)
def sparse_classes(name):
    """The rays of a sparse set by what the early out does with them (boolean masks over the rays):
      skipped        the model's early out ends the ray (it reaches the early out and no point's block is near)
      marched_empty  marched, and the oracle's walk emits nothing
      few            the walk emits 1 or 2 samples
      dilation_only  the walk emits although no early-out point lies in an occupied block: only the dilation keeps it
      clamped        an early-out point lies outside the grid (a clamped face cell)
      second_window  more than 64 early-out points: the kernel's loop goes round a second time"""
    s, ref = march_set(name), march_set_ref(name)
    c = s.cfg
    summ, dil = summary_ref(s.bf, c["grid"], 1)
    m = early_out_model(s.o.numpy(), s.d.numpy(), start_t(s.ht, s.noise, c), s.ht[:, 1].numpy(), dil, c["scale"], c["grid"])
    cnt = ref.counts.numpy()
    in_occ = np.array([bool(summ[b].any()) for b in m.blocks])
    return types.SimpleNamespace(model=m, counts=cnt, skipped=m.valid & ~m.marched, marched_empty=m.marched & (cnt == 0),
                                 few=(cnt == 1) | (cnt == 2), dilation_only=(cnt > 0) & ~in_occ, clamped=m.clamped,
                                 second_window=m.npts > 64)
