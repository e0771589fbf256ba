"""Conditions on the designed inputs of march_ref.py (no GPU): every set really
contains what it is for, the summary reference gives its known answers, and the
early out's exactness claim holds on the sparse sets -- in the fp32 model against
the oracle's walk.  These are statements about the inputs, not measurements;
`pytest -s` prints the class counts.  Last, the march entry points' argument
checks, which run on the host before any launch."""
import numpy as np
import pytest
import torch

import march_ref as MR
import oracle as O
import render_ref as RR


def _one_bit(grid, cascades, cascade, cell):
    return MR.cells_bitfield([(cascade,) + tuple(cell)], grid, cascades)


def _blocks(bits, grid, cascade=0):
    """the set bits of one cascade as a set of block coordinates"""
    bpc = grid ** 3 // 64
    w = np.nonzero(bits[cascade * bpc:(cascade + 1) * bpc])[0]
    return set(zip(MR.compact3(w).tolist(), MR.compact3(w >> 1).tolist(), MR.compact3(w >> 2).tolist()))


# ------------------------------------------------------------------ summary
def test_morton_helpers_agree_with_the_oracle():
    g = torch.Generator().manual_seed(0)
    c = torch.randint(0, 1024, (5000, 3), generator=g, dtype=torch.int32)
    m = MR.morton3(c[:, 0].numpy(), c[:, 1].numpy(), c[:, 2].numpy())
    assert np.array_equal(m, O.morton3D(c).numpy().astype(np.int64))
    assert all(np.array_equal(MR.compact3(m >> k), c[:, k].numpy()) for k in range(3))


def test_summary_ref_known_answers():
    # one bit in block (0, 0, 0) of a 16^3 grid (4^3 blocks): the 8 blocks with every coordinate <= 1
    s, d = MR.summary_ref(_one_bit(16, 1, 0, (1, 2, 3)), 16, 1)
    assert _blocks(s, 16) == {(0, 0, 0)}
    assert _blocks(d, 16) == {(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)}
    # one bit in a centre block: all 27
    s, d = MR.summary_ref(_one_bit(16, 1, 0, (9, 6, 10)), 16, 1)
    assert _blocks(s, 16) == {(2, 1, 2)}
    assert _blocks(d, 16) == {(x, y, z) for x in (1, 2, 3) for y in (0, 1, 2) for z in (1, 2, 3)} and int(d.sum()) == 27
    # one bit in the last block of cascade 0 of 2: nothing in cascade 1
    s, d = MR.summary_ref(_one_bit(16, 2, 0, (15, 15, 15)), 16, 2)
    assert int(s.sum()) == 1 and bool(s[63]) and int(d[:64].sum()) == 8 and not d[64:].any()
    # ... and the first block of cascade 1 does not reach back into cascade 0
    s, d = MR.summary_ref(_one_bit(16, 2, 1, (0, 0, 0)), 16, 2)
    assert bool(s[64]) and int(d[64:].sum()) == 8 and not d[:64].any()
    # grid 8, one cascade: 8 words, no whole wave of blocks -> the dilated half is all ones below n_words
    bf = _one_bit(8, 1, 0, (5, 1, 1))
    assert not MR.summary_dilates(8, 8)
    s, d = MR.summary_ref(bf, 8, 1)
    assert int(s.sum()) == 1 and d.all() and d.size == 8
    w = MR.pack_summary(s, d).numpy().view(np.uint32)
    assert w.size == 2 and int(w[1]) == 0xff and int(w[0]) == 1 << int(np.nonzero(s)[0][0])  # bits past n_words: 0
    # grid 4 with 64 cascades: one block per cascade, no neighbour but itself
    bf = torch.zeros(64 * 8, dtype=torch.uint8)
    bf[8 * 5 + 2], bf[8 * 63] = 4, 1
    s, d = MR.summary_ref(bf, 4, 64)
    assert MR.summary_dilates(64, 4) and np.array_equal(s, d) and np.nonzero(s)[0].tolist() == [5, 63]


def test_pack_summary_layout():
    g = np.random.default_rng(0)
    s, d = g.random(32768) < 0.3, g.random(32768) < 0.6
    w = MR.pack_summary(s, d).numpy().view(np.uint32)
    assert w.size == 2 * 1024
    for i in (0, 31, 32, 1000, 32767):
        assert (int(w[i >> 5]) >> (i & 31)) & 1 == int(s[i]) and (int(w[1024 + (i >> 5)]) >> (i & 31)) & 1 == int(d[i])


# ------------------------------------------------------------- sparse sets
def test_sparse_bitfield_holds_what_it_is_for():
    s = MR.march_set("sparse")
    G = s.cfg["grid"]
    cells = s.cells
    bits = np.unpackbits(s.bf.numpy(), bitorder="little")
    assert int(bits.sum()) == len(cells) == 40
    for axis in range(3):
        assert 0 in cells[:, axis] and G - 1 in cells[:, axis]  # the box's faces
    corner = np.isin(cells % 4, (0, 3)).all(1)
    assert int(corner.sum()) >= 20
    m = np.sort(MR.morton3(cells[:, 0], cells[:, 1], cells[:, 2]))
    pair = np.nonzero(np.diff(m) == 1)[0]
    assert pair.size == 1 and int(m[pair[0]]) % 64 == 63  # Morton neighbours across a block boundary
    # every other cell is isolated: alone within two blocks
    dist = np.abs(cells[:, None, :] - cells[None, :, :]).max(2) + 99 * np.eye(len(cells), dtype=np.int64)
    assert int((dist.min(1) < 9).sum()) == 2
    summ, dil = MR.summary_ref(s.bf, G, 1)
    assert int(summ.sum()) == 40 and int(summ.sum()) < int(dil.sum()) <= 27 * 40


def test_sparse_rays_fill_every_class_of_the_early_out():
    s, c = MR.march_set("sparse"), MR.sparse_classes("sparse")
    n = {k: int(getattr(c, k).sum()) for k in ("skipped", "marched_empty", "few", "dilation_only", "clamped", "second_window")}
    per_d = [int((c.dilation_only & (s.dclass == k)).sum()) for k in range(3)]
    print(f"sparse classes of {s.n_rays} rays: {n}, dilation_only per |d| {dict(zip(MR.D_CLASSES, per_d))}, "
          f"inside the box {int(s.inside.sum())}, of them with a second window {int((s.inside & c.second_window).sum())}, "
          f"emitting {int((c.counts > 0).sum())}, samples {int(c.counts.sum())}")
    assert s.n_rays == 2048
    assert n["skipped"] >= 200 and n["marched_empty"] >= 200 and n["few"] >= 100
    assert n["dilation_only"] >= 20 and min(per_d) >= 3
    assert n["clamped"] >= 5 and n["second_window"] >= 20
    # a quarter of the rays start inside the box at t0 = near (before the noise), and some of those take the early-out
    # loop round a second time
    assert int(s.inside.sum()) == s.n_rays // 4 and bool((s.ht[torch.from_numpy(s.inside), 0] == MR.NEAR).all())
    assert int((s.inside & c.second_window).sum()) >= 20
    # |d| really is 0.1, 1 or 10
    dn = s.d.double().norm(dim=1).numpy()
    assert np.allclose(dn, np.array(MR.D_CLASSES)[s.dclass], rtol=1e-6) and min(np.bincount(s.dclass)) > 500


@pytest.mark.parametrize("name", ["sparse", "sparse_quarter", "sparse_wide"])
def test_the_early_out_is_exact(name):
    """The claim of lat_near_occupied's comment (march.h): no ray the early out ends has a sample in the oracle's walk."""
    s, c = MR.march_set(name), MR.sparse_classes(name)
    n_skip, n_emit, n_dil = int(c.skipped.sum()), int((c.counts > 0).sum()), int(c.dilation_only.sum())
    print(f"{name}: {n_skip} of {s.n_rays} rays skipped, {n_emit} emit, {n_dil} of them kept by the dilation only")
    assert n_skip >= s.n_rays // 5 and n_emit >= s.n_rays // 8 and n_dil >= 3
    assert int((c.skipped & (c.counts > 0)).sum()) == 0
    if name == "sparse_quarter":
        assert min(0.5, s.cfg["scale"]) < 0.5
    if name == "sparse_wide":  # the box is larger than the grid: every ray has early-out points outside it
        assert s.cfg["scale"] > 0.5 and s.cfg["cascades"] == 1 and bool(c.clamped.all()) and s.n_rays == 512


# -------------------------------------------------------------------- room
def _lattice_points(t0, t2, dt):
    """the points t0, fl(t0 + dt), ... below t2, counted serially in fp32"""
    n, t = 0, np.float32(t0)
    while 0 <= t < t2:
        n, t = n + 1, np.float32(t + dt)
    return n


@pytest.mark.parametrize("max_samples", MR.ROOM_MAX_SAMPLES)
def test_room_rays_are_cut_by_max_samples(max_samples):
    s, r = MR.march_set("room", max_samples, 5), MR.march_set_ref("room", max_samples, 5)
    assert bool((s.bf == 255).all())
    t0 = MR.start_t(s.ht, s.noise, s.cfg)
    dt = np.float32(O.lib().or_calc_dt(1.0, 0.0, max_samples, 128, 0.5))
    pts = [_lattice_points(t0[i], np.float32(s.ht[i, 1]), dt) for i in range(5)]
    cnt = r.counts.tolist()
    print(f"room max_samples {max_samples}: lattice points {pts}, counts {cnt}")
    assert cnt == [min(p, max_samples) for p in pts]
    more = [p > max_samples for p in pts]
    assert more == [True, False, True, True, False]  # three rays are cut, two cross fewer points than max_samples
    assert all(p < max_samples for p, m in zip(pts, more) if not m)
    for n in MR.ROOM_N_RAYS:  # the smaller launches are prefixes
        sn = MR.march_set("room", max_samples, n)
        assert sn.n_rays == n and torch.equal(sn.o, s.o[:n]) and torch.equal(MR.march_set_ref("room", max_samples, n).counts,
                                                                             r.counts[:n])


# -------------------------------------------------------------------- scan
@pytest.mark.parametrize("n", MR.SCAN_N_RAYS + (MR.SCAN_TILE_N_RAYS,))
def test_scan_sets_interleave_misses(n):
    s, r = MR.march_set("scan", n), MR.march_set_ref("scan", n)
    miss = s.ht[:, 0] < 0
    print(f"scan {n}: {int(miss.sum())} rays miss the box, {r.total} samples")
    assert n > 1024 and n % 1024 and 0.25 * n < int(miss.sum()) < 0.4 * n
    assert bool((s.ht[miss] == -1).all()) and bool((r.counts[miss] == 0).all())
    assert bool(miss[2::3].all()) and int((r.counts[0::3] > 0).sum()) > 0.3 * n  # interleaved with hits
    assert int(r.counts[1024]) > 0 and r.total > 20 * n
    assert torch.equal(r.rays_a[:, 1], torch.cumsum(r.rays_a[:, 2], 0) - r.rays_a[:, 2])
    if n == MR.SCAN_N_RAYS[-1]:  # what the wave march's register-held segment has to get right (render_ref)
        dt = float(np.float32(O.lib().or_calc_dt(1.0, 0.0, s.cfg["max_samples"], s.cfg["grid"], s.cfg["scale"])))
        straddle, leave = RR.segment_crossings([r.ts[a:a + c].numpy() for _, a, c in r.rays_a.tolist()], dt)
        print(f"scan {n}: {straddle} rays' samples span a power of two, {leave} rays jump out of a binade")
        assert straddle >= 1 and leave >= 1


# ---------------------------------------------------------------- cascaded
@pytest.mark.parametrize("n", MR.CASCADED_N_RAYS)
def test_cascaded_sets_emit_in_every_cascade(n):
    s, r = MR.march_set("cascaded", n), MR.march_set_ref("cascaded", n)
    c = s.cfg
    assert c == RR.CASCADED and s.n_rays == n and int(r.counts[0]) > 0 and r.total > 0
    if n < MR.CASCADED_N_RAYS[-1]:
        return
    G, C = c["grid"], c["cascades"]
    words = s.bf.numpy().view(np.uint64).reshape(C, -1)
    bits = np.unpackbits(s.bf.numpy(), bitorder="little").reshape(C, -1)
    assert int(bits[0].sum()) == 12 and int((words[0] != 0).sum()) <= 12       # cascade 0: single cells
    for k in (1, 2):                                                             # cascades 1, 2: sparse whole blocks
        occ = words[k] != 0
        assert 0.01 < occ.mean() < 0.03 and bool((words[k][occ] == np.uint64(2 ** 64 - 1)).all())
    # the cascade of every emitted sample, as the walk chooses it
    L = O.lib()
    mip = np.array([max(L.or_mip_from_pos(*(float(v) for v in x), C), L.or_mip_from_dt(float(dt), G, C))
                    for x, dt in zip(r.xyzs, r.deltas)])
    per = np.bincount(mip, minlength=C)
    print(f"cascaded: {int((r.counts > 0).sum())} of {n} rays emit {r.total} samples, per cascade {per.tolist()}")
    assert per.min() >= 20 and int((r.counts == 0).sum()) >= 30
    assert float(r.deltas.max()) > 2 * float(r.deltas.min())  # dt is not a constant here
    assert [k for k in MR.CASCADED_N_RAYS if k % 16 == 0] == [16] and 300 > 4 * 16 * 4  # off 16 / 64, several blocks


# ------------------------------------------------- the entry points' host checks
def test_march_entry_points_reject_bad_arguments_before_any_launch():
    """march_params, march_attach_summary and the NGP_CHECK_ARG lines run on the host before a launch (no GPU needed):
    every call below fails one of them, or is a zero-size no-op that launches nothing.  The pointers are made-up
    addresses: no call here may pass its checks."""
    import vren
    from capi import C
    L, OK, EINVAL, ERANGE = vren.lib(), C["NGP_OK"], C["NGP_EINVAL"], C["NGP_ERANGE"]
    P, ODD = 0x10000, 0x10004  # 8-byte aligned / not
    # ngp_bitfield_summary(bitfield, n_bytes, grid_size, summary, stream)
    assert L.ngp_bitfield_summary(P, -8, 128, P, None) == EINVAL
    assert L.ngp_bitfield_summary(None, 0, 128, None, None) == OK          # nothing to do
    assert L.ngp_bitfield_summary(P, 12, 128, P, None) == EINVAL           # no whole 64-bit words
    assert L.ngp_bitfield_summary(ODD, 64, 8, P, None) == EINVAL           # 64-bit loads need 8-byte alignment
    assert L.ngp_bitfield_summary(P, 64, 8, None, None) == EINVAL

    def slots(n=4, bf=P, cascades=1, grid=128, ms=1024, rays=P, total=P, summary=None):
        return L.ngp_march_train_slots(rays, rays, rays, n, bf, cascades, grid, 0.5, 0.0, rays, ms, P, P, total, P, P,
                                       summary, None)

    def count(n=4, bf=P, cascades=1, grid=128, ms=1024, rays=P, total=P):
        return L.ngp_march_train_count(rays, rays, rays, n, bf, cascades, grid, 0.5, 0.0, rays, ms, P, P, total, None)

    def write(n=4, bf=P, cascades=1, grid=128, ms=1024, rays=P, out=P):
        return L.ngp_march_train_write(rays, rays, rays, n, bf, cascades, grid, 0.5, 0.0, rays, ms, P, out, out, out, out,
                                       None)

    for f in (slots, count, write):  # march_params
        assert f(bf=None) == EINVAL and f(bf=ODD) == EINVAL, f.__name__
        assert f(cascades=0) == EINVAL and f(grid=3) == EINVAL and f(grid=1025) == EINVAL and f(ms=0) == EINVAL, f.__name__
        assert f(n=-1) == EINVAL and f(rays=None) == EINVAL, f.__name__
    assert slots(total=None) == EINVAL and count(total=None) == EINVAL and write(out=None) == EINVAL
    assert write(n=0, rays=None, out=None) == OK                           # nothing to do
    # march_attach_summary: whole 2048-cell summary words, and no more than the LDS copy holds
    assert slots(grid=8, summary=P) == EINVAL and slots(grid=512, summary=P) == ERANGE
    # ngp_march_train_compact(rays_o, rays_d, rays_a, n_rays, slot_t, slot_dt, max_samples, xyzs, dirs, deltas, ts, stream)
    assert L.ngp_march_train_compact(P, P, P, -1, P, P, 1024, P, P, P, P, None) == EINVAL
    assert L.ngp_march_train_compact(P, P, P, 4, P, P, 0, P, P, P, P, None) == EINVAL
    assert L.ngp_march_train_compact(P, P, P, 4, P, P, 1024, P, P, P, None, None) == EINVAL
    assert L.ngp_march_train_compact(None, None, None, 0, None, None, 1024, None, None, None, None, None) == OK
