"""Conditions on the designed inputs of render_ref.py (no GPU): every set really
contains what it is for, and the derived thresholds sit where the kernels'
constants put them.  These are statements about the inputs, not measurements."""
import math

import numpy as np
import pytest
import torch

import composite_ref as CR
import oracle as O
import render_ref as RR


def test_iteration_rule_boundaries():
    assert RR.iteration_rule(100, 0, 0, 10, 1) is None and RR.iteration_rule(100, 5, 10, 10, 1) is None
    assert RR.iteration_rule(100, 5, 9, 10, 1) == 20
    for q, want1, want4 in ((1, 1, 4), (15, 15, 15), (16, 16, 16), (17, 17, 17), (63, 63, 63), (64, 64, 64), (65, 64, 64)):
        for rem in (0, 4):
            assert RR.iteration_rule(q * 5 + rem, 5, 0, 1 << 40, 1) == want1
            assert RR.iteration_rule(q * 5 + rem, 5, 0, 1 << 40, 4) == want4


def test_thresholds_follow_the_constants():
    """the figures the kernels' constants give today; the tests use the functions, these only pin the derivation"""
    assert RR.flush_trips(RR.NS_MAX) == 8 and RR.flush_trips(RR.WAVE_NS) == 29
    assert RR.flush_n_alive(RR.NS_MAX) == 7 * 2048 * 4 + 1
    assert RR.lane_second_trip_n_alive() == 2048 * 256 + 1
    assert RR.composite_second_pass_n_alive() == 4 * 1024 * 256 + 1
    # a full trip of NS_MAX-sample rays fits the stage behind the flush level, with no slack
    assert RR.STAGE - RR.FLUSH_SLACK + RR.WAVE_RAYS * RR.NS_MAX == RR.STAGE


def test_march_ref_puts_the_oracle_walk_into_sample_major_slots():
    s = RR.march_set("wave16")
    r = RR.march_set_ref("wave16")
    c = s.cfg
    ht = s.ht.clone()
    x, dd, dl, t, ne = O.raymarching_test(s.o, s.d, ht, s.alive.long(), RR.bitfield(s.bf_kind), c["cascades"], c["scale"],
                                          c["esf"], c["grid"], c["max_samples"], s.Ns)
    assert torch.equal(ne, r.n_eff) and torch.equal(ht, r.hits_t) and int(r.valid.sum()) == int(ne.sum())
    for n in (0, 1, 57, s.n_alive - 1):
        for k in range(int(ne[n])):
            q = k * s.n_alive + n
            assert bool(r.valid[q]) and torch.equal(r.xyzs[q], x[n, k]) and float(r.ts[q]) == float(t[n, k])
            assert torch.equal(r.dirs[q], s.d[int(s.alive[n])]) and float(r.deltas[q]) == float(dl[n, k])
        for k in range(int(ne[n]), s.Ns):
            assert not bool(r.valid[k * s.n_alive + n])
    assert not torch.equal(s.alive.long(), torch.arange(s.n_alive))


@pytest.mark.parametrize("name", ["lane1", "lane15", "cascaded", "wave16", "wave64", "blocks16"])
def test_general_sets_hold_misses_zero_sample_and_full_rays(name):
    s, r = RR.march_set(name), RR.march_set_ref(name)
    assert RR.iteration_rule(s.n_rays, s.n_alive, 0, 1 << 40, s.min_samples) == s.Ns
    assert bool((r.n_eff[s.tags["miss"]] == 0).all()) and bool((r.n_eff[s.tags["t0_ge_t2"]] == 0).all())
    assert bool((s.ht[s.alive.long()[s.tags["miss"]]] == -1).all())
    hit = torch.ones(s.n_alive, dtype=torch.bool)
    hit[s.tags["miss"] + s.tags["t0_ge_t2"]] = False
    if name == "blocks16":  # most rays cross the box and meet nothing
        assert int(((r.n_eff == 0) & hit).sum()) > s.n_alive // 4 and int((r.n_eff > 0).sum()) > 20
    elif name == "cascaded":
        assert int((r.n_eff == s.Ns).sum()) > 20 and int((r.n_eff > 0).sum()) > s.n_alive // 2
    else:
        assert int((r.n_eff == s.Ns).sum()) > s.n_alive // 2
    if name not in ("lane1", "blocks16", "cascaded"):  # rays that run out of box before N_samples
        short = r.n_eff[s.tags["short"]]
        assert int(((short > 0) & (short < s.Ns)).sum()) >= 3
    assert s.n_alive % RR.BLOCK and s.n_alive > RR.BLOCK  # more than one block, a partial last one
    # which march mode the launch takes
    simple = s.cfg["cascades"] == 1 and s.cfg["esf"] == 0
    assert (simple and s.Ns >= RR.WAVE_NS) == (name in ("wave16", "wave64", "blocks16"))
    if name == "cascaded":  # the plain rule alone would reach the wave mode's N_samples
        assert s.Ns >= RR.WAVE_NS and not simple
        assert float(r.deltas[r.valid].max()) > 2 * float(r.deltas[r.valid].min())  # dt is not a constant here


@pytest.mark.parametrize("name", ["dense16", "dense64"])
def test_dense_sets_truncate_by_room_and_continue(name):
    s, r0, r1 = RR.march_set(name), RR.march_set_ref(name, 0), RR.march_set_ref(name, 1)
    assert bool((r0.n_eff == s.Ns).all())  # every ray stopped by N_samples with occupied points left:
    assert bool((r1.n_eff == s.Ns).all())  # the next march emits again
    # and it continues exactly one step behind the last emitted sample
    last = r0.ts[(s.Ns - 1) * s.n_alive:][:s.n_alive]
    assert torch.equal(r1.ts[:s.n_alive], last + torch.tensor(RR.DT, dtype=torch.float32))
    assert torch.equal(r0.hits_t[s.alive.long(), 0], r1.ts[:s.n_alive])


def test_fallback_ray_needs_more_binades_than_the_table_holds():
    s, r = RR.march_set("fallback16"), RR.march_set_ref("fallback16")
    (i,) = s.tags["far"]
    t0, t2 = (float(v) for v in s.ht[int(s.alive[i])])
    assert t0 == float(np.float32(1e-12)) and t2 == RR.FAR_T2
    # the walk's first step lands at dt; every binade from dt's to t2's holds lattice points
    assert math.frexp(t2)[1] - math.frexp(float(np.float32(RR.DT)))[1] > RR.LSEG
    assert int(r.n_eff[i]) == s.Ns  # (the serial walk itself stops after N_samples points)
    assert s.Ns >= RR.WAVE_NS


def test_degenerate_ray_cannot_advance():
    s, r = RR.march_set("degenerate16"), RR.march_set_ref("degenerate16")
    (i,) = s.tags["degenerate"]
    t0, t2 = s.ht[int(s.alive[i])]
    dt = torch.tensor(RR.DT, dtype=torch.float32)
    assert float(t0) < float(t2) and float(t0 + dt) == float(t0)  # dt below half an ulp of t0
    assert s.skip == (i,) and int(r.n_eff[i]) == 0
    assert int((r.n_eff[s.tags["through"]] > 0).sum()) > 20  # other rays of the launch do meet the occupied cell


@pytest.mark.parametrize("name", ["zero16", "zero64"])
def test_zero_sets_start_below_every_binade(name):
    s, r = RR.march_set(name), RR.march_set_ref(name)
    ids = s.alive.long()
    assert bool((s.ht[ids[s.tags["zero"]], 0] == 0).all())
    sub = s.ht[ids[s.tags["subnormal"]], 0]
    assert bool((sub > 0).all()) and bool((sub == 2.0 ** -149).all())
    assert int((r.n_eff[s.tags["zero"]] == s.Ns).sum()) > 10
    if name == "zero16":
        # the serial lattice from 0 is not fl(k dt): they part within N_samples points
        n = s.tags["zero"][0]
        ts = r.ts[n::s.n_alive][:s.Ns].numpy()
        closed = (np.arange(s.Ns, dtype=np.float32) * np.float32(RR.DT)).astype(np.float32)
        assert ts[0] == 0 and ts[1] == np.float32(RR.DT) and (ts != closed).any()


@pytest.mark.parametrize("name", ["wave16", "wave64", "zero64", "blocks16", "zero16"])
def test_wave_sets_cross_lattice_segments(name):
    """the wave mode walks a window on one register-held segment: the sets hold windows that straddle a segment's end
    and jumps that leave it (zero16's rays cross a dense grid: no jumps there)"""
    s, r = RR.march_set(name), RR.march_set_ref(name)
    assert s.cfg["cascades"] == 1 and s.cfg["esf"] == 0 and s.Ns >= RR.WAVE_NS  # the launch takes the wave mode
    straddle, leave = RR.segment_crossings([r.ts[n::s.n_alive][:int(r.n_eff[n])].numpy() for n in range(s.n_alive)], RR.DT)
    print(f"{name}: {straddle} rays' samples span a power of two, {leave} rays jump out of a binade")
    assert straddle >= 1
    if name != "zero16":
        assert leave >= 1


def test_flush_sets_sit_on_both_sides_of_the_flush_level():
    level = RR.STAGE - RR.FLUSH_SLACK
    f, n = RR.march_set("flush"), RR.march_set("noflush")
    rf, rn = RR.march_set_ref("flush"), RR.march_set_ref("noflush")
    assert f.Ns == n.Ns == RR.NS_MAX and f.n_rays == RR.NS_MAX * f.n_alive and n.n_rays == RR.NS_MAX * n.n_alive
    assert RR.march_grid(f.n_rays) == RR.march_grid(n.n_rays) == RR.MARCH_BLOCKS
    assert bool((rf.n_eff == RR.NS_MAX).all()) and bool((rn.n_eff == RR.NS_MAX).all())
    pf, pn = RR.staged_peak(rf.n_eff, f.n_rays), RR.staged_peak(rn.n_eff, n.n_rays)
    assert int(pf.max()) > level and int((pf > level).sum()) == 2  # blocks 0 and 1 take the extra trip
    assert int(pf.max()) <= RR.STAGE                               # ... and fill the stage to no more than its size
    assert int(pn.max()) == level                                  # the twin stops exactly at the level
    assert f.n_alive - n.n_alive == 5


def test_flush2_needs_the_flush_at_exactly_its_level():
    level = RR.STAGE - RR.FLUSH_SLACK
    s, r = RR.march_set("flush2"), RR.march_set_ref("flush2")
    run = RR.staged_running(r.n_eff, s.n_rays)[:, 0]  # block 0, trip by trip
    k = RR.flush_trips(s.Ns) - 1
    assert run.numel() == k + 2 and int(run[k - 1]) == level  # at the level: no flush yet
    assert level < int(run[k]) <= level + 2                   # over it by the short ray's 1-2 samples: flush here,
    assert int(run[k + 1] - run[k]) == RR.WAVE_RAYS * s.Ns    # since the next trip is a full one
    assert int(run[k + 1]) > RR.STAGE                         # and would not fit the stage behind it
    assert int(r.n_eff[s.tags["short"][0]]) in (1, 2) and bool((r.n_eff[s.tags["miss"]] == 0).all())


def test_lane_second_trip_set():
    s, r = RR.march_set("lane2trips"), RR.march_set_ref("lane2trips")
    assert s.Ns == 1 and s.n_rays == s.n_alive
    assert s.n_alive > RR.march_grid(s.n_rays) * RR.BLOCK and s.n_alive % RR.BLOCK
    assert bool((r.n_eff == 1).all())


@pytest.mark.parametrize("shape", sorted(RR.COMPOSITE_SHAPES))
def test_composite_sets(shape):
    n_alive, Ns, n_rays = RR.COMPOSITE_SHAPES[shape]
    s, ref = RR.composite_set(n_alive, Ns, n_rays, 3), RR.composite_set_ref(n_alive, Ns, n_rays, 3)
    # no ray inside the termination margin (0 rays excluded)
    bad, _ = CR.margin_violations(RR.ray_major(s.sig, n_alive, Ns).reshape(-1),
                                  RR.ray_major(s.deltas, n_alive, Ns).reshape(-1), s.rays_a, s.T_thr, s.T0)
    assert int(bad.sum()) == 0
    f = ref.f
    term = f.K < f.N
    assert int((s.n_eff == 0).sum()) > 0 and int((term & (f.K == 0)).sum()) > 0
    assert int((term & (f.K == f.N - 1) & (f.N > 1)).sum()) > 0 and int((~term & (f.N > 0)).sum()) > 0
    assert float(s.op0[s.alive.long()].min()) >= 0 and float(s.op0[s.alive.long()].max()) > 0.5
    survivors = int((ref.alive >= 0).sum())
    assert 0 < survivors < n_alive
    # which path the launch takes
    threads = RR.composite_grid(n_rays) * RR.BLOCK
    if shape == "thread":
        assert n_alive <= threads and RR.composite_rpt(n_alive, n_rays) == 1
    else:
        assert RR.composite_rpt(n_alive, n_rays) == RR.CRPT and n_alive % RR.BLOCK and n_alive % (RR.BLOCK * RR.CRPT)
        assert (n_alive > threads * RR.CRPT) == (shape == "pass2")
    assert not torch.equal(s.alive.long(), torch.arange(n_alive)) and s.n_buf > n_alive


def test_loop_reference_runs_both_modes_and_parities():
    ref = RR.loop_ref()
    ns = [it.Ns for it in ref.iters]
    assert ref.n_iters >= 4 and min(ns) < RR.WAVE_NS <= max(ns)
    assert ref.iters[0].n_alive == RR.LOOP["n_rays"] and ns[0] == 1
    alive = [it.n_alive for it in ref.iters]
    assert all(a > b for a, b in zip(alive, alive[1:]))
    assert ref.total_samples == ref.iters[-1].total_samples == sum(int(it.n_eff.sum()) for it in ref.iters)
    op = ref.opacity
    assert int((op == 0).sum()) > 100 and int((op > 0.99).sum()) > 1000 and bool(((op == 0) | (op > 0.99)).all())
    assert bool((ref.b_op[op == 0] == 0).all())
