"""The device render loop's kernels (csrc/render.hip), each called on its own
through the C ABI with hand-built state, against the per-ray CPU reference of
render_ref.py: ngp_render_test_begin / _march / _composite / _finish.

The state words are written by the test, the alive list is a shuffled subset
of the ray ids (ray id != list position), and every output buffer is filled
with junk first, so memory a kernel must not touch is visible.  The march is
compared bit for bit (positions, directions, steps, t, counts, hits_t, the
sample list as a set), the composite within composite_ref.py's bound of
composite_test_fw and bit for bit with ngp_composite_test_fw, the survivor set
exactly.  The sizes at which a launch takes another path (the wave mode's
mid-loop flush, the lane mode's second grid-stride trip, the composite's second
pass) come from render_ref.py's derivations of the kernels' constants.
test_render_ref_cpu.py shows that every designed set contains what it is for.
"""
import ctypes
import types

import pytest
import torch

import composite_ref as CR
import oracle as O
import render_ref as RR
import vren

pytestmark = pytest.mark.gpu
DEV = "cuda"
JUNK_F = -7.25
JUNK_I = -77
PAD = 64  # junk entries behind every buffer's used part
BIG = 1 << 40


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _junk(n, *shape, dtype=torch.float32):
    return torch.full((n + PAD,) + shape, JUNK_I if dtype != torch.float32 else JUNK_F, dtype=dtype, device=DEV)


def _bits(t):
    t = t.cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    """bit for bit (-0.0 != 0.0, junk included)"""
    return torch.equal(_bits(a), _bits(b))


def _state(**words):
    st = torch.zeros(RR.STATE_WORDS, dtype=torch.int64)
    for k, v in words.items():
        st[getattr(RR, "RS_" + k)] = v
    return st


@pytest.fixture(scope="module")
def bitfields():
    cache = {}

    def get(kind, cascades=1, grid=128):
        key = (kind, cascades, grid)
        if key not in cache:
            bf = RR.bitfield(kind, cascades, grid).to(DEV)
            cache[key] = (bf, vren.bitfield_summary(bf, grid))
        return cache[key]
    return get


class Launch:
    """One hand-built iteration: device copies of a designed set's rays, a state and junk-filled outputs."""

    def __init__(self, s, ht, state, parity, bf, summary, Ns=None):
        c = s.cfg
        self.s, self.parity, self.cfg = s, parity, c
        self.o, self.d, self.ht = s.o.to(DEV), s.d.to(DEV), ht.to(DEV).contiguous()
        self.ht0 = ht.clone()
        self.state0 = state.clone()
        self.state = state.to(DEV)
        self.alive = torch.cat([s.alive.to(DEV), _junk(0, dtype=torch.int32)])
        self.bf, self.summary = bf, summary
        self.cap = (s.Ns if Ns is None else Ns) * s.n_alive
        self.xyzs, self.dirs = _junk(self.cap, 3), _junk(self.cap, 3)
        self.deltas, self.ts = _junk(self.cap), _junk(self.cap)
        self.n_eff = _junk(s.n_alive, dtype=torch.int32)
        self.sample_idx = _junk(self.cap, dtype=torch.int32)

    def march(self, n_rays=None, min_samples=None, budget=BIG):
        s, c = self.s, self.cfg
        vren._ok(vren.lib().ngp_render_test_march(
            _p(self.o), _p(self.d), _p(self.ht), s.n_rays if n_rays is None else n_rays, _p(self.bf), c["cascades"],
            c["grid"], ctypes.c_float(c["scale"]), ctypes.c_float(c["esf"]), c["max_samples"],
            s.min_samples if min_samples is None else min_samples, budget, self.parity, _p(self.state), _p(self.alive),
            _p(self.summary), _p(self.xyzs), _p(self.dirs), _p(self.deltas), _p(self.ts), _p(self.n_eff),
            _p(self.sample_idx), vren._stream()), "render_test_march")
        torch.cuda.synchronize()
        return self

    def untouched(self):
        """every output still junk, hits_t as given"""
        return all(bool((b == (JUNK_F if b.dtype == torch.float32 else JUNK_I)).all())
                   for b in (self.xyzs, self.dirs, self.deltas, self.ts, self.n_eff, self.sample_idx)) \
            and _same(self.ht, self.ht0)


def _check_march(L, ref, samples0=0, iters0=0, total0=0):
    """the launch's outputs against march_ref: values bit for bit in their slots, everything else as it was"""
    s, n, Ns = L.s, L.s.n_alive, ref.Ns
    assert L.cap == Ns * n
    st = L.state.cpu()
    want = L.state0.clone()
    want[RR.RS_NS], want[RR.RS_SAMPLES], want[RR.RS_ITERS] = Ns, samples0 + Ns, iters0 + 1
    want[L.parity ^ 1], want[RR.RS_VALID] = 0, int(ref.n_eff.sum())
    assert st.tolist() == want.tolist()
    assert torch.equal(L.n_eff[:n].cpu(), ref.n_eff) and bool((L.n_eff[n:] == JUNK_I).all())
    assert _same(L.ht, ref.hits_t)  # listed rays advanced exactly, every other ray unchanged
    for name in ("xyzs", "dirs", "deltas", "ts"):
        got, val = getattr(L, name).cpu(), getattr(ref, name)
        exp = torch.full_like(got, JUNK_F)
        exp[:L.cap][ref.valid] = val[ref.valid]
        assert _same(got, exp), name  # valid slots hold the walk's values, all other slots their junk
    nv = int(ref.n_eff.sum())
    idx = L.sample_idx.cpu()
    assert torch.equal(torch.sort(idx[:nv].long()).values, torch.nonzero(ref.valid)[:, 0])  # a permutation
    assert bool((idx[nv:] == JUNK_I).all())
    assert torch.equal(L.alive[:n].cpu(), s.alive)


def _launch(name, bitfields, parity=0, summary=True, iteration=0, **state):
    s = RR.march_set(name)
    bf, summ = bitfields(s.bf_kind, s.cfg["cascades"], s.cfg["grid"])
    ht = s.ht if iteration == 0 else RR.march_set_ref(name, iteration - 1).hits_t
    words = dict(ACTIVE=1, SAMPLES=5, ITERS=3, TOTAL=11, NS=99, VALID=12345)
    words.update(state)
    st = _state(**words)
    st[parity], st[parity ^ 1] = s.n_alive, 4321  # (the other list's length is zeroed by the iteration)
    return Launch(s, ht, st, parity, bf, summ if summary else None)


# ---------------------------------------------------------------------- begin
@pytest.mark.parametrize("n_rays", [0, 1, 7, 8, 9, 257])
def test_begin_writes_the_state_and_exactly_n_rays(n_rays):
    state = torch.full((RR.STATE_WORDS + PAD,), JUNK_I, dtype=torch.int64, device=DEV)
    alive0, op, dep, rgb = _junk(n_rays, dtype=torch.int32), _junk(n_rays), _junk(n_rays), _junk(n_rays, 3)
    vren._ok(vren.lib().ngp_render_test_begin(n_rays, _p(state), _p(alive0), _p(op), _p(dep), _p(rgb), vren._stream()),
             "render_test_begin")
    torch.cuda.synchronize()
    assert state[:RR.STATE_WORDS].tolist() == _state(ALIVE0=n_rays, ACTIVE=1).tolist()
    assert bool((state[RR.STATE_WORDS:] == JUNK_I).all())
    assert torch.equal(alive0[:n_rays].cpu(), torch.arange(n_rays, dtype=torch.int32))
    assert bool((alive0[n_rays:] == JUNK_I).all())
    for b in (op, dep, rgb):
        assert _same(b[:n_rays], torch.zeros_like(b[:n_rays])) and bool((b[n_rays:] == JUNK_F).all())


# ------------------------------------------------------------- iteration rule
@pytest.mark.parametrize("min_samples", [1, 4])
@pytest.mark.parametrize("quotient", [1, 15, 16, 17, 63, 64, 65, 200])
def test_iteration_rule_sets_n_samples_at_its_boundaries(quotient, min_samples, bitfields):
    """n_rays // n_alive at 1, around the wave mode's threshold and around the clamp, with and without a remainder
    and with a single alive ray: the whole march agrees with the reference run at the reference's N_samples (state
    words included)."""
    s0 = RR.march_set("dense16")
    for n_alive, rem, parity in ((5, 0, 0), (5, 4, 1), (1, 0, 1)):
        n_rays = quotient * n_alive + rem
        Ns = RR.iteration_rule(n_rays, n_alive, 7, BIG, min_samples)
        assert Ns == max(min(quotient, 64), min_samples)
        s = types.SimpleNamespace(**{**vars(s0), "alive": s0.alive[:n_alive].contiguous(), "n_alive": n_alive,
                                     "n_rays": n_rays, "min_samples": min_samples, "Ns": Ns})
        bf, summ = bitfields("dense")
        st = _state(ACTIVE=1, SAMPLES=7, ITERS=2, TOTAL=9, NS=3, VALID=55)
        st[parity], st[parity ^ 1] = n_alive, 77
        L = Launch(s, s.ht, st, parity, bf, summ).march()
        c = s.cfg
        ref = RR.march_ref(s.o, s.d, s.ht, s.alive, RR.bitfield("dense"), c["cascades"], c["scale"], c["esf"], c["grid"],
                           c["max_samples"], Ns)
        _check_march(L, ref, samples0=7, iters0=2)


@pytest.mark.parametrize("why", ["budget", "no_rays_alive", "n_rays_0"])
def test_the_loop_stops_and_later_launches_do_nothing(why, bitfields):
    """samples == budget stops the loop, budget - 1 does not; so does an empty alive list.  After the stop the
    state is inactive and a further march + composite leave every buffer and hits_t untouched."""
    s = RR.march_set("dense16")
    bf, summ = bitfields("dense")
    budget = 1000
    if why == "budget":  # just below the budget: the iteration runs
        st = _state(ACTIVE=1, SAMPLES=budget - 1, ITERS=4, TOTAL=6)
        st[0], st[1] = s.n_alive, 9
        L = Launch(s, s.ht, st, 0, bf, summ).march(budget=budget)
        _check_march(L, RR.march_set_ref("dense16"), samples0=budget - 1, iters0=4)
    st = _state(ACTIVE=1, SAMPLES=budget if why == "budget" else 0, ITERS=4, TOTAL=6, NS=9, VALID=31)
    st[1], st[0] = (s.n_alive, 9) if why == "budget" else (0, 9)
    L = Launch(s, s.ht, st, 1, bf, summ)
    L.march(budget=budget, n_rays=0 if why == "n_rays_0" else None)
    want = st.clone()
    want[RR.RS_ACTIVE], want[RR.RS_VALID] = 0, 0  # nothing else moves: no iteration counted, no list length zeroed
    assert L.state.cpu().tolist() == want.tolist() and L.untouched()
    # the no-op iterations behind the stop (a captured graph replays them)
    n, cap = s.n_alive, L.cap
    sig, rgbs = _junk(cap), _junk(cap, 3)
    alive_out, op, dep, rgb = _junk(n, dtype=torch.int32), _junk(s.n_buf), _junk(s.n_buf), _junk(s.n_buf, 3)
    for parity in (0, 1, 0):
        L.parity = parity
        L.march(budget=budget)
        vren._ok(vren.lib().ngp_render_test_composite(
            _p(sig), _p(rgbs), _p(L.deltas), _p(L.ts), _p(L.n_eff), s.n_rays, parity, _p(L.state), _p(L.alive),
            _p(alive_out), ctypes.c_float(1e-4), _p(op), _p(dep), _p(rgb), vren._stream()), "render_test_composite")
    torch.cuda.synchronize()
    assert L.state.cpu().tolist() == want.tolist() and L.untouched()
    assert bool((alive_out == JUNK_I).all()) and all(bool((b == JUNK_F).all()) for b in (op, dep, rgb))


# ---------------------------------------------------------------------- march
@pytest.mark.parametrize("name,parity,summary", [
    ("lane1", 0, True), ("lane15", 1, True), ("lane15", 0, False), ("cascaded", 1, True),
    ("wave16", 0, True), ("wave64", 1, True), ("wave64", 0, False), ("blocks16", 0, True), ("blocks16", 1, False),
    ("dense16", 1, False), ("dense64", 0, True), ("fallback16", 0, True), ("fallback16", 1, False),
    ("zero16", 0, True), ("zero64", 1, True), ("zero64", 0, False)])
def test_march_matches_the_serial_walk_bit_for_bit(name, parity, summary, bitfields):
    """Lane-per-ray (N_samples 1 and 15; a cascaded exp-step grid whose N_samples alone would reach the wave mode)
    and wave-per-ray launches (exactly WAVE_NS and NS_MAX): rays that miss, t0 >= t2, empty neighbourhoods with and
    without the occupancy summary, rays cut by N_samples (then a second march from the updated hits_t, which
    continues where the serial walk does), a ray over more binades than the segment table holds, and rays that
    start at t0 == 0.0 or the smallest subnormal, below every binade."""
    L = _launch(name, bitfields, parity, summary).march()
    _check_march(L, RR.march_set_ref(name, 0), samples0=5, iters0=3)
    L2 = _launch(name, bitfields, parity ^ 1, summary, iteration=1).march()
    _check_march(L2, RR.march_set_ref(name, 1), samples0=5, iters0=3)


def test_march_ends_a_degenerate_ray_inside_a_wave_launch(bitfields):
    """dt below half an ulp of t0: the reference's walk would never end; the wave mode hands the ray to its serial
    fallback, which ends it with no sample and counts a guard hit (as the training march does,
    test_march_ends_a_degenerate_ray_instead_of_spinning); every other ray is marched as usual."""
    lib = vren.lib()
    assert lib.ngp_guard_reset() == 0
    try:
        L = _launch("degenerate16", bitfields, 0, True).march()
        assert int(lib.ngp_guard_hits()) >= 1
        ref = RR.march_set_ref("degenerate16")
        assert int(L.n_eff[0]) == 0 and int(ref.n_eff[0]) == 0
        _check_march(L, ref, samples0=5, iters0=3)
    finally:
        assert lib.ngp_guard_reset() == 0


@pytest.mark.parametrize("name", ["flush", "noflush", "flush2", "lane2trips"])
def test_march_list_is_exact_across_flushes_and_trips(name, bitfields):
    """flush / noflush: N_samples 64 and n_alive just over / at the size at which a block of the wave mode flushes
    its staged indices inside its loop (every ray emits 64 samples: the stage fills to its last entry); flush2: a
    block that crosses the flush level by one or two samples and then stages a full trip -- a flush any later than
    the kernel's would overrun the stage; lane2trips: the lane mode's second grid-stride trip through
    block_append's shared memory."""
    L = _launch(name, bitfields, 0, True).march()
    _check_march(L, RR.march_set_ref(name), samples0=5, iters0=3)


# ------------------------------------------------------------------ composite
@pytest.mark.parametrize("shape", sorted(RR.COMPOSITE_SHAPES))
def test_composite_values_survivors_and_bookkeeping(shape):
    n_alive, Ns, n_rays = RR.COMPOSITE_SHAPES[shape]
    s, ref = RR.composite_set(n_alive, Ns, n_rays, 3), RR.composite_set_ref(n_alive, Ns, n_rays, 3)
    D = lambda x: x.to(DEV).contiguous()  # noqa: E731
    for parity in ((0, 1) if shape != "pass2" else (1,)):
        st = _state(ACTIVE=1, SAMPLES=40, ITERS=3, TOTAL=1000, NS=Ns, VALID=17)
        st[parity], st[parity ^ 1] = n_alive, 0
        state = st.to(DEV)
        alive_in, alive_out = D(s.alive), _junk(n_alive, dtype=torch.int32)
        op, dep, rgb = D(s.op0), D(s.dep0), D(s.rgb0)
        sig, rgbs, deltas, ts, n_eff = D(s.sig), D(s.rgbs), D(s.deltas), D(s.ts), D(s.n_eff)
        vren._ok(vren.lib().ngp_render_test_composite(
            _p(sig), _p(rgbs), _p(deltas), _p(ts), _p(n_eff), n_rays, parity, _p(state), _p(alive_in), _p(alive_out),
            ctypes.c_float(s.T_thr), _p(op), _p(dep), _p(rgb), vren._stream()), "render_test_composite")
        torch.cuda.synchronize()
        # bookkeeping: the survivor count, the running total, nothing else
        keep = ref.alive[ref.alive >= 0]
        want = st.clone()
        want[parity ^ 1], want[RR.RS_TOTAL] = keep.numel(), 1000 + ref.n_eff_sum
        assert state.cpu().tolist() == want.tolist()
        out = alive_out.cpu()
        got = out[:keep.numel()].long()
        assert torch.equal(torch.sort(got).values, torch.sort(keep).values)  # the survivor set, exactly
        assert bool((out[keep.numel():] == JUNK_I).all()) and torch.equal(alive_in.cpu(), s.alive)
        # within a block's pass the survivors keep their alive-list order, each pass one contiguous run
        where = torch.full((s.n_buf,), -1, dtype=torch.int64)
        where[s.alive.long()] = torch.arange(n_alive)
        pos = where[got]
        chunk = pos // (RR.BLOCK * RR.composite_rpt(n_alive, n_rays))
        new_run = torch.ones_like(chunk, dtype=torch.bool)
        new_run[1:] = chunk[1:] != chunk[:-1]
        assert int(new_run.sum()) == torch.unique(chunk).numel()
        assert bool((pos[1:] > pos[:-1])[~new_run[1:]].all())
        # values: the fp64 reference within composite_test_fw's bound; a bound of 0 (unlisted rays, n_eff == 0) is exact
        ratios = {"op": CR.ratio((op.cpu().double() - ref.op).abs(), ref.b_op),
                  "dep": CR.ratio((dep.cpu().double() - ref.dep).abs(), ref.b_dep),
                  "rgb": CR.ratio((rgb.cpu().double() - ref.rgb).abs(), ref.b_rgb)}
        print(f"render composite {shape} parity {parity}: worst err / bound " +
              ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        assert all(v <= 1 for v in ratios.values()), ratios
        assert int((ref.b_op == 0).sum()) >= s.n_buf - n_alive + int((s.n_eff == 0).sum())
        # bit for bit with the reference-shaped composite_test_fw on the same inputs in its (n_alive, Ns) layout
        al2, op2, dep2, rgb2 = D(s.alive.long()), D(s.op0), D(s.dep0), D(s.rgb0)
        rm = lambda a: D(RR.ray_major(a, n_alive, Ns))  # noqa: E731
        vren.composite_test_fw(rm(s.sig), rm(s.rgbs), rm(s.deltas), rm(s.ts), None, al2, s.T_thr, n_eff, op2, dep2, rgb2)
        torch.cuda.synchronize()
        assert _same(op, op2) and _same(dep, dep2) and _same(rgb, rgb2)
        assert torch.equal(al2.cpu(), ref.alive)


# --------------------------------------------------------------------- finish
@pytest.mark.parametrize("n_rays", [0, 1, 257])
def test_finish_blends_the_background(n_rays):
    g = torch.Generator().manual_seed(n_rays)
    op = torch.rand(n_rays + PAD, generator=g)
    op[:1] = 1.0
    rgb = torch.rand(n_rays + PAD, 3, generator=g)
    bg = (0.9, 0.25, 0.6)
    rgb_d = rgb.to(DEV)
    vren._ok(vren.lib().ngp_render_test_finish(_p(op.to(DEV)), n_rays, (ctypes.c_float * 3)(*bg), _p(rgb_d),
                                               vren._stream()), "render_test_finish")
    torch.cuda.synchronize()
    want, bound = RR.finish_ref(op[:n_rays], rgb[:n_rays], bg)
    assert CR.ratio((rgb_d[:n_rays].cpu().double() - want).abs(), bound) <= 1
    assert _same(rgb_d[n_rays:], rgb[n_rays:])
    if n_rays:
        assert _same(rgb_d[0], rgb[0])  # opacity 1: the background adds exactly 0


# ----------------------------------------------------------------------- loop
def test_chained_loop_follows_the_reference_iteration_by_iteration(bitfields):
    """begin, then march / field / composite until the state goes inactive, with the sigmas of RR.field_bits computed
    from the kernels' own sample positions: per iteration the alive count, N_samples and the alive SET equal the
    reference loop's; at the end total_samples, the iteration count and the images (fp64 reference within
    composite_test_fw's bound; rays nothing opaque touched are exactly 0).  Both march modes and both list parities
    occur (test_render_ref_cpu.py)."""
    ref = RR.loop_ref()
    o, d, ht = RR.loop_inputs()
    n_rays, c, lib = o.shape[0], RR.SIMPLE, vren.lib()
    bf, summ = bitfields("dense")
    o, d, ht = o.to(DEV), d.to(DEV), ht.to(DEV).contiguous()
    state = torch.full((RR.STATE_WORDS,), JUNK_I, dtype=torch.int64, device=DEV)
    alive = [_junk(n_rays, dtype=torch.int32), _junk(n_rays, dtype=torch.int32)]
    op, dep, rgb = _junk(n_rays), _junk(n_rays), _junk(n_rays, 3)
    cap = int(lib.ngp_render_test_capacity(n_rays, 1))
    xyzs, dirs, deltas, ts = _junk(cap, 3), _junk(cap, 3), _junk(cap), _junk(cap)
    sig, rgbs = _junk(cap), _junk(cap, 3)
    n_eff, sample_idx = _junk(n_rays, dtype=torch.int32), _junk(cap, dtype=torch.int32)
    vren._ok(lib.ngp_render_test_begin(n_rays, _p(state), _p(alive[0]), _p(op), _p(dep), _p(rgb), vren._stream()), "begin")
    for k in range(ref.n_iters + 2):
        par = k & 1
        vren._ok(lib.ngp_render_test_march(
            _p(o), _p(d), _p(ht), n_rays, _p(bf), c["cascades"], c["grid"], ctypes.c_float(c["scale"]),
            ctypes.c_float(c["esf"]), c["max_samples"], 1, RR.LOOP["budget"], par, _p(state), _p(alive[par]), _p(summ),
            _p(xyzs), _p(dirs), _p(deltas), _p(ts), _p(n_eff), _p(sample_idx), vren._stream()), "march")
        st = state.cpu()
        if k >= ref.n_iters:
            assert int(st[RR.RS_ACTIVE]) == 0
            continue
        it = ref.iters[k]
        assert int(st[RR.RS_ACTIVE]) == 1 and int(st[par]) == it.n_alive and int(st[RR.RS_NS]) == it.Ns, k
        assert torch.equal(torch.sort(alive[par][:it.n_alive].cpu()).values, it.alive), k
        nv = int(st[RR.RS_VALID])
        assert nv == int(it.n_eff.sum())
        idx = sample_idx[:nv].long()
        sig[idx], rgbs[idx] = RR.field_bits(xyzs[idx])
        vren._ok(lib.ngp_render_test_composite(
            _p(sig), _p(rgbs), _p(deltas), _p(ts), _p(n_eff), n_rays, par, _p(state), _p(alive[par]),
            _p(alive[par ^ 1]), ctypes.c_float(RR.LOOP["T_thr"]), _p(op), _p(dep), _p(rgb), vren._stream()), "composite")
        assert int(state[RR.RS_TOTAL]) == it.total_samples, k
    st = state.cpu()
    assert int(st[RR.RS_ITERS]) == ref.n_iters and int(st[RR.RS_TOTAL]) == ref.total_samples
    assert _same(ht, ref.hits_t)
    ratios = {"op": CR.ratio((op[:n_rays].cpu().double() - ref.opacity).abs(), ref.b_op),
              "dep": CR.ratio((dep[:n_rays].cpu().double() - ref.depth).abs(), ref.b_dep),
              "rgb": CR.ratio((rgb[:n_rays].cpu().double() - ref.rgb).abs(), ref.b_rgb)}
    print("render loop: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1 for v in ratios.values()), ratios
    assert all(bool((b[n_rays:] == JUNK_F).all()) for b in (op, dep, rgb))


# ------------------------------------------------- t0 == 0, the training march
@pytest.mark.parametrize("occ", ["dense", "rand0.2"])
def test_march_train_from_t0_zero_bit_exact(occ):
    """hits_t[:, 0] == 0 with noise 0 (the C ABI and the vren drop-ins take any hits_t; the product's callers clamp to
    NEAR_DISTANCE): the training march's wave kernel starts its lattice at 0, below every binade, where the serial
    walk's fl(fl(..) + dt) is not fl(k dt).  256 rays from inside the box against the oracle, bit for bit."""
    o, d, ht = RR.box_rays(256, 17, 0.5, inside=True)
    ht[:, 0] = 0.0
    ht[1::4, 0] = 2.0 ** -149
    noise = torch.zeros(256)
    bf = RR.bitfield(occ)
    ref = O.raymarching_train(o, d, ht, bf, 1, 0.5, 0.0, noise, 128, 1024)
    out = vren.raymarching_train(o.to(DEV), d.to(DEV), ht.to(DEV), bf.to(DEV), 1, 0.5, 0.0, noise.to(DEV), 128, 1024)
    assert int(out[5][0]) == int(ref[5][0]) and int(ref[5][0]) > 256 * 20
    for a, b in zip(out[:5], ref[:5]):
        assert _same(a, b)
