"""The training march (csrc/march.hip) on the designed sets of march_ref.py, each
entry point called on its own: ngp_bitfield_summary word for word against
summary_ref; ngp_march_train_slots (the wave-per-ray lattice walk, or the
16-rays-per-wave walk of a cascaded grid) with the kernel's summary, without one
and with summary_ref's words uploaded, then ngp_march_train_compact; and the
two-pass path ngp_march_train_count / ngp_march_train_write -- all bit for bit
against the oracle's serial walk (floats compared as int32: -0.0 != 0.0).

Every output buffer is filled with junk and padded first, so memory a kernel must
not touch is visible.  test_march_ref_cpu.py shows that every designed set
contains what it is for."""
import types

import numpy as np
import pytest
import torch

import march_ref as MR
import vren

pytestmark = pytest.mark.gpu
DEV = "cuda"
JUNK_F = -7.25
JUNK_I = -77
PAD = 64  # junk entries behind every buffer's used part

SETS = [("sparse",), ("sparse_quarter",), ("sparse_wide",)] \
    + [("room", ms, n) for ms in MR.ROOM_MAX_SAMPLES for n in MR.ROOM_N_RAYS] \
    + [("scan", n) for n in MR.SCAN_N_RAYS] + [("cascaded", n) for n in MR.CASCADED_N_RAYS]
_id = lambda key: "-".join(str(k) for k in key)  # noqa: E731


def _junk(n, *shape, dtype=torch.float32):
    return torch.full((n + PAD,) + shape, JUNK_I if dtype != torch.float32 else JUNK_F, dtype=dtype, device=DEV)


def _bits(t):
    t = t.cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    """bit for bit (-0.0 != 0.0, junk included)"""
    return torch.equal(_bits(a), _bits(b))


def _is_junk(t):
    return bool((t == (JUNK_F if t.dtype == torch.float32 else JUNK_I)).all())


@pytest.fixture(scope="module")
def on_device():
    """device copies of a designed set, its kernel-made summary and summary_ref's words (made once per module)"""
    cache = {}

    def get(key):
        if key not in cache:
            s = MR.march_set(*key)
            c = s.cfg
            bkey = ("bf", s.name)
            if bkey not in cache:
                bf = s.bf.to(DEV)
                cache[bkey] = (bf, vren.bitfield_summary(bf, c["grid"]),
                               MR.summary_words(s.bf, c["grid"], c["cascades"]).to(DEV))
            bf, summ, summ_ref = cache[bkey]
            cache[key] = types.SimpleNamespace(o=s.o.to(DEV), d=s.d.to(DEV), ht=s.ht.to(DEV), noise=s.noise.to(DEV), bf=bf,
                                               summaries={"kernel": summ, "none": None, "reference": summ_ref})
        return cache[key]
    return get


def _cfg_args(c):
    return c["cascades"], c["grid"], c["scale"], c["esf"]


def _slots(s, D, summary):
    """ngp_march_train_slots into junk-filled, padded buffers"""
    n, ms = s.n_rays, s.cfg["max_samples"]
    out = types.SimpleNamespace(counts=_junk(n, dtype=torch.int32), rays_a=_junk(n, 3, dtype=torch.int64),
                                total=_junk(1, dtype=torch.int64), slot_t=_junk(n * ms), slot_dt=_junk(n * ms))
    vren._ok(vren.lib().ngp_march_train_slots(D.o, D.d, D.ht, n, D.bf, *_cfg_args(s.cfg), D.noise, ms, out.counts,
                                              out.rays_a, out.total, out.slot_t, out.slot_dt, summary, vren._stream()),
             "march_train_slots")
    torch.cuda.synchronize()
    return out


def _check_scan(out, ref, n):
    """counts, rays_a, total equal the oracle's; everything past n_rays keeps its junk"""
    assert torch.equal(out.counts[:n].cpu(), ref.counts) and _is_junk(out.counts[n:])
    assert torch.equal(out.rays_a[:n].cpu(), ref.rays_a) and _is_junk(out.rays_a[n:])
    assert int(out.total[0]) == ref.total and _is_junk(out.total[1:])


def _check_slots(out, ref, s):
    """slot_t / slot_dt [r, :count] hold the walk's t / dt; slots at and past each ray's count, and everything past
    n_rays, keep their junk"""
    n, ms = s.n_rays, s.cfg["max_samples"]
    _check_scan(out, ref, n)
    emitted = torch.arange(ms)[None, :] < ref.counts[:, None]
    for got, val, what in ((out.slot_t, ref.ts, "slot_t"), (out.slot_dt, ref.deltas, "slot_dt")):
        exp = torch.full((n * ms + PAD,), JUNK_F)
        exp[:n * ms].view(n, ms)[emitted] = val  # (ray-ordered, like the oracle's outputs)
        assert _same(got, exp), what


def _compact(s, D, out, total):
    res = [_junk(total, 3), _junk(total, 3), _junk(total), _junk(total)]
    vren._ok(vren.lib().ngp_march_train_compact(D.o, D.d, out.rays_a, s.n_rays, out.slot_t, out.slot_dt,
                                                s.cfg["max_samples"], *res, vren._stream()), "march_train_compact")
    torch.cuda.synchronize()
    return res


def _check_samples(res, ref):
    """xyzs, dirs, deltas, ts equal the oracle's bit for bit; the padding behind `total` is untouched"""
    for got, val, what in zip(res, (ref.xyzs, ref.dirs, ref.deltas, ref.ts), ("xyzs", "dirs", "deltas", "ts")):
        assert _same(got[:ref.total], val), what
        assert got.shape[0] == ref.total + PAD and _is_junk(got[ref.total:]), what


def _two_pass(s, D):
    """vren.march_train_count, then march_train_write into junk-filled buffers of capacity total + padding"""
    args = (D.o, D.d, D.ht, D.bf, s.cfg["cascades"], s.cfg["scale"], s.cfg["esf"], D.noise, s.cfg["grid"],
            s.cfg["max_samples"])
    counts, rays_a, total = vren.march_train_count(*args)
    N = int(total.item())
    res = [_junk(N, 3), _junk(N, 3), _junk(N), _junk(N)]
    vren.march_train_write(*args, rays_a, *res)
    torch.cuda.synchronize()
    return types.SimpleNamespace(counts=counts, rays_a=rays_a, total=N), res


# ------------------------------------------------------------------ summary
def _summary_cases(grid, cascades):
    """name -> bitfield: one bit in a corner, an edge, a face and an interior block (each in another cascade, the
    last one included), the last word only, all zero, 1 % random bits, 1 % random blocks"""
    side, G3 = grid // 4, grid ** 3
    h = side // 2
    cases = {}
    for k, (name, blocks) in enumerate([("corner", [(0, 0, 0), (side - 1,) * 3]), ("edge", [(0, 0, h), (side - 1, h, 0)]),
                                        ("face", [(0, h, h), (h, side - 1, h)]), ("interior", [(h, h, h)])]):
        cells = [((cascades - 1 - k - i) % cascades, 4 * b[0] + (k + i) % 4, 4 * b[1] + 3 - i, 4 * b[2] + k)
                 for i, b in enumerate(blocks)]
        cases[name] = MR.cells_bitfield(cells, grid, cascades)
    last = torch.zeros(cascades * G3 // 8, dtype=torch.uint8)
    last[-3] = 0x10
    cases["last_word"] = last
    cases["zero"] = torch.zeros_like(last)
    g = torch.Generator().manual_seed(grid + cascades)
    bits = (torch.rand(cascades * G3, generator=g) < 0.01).to(torch.uint8)
    cases["rand0.01"] = (bits.view(-1, 8) << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8)
    # (at 1 % of the cells half the blocks of a 128^3 grid are occupied and the dilation is all ones: also 1 % of the
    # blocks, one cell each)
    words = torch.nonzero(torch.rand(cascades * G3 // 64, generator=g) < 0.01)[:, 0]
    few = torch.zeros_like(last)
    few[words * 8 + torch.randint(0, 8, words.shape, generator=g)] = 0x20
    cases["blocks0.01"] = few
    return cases


@pytest.mark.parametrize("grid,cascades", [(4, 64), (8, 1), (8, 8), (16, 1), (16, 2), (128, 1), (128, 3)])
def test_bitfield_summary_word_for_word(grid, cascades):
    """Both halves against summary_ref on single bits in corner / edge / face / interior blocks, the last word, an
    empty and two random bitfields.  (4, 64): one block per cascade, the dilation must not cross cascades; (8, 1): 8
    words, no block geometry -- every dilated bit below n_words set.  Exactly 2 x ((n_words + 31) // 32) words are
    written; the same bitfield at an 8-byte (not 256-byte) aligned address gives the same words; a second call
    overwrites the first one's result completely."""
    lib = vren.lib()
    n_bytes = cascades * grid ** 3 // 8
    n32 = 2 * ((n_bytes // 8 + 31) // 32)
    assert MR.summary_dilates(n_bytes // 8, grid) == ((grid, cascades) != (8, 1))
    out = _junk(n32, dtype=torch.int32)
    shifted = torch.zeros(n_bytes + 264, dtype=torch.uint8, device=DEV)
    view = shifted[8:8 + n_bytes]
    assert view.data_ptr() % 8 == 0 and view.data_ptr() % 256 != 0
    prev = None
    for name, bf in _summary_cases(grid, cascades).items():
        want = MR.summary_words(bf, grid, cascades)
        assert want.numel() == n32
        dbf = bf.to(DEV)
        if prev is None:
            assert _is_junk(out)
        else:  # the buffer still holds the previous bitfield's words: none of them may survive
            assert torch.equal(out[:n32].cpu(), prev)
        vren._ok(lib.ngp_bitfield_summary(dbf, n_bytes, grid, out, vren._stream()), "bitfield_summary")
        got = out.cpu()
        half = n32 // 2
        assert torch.equal(got[:half], want[:half]), f"{name}: summary half"
        assert torch.equal(got[half:n32], want[half:]), f"{name}: dilated half"
        assert _is_junk(got[n32:]), f"{name}: written past 2 x ((n_words + 31) // 32) words"
        view.copy_(dbf)
        out2 = _junk(n32, dtype=torch.int32)
        vren._ok(lib.ngp_bitfield_summary(view, n_bytes, grid, out2, vren._stream()), "bitfield_summary")
        assert torch.equal(out2.cpu(), got), f"{name}: offset view"
        prev = want
    assert torch.equal(vren.bitfield_summary(dbf, grid).cpu(), want)  # the wrapper's own allocation: the same size


# --------------------------------------------------------------- slot march
@pytest.mark.parametrize("key", SETS, ids=_id)
def test_slot_march_three_ways_bit_for_bit(key, on_device):
    """ngp_march_train_slots with the kernel's summary, with occ_summary = NULL and with summary_ref's words: counts,
    rays_a, total and the emitted slots equal the oracle's raymarching_train bit for bit, every other slot and the
    padding keep their junk; ngp_march_train_compact then gives the oracle's xyzs / dirs / deltas / ts."""
    s, ref, D = MR.march_set(*key), MR.march_set_ref(*key), on_device(key)
    for how, summary in D.summaries.items():
        out = _slots(s, D, summary)
        try:
            _check_slots(out, ref, s)
            _check_samples(_compact(s, D, out, ref.total), ref)
        except AssertionError as e:
            raise AssertionError(f"summary: {how}") from e


def test_early_out_classes_on_the_device(on_device):
    """On `sparse`, per class and for each of the three runs: the rays the model's early out ends have count 0, the
    rays only the dilation keeps (no early-out point in an occupied block) have the oracle's count -- an under-set
    dilated bit, a step not divided by |d| or an early out reading the plain summary drops exactly these --, marched
    rays that meet nothing have 0, and rays with 1 or 2 samples have them."""
    key = ("sparse",)
    s, ref, D, c = MR.march_set(*key), MR.march_set_ref(*key), on_device(key), MR.sparse_classes("sparse")
    want = ref.counts.numpy()
    for how, summary in D.summaries.items():
        got = _slots(s, D, summary).counts[:s.n_rays].cpu().numpy()
        assert not got[c.skipped].any(), f"{how}: a skipped ray emits"
        for k, dn in enumerate(MR.D_CLASSES):
            m = c.dilation_only & (s.dclass == k)
            assert m.sum() >= 3 and np.array_equal(got[m], want[m]), \
                f"{how}: dilation-only rays, |d| = {dn}: lost {int((got[m] < want[m]).sum())} of {int(m.sum())}"
        assert not got[c.marched_empty].any(), f"{how}: marched, nothing to meet"
        assert np.array_equal(got[c.few], want[c.few]), f"{how}: rays with 1 or 2 samples"
        for name in ("clamped", "second_window"):
            m = getattr(c, name)
            assert np.array_equal(got[m], want[m]), f"{how}: {name}"


# ----------------------------------------------------------------- two pass
@pytest.mark.parametrize("key", [k for k in SETS if k[0] in ("sparse", "scan", "cascaded")]
                         + [("scan", MR.SCAN_TILE_N_RAYS)], ids=_id)
def test_two_pass_path_bit_for_bit(key, on_device):
    """vren.march_train_count / march_train_write (march_count_kernel, scan_rays_kernel, march_write_kernel; both
    template instantiations over the sets): counts, rays_a, total and the four outputs equal the oracle's and the
    slot path's bit for bit, with and without the summary on the slot side; the padding is untouched.  The starts
    in rays_a are the exclusive cumsum of the counts (SCAN_TILE_N_RAYS: across the block scan's tile carry)."""
    s, ref, D = MR.march_set(*key), MR.march_set_ref(*key), on_device(key)
    scan, res = _two_pass(s, D)
    assert torch.equal(scan.counts.cpu(), ref.counts) and torch.equal(scan.rays_a.cpu(), ref.rays_a)
    cnt = scan.counts.cpu().long()
    assert torch.equal(scan.rays_a[:, 1].cpu(), torch.cumsum(cnt, 0) - cnt) and scan.total == int(cnt.sum())
    assert scan.total == ref.total
    _check_samples(res, ref)
    for how in ("kernel", "none"):
        out = _slots(s, D, D.summaries[how])
        assert torch.equal(out.counts[:s.n_rays], scan.counts) and torch.equal(out.rays_a[:s.n_rays], scan.rays_a), how
        for a, b in zip(_compact(s, D, out, ref.total), res):
            assert _same(a, b), how


@pytest.mark.parametrize("cascaded", [False, True])
def test_two_pass_path_with_no_rays(cascaded, on_device):
    """n_rays = 0: total 0, nothing else written (either instantiation)"""
    key = ("cascaded", 1) if cascaded else ("room", 64, 1)
    s, D = MR.march_set(*key), on_device(key)
    lib, c = vren.lib(), s.cfg
    counts, rays_a, total = _junk(0, dtype=torch.int32), _junk(0, 3, dtype=torch.int64), _junk(1, dtype=torch.int64)
    vren._ok(lib.ngp_march_train_count(None, None, None, 0, D.bf, *_cfg_args(c), None, c["max_samples"], counts, rays_a,
                                       total, vren._stream()), "march_train_count")
    assert int(total[0]) == 0 and _is_junk(total[1:]) and _is_junk(counts) and _is_junk(rays_a)
    res = [_junk(0, 3), _junk(0, 3), _junk(0), _junk(0)]
    vren._ok(lib.ngp_march_train_write(None, None, None, 0, D.bf, *_cfg_args(c), None, c["max_samples"], rays_a, *res,
                                       vren._stream()), "march_train_write")
    torch.cuda.synchronize()
    assert all(_is_junk(b) for b in res) and _is_junk(rays_a)
