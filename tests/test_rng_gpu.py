"""Every random draw of the device against its host model (tests/rng_ref.py),
bit for bit: the raw Philox-4x32-10 (published known answers included), the
batch draw, the random background, the counter increment, the occupancy draws
(unsorted and sorted) and the stream the trainer follows over 40 steps.

Every comparison is torch.equal / np.array_equal.  The sorted draw's cells
come from fp64 sums whose last places device and host need not share; its
equality is exact all the same because tests/test_rng_ref_cpu.py shows that no
sample of the inputs used here (rng_ref.SORTED_CASES) lies within 64 tau of a
cell boundary, tau bounding |device - model| (rng_ref's docstring)."""
import numpy as np
import pytest
import torch

import rng_ref as R
import synthetic as S
import vren
from trainer import NGPTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64  # junk-filled elements (rows) past every output: they keep their bits
JUNK32 = 0x5A5AA5A5


def _junk(n, dtype, cols=None, pad=PAD):
    """(n + pad [, cols]) of `dtype`, every 32-bit word JUNK32"""
    shape = (n + pad,) if cols is None else (n + pad, cols)
    words = torch.full((int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4,), JUNK32,
                       dtype=torch.int32, device=DEV)
    return words.view(dtype).view(shape)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64).cpu().numpy()


def _tail_untouched(t, n):
    return bool((t[n:].contiguous().view(torch.int32) == JUNK32).all())


def _f32bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------ the raw generator
def test_philox_equals_the_published_vectors_and_the_model():
    """ngp_philox4x32: the three Random123 known answers, then 4099 random
    (counter, key) rows (17 blocks, the last one of 3 rows): all 128 bits."""
    kat_c = [(0,) * 4, (0xffffffff,) * 4, (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)]
    kat_k = [(0,) * 2, (0xffffffff,) * 2, (0xa4093822, 0x299f31d0)]
    kat_o = [(0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd),
             (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)]
    g = np.random.default_rng(20)
    c = np.concatenate([np.array(kat_c, dtype=np.uint32), g.integers(0, 2 ** 32, (4099, 4), dtype=np.uint32)])
    k = np.concatenate([np.array(kat_k, dtype=np.uint32), g.integers(0, 2 ** 32, (4099, 2), dtype=np.uint32)])
    n = c.shape[0]
    out = _junk(n, torch.int32, 4)
    vren.kernels().ngp_philox4x32(torch.from_numpy(c.view(np.int32)).to(DEV), torch.from_numpy(k.view(np.int32)).to(DEV),
                                  n, out, vren._stream())
    got = out[:n].cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:3], np.array(kat_o, dtype=np.uint32))
    want = np.stack(R.philox4x32(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1]), -1).astype(np.uint32)
    assert np.array_equal(got, want)
    assert _tail_untouched(out, n)


# ------------------------------------------------------------------ the batch draw
N_IMG, HW, N_RAYS = 3, 35, 1000  # (four blocks of 256, the last one partial)
SEED_HI = 0xABCDEF0100000005  # a seed with a live high word


def _batch_scene(f32):
    g = torch.Generator().manual_seed(4)
    if f32:
        gt = torch.rand(N_IMG, HW, 3, generator=g)
    else:
        gt = torch.randint(0, 256, (N_IMG, HW, 3), dtype=torch.uint8, generator=g)
    dirs = torch.nn.functional.normalize(torch.randn(HW, 3, generator=g), dim=1)
    poses = torch.cat([torch.linalg.qr(torch.randn(N_IMG, 3, 3, generator=g))[0],
                       torch.randn(N_IMG, 3, 1, generator=g) * 0.3], 2).contiguous()
    return dict(gt=gt.to(DEV), dirs=dirs.to(DEV), poses=poses.to(DEV), center=torch.zeros(1, 3, device=DEV),
                half=torch.full((1, 3), 0.5, device=DEV))


def _draw_batch(sc, seed, step, offset, step_dev=None):
    o = dict(img=_junk(N_RAYS, torch.int64), pix=_junk(N_RAYS, torch.int64), rgb=_junk(N_RAYS, torch.float32, 3),
             noise=_junk(N_RAYS, torch.float32), o=_junk(N_RAYS, torch.float32, 3), d=_junk(N_RAYS, torch.float32, 3),
             ht=_junk(N_RAYS, torch.float32, 2))
    tail = (sc["gt"], int(sc["gt"].dtype == torch.float32), N_IMG, HW, sc["dirs"], sc["poses"], N_RAYS, sc["center"],
            sc["half"], 0.01, o["img"], o["pix"], o["rgb"], o["noise"], o["o"], o["d"], o["ht"], vren._stream())
    if step_dev is None:
        vren.kernels().ngp_sample_batch(seed, step, offset, *tail)
    else:
        vren.kernels().ngp_sample_batch_dev(seed, step_dev, step, offset, *tail)
    torch.cuda.synchronize()
    for name, t in o.items():
        assert _tail_untouched(t, N_RAYS), name
    return o


@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("seed,step,offset", [(SEED_HI, 1, 0), (SEED_HI, 2 ** 32 - 1, 0), (SEED_HI, 2 ** 32, 0),
                                              (5, 1, 2 ** 32 - 500)],
                         ids=["seed-high-word", "step-2^32-1", "step-2^32", "offset-crosses-2^32"])
def test_batch_draw_equals_the_model(seed, step, offset, f32):
    """ngp_sample_batch: img, pix, noise bit for bit; the ground truth is the
    gather at the model's indices, the rays those of the model's pixels."""
    sc = _batch_scene(f32)
    o = _draw_batch(sc, seed, step, offset)
    img, pix, noise = R.sample_batch(seed, step, offset, N_RAYS, N_IMG, HW)
    assert np.array_equal(o["img"][:N_RAYS].cpu().numpy(), img)
    assert np.array_equal(o["pix"][:N_RAYS].cpu().numpy(), pix)
    assert np.array_equal(_bits(o["noise"][:N_RAYS]), _f32bits(noise))
    ti, tp = torch.from_numpy(img).to(DEV), torch.from_numpy(pix).to(DEV)
    g = sc["gt"][ti, tp]
    if not f32:
        g = g.float()
        g = g / torch.full_like(g, 255.0)  # a true division (numpy's astype(float32) / 255)
    assert torch.equal(o["rgb"][:N_RAYS], g)
    ro, rd, ht = vren.raygen_aabb(sc["dirs"], sc["poses"], ti, tp, sc["center"], sc["half"], 0.01)
    assert torch.equal(o["o"][:N_RAYS], ro) and torch.equal(o["d"][:N_RAYS], rd) and torch.equal(o["ht"][:N_RAYS], ht)


def test_batch_draw_step_words_are_not_aliased():
    """the draws at step 1, 2^32 and 2^32 + 1 differ (a dropped high step word would equate two)"""
    pix = [R.sample_batch(SEED_HI, s, 0, N_RAYS, N_IMG, HW)[1] for s in (1, 2 ** 32, 2 ** 32 + 1)]
    sc = _batch_scene(False)
    for s, want in zip((1, 2 ** 32, 2 ** 32 + 1), pix):
        assert np.array_equal(_draw_batch(sc, SEED_HI, s, 0)["pix"][:N_RAYS].cpu().numpy(), want)
    assert not any(np.array_equal(a, b) for i, a in enumerate(pix) for b in pix[i + 1:])


@pytest.mark.parametrize("c,a", [(0, 0), (41, 1), (2 ** 32 - 1, 1)])
def test_batch_draw_with_the_device_counter_is_the_host_step_draw(c, a):
    """ngp_sample_batch_dev at *step_dev = c, step_add = a: every output equals ngp_sample_batch's at c + a"""
    sc = _batch_scene(False)
    ctr = torch.tensor([c, -7], dtype=torch.int64, device=DEV)
    dev = _draw_batch(sc, SEED_HI, a, 24, step_dev=ctr)
    host = _draw_batch(sc, SEED_HI, c + a, 24)
    for name in host:
        assert np.array_equal(_bits(dev[name]), _bits(host[name])), name
    assert ctr.tolist() == [c, -7]
    assert np.array_equal(dev["pix"][:N_RAYS].cpu().numpy(), R.sample_batch(SEED_HI, c + a, 24, N_RAYS, N_IMG, HW)[1])


# ------------------------------------------------------------------ background, counters
@pytest.mark.parametrize("add", [0, 1])
@pytest.mark.parametrize("counter", [0, 5, 2 ** 32])
def test_random_background_equals_the_model(counter, add):
    ctr = torch.tensor([counter], dtype=torch.int64, device=DEV)
    bg = _junk(3, torch.float32, pad=1)
    vren.kernels().ngp_random_bg(SEED_HI ^ R.BG_KEY_XOR, ctr, add, bg, vren._stream())
    want = R.random_bg(SEED_HI ^ R.BG_KEY_XOR, counter + add)
    assert np.array_equal(_bits(bg[:3]), _f32bits(want))
    assert _tail_untouched(bg, 3) and int(ctr) == counter
    assert 0.0 <= float(want.min()) and float(want.max()) < 1.0


@pytest.mark.parametrize("n", [1, 3, 64])
def test_counters_inc_adds_one_to_the_first_n(n):
    base = torch.tensor([-1, 0, 2 ** 32 - 1, 2 ** 32, 2 ** 62, -2 ** 40, 17], dtype=torch.int64).repeat(10)[:65]
    c = base.to(DEV)
    for calls in (1, 2):
        vren.kernels().ngp_counters_inc(c, n, vren._stream())
        want = base.clone()
        want[:n] += calls
        assert torch.equal(c.cpu(), want)


# ------------------------------------------------------------------ occupancy draw, unsorted
def _occ_buffers(n):
    return _junk(n, torch.float32, 3), _junk(n, torch.int64)


def _check_occ(xyz, flat, n, want_flat, want_xyz, what):
    assert np.array_equal(flat[:n].cpu().numpy(), want_flat), what
    assert np.array_equal(_bits(xyz[:n]), _f32bits(want_xyz)), what
    assert _tail_untouched(xyz, n) and _tail_untouched(flat, n), what


@pytest.mark.parametrize("cascade", [0, 3])
@pytest.mark.parametrize("G", [16, 12])
def test_unsorted_occupancy_draw_equals_the_model(G, cascade):
    """ngp_occupancy_samples, M = 1000 (eight blocks, the last partial), a
    list of 700 cells with its count on the device: the whole list, a shard
    that crosses M, the empty list, and a count past the list's capacity
    (clamped to G^3 and counted once)."""
    K, L = vren.kernels(), vren.lib()
    M, n_list, s = 1000, 700, 0.5
    hgs = s / G
    smh, hgs32 = float(np.float32(s - hgs)), float(np.float32(hgs))
    head = R.sorted_occ_list(G, n_list)
    rest = np.setdiff1d(np.arange(G ** 3, dtype=np.int32), head)
    full = np.concatenate([head, rest[::-1]]).astype(np.int32)  # capacity G^3: what a count past it may reach
    lst = torch.from_numpy(full).to(DEV)
    cnt = torch.tensor([n_list], dtype=torch.int64, device=DEV)
    ctr = torch.tensor([7, 1 << 40], dtype=torch.int64, device=DEV)
    seed = 99

    def draw(lo, hi):
        xyz, flat = _occ_buffers(hi - lo)
        K.ngp_occupancy_samples(seed, ctr, cascade, G, M, smh, hgs32, lst, cnt, lo, hi, xyz, flat, vren._stream())
        torch.cuda.synchronize()
        return xyz, flat

    for lo, hi in ((0, 2 * M), (300, 1777)):
        wf, wx = R.occupancy_samples(seed, 7, cascade, G, M, smh, hgs32, head, lo, hi)
        _check_occ(*draw(lo, hi), hi - lo, wf, wx, (lo, hi))
    assert int(wf.min()) >= cascade * G ** 3
    cnt.zero_()
    wf, wx = R.occupancy_samples(seed, 7, cascade, G, M, smh, hgs32, head, 0, 2 * M, count=0)
    assert (wf[M:] == -1).all() and not wx[M:].any()
    _check_occ(*draw(0, 2 * M), 2 * M, wf, wx, "empty list")
    assert L.ngp_guard_hits() == 0
    cnt.fill_(G ** 3 + 5)
    try:
        wf, wx = R.occupancy_samples(seed, 7, cascade, G, M, smh, hgs32, full, 0, 2 * M, count=G ** 3 + 5)
        _check_occ(*draw(0, 2 * M), 2 * M, wf, wx, "count past the capacity")
        assert L.ngp_guard_hits() == 1
        _check_occ(*draw(M + 3, 2 * M - 1), M - 4, wf[M + 3:2 * M - 1], wx[M + 3:2 * M - 1], "clamped shard")
        assert L.ngp_guard_hits() == 2
    finally:
        assert L.ngp_guard_reset() == 0


# ------------------------------------------------------------------ occupancy draw, sorted
def _explain(i, M, n_cells, lst, got_flat, want_flat, dist, cascade):
    """a disagreeing sample: where it sits and how far device and model are apart"""
    half, k = int(i >= M), int(i - M if i >= M else i)
    got, want = int(got_flat) - cascade * n_cells, int(want_flat) - cascade * n_cells
    msg = (f"sample {i} (half {half}, exponential {k}, block {k // R.OSC_CH}, {k % R.OSC_CH} in it): device cell {got}, "
           f"model cell {want}, frac_dist {dist:.3e}")
    if half:
        pos = {int(c): j for j, c in enumerate(lst.tolist())}
        pw = pos.get(want)
        msg += (f"; list positions: device {pos.get(got)}, model {pw}, model's neighbours "
                f"{[int(lst[j]) for j in (pw - 1, pw + 1) if pw is not None and 0 <= j < len(lst)]}")
    else:
        msg += f"; device - model = {got - want} cells"
    return msg


@pytest.mark.parametrize("seed,ctr_v,cascade,M", R.SORTED_CASES)
def test_sorted_occupancy_draw_equals_the_model(seed, ctr_v, cascade, M):
    """ngp_occupancy_samples_sorted on a junk-filled workspace: the whole list,
    again on the used workspace, and shards that start and end inside blocks
    and cross M."""
    K = vren.kernels()
    G, s = R.SORTED_G, 0.5
    n_cells = G ** 3
    hgs = s / G
    smh, hgs32 = float(np.float32(s - hgs)), float(np.float32(hgs))
    head = R.sorted_occ_list()
    lst = torch.from_numpy(np.concatenate([head, np.zeros(n_cells - head.size, dtype=np.int32)])).to(DEV)
    cnt = torch.tensor([head.size], dtype=torch.int64, device=DEV)
    ctr = torch.tensor([ctr_v], dtype=torch.int64, device=DEV)
    ws_bytes = K.ngp_occupancy_sorted_workspace(M)
    nb = (M + 1 + R.OSC_CH - 1) // R.OSC_CH
    assert ws_bytes == 8 * (2 * nb + 2)
    ws = _junk(ws_bytes // 8, torch.float64)
    wf, wx, dist = R.occupancy_samples_sorted(seed, ctr_v, cascade, G, M, smh, hgs32, head, 0, 2 * M)

    def draw(lo, hi):
        xyz, flat = _occ_buffers(hi - lo)
        K.ngp_occupancy_samples_sorted(seed, ctr, cascade, G, M, smh, hgs32, lst, cnt, lo, hi, ws, xyz, flat,
                                       vren._stream())
        torch.cuda.synchronize()
        assert _tail_untouched(ws, ws_bytes // 8)
        return xyz, flat

    def check(lo, hi, what):
        xyz, flat = draw(lo, hi)
        got = flat[:hi - lo].cpu().numpy()
        bad = np.nonzero(got != wf[lo:hi])[0]
        for j in bad[:8]:
            print(_explain(lo + j, M, n_cells, head, got[j], wf[lo + j], dist[lo + j], cascade))
        assert bad.size == 0, f"{what}: {bad.size} of {hi - lo} cells differ, the first at sample {lo + bad[0]}"
        _check_occ(xyz, flat, hi - lo, wf[lo:hi], wx[lo:hi], what)
        return xyz, flat

    x0, f0 = check(0, 2 * M, "whole list")
    x1, f1 = check(0, 2 * M, "second call on the used workspace")
    assert torch.equal(f0, f1) and np.array_equal(_bits(x0), _bits(x1))
    shards = {(M // 3, M + M // 2 + 1), (max(M - 5, 0), min(M + 7, 2 * M)), (1, 2 * M)}
    if M > R.OSC_CH:
        shards |= {(R.OSC_CH + 17, min(M + R.OSC_CH + 33, 2 * M)), (R.OSC_CH - 1, M + R.OSC_CH), (M - 1, M + 1)}
    for lo, hi in sorted(shards):
        check(lo, hi, f"shard [{lo}, {hi})")


# ------------------------------------------------------------------ the trainer follows the stream
# The batch counter a step's draws use.  trainer.py: dctr[1] counts the batches drawn and every step
# ends with ngp_counters_inc; step k's batch is drawn either inline at its start (_step: add 0 at
# dctr[1] = k), ahead during step k - 1 (prefetch, _graph_body: add 1 at dctr[1] = k - 1), or after
# step k - 1's increment behind an occupancy update (_graph_body: add 0 at dctr[1] = k).  All three
# give counter k + C0 with C0 = 0; the background is drawn inside step k at add 0: counter k as well.
C0 = 0


@pytest.mark.parametrize("random_bg,kw", [(False, {}), (True, {}), (True, {"warmup_steps": 4})],
                         ids=["default", "random_bg", "random_bg-graphs-from-step-4"])
def test_trainer_draws_follow_the_model_stream(random_bg, kw):
    """40 train_steps: after step k the bound batch (indices, noise, ground
    truth) is the model's draw at (sample_seed, k + C0, rank * R), the random
    background the model's at (bg_seed, k + C0).  With the default warm-up
    (256 steps) the 40 steps run eagerly with warm-up occupancy updates at 0,
    16 and 32; warmup_steps = 4 adds what the steady state does: the step as
    a captured graph and its replays, the occupancy updates at 16 and 32
    drawn on the device inside the graph, the batch behind them drawn after
    the increment."""
    sc = S.AnalyticScene(W=200, H=200, n_images=10)
    dirs, poses = sc.directions.to(DEV), sc.poses.to(DEV)
    gt = sc.gt_images(device=DEV)
    R_ = 512
    tr = NGPTrainer(scale=0.5, batch_size=R_, device=DEV, seed=3, random_bg=random_bg, **kw)
    assert tr.rank == 0 and (tr.sample_seed, tr.bg_seed) == (1000003 * 4, (1000003 * 4) ^ 0x6267)
    seen = []
    for k in range(40):
        tr.train_step(gt, dirs, poses)
        img, pix, noise = R.sample_batch(tr.sample_seed, k + C0, tr.rank * R_, R_, 10, 200 * 200)
        assert np.array_equal(tr.img_idxs.cpu().numpy(), img), k
        assert np.array_equal(tr.pix_idxs.cpu().numpy(), pix), k
        assert np.array_equal(_bits(tr.noise), _f32bits(noise)), k
        g = gt[tr.img_idxs, tr.pix_idxs].float()
        assert torch.equal(tr.rgb_gt, g / torch.full_like(g, 255.0)), k
        if random_bg:
            assert np.array_equal(_bits(tr._bg_rand), _f32bits(R.random_bg(tr.bg_seed, k + C0))), k
        seen.append(pix.tobytes() + img.tobytes())
    tr.drain()
    torch.cuda.synchronize()
    assert len(set(seen)) == 40
    assert int(tr.dctr[1]) == 40 and int(tr.dctr[0]) == 40
    if kw:
        assert len(tr._graphs) >= 2 and int(tr.dctr[2]) == 2  # replayed, and two updates drawn on the device
    else:
        assert not tr._graphs and int(tr.dctr[2]) == 0
