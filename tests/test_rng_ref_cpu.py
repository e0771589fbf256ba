"""The host model of the device's random draws (tests/rng_ref.py) against what
is published or provable without a GPU: the Philox-4x32-10 known answers, the
edges of the two integer / float maps, the stream map's disjointness, and the
precondition under which tests/test_rng_gpu.py may ask the sorted occupancy
draw for bitwise equality."""
import numpy as np
import pytest

import rng_ref as R
import trainer

# Random123 kat_vectors, philox4x32 10: counter, key, output
KAT = [((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(w) for w in R.philox4x32(*ctr, *key)) == want


def test_philox_known_answers_vectorised_and_round_count_matters():
    c = np.array([k[0] for k in KAT], dtype=np.uint64)
    k = np.array([k[1] for k in KAT], dtype=np.uint64)
    out = np.stack(R.philox4x32(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1]), -1)
    assert np.array_equal(out, np.array([k[2] for k in KAT], dtype=np.uint64))
    nine = np.stack(R.philox4x32(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1], rounds=9), -1)
    assert not (nine == out).any()


@pytest.mark.parametrize("n", [1, 3, 20, 40000, 2 ** 31])
def test_uniform_index_edges(n):
    assert int(R.uniform_index(0, n)) == 0
    assert int(R.uniform_index(0xFFFFFFFF, n)) == n - 1
    u = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint64)
    assert R.uniform_index(u, n).tolist() == [(int(v) * n) >> 32 for v in u]


def test_unit24_stays_below_one():
    top = R.unit24(0xFFFFFFFF)
    assert top.dtype == np.float32 and float(top) == 1.0 - 2.0 ** -24 and float(top) < 1.0
    assert float(R.unit24(0)) == 0.0 and float(R.unit24(0xFF)) == 0.0 and float(R.unit24(0x100)) == 2.0 ** -24


def test_morton_roundtrip_and_bit_order():
    assert int(R.morton3(1, 0, 0)) == 1 and int(R.morton3(0, 1, 0)) == 2 and int(R.morton3(0, 0, 1)) == 4
    c = np.arange(1024, dtype=np.uint64)
    m = R.morton3(c, c[::-1], (c * np.uint64(7)) % np.uint64(1024))
    assert np.array_equal(R.compact3(m), c) and np.array_equal(R.compact3(m >> np.uint64(1)), c[::-1])


@pytest.mark.parametrize("seed", range(16))
def test_stream_domains_of_one_trainer_are_pairwise_disjoint(seed):
    """batch, background, jitter, uniform cell and exponentials (both halves),
    cascades 0..7, under the trainer's own three keys"""
    sample_key, bg_key, occ_key = trainer.rng_keys(seed)
    assert bg_key == sample_key ^ R.BG_KEY_XOR
    assert all(0 <= k < 2 ** 64 for k in (sample_key, bg_key, occ_key))
    doms = R.stream_domains(sample_key, bg_key, occ_key)
    assert len(doms) == 2 + 8 * 4
    for i, a in enumerate(doms):
        assert not R.domains_disjoint(a, a)  # (the check can fail)
        for b in doms[i + 1:]:
            assert R.domains_disjoint(a, b), (a[0], b[0])
    # the separation by word 3 alone: with one key for everything only batch (no pinned
    # word 3) and background (words 0, 1) are left to their keys
    same = R.stream_domains(occ_key, occ_key, occ_key)
    clash = [(a[0], b[0]) for i, a in enumerate(same) for b in same[i + 1:] if not R.domains_disjoint(a, b)]
    assert all(a in ("batch", "background") for a, _ in clash) and len(clash) == 1 + 2 * 32


def test_trainer_keys_are_the_documented_derivation():
    for seed in range(16):
        base = (1000003 * (seed + 1)) & 0xFFFFFFFFFFFFFFFF
        assert trainer.rng_keys(seed) == (base, base ^ 0x6267, base ^ 0x5DEECE66D)


def test_batch_model_is_sliced_by_ray_offset_and_keyed_by_all_64_bits():
    a = R.sample_batch(5, 1, 0, 100, 20, 40000)
    b = R.sample_batch(5, 1, 40, 60, 20, 40000)
    assert all(np.array_equal(x[40:], y) for x, y in zip(a, b))
    assert a[0].min() >= 0 and a[0].max() < 20 and a[1].max() < 40000 and a[2].dtype == np.float32
    for other in (R.sample_batch(5 + 2 ** 32, 1, 0, 100, 20, 40000), R.sample_batch(5, 1 + 2 ** 32, 0, 100, 20, 40000),
                  R.sample_batch(5, 1, 2 ** 32, 100, 20, 40000)):
        assert not np.array_equal(other[1], a[1])


def test_unsorted_model_shards_are_slices_and_the_empty_list_gives_minus_one():
    lst = R.sorted_occ_list(12, 700)
    f, x = R.occupancy_samples(99, 7, 3, 12, 1000, 0.5 - 0.5 / 12, 0.5 / 12, lst, 0, 2000)
    f2, x2 = R.occupancy_samples(99, 7, 3, 12, 1000, 0.5 - 0.5 / 12, 0.5 / 12, lst, 300, 1777)
    assert np.array_equal(f2, f[300:1777]) and np.array_equal(x2, x[300:1777]) and x.dtype == np.float32
    assert set((f[1000:] - 3 * 12 ** 3).tolist()) <= set(lst.tolist())
    cells = f[:1000] - 3 * 12 ** 3
    assert all(int(R.compact3(cells >> s).max()) < 12 for s in (0, 1, 2))
    f3, x3 = R.occupancy_samples(99, 7, 3, 12, 1000, 0.5 - 0.5 / 12, 0.5 / 12, lst, 0, 2000, count=0)
    assert (f3[1000:] == -1).all() and not x3[1000:].any() and np.array_equal(f3[:1000], f[:1000])


def test_order_statistics_are_exact_on_a_hand_case():
    """e = (1, 1, 2): S = 1, 2 of 4 -> U n = n / 4, n / 2"""
    cell, dist = R._order_statistics(np.array([1.0, 1.0, 2.0]), 10)
    assert cell.tolist() == [2, 5] and dist.tolist() == [0.5, 0.0]
    cell, dist = R._order_statistics(np.array([2.0 ** -43, 0.0, 3 * 2.0 ** -43]), 8)
    assert cell.tolist() == [2, 2] and dist.tolist() == [0.0, 0.0]


def test_sorted_scan_depth():
    """D = 75 + (nb - 1) // 64 (rng_ref's docstring counts it from the three kernels)"""
    assert [R.sorted_scan_depth(M) for M in (1, 4095, 4096, 12293, 64 * 4096 - 1, 64 * 4096)] == [75] * 5 + [76]


@pytest.mark.parametrize("seed,ctr,cascade,M", R.SORTED_CASES)
def test_sorted_draw_inputs_stay_clear_of_cell_boundaries(seed, ctr, cascade, M):
    """The precondition of test_rng_gpu's sorted draws: in each half no sample's
    U_(k) n lies within 64 tau of an integer, tau = (D + 4) 2^-52 n the bound on
    |device - model| (rng_ref's docstring; the model's own error is zero, below
    tau / 64).  Both halves ascend and the occupied half stays in the list."""
    G, lst = R.SORTED_G, R.sorted_occ_list()
    assert lst.size == R.SORTED_LIST_N and (np.diff(lst) > 0).all() and lst.min() >= 0 and lst.max() < G ** 3
    hgs = 0.5 / G
    flat, xyz, dist = R.occupancy_samples_sorted(seed, ctr, cascade, G, M, 0.5 - hgs, hgs, lst, 0, 2 * M)
    assert np.isfinite(dist).all() and flat.shape == (2 * M,) and xyz.shape == (2 * M, 3)
    for name, d, n in (("uniform", dist[:M], G ** 3), ("occupied", dist[M:], lst.size)):
        bound = 64 * R.sorted_tau(M, n)
        print(f"seed {seed:#x} ctr {ctr} cascade {cascade} M {M} {name} half (n = {n}): min frac_dist "
              f"{d.min():.3e}, 64 tau {bound:.3e}")
        assert d.min() >= bound
    cells = flat - cascade * G ** 3
    assert (np.diff(cells[:M]) >= 0).all() and cells[:M].min() >= 0 and cells[:M].max() < G ** 3
    pos = np.searchsorted(lst, cells[M:])
    assert np.array_equal(lst[pos], cells[M:]) and (np.diff(pos) >= 0).all()
    assert np.abs(xyz).max() <= 0.5
