"""Conditions on the exact input sets of field_fwd_ref.py (no GPU): statements
about the inputs that test_field_fwd_gpu.py's bit-for-bit assertions rest on,
not measurements.

* every family member at every size used on the GPU satisfies check_exact_fwd;
* mlp_fwd_ref64 equals oracle.mlp_forward (torch fp32, fp16 storage points)
  bit for bit on these sets;
* the cyclic family's coverage claim, element by element; what the lattice
  sets reach (h0 of both signs, rows on both sides of every ReLU); the SH
  probes' 16 columns x 2 signs;
* the constant-level table encodes to its codes exactly, at both scales, with
  two hashed levels on the generic modulo, inside, on and outside the box;
* the multi-pass sizes from constants parsed out of the sources;
* round 1's rows sit a factor 2 from T_thr on the log scale."""
import numpy as np
import pytest
import torch

import field_fwd_ref as FR
import oracle as O

CUS = 256
MP = FR.multipass_sizes(CUS)
GPU_SIZES = FR.SIZES + [MP.fwd]  # (the nets alone; the gathering kernels see one encoding row per table)


def _case(family, key, n, seed):
    enc, dirs = FR.enc_rows(n, seed), FR.dir_rows(n, seed)
    return enc, FR.sh16(dirs), FR.weights(family, key)


@pytest.mark.parametrize("n", GPU_SIZES)
def test_every_lattice_set_is_exact(n):
    for seed in (0, 1):
        enc, sh, W = _case("lattice", seed, n, seed)
        assert W["W2"][0].any() and not W["W3"][:, :16].any() and W["W5"][3:].any(1).all()
        assert ((W["W4"] == 1).sum(1) >= 1).all()
        assert all({-1.0, 1.0} <= set(W["W5"][r]) for r in range(3))
        for name in FR.OW:
            assert ((W[name] != 0).sum(1) == 3).all(), name
        FR.check_exact_fwd(enc, sh, W)


def test_every_cyclic_and_probe_set_is_exact():
    for k in range(64):
        FR.check_exact_fwd(*_case("cyclic", k, 64, 0))
    for key in FR.PROBES:
        h = FR.check_exact_fwd(*_case("probe", key, 65, 0))
        assert np.count_nonzero(h[4][:, :3]) > 20  # (the probes show values, not only ReLU zeros)


def test_every_constant_table_set_is_exact():
    """the gathering kernels' sets: one encoding row (the level codes) for every point"""
    for n in (65, 513):
        sh = FR.sh16(FR.dir_rows(n, 0))
        for cs in (0, 1):
            enc = np.tile(FR.level_codes(cs).reshape(1, 32), (n, 1))
            for seed in (0, 1):
                FR.check_exact_fwd(enc, sh, FR.lattice_fwd_weights(seed))
            for key in FR.PROBES:
                FR.check_exact_fwd(enc, sh, FR.sh_probe_weights(*key))


@pytest.mark.parametrize("family,key,n", [("lattice", 0, 257), ("lattice", 1, 513), ("cyclic", 5, 64),
                                          ("cyclic", 62, 64), ("probe", (3, 1), 65), ("probe", (12, -1), 65)])
def test_ref64_equals_the_oracle_mlp(family, key, n):
    enc, sh, W = _case(family, key, n, 0)
    h1, h, h3, h4, o = FR.mlp_fwd_ref64(enc, sh, W)
    t = lambda a: torch.from_numpy(a).float()  # noqa: E731
    h_o = O.mlp_forward(t(enc).half(), [t(W["W1"]), t(W["W2"])])
    o_o = O.mlp_forward(torch.cat([t(sh), h_o], 1).half(), [t(W["W3"]), t(W["W4"]), t(W["W5"])])
    bits = lambda a: np.asarray(a, dtype=np.float64).astype(np.float16).view(np.int16)  # noqa: E731
    assert np.array_equal(bits(h), h_o.half().numpy().view(np.int16))
    assert np.array_equal(bits(o), o_o.half().numpy().view(np.int16))
    assert np.array_equal(h.astype(np.float16).astype(np.float64), h) and np.array_equal(o.astype(np.float16), o)


def test_cyclic_sets_cover_every_element():
    seen = {name: np.zeros((od, idim), dtype=bool) for name, (_, od, idim) in FR.OW.items()}
    for k in range(64):
        W = FR.cyclic_weights(k)
        for name in seen:
            assert ((W[name] != 0).sum(1) == 1).all() and set(np.unique(W[name])) <= {-1.0, 0.0, 1.0}
            seen[name] |= W[name] != 0
        # the sign rule: no unit of h3 or h4 is dead by construction
        enc, sh, _ = _case("cyclic", k, 64, 0)
        h1, h, h3, h4, o = FR.mlp_fwd_ref64(enc, sh, W)
        assert (W["W4"] >= 0).all() and (h3.max(0) > 0).all() and (h4.max(0) > 0).all()
        assert o[:, :3].any(0).all() and (o[:, :3] < 0).any() and (o[:, :3] > 0).any()
    for name in ("W1", "W2", "W4", "W5"):
        assert seen[name].all(), name
    assert seen["W3"][:, 16:].all() and not seen["W3"][:, :16].any()


def test_lattice_sets_reach_both_sides():
    for seed in (0, 1):
        for n in (255, 513):
            enc, sh, W = _case("lattice", seed, n, seed)
            h1, h, h3, h4, o = FR.mlp_fwd_ref64(enc, sh, W)
            assert (h[:, 0] > 0).any() and (h[:, 0] < 0).any() and len(np.unique(h[:, 0])) >= 8
            pre = {"h1": enc @ W["W1"].T, "h3": h @ W["W3"][:, 16:].T, "h4": h3 @ W["W4"].T}
            for name, p in pre.items():  # every unit passes some rows and clips others
                assert ((p > 0).any(0) & (p <= 0).any(0)).all(), (seed, n, name)
            assert (o[:, :3] > 0).any(0).all() and (o[:, :3] < 0).any(0).all()
            assert o[:, 3:].any(0).all()  # (rows 3..15 carry values that must not leak)


def test_probes_reach_every_sh_column_with_both_signs():
    seen = set()
    for k, s in FR.PROBES:
        W = FR.sh_probe_weights(k, s)
        sh = np.arange(1.0, 17.0)[None, :]  # (a direction-free stand-in: column c holds c + 1)
        o = FR.mlp_fwd_ref64(np.zeros((1, 32)), sh, W)[4][0]
        for r in range(3):
            col, sg = FR.probe_column(k, r, s)
            assert o[r] == max(sg * (col + 1.0), 0.0)
            seen.add((col, sg))
        assert len({FR.probe_column(k, r, s)[0] for r in range(3)}) == 3
    assert seen == {(c, sg) for c in range(16) for sg in (1, -1)}


def _point_sets(scale):
    g = np.random.default_rng(3)
    inside = (g.random((100000, 3)) * 2 - 1) * scale
    outside = (g.random((99960, 3)) * 2 - 1) * scale * 3
    faces = FR.point_rows(40, scale)[-14:]
    edge = inside[:26].copy()
    edge[:13, 0] = scale
    edge[13:, 2] = -scale
    return np.concatenate([inside, outside, faces, edge]).astype(np.float32)


@pytest.mark.parametrize("shrink", [(), (7, 12)])
@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_constant_table_encodes_to_its_codes(scale, shrink):
    spec = O.HashGridSpec(16, 19, 16, scale=scale)
    for l in shrink:
        spec.sizes[l] = 2 ** 19 - 8  # the generic modulo (offsets and table as they are)
    x = torch.from_numpy(_point_sets(scale))
    assert x.shape[0] == 200000
    for cs in (0, 1):
        c = FR.level_codes(cs)
        assert np.abs(c).max() <= 2 and c.any()
        tab = torch.from_numpy(FR.const_level_table(spec, c)).float().reshape(-1)
        enc = O.hash_encode_fwd(spec, x, -scale * torch.ones(3), scale * torch.ones(3), tab)
        want = torch.from_numpy(c.reshape(1, 32)).half().expand(x.shape[0], 32)
        bad = int((enc.view(torch.int16) != want.contiguous().view(torch.int16)).sum())
        assert bad == 0, f"{bad} mismatches at scale {scale}, codes {cs}"


def test_multipass_sizes_follow_from_the_sources():
    k = FR.source_constants()
    assert (k.R32, k.R64, k.FEM2_WAVES) == (40, 72, 8) and k.image_bytes == 24064
    assert k.launch_bounds["field_fwd_kernel"] == "256"
    assert k.launch_bounds["field_encode_mlp_reg_kernel"].startswith("64 * FEM2_WAVES")
    assert k.launch_bounds["field_first_chunk_kernel"].startswith("64 * FEM2_WAVES")
    # 24 KB of LDS per block: at most 6 blocks per CU; 32 wave slots: 8 blocks of 4 waves, 4 blocks of 8 waves
    assert FR.LDS_PER_CU // k.image_bytes == 6 and FR.resident_block_bounds() == (6, 4)
    for cus in (64, 256, 304):
        m = FR.multipass_sizes(cus)
        assert (m.fwd, m.reg, m.first) == (2 * 64 * 6 * cus + 37, 512 * 4 * cus + 64 * 37 + 5, 8 * 4 * cus + 133)
        # whatever the resident blocks b per CU (1..bound): more rows than one iteration of the whole grid covers
        for b in range(1, 7):
            assert m.fwd > 64 * b * cus
        for b in range(1, 5):
            assert m.reg - 64 * 37 - 5 >= 512 * b * cus and m.first - 133 >= 8 * b * cus
        assert m.fwd % 16 and m.reg % 64 and m.first % 8


@pytest.mark.parametrize("R", FR.ROUND1_R + [MP.first])
def test_round1_rows_sit_a_factor_two_from_the_threshold(R):
    for sigma in (np.exp(-7.0), 1.0, np.exp(9.0)):
        for kind in ("all", "list"):
            c = FR.round1_rows(R, sigma, kind)  # (asserts the factor 2 itself)
            assert c.evaluated == c.first.size and c.total2 == c.list2.size
            assert (c.rest[c.done] >= 0).all() and c.n_samples >= c.first.max(initial=0) + 1
            if R >= 18:
                assert (c.rest > 0).any() and ((c.rest == 0) & (c.N > 64)).any()
            if kind == "list" and R > 1 and R <= 400:
                assert (c.rest == -9).sum() == R - c.count > 0 or R < 5
            # rows do not overlap and leave samples no row owns
            owned = np.zeros(c.n_samples, dtype=int)
            for s, n in zip(c.start, c.N):
                owned[s:s + n] += 1
            assert owned.max() <= 1 and (owned == 0).any()
