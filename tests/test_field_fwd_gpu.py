"""The field forward, value for value: every forward entry point of field.hip
on the exact input sets of field_fwd_ref.py (test_field_fwd_ref_cpu.py asserts
the conditions), at the sizes where a block, a chunk or a column block ends and
at one size per kernel family where the persistent loop takes a second
iteration (field_fwd_ref.multipass_sizes, from the device's CU count).

A. the nets alone (ngp_field_mlp_forward, colour and density-only) on
   hand-built pair-major integer encodings: lattice weights at every size and
   layout, the cyclic sweep (64 sets) at n = 64, the SH probes (32 sets) at 65;
B. the gathering kernels on the constant-level table (every point encodes to
   the level codes exactly): ngp_field_forward_act, ngp_density_forward,
   ngp_field_forward_indexed, ngp_field_encode_mlp_act (with / without a list,
   with / without dirs, with h), ngp_hash_encode; the four colour modes on the
   lattice sets, the SH probes through the two _act entry points;
C. round 1 (ngp_field_forward_first_pre_act, pre_levels 0 and 8 after
   ngp_field_encode_first_coarse): the density is a known constant per set, so
   rest / total2 / evaluated / the round-2 list follow from fp64;
D. test_field_gpu's oracle parameters and points at the edge and multi-pass
   sizes: encoding bit-equal to the oracle, h / sigma / rgb within
   oracle.mlp_forward_bound, and every entry point bit-equal to the fused one
   over all rows.

Asserted: h and the encoding bit for bit (as int16); rgb bit for bit under
none, ReLU and leaky ReLU; sigma within 4 x 2^-24 relative of fp64 exp(h0);
sigmoid rgb within one fp16 ulp of fp64; the SH probes within one fp16 ulp of
fp16(oracle.sh4) with the number of values that are not bit-equal reported;
every row at or past the count, every unlisted sample and every pad keeps its
junk bits.  Every output starts as junk with a junk pad behind it."""
import contextlib
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import field_fwd_ref as FR
import hashgrid as HG
import oracle as O
import vren

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 37          # junk rows behind every output
JUNK = -7.5       # no integer, no sigma, no colour
SCALE = 0.5
F16, F32, F64 = torch.float16, torch.float32, torch.float64


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _mp():
    return FR.multipass_sizes(_cus())


def _size(n, family):
    return getattr(_mp(), family) if n == "multipass" else n


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)


def _junk(shape, dt=F32, fill=JUNK):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dt, device=DEV)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _ok(st, what):
    vren._ok(st, what)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- rows of a launch
def _plan(n, layout):
    """-> (rows: the samples the launch processes, in launch order; n_dev; sample list), layout:
    all / ndev (a device count below n) / capped (a device count past n) / list (a shuffled third, count on the
    device) / perm (every sample once, shuffled, no device count)"""
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=DEV)  # noqa: E731
    if layout == "all":
        return np.arange(n), None, None
    if layout == "ndev":
        cnt = n - (n + 3) // 4
        return np.arange(cnt), i64(cnt), None
    if layout == "capped":
        return np.arange(n), i64(n + 1000), None
    if layout == "list":
        rows = FR.list_rows(n)
        full = np.zeros(n, dtype=np.int32)  # (entries past the count: valid samples, never to be read)
        full[:len(rows)] = rows
        return rows.astype(np.int64), i64(len(rows)), _dev(full, torch.int32)
    rows = FR.perm_rows(n)
    return rows.astype(np.int64), None, _dev(rows, torch.int32)


@contextlib.contextmanager
def _guard(layout):
    """a count past the capacity is capped and counted: expected here, and reset (conftest asserts zero hits)"""
    L = vren.lib()
    if layout == "capped":
        assert L.ngp_guard_reset() == 0
    try:
        yield
        if layout == "capped":
            assert int(L.ngp_guard_hits()) >= 1, "a count past the capacity is capped and counted"
    finally:
        if layout == "capped":
            assert L.ngp_guard_reset() == 0


# ------------------------------------------------------------------------------------------------- assertions
def _rows2d(t):
    """(m, ...) -> (m, k), also for m = 0"""
    return t.reshape(t.shape[0], max(1, t.numel() // max(1, t.shape[0])))


def _first(mask):
    return int(torch.nonzero(mask)[0, 0])


def _untouched(label, name, got, rt):
    """every row of got (m, ...) outside rt keeps its junk bits"""
    keep = torch.ones(got.shape[0], dtype=torch.bool, device=DEV)
    keep[rt] = False
    junk = _bits(torch.full((1,), JUNK, dtype=got.dtype, device=DEV))
    wrote = (_bits(_rows2d(got)) != junk).any(1) & keep
    assert not bool(wrote.any()), (f"{label}: {name}: {int(wrote.sum())} rows outside the processed ones were written "
                                   f"(of {got.shape[0]} with the pad), first sample {_first(wrote) if wrote.any() else -1}")


def _equal_bits(label, name, got, want, rows, rt):
    """got (m >= n, k) == want (n, k) bit for bit on the processed samples, junk elsewhere"""
    g, w = _rows2d(got[rt]), _rows2d(want[rt])
    bad = (_bits(g) != _bits(w)).any(1)
    if bool(bad.any()):
        j = _first(bad)
        cols = torch.nonzero(_bits(g[j]) != _bits(w[j]))[:, 0].tolist()
        raise AssertionError(f"{label}: {name}: {int(bad.sum())} of {len(rows)} rows differ; first at launch "
                             f"{FR.row_position(j)} = sample {int(rows[j])}, columns {cols[:8]}: got "
                             f"{g[j][cols[:8]].tolist()}, want {w[j][cols[:8]].tolist()}")
    _untouched(label, name, got, rt)


def _close(label, name, got, want, tol, rows, rt):
    """|got - want| <= tol (fp64) on the processed samples, junk elsewhere -> the errors / tol"""
    g = _rows2d(got[rt]).double()
    w, t = _rows2d(want[rt]), _rows2d(tol[rt])
    err = (g - w).abs()
    bad = (~(err <= t)).any(1)
    if bool(bad.any()):
        j = _first(bad)
        raise AssertionError(f"{label}: {name}: {int(bad.sum())} of {len(rows)} rows past the tolerance; first at "
                             f"launch {FR.row_position(j)} = sample {int(rows[j])}: got {g[j].tolist()}, want "
                             f"{w[j].tolist()}, tolerance {t[j].tolist()}")
    _untouched(label, name, got, rt)
    return err / t.clamp_min(1e-300)


SIG_REL = 4 * 2.0 ** -24   # fp32 expf against fp64 exp (test_field_gpu's margin)
_seen = {"sigmoid": [0, 0], "probe": [0, 0, set()]}


def _want(h, o, enc=None):
    """fp64 references (n, 16), (n, >= 3), (n, 32) -> what the device must hold"""
    return SimpleNamespace(h16=_dev(h, F16), sig64=_dev(np.exp(h[:, 0]), F64), o=np.asarray(o)[:, :3],
                           enc16=None if enc is None else _dev(enc, F16), rgb={})


def _want_rgb(want, act):
    if act not in want.rgb:
        r = FR.rgb_ref(want.o, act)
        want.rgb[act] = _dev(r, F64 if act == FR.RGB_SIGMOID else F32)
    return want.rgb[act]


def _check(label, got, want, rows, act, probe_cols=None):
    """the outputs of one launch (got: name -> (n + PAD, k) tensors) against want"""
    rt = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(DEV)
    if "enc" in got:
        _equal_bits(label, "the encoding", got["enc"], want.enc16, rows, rt)
    if "h" in got:
        _equal_bits(label, "h (W1, W2)", got["h"], want.h16, rows, rt)
    if "sig" in got:
        _close(label, "sigma = exp(h0)", got["sig"], want.sig64, want.sig64 * SIG_REL, rows, rt)
    if "rgb" not in got:
        return
    w = _want_rgb(want, act)
    if probe_cols is not None:
        # relu(+-SH component) of the sample's own direction: expected bit-equal to fp16(oracle.sh4); a value that
        # is not is counted and held to one fp16 ulp
        assert act == FR.RGB_NONE
        tol = O.ulp16(w.double().cpu()).to(DEV)
        _close(label, f"rgb = relu(+-SH columns {probe_cols})", got["rgb"], w.double(), tol, rows, rt)
        ne = _bits(got["rgb"][rt]) != _bits(w[rt])
        _seen["probe"][0] += int(ne.sum())
        _seen["probe"][1] += ne.numel()
        for ch in torch.nonzero(ne.any(0))[:, 0].tolist():
            _seen["probe"][2].add(probe_cols[ch])
    elif act == FR.RGB_SIGMOID:
        tol = O.ulp16(w.cpu()).to(DEV)
        _close(label, "rgb = sigmoid(o) (W3, W4, W5)", got["rgb"], w, tol, rows, rt)
        model = O.rh(torch.sigmoid(torch.from_numpy(want.o).float())).to(DEV)
        _seen["sigmoid"][0] += int((_bits(got["rgb"][rt]) == _bits(model[rt])).sum())
        _seen["sigmoid"][1] += 3 * len(rows)
    else:
        _equal_bits(label, "rgb (W3, W4, W5)", got["rgb"], w, rows, rt)


# ----------------------------------------------------------------------------------------------- entry points
def _pm_buffer(n):
    """a pair-major encoding (8, n, 4) of junk with PAD junk rows behind the whole buffer"""
    return _junk(8 * n * 4 + 4 * PAD, F16)


def _pm_rows(buf, n):
    """the buffer as sample rows (n + PAD, 32): the planes' rows, then the pad (as rows of junk x 8 planes)"""
    rows = buf[:32 * n].view(8, n, 4).permute(1, 0, 2).reshape(n, 32)
    pad = buf[32 * n:].view(PAD, 4).repeat(1, 8)
    return torch.cat([rows, pad])


def _run(entry, p, layout, act=FR.RGB_SIGMOID):
    """one launch of `entry` over the problem p (n, x, dirs, enc_pm, w16, table, desc) -> (rows, outputs)"""
    n = p.n
    rows, n_dev, sidx = _plan(n, layout)
    L, s = vren.lib(), vren._stream()
    sig, rgb, h = _junk(n + PAD), _junk((n + PAD, 3)), _junk((n + PAD, 16), F16)
    desc = None if p.desc is None else ctypes.byref(p.desc)
    got = {"sig": sig}
    with _guard(layout):
        if entry in ("mlp_forward", "mlp_density"):
            color = entry == "mlp_forward"
            _ok(L.ngp_field_mlp_forward(p.enc_pm, p.dirs if color else None, n, n_dev, sidx, p.w16, sig,
                                        rgb if color else None, h, s), entry)
            got.update({"h": h, **({"rgb": rgb} if color else {})})
        elif entry == "forward_act":
            enc = _junk((n + PAD, 32), F16)
            _ok(L.ngp_field_forward_act(p.x, p.dirs, n, n_dev, desc, p.table, p.w16, sig, rgb, enc, h, act, s), entry)
            got.update({"h": h, "rgb": rgb, "enc": enc})
        elif entry == "density":
            _ok(L.ngp_density_forward(p.x, n, n_dev, desc, p.table, p.w16, sig, h, s), entry)
            got["h"] = h
        elif entry == "indexed":
            enc = _junk((n + PAD, 32), F16)
            _ok(L.ngp_field_forward_indexed(p.x, p.dirs, n, n_dev, sidx, desc, p.table, p.w16, sig, rgb, enc, s), entry)
            got.update({"rgb": rgb, "enc": enc})
        elif entry in ("encode_mlp", "encode_density"):
            color = entry == "encode_mlp"
            pm = _pm_buffer(n)
            _ok(L.ngp_field_encode_mlp_act(p.x, p.dirs if color else None, n, n_dev, sidx, desc, p.table, p.w16, pm, sig,
                                           rgb if color else None, h, act, s), entry)
            got.update({"h": h, "enc": _pm_rows(pm, n), **({"rgb": rgb} if color else {})})
        elif entry == "hash_encode":
            pm = _pm_buffer(n)
            _ok(L.ngp_hash_encode(p.x, n, n_dev, sidx, desc, p.table, pm, s), entry)
            got = {"enc": _pm_rows(pm, n)}
        else:
            raise KeyError(entry)
    return rows, got


# -------------------------------------------------------------------------------------------- A. the nets alone
A_LAYOUTS = ["all", "ndev", "list", "perm", "capped"]


@functools.lru_cache(maxsize=4)
def _nets_inputs(n, seed):
    enc, dirs = FR.enc_rows(n, seed), FR.dir_rows(n, seed)
    return enc, FR.sh16(dirs), _dev(FR.to_pair_major(enc, n), F16), _dev(dirs, F32)


@functools.lru_cache(maxsize=4)
def _nets_want(family, key, n, seed):
    enc, sh, _, _ = _nets_inputs(n, seed)
    h1, h, h3, h4, o = FR.mlp_fwd_ref64(enc, sh, FR.weights(family, key))
    return _want(h, o)


def _nets_problem(family, key, n, seed):
    _, _, enc_pm, dirs = _nets_inputs(n, seed)
    return SimpleNamespace(n=n, x=None, dirs=dirs, enc_pm=enc_pm, desc=None, table=None,
                           w16=_dev(FR.flat_weights(FR.weights(family, key)), F16))


def _nets_case(family, key, n, seed, layout):
    p, want = _nets_problem(family, key, n, seed), _nets_want(family, key, n, seed)
    for entry in ("mlp_forward", "mlp_density"):
        rows, got = _run(entry, p, layout)
        _check(f"ngp_field_mlp_forward ({entry}), n = {n}, layout {layout}, weights {family}({key})", got, want, rows,
               FR.RGB_SIGMOID)


@pytest.mark.parametrize("layout", A_LAYOUTS)
@pytest.mark.parametrize("n", FR.SIZES + ["multipass"])
def test_nets_alone_on_the_lattice_sets(n, layout):
    n = _size(n, "fwd")
    for seed in (0, 1):
        _nets_case("lattice", seed, n, seed, layout)


@pytest.mark.parametrize("k", range(64))
def test_nets_alone_on_the_cyclic_sweep(k):
    """one nonzero per row at (o, (o + k) % K): a weight at another place of the LDS image shows in h or rgb"""
    _nets_case("cyclic", k, 64, 0, "all")


@pytest.mark.parametrize("k,sign", FR.PROBES)
def test_nets_alone_on_the_sh_probes(k, sign):
    """(sigmoid only at this entry point: the probe's own values are held under colour mode none in B)"""
    _nets_case("probe", (k, sign), 65, 0, "all")


# ------------------------------------------------------------------ B. the gathering kernels, constant-level table
@functools.lru_cache(maxsize=None)
def _spec(scale, shrink=()):
    spec, grid = O.HashGridSpec(16, 19, 16, scale=scale), HG.HashGrid(scale)
    assert grid.offsets == spec.offsets.tolist() and grid.n_entries == spec.n_entries
    for l in shrink:  # hashed levels on the generic modulo (2^19 - 8: a multiple of 8; offsets and table as they are)
        grid.desc.sizes[l] = 2 ** 19 - 8
    return spec, grid


@functools.lru_cache(maxsize=2)
def _const_table(scale, cs):
    return _dev(FR.const_level_table(_spec(scale)[0], FR.level_codes(cs)), F16)


@functools.lru_cache(maxsize=3)
def _gather_inputs(n, scale):
    dirs = FR.dir_rows(n, 2)
    return _dev(FR.point_rows(n, scale), F32), _dev(dirs, F32), FR.sh16(dirs)


def _gather_problem(W, n, cs, scale=SCALE, shrink=()):
    x, dirs, _ = _gather_inputs(n, scale)
    return SimpleNamespace(n=n, x=x, dirs=dirs, enc_pm=None, desc=_spec(scale, shrink)[1].desc,
                           table=_const_table(scale, cs), w16=_dev(FR.flat_weights(W), F16))


def _const_want(W, n, cs):
    """every point encodes to the level codes: one row of references for all of them"""
    enc = FR.level_codes(cs).reshape(1, 32)
    h1, h, h3, h4, o = FR.mlp_fwd_ref64(enc, np.zeros((1, 16)), W)
    return _want(np.tile(h, (n, 1)), np.tile(o, (n, 1)), np.tile(enc, (n, 1)))


B_VARIANTS = [("forward_act", "all"), ("forward_act", "ndev"), ("forward_act", "capped"), ("density", "all"),
              ("density", "ndev"), ("indexed", "list"), ("indexed", "perm"), ("encode_mlp", "all"),
              ("encode_mlp", "ndev"), ("encode_mlp", "list"), ("encode_mlp", "perm"), ("encode_mlp", "capped"),
              ("encode_density", "all"), ("encode_density", "list"), ("hash_encode", "all"), ("hash_encode", "ndev"),
              ("hash_encode", "list")]
B_FAMILY = {"forward_act": "fwd", "density": "fwd", "indexed": "fwd", "encode_mlp": "reg", "encode_density": "reg",
            "hash_encode": "reg"}
B_NAMES = {"forward_act": "ngp_field_forward_act", "density": "ngp_density_forward", "indexed": "ngp_field_forward_indexed",
           "encode_mlp": "ngp_field_encode_mlp_act", "encode_density": "ngp_field_encode_mlp_act (density only)",
           "hash_encode": "ngp_hash_encode"}


@pytest.mark.parametrize("entry,layout", B_VARIANTS)
@pytest.mark.parametrize("n", FR.SIZES + ["multipass"])
def test_gathering_kernels_on_the_constant_table(n, entry, layout):
    n = _size(n, B_FAMILY[entry])
    acts = list(FR.ACTS.values()) if entry in ("forward_act", "encode_mlp") else [FR.RGB_SIGMOID]
    for seed in (0, 1):
        W = FR.lattice_fwd_weights(seed)
        p, want = _gather_problem(W, n, seed), _const_want(W, n, seed)
        for act in acts:
            rows, got = _run(entry, p, layout, act)
            _check(f"{B_NAMES[entry]}, n = {n}, layout {layout}, colour mode {act}, weights lattice({seed}), "
                   f"codes {seed}", got, want, rows, act)


@pytest.mark.parametrize("scale,shrink", [(16.0, ()), (0.5, (7, 12))])
@pytest.mark.parametrize("entry", ["forward_act", "encode_mlp", "hash_encode"])
def test_gathering_kernels_at_scale_16_and_on_the_generic_modulo(entry, scale, shrink):
    n, W = 513, FR.lattice_fwd_weights(0)
    p, want = _gather_problem(W, n, 1, scale, shrink), _const_want(W, n, 1)
    rows, got = _run(entry, p, "all", FR.RGB_NONE)
    _check(f"{B_NAMES[entry]}, n = {n}, scale {scale}, levels {shrink} of size 2^19 - 8", got, want, rows, FR.RGB_NONE)


def _probe_want(k, sign, n, cs, sh):
    """colour mode none: rgb[r] = relu(+-SH column probe_column(k, r)) of the sample's own direction"""
    W = FR.sh_probe_weights(k, sign)
    enc = FR.level_codes(cs).reshape(1, 32)
    h = FR.mlp_fwd_ref64(enc, np.zeros((1, 16)), W)[1]
    cols = [FR.probe_column(k, r, sign) for r in range(3)]
    o = np.stack([np.maximum(sg * sh[:, c], 0.0) + 0.0 for c, sg in cols], 1)
    if n <= 513:  # (the closed form is the reference's: test_probes_reach_every_sh_column_with_both_signs)
        assert np.array_equal(o, FR.mlp_fwd_ref64(np.tile(enc, (n, 1)), sh, W)[4][:, :3])
    return W, _want(np.tile(h, (n, 1)), o, np.tile(enc, (n, 1))), [c for c, _ in cols]


@pytest.mark.parametrize("entry", ["forward_act", "encode_mlp"])
@pytest.mark.parametrize("n", [65, 513, "multipass"])
def test_sh_probes_through_the_gathering_kernels(n, entry):
    """each sample shows three SH components of its own direction: a sample, a lane group or an SH component in the
    wrong place shows as another value"""
    n = _size(n, B_FAMILY[entry])
    sh = _gather_inputs(n, SCALE)[2]
    for k, sign in FR.PROBES:
        W, want, cols = _probe_want(k, sign, n, 0, sh)
        rows, got = _run(entry, _gather_problem(W, n, 0), "all", FR.RGB_NONE)
        _check(f"{B_NAMES[entry]}, n = {n}, SH probe k = {k}, sign {sign}", got, want, rows, FR.RGB_NONE, probe_cols=cols)


# ---------------------------------------------------------------------------------------------------- C. round 1
@pytest.mark.parametrize("kind", ["all", "list"])
@pytest.mark.parametrize("pre", [0, 8])
@pytest.mark.parametrize("R", FR.ROUND1_R + ["multipass"])
def test_round_1_on_the_constant_table(R, pre, kind):
    R = _size(R, "first")
    L, s = vren.lib(), vren._stream()
    codes = FR.level_codes(0).reshape(1, 32)
    h0 = FR.mlp_fwd_ref64(codes, np.zeros((1, 16)), FR.lattice_fwd_weights(0))[1][0, 0]
    c = FR.round1_rows(R, float(np.exp(h0)), kind)  # (the probes share the lattice set's W1 and W2: one density)
    n = c.n_samples
    x, dirs, sh = _gather_inputs(n, SCALE)
    grid = _spec(SCALE)[1]
    table = _const_table(SCALE, 0)
    rays_a, deltas = _dev(c.rays_a, torch.int64), _dev(c.deltas, F32)
    rows = None if c.rows is None else _dev(c.rows, torch.int32)
    n_rows_dev = None if c.rows is None else torch.tensor([c.count], dtype=torch.int64, device=DEV)
    first = c.first
    sets = [("lattice(0)", FR.lattice_fwd_weights(0), None, (FR.RGB_NONE, FR.RGB_SIGMOID)),
            ("SH probe (3, +1)", None, (3, 1), (FR.RGB_NONE,)), ("SH probe (12, -1)", None, (12, -1), (FR.RGB_NONE,))]
    for name, W, probe, acts in sets:
        if probe is None:
            want, cols = _const_want(W, n, 0), None
        else:
            W, want, cols = _probe_want(*probe, n, 0, sh)
        w16 = _dev(FR.flat_weights(W), F16)
        for act in acts:
            label = (f"ngp_field_forward_first_pre_act, R = {R} rows ({kind}), pre_levels {pre}, colour mode {act}, "
                     f"weights {name}")
            pm = _pm_buffer(n)
            sig, rgb = _junk(n + PAD), _junk((n + PAD, 3))
            rest = _junk(R + PAD, torch.int32, -9)
            list2 = _junk(n + PAD, torch.int32, -1) if kind == "list" else None
            total2 = torch.zeros(1, dtype=torch.int64, device=DEV) if kind == "list" else None
            ev = torch.zeros(1, dtype=torch.int64, device=DEV)
            if pre:
                _ok(L.ngp_field_encode_first_coarse(x, rays_a, rows, n_rows_dev, R, n, ctypes.byref(grid.desc), table, pm,
                                                    s), "encode_first_coarse")
                got = _pm_rows(pm, n)
                rt = torch.from_numpy(first).to(DEV)
                _equal_bits(label + ": ngp_field_encode_first_coarse", "levels 0-7", got[:, :16], want.enc16[:, :16],
                            first, rt)
                assert bool((got[:, 16:] == JUNK).all()), label + ": the pre-encode wrote past pair 3"
            _ok(L.ngp_field_forward_first_pre_act(x, dirs, deltas, rays_a, rows, n_rows_dev, R, n, FR.T_THR,
                                                  ctypes.byref(grid.desc), table, w16, pm, sig, rgb, rest, list2, total2,
                                                  ev, pre, act, s), "forward_first_pre_act")
            _check(label, {"enc": _pm_rows(pm, n), "sig": sig, "rgb": rgb}, want, first, act, probe_cols=cols)
            # the round-2 outputs, known from fp64 (each row a factor 2 from T_thr on the log scale)
            got_rest = rest.cpu().numpy().astype(np.int64)
            bad = np.nonzero(got_rest[:R] != c.rest)[0]
            assert bad.size == 0, (f"{label}: rest differs for {bad.size} rows, first row {bad[:1]} (N = "
                                   f"{c.N[bad[:1]]}, ln T = {c.lnT[bad[:1]]}): got {got_rest[bad[:1]]}, want "
                                   f"{c.rest[bad[:1]]}")
            assert (got_rest[R:] == -9).all(), label + ": rest was written past the rows"
            if kind == "list":
                T = int(total2)
                assert T == c.total2 and int(ev) == c.evaluated + c.total2, (label, T, c.total2, int(ev), c.evaluated)
                got2 = list2.cpu().numpy().astype(np.int64)
                assert np.array_equal(np.sort(got2[:T]), c.list2), label + ": the round-2 list holds other samples"
                assert (got2[T:] == -1).all(), label + ": the round-2 list was written past its length"
                steps = got2[1:T] - got2[:T - 1]  # each row's run contiguous and ascending
                assert int((steps == 1).sum()) == T - int((c.rest > 0).sum()), label + ": a row's run is broken"
            else:
                assert int(ev) == c.evaluated, (label, int(ev), c.evaluated)


# ---------------------------------------------------------------------------- D. real parameters at the edges
@functools.lru_cache(maxsize=None)
def _real_field():
    import test_field_gpu as TF
    f, flat = TF._oracle_and_params(SCALE)
    x, d = TF._points(20000, SCALE)
    return f, flat.to(DEV).half(), x, d


@functools.lru_cache(maxsize=2)
def _real_points(n):
    """half marched samples, half random points with the box corners first; past test_field_gpu's 20512 points:
    points inside and up to 3x outside the box"""
    _, _, x, d = _real_field()
    m = x.shape[0] - 512
    if n <= x.shape[0]:
        ix = torch.cat([torch.arange(n // 2), m + torch.arange(n - n // 2)])
        return x[ix].contiguous(), d[ix].contiguous()
    extra = n - x.shape[0]
    return (torch.cat([x, torch.from_numpy(FR.point_rows(extra, SCALE, 3))]).contiguous(),
            torch.cat([d, torch.from_numpy(FR.dir_rows(extra, 3))]).contiguous())


def _oracle_rows(n):
    """the rows the oracle evaluates: all of a small set; of a multi-pass one the first 1024, the last 1024 and
    8192 random rows, 1500 of them past the rows any first iteration of the register kernel (or, at the smaller
    size, of field_fwd_kernel) can reach"""
    if n <= 4096:
        return np.arange(n)
    mp = _mp()
    past = mp.reg_first_pass if n > mp.reg_first_pass else mp.fwd_first_pass
    assert n - past >= 1500
    rng = np.random.default_rng(n)
    pick = np.concatenate([np.arange(1024), np.arange(n - 1024, n), past + rng.choice(n - past, 1500, replace=False),
                           rng.choice(n, 8192 - 1500, replace=False)])
    return np.unique(pick)


D_VARIANTS = [("density", "all"), ("indexed", "perm"), ("encode_mlp", "all"), ("encode_mlp", "perm"),
              ("encode_mlp", "ndev"), ("encode_density", "all"), ("hash_encode", "all"), ("hash_encode", "perm"),
              ("split", "all"), ("split", "perm")]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, "multipass_fwd", "multipass_reg"])
def test_real_parameters_at_the_edges(n):
    """The fused forward (ngp_field_forward_act) against the oracle on the stated rows: the encoding bit for bit, h,
    sigma and rgb within oracle.mlp_forward_bound per point (test_field_forward_parity's bar); every other entry
    point, and the split ngp_hash_encode + ngp_field_mlp_forward, bit-equal to it over ALL processed rows."""
    n = {"multipass_fwd": _mp().fwd, "multipass_reg": _mp().reg}.get(n, n)
    f, p16, _, _ = _real_field()
    x, d = _real_points(n)
    p = SimpleNamespace(n=n, x=x.to(DEV), dirs=d.to(DEV), enc_pm=None, desc=HG.HashGrid(SCALE).desc,
                        table=p16[HG.MLP_PARAMS:], w16=p16[:HG.MLP_PARAMS].contiguous())
    _, base = _run("forward_act", p, "all", FR.RGB_SIGMOID)
    assert all(bool((v[n:] == JUNK).all()) for v in base.values()), "ngp_field_forward_act wrote into the pad"
    # against the oracle
    pick = _oracle_rows(n)
    ix = torch.from_numpy(pick)
    xs, ds = x[ix], d[ix]
    enc_ref = O.hash_encode_fwd(f.spec, xs, f.xyz_min, f.xyz_max, f.xyz_params.detach()[f.n_dens:])
    got = {k: v[:n][ix.to(DEV)].cpu() for k, v in base.items()}
    bad = (got["enc"].view(torch.int16) != enc_ref.view(torch.int16)).any(1)
    assert not bool(bad.any()), (f"ngp_field_forward_act, n = {n}: the encoding differs from the oracle's in "
                                 f"{int(bad.sum())} of {len(pick)} rows, first {FR.row_position(int(pick[_first(bad)]))}")
    Wd, _ = O.mlp_layers(f.xyz_params.detach()[:f.n_dens], f.dens_dims)
    h_ref, hb = O.mlp_forward_bound(enc_ref, Wd)
    dh = (got["h"].float() - h_ref).abs()
    assert bool((dh <= hb).all()), f"n = {n}: h past the bound, worst ratio {float((dh / hb).max()):.3f}"
    dls = (torch.log(got["sig"].double()) - h_ref[:, 0].double()).abs()
    assert bool((dls <= hb[:, 0] + SIG_REL).all()), f"n = {n}: ln sigma past the bound"
    Wc, _ = O.mlp_layers(f.rgb_params.detach(), f.color_dims)
    cin = torch.cat([O.sh4(ds).float(), h_ref], 1)
    out, lb = O.mlp_forward_bound(cin.half(), Wc, d_in=torch.cat([torch.zeros(cin.shape[0], 16), hb], 1))
    rgb_ref = O.rh(torch.sigmoid(out[:, :3]))
    assert bool(((got["rgb"] - rgb_ref).abs() <= 0.25 * lb[:, :3] + O.ulp16(rgb_ref)).all()), f"n = {n}: rgb past the bound"
    print(f"n = {n}: {len(pick)} oracle rows, worst |dh| / bound {float((dh / hb).max()):.3f}")
    # every other entry point against the fused one, all rows, bit for bit
    want = SimpleNamespace(enc16=base["enc"][:n], h16=base["h"][:n], sig=base["sig"][:n], rgb=base["rgb"][:n])
    for entry, layout in D_VARIANTS:
        if entry == "split":
            rows, enc_got = _run("hash_encode", p, layout)
            p2 = SimpleNamespace(**{**vars(p), "enc_pm": enc_got["enc"][:n].reshape(n, 8, 4).permute(1, 0, 2).contiguous()})
            rows, outs = _run("mlp_forward", p2, layout)
        else:
            rows, outs = _run(entry, p, layout, FR.RGB_SIGMOID)
        rt = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(DEV)
        label = f"{entry} ({layout}) against ngp_field_forward_act, n = {n}"
        for key, ref in (("enc", want.enc16), ("h", want.h16), ("sig", want.sig), ("rgb", want.rgb)):
            if key in outs:
                _equal_bits(label, key, outs[key], ref, rows, rt)


def test_zz_report():
    """(runs last in this file) what the tolerant comparisons saw"""
    s, p = _seen["sigmoid"], _seen["probe"]
    print(f"sigmoid rgb bit-equal to oracle.rh(sigmoid) in fp32: {s[0]} of {s[1]} values")
    print(f"SH probe values not bit-equal to fp16(oracle.sh4): {p[0]} of {p[1]}, SH columns {sorted(p[2])}")
