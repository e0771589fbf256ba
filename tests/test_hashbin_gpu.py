"""The hash-table backward -- per-sample atomics (hash_bwd.hip) and the binned
path (hashbin.hip) -- and the FusedAdam folded into the binned accumulation,
each held to an fp64 reference outside the product, entry by entry and per
level: tests/hash_ref.py's scatter_ref64 / adam_ref64 (built from the oracle's
corner indices and weights) and the rounding bounds derived there.  The input
sets are built to reach one branch each (hash_ref.input_set asserts that they
do): a partial last tile behind a sample_idx subset, runs along rays, buckets
of several chunks, empty buckets, x pairs split by a bucket boundary on dense
and on hashed levels, a device count of 0.  Every check prints its worst
err / bound per level."""
import ctypes

import pytest
import torch

import hash_ref as R
import hashgrid as HG
import vren

pytestmark = pytest.mark.gpu
DEV = "cuda"
B1, B2, EPS, LR = 0.9, 0.999, 1e-15, 1e-2
# (level_lo, merge_hi): the trainer's two defaults (one cascade / cascaded) and their unmerged forms
CONFIGS = [(8, 11), (8, 8), (0, 16), (0, 0)]
SETS = [("scattered", 0.5), ("rays", 0.5), ("rays", 16.0), ("pile", 0.5), ("sparse", 0.5), ("straddle", 0.5),
        ("straddle", 16.0), ("none", 0.5)]
CAP = 40192  # workspace samples: the largest set (pile, 40 007) in whole tiles

_cache = {}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _case(name, scale):
    """the set's device buffers + its fp64 reference on the device (built once, read-only)"""
    key = (name, scale)
    if key not in _cache:
        s = R.input_set(name, scale)
        ref, mag, cnt = (t.to(DEV) for t in R.reference(name, scale))
        grid = HG.HashGrid(scale)
        sp = R.spec(scale)
        assert list(grid.offsets) == [int(o) for o in sp.offsets]
        _cache[key] = dict(s=s, sp=sp, grid=grid, desc=ctypes.byref(grid.desc), n=s.x.shape[0], x=s.x.to(DEV),
                           sidx=s.sidx.to(DEV) if s.sidx is not None else None, denc=s.denc.to(DEV),
                           n_dev=torch.tensor([s.m], dtype=torch.int64, device=DEV), ref=ref, mag=mag, cnt=cnt,
                           n2=2 * sp.n_entries)
    return _cache[key]


def _n32(c, lo, mh):
    key = ("n32", c["s"].name, c["s"].scale, lo, mh)
    if key not in _cache:
        _cache[key] = R.info(c["s"].name, c["s"].scale, lo, mh).n32.to(DEV)
    return _cache[key]


def _ws(cap):
    if ("ws", cap) not in _cache:
        nbytes = HG._lib().ngp_hash_backward_binned_workspace(cap)
        _cache[("ws", cap)] = torch.empty((nbytes + 255) // 256, 64, dtype=torch.int32, device=DEV)
    return _cache[("ws", cap)]


def _base(c, kind):
    if kind == "zero":
        return torch.zeros(c["n2"], device=DEV)
    g = torch.Generator(device=DEV).manual_seed(77)
    return torch.randn(c["n2"], generator=g, device=DEV) * 1e-2


def _bits(t):
    return t.view(torch.int32)


def _check_scatter(c, out, base, n32, lo, what):
    """out vs base + ref at every element: within the bound; bitwise the base where nothing contributes"""
    torch.cuda.synchronize()
    sp = c["sp"]
    err = (out.double() - (base.double() + c["ref"])).abs()
    bound = R.scatter_bound(sp, c["ref"], c["mag"], c["cnt"], n32=n32, level_lo=lo,
                            base=base if float(base.abs().max()) > 0 else None)
    ratios = R.level_ratios(sp, err, bound)
    print(f"{what}: worst err/bound {max(ratios):.3f} | per level " + " ".join(f"{r:.2f}" for r in ratios))
    dead = c["mag"] == 0
    assert torch.equal(_bits(out)[dead], _bits(base)[dead]), what
    assert bool(torch.isfinite(out).all()), what
    assert max(ratios) <= 1.0, (what, ratios)
    return max(ratios)


def _binned(c, out, ws, cap, lo, mh):
    L = HG._lib()
    vren._ok(L.ngp_hash_backward_binned(_p(c["x"]), c["n"], _p(c["n_dev"]), _p(c["sidx"]), c["desc"], _p(c["denc"]),
                                        _p(out), _p(ws), cap, lo, mh, vren._stream()), "hash_backward_binned")
    vren._ok(L.ngp_hash_backward_levels(_p(c["x"]), c["n"], _p(c["n_dev"]), _p(c["sidx"]), c["desc"], _p(c["denc"]),
                                        _p(out), 0, lo, vren._stream()), "hash_backward_levels")


@pytest.mark.parametrize("name,scale", [("scattered", 0.5), ("pile", 0.5), ("straddle", 0.5), ("straddle", 16.0)])
def test_atomic_scatter_matches_fp64_reference(name, scale):
    """ngp_hash_backward (per-sample fp32 atomics, run heads merged per wave),
    all 16 levels: (cnt + 16) u mag per element, onto a zero and a random base."""
    c = _case(name, scale)
    for kind in ("zero", "random"):
        base = _base(c, kind)
        out = base.clone()
        vren._ok(HG._lib().ngp_hash_backward(_p(c["x"]), c["n"], _p(c["n_dev"]), _p(c["sidx"]), c["desc"],
                                             _p(c["denc"]), _p(out), vren._stream()), "hash_backward")
        _check_scatter(c, out, base, None, R.N_LEVELS, f"atomic {name}@{scale} {kind} base")


@pytest.mark.parametrize("lo,mh", CONFIGS)
@pytest.mark.parametrize("name,scale", SETS)
def test_binned_scatter_matches_fp64_reference(name, scale, lo, mh):
    """ngp_hash_backward_binned (+ ngp_hash_backward_levels below level_lo):
    10 u mag on the binned levels whatever the number of terms, (n32 + 10) u
    mag where n32 fp32 terms pass through memory (split pairs' x+1 corners,
    buckets of several chunks), (cnt + 16) u mag on the atomic levels."""
    c = _case(name, scale)
    n32 = _n32(c, lo, mh)
    if name == "pile" and mh == 0:
        assert int(R.info(name, scale, lo, mh).nch[lo:].max(1).values.min()) >= 2  # several chunks on every binned level
    if name == "straddle" and (lo == 0 or scale == 16.0):  # (scale 0.5: split pairs on dense levels 1-5 only)
        assert int((n32 > 0).sum()) >= 40
    for kind in ("zero", "random"):
        base = _base(c, kind)
        out = base.clone()
        _binned(c, out, _ws(CAP), CAP, lo, mh)
        _check_scatter(c, out, base, n32, lo, f"binned({lo},{mh}) {name}@{scale} {kind} base")


@pytest.mark.parametrize("order", ["coarse_first", "fine_first"])
@pytest.mark.parametrize("name,scale,mh", [("scattered", 0.5, 11), ("pile", 0.5, 8), ("straddle", 16.0, 11)])
def test_split_entry_points_accumulate_level_ranges(name, scale, mh, order):
    """plan -> write -> accum_levels over [8, 12) and [12, 16) (the
    data-parallel trainer's segments), in either order: after the first range
    the other range still holds what the write left there -- the base, bit for
    bit, except the x+1 corners of split pairs, which the write adds directly --
    and the whole matches the fp64 reference."""
    c = _case(name, scale)
    L, lo = HG._lib(), 8
    n32 = _n32(c, lo, mh)
    off = [2 * int(o) for o in c["sp"].offsets]
    ranges = [(8, 12), (12, 16)] if order == "coarse_first" else [(12, 16), (8, 12)]
    ws = _ws(CAP)
    for kind in ("zero", "random"):
        base = _base(c, kind)
        out = base.clone()
        args = (_p(c["x"]), c["n"], _p(c["n_dev"]), _p(c["sidx"]), c["desc"])
        vren._ok(L.ngp_hash_binned_plan(*args, _p(ws), CAP, lo, mh, vren._stream()), "plan")
        vren._ok(L.ngp_hash_binned_write(*args, _p(c["denc"]), _p(out), _p(ws), CAP, lo, mh, vren._stream()), "write")
        written = out.clone()
        direct = R.info(name, scale, lo, mh).nstr.to(DEV) > 0
        assert torch.equal(_bits(written)[~direct], _bits(base)[~direct])
        (a0, a1), (b0, b1) = ranges
        vren._ok(L.ngp_hash_binned_accum_levels(c["desc"], _p(out), _p(ws), CAP, lo, mh, a0, a1, vren._stream()), "accum")
        torch.cuda.synchronize()
        assert torch.equal(_bits(out)[off[b0]:off[b1]], _bits(written)[off[b0]:off[b1]])
        assert torch.equal(_bits(out)[:off[lo]], _bits(base)[:off[lo]])
        assert not torch.equal(out[off[a0]:off[a1]], written[off[a0]:off[a1]])
        vren._ok(L.ngp_hash_binned_accum_levels(c["desc"], _p(out), _p(ws), CAP, lo, mh, b0, b1, vren._stream()), "accum")
        vren._ok(L.ngp_hash_backward_levels(*args, _p(c["denc"]), _p(out), 0, lo, vren._stream()), "levels")
        _check_scatter(c, out, base, n32, lo, f"split {order} {name}@{scale} {kind} base")


@pytest.mark.parametrize("lo,mh", CONFIGS)
def test_workspace_overflow_spills_to_atomics(lo, mh):
    """max_samples = 256 on `scattered`: every tile but the first takes the
    per-sample atomic path and every bucket is flushed with atomics --
    (cnt + 16) u mag."""
    c = _case("scattered", 0.5)
    assert c["s"].m > 4 * 256
    for kind in ("zero", "random"):
        base = _base(c, kind)
        out = base.clone()
        _binned(c, out, _ws(256), 256, lo, mh)
        _check_scatter(c, out, base, None, R.N_LEVELS, f"overflow({lo},{mh}) {kind} base")


@pytest.mark.parametrize("lo,mh", [(0, 16), (0, 0), (8, 11)])
def test_one_workspace_across_different_inputs(lo, mh):
    """one workspace allocation (filled with junk first) for pile, then sparse,
    then straddle, then nothing, then pile again: no stale counter, flag or
    plan survives a call"""
    ws = torch.randint(-2 ** 31, 2 ** 31 - 1, _ws(CAP).shape, dtype=torch.int32, device=DEV)
    for name, scale in [("pile", 0.5), ("sparse", 0.5), ("straddle", 0.5), ("none", 0.5), ("pile", 0.5)]:
        c = _case(name, scale)
        base = _base(c, "zero")
        out = base.clone()
        _binned(c, out, ws, CAP, lo, mh)
        _check_scatter(c, out, base, _n32(c, lo, mh), lo, f"reused workspace({lo},{mh}) {name}")


ADAM_CASES = [("scattered", 0.5, 8, 11, CAP), ("sparse", 0.5, 8, 11, CAP), ("pile", 0.5, 0, 0, CAP),
              ("straddle", 0.5, 0, 0, CAP), ("straddle", 16.0, 0, 16, CAP), ("scattered", 0.5, 8, 11, 256),
              ("none", 0.5, 8, 11, CAP)]


@pytest.mark.parametrize("step_dev,grad_scale", [(0, 1.0), (999, 0.5), (0, 0.5), (999, 1.0)])
@pytest.mark.parametrize("name,scale,lo,mh,cap", ADAM_CASES)
def test_fused_adam_matches_fp64_adam(name, scale, lo, mh, cap, step_dev, grad_scale):
    """ngp_hash_binned_apply_adam (after plan) and ngp_hash_binned_accum_adam
    (after plan + write) vs adam_ref64 fed scatter_ref64's gradient, from
    non-zero moments: m, v, p within dm, dv, dp per element of the binned
    levels; the fp16 shadow is the rounded master; the gradient is left zero;
    an element without contribution decays exactly (m = fp32(b1 m0), v =
    fp32(b2 v0)) and moves; nothing below level_lo is touched.  pile: buckets
    of several chunks (residual kernel); straddle: flagged buckets under the
    fused flush; cap 256: overflow, every bucket through the residual kernel;
    sparse / none: most elements have no contribution (the empty-bucket loop)."""
    c = _case(name, scale)
    L, sp, n2 = HG._lib(), c["sp"], c["n2"]
    split = 2 * int(sp.offsets[lo])
    overflow = c["s"].m > cap
    n32 = None if overflow else _n32(c, lo, mh)
    info = R.info(name, scale, lo, mh)
    if name == "pile":
        assert int(info.nch[lo:].max(1).values.min()) >= 2
    if name == "straddle":
        assert int((info.nstr > 0).sum()) >= 40
    dg = R.scatter_bound(sp, c["ref"], c["mag"], c["cnt"], n32=n32, level_lo=lo if not overflow else R.N_LEVELS)
    p0, m0, v0 = R.adam_state(n2, seed=91, device=DEV)
    r = R.adam_ref64(p0, m0, v0, c["ref"], LR, step_dev + 1, B1, B2, EPS, grad_scale, dg=dg)
    lr_dev = torch.tensor([LR], device=DEV)
    st_dev = torch.tensor([step_dev], dtype=torch.int64, device=DEV)
    g0 = torch.zeros(n2, device=DEV)
    g0[:split] = torch.randn(split, device=DEV, generator=torch.Generator(device=DEV).manual_seed(92))
    h0 = torch.full((n2,), 7.0, dtype=torch.float16, device=DEV)
    empty = (c["cnt"] == 0)[split:]
    if name in ("sparse", "none"):
        assert float(empty.float().mean()) > 0.5  # the majority: all of it for `none`
    res = (r.dupd / r.upd.abs())[split:][~r.cancel[split:]]
    assert float(res.max()) <= 0.1 and float(r.cancel[split:].float().mean()) < 0.02, float(res.max())
    ws = _ws(cap)
    args = (_p(c["x"]), c["n"], _p(c["n_dev"]), _p(c["sidx"]), c["desc"])
    for entry in ("apply_adam", "accum_adam"):
        p, m, v, grad, p16 = p0.clone(), m0.clone(), v0.clone(), g0.clone(), h0.clone()
        adam = (_p(p), _p(m), _p(v), _p(p16), _p(lr_dev), B1, B2, EPS, _p(st_dev), grad_scale, vren._stream())
        vren._ok(L.ngp_hash_binned_plan(*args, _p(ws), cap, lo, mh, vren._stream()), "plan")
        if entry == "apply_adam":
            vren._ok(L.ngp_hash_binned_apply_adam(*args, _p(c["denc"]), _p(grad), _p(ws), cap, lo, mh, *adam), entry)
        else:
            vren._ok(L.ngp_hash_binned_write(*args, _p(c["denc"]), _p(grad), _p(ws), cap, lo, mh, vren._stream()),
                     "write")
            vren._ok(L.ngp_hash_binned_accum_adam(c["desc"], _p(grad), _p(ws), cap, lo, mh, *adam), entry)
        torch.cuda.synchronize()
        what = f"{entry} {name}@{scale} ({lo},{mh}) cap {cap} step_dev {step_dev} x{grad_scale}"
        rm = float(((m.double() - r.m).abs() / r.dm)[split:].max())
        rv = float(((v.double() - r.v).abs() / r.dv)[split:].max())
        rp = float(((p.double() - r.p).abs() / r.dp)[split:].max())
        print(f"{what}: worst err/bound m {rm:.3f} v {rv:.3f} p {rp:.3f}; dupd/|upd| <= {float(res.max()):.3f}; "
              f"{float(empty.float().mean()):.3f} of the elements without contribution")
        assert rm <= 1 and rv <= 1 and rp <= 1, what
        assert torch.equal(p16[split:].view(torch.int16), p[split:].half().view(torch.int16)), what
        assert float(grad[split:].abs().max()) == 0.0, what
        # no contribution: exact decay of the moments, and the parameter moves
        b1m = torch.tensor(B1, device=DEV) * m0[split:]
        b2v = torch.tensor(B2, device=DEV) * v0[split:]
        assert torch.equal(_bits(m[split:])[empty], _bits(b1m)[empty]), what
        assert torch.equal(_bits(v[split:])[empty], _bits(b2v)[empty]), what
        must_move = empty & (r.upd[split:].abs() > 4 * R.U * p0[split:].abs().double())
        if int(empty.sum()):
            assert float(must_move.sum()) > 0.99 * float(empty.sum()), what
            assert bool((p[split:] != p0[split:])[must_move].all()), what
        # below level_lo: untouched
        for a, b in ((p, p0), (m, m0), (v, v0), (grad, g0)):
            assert torch.equal(_bits(a[:split]), _bits(b[:split])), what
        assert torch.equal(p16[:split].view(torch.int16), h0[:split].view(torch.int16)), what
