"""The fp64 references and rounding bounds of tests/hash_ref.py are sound:
the oracle's own fp32 scatter and fp32 Adam (plain C loops) lie within them,
and every input set of test_hashbin_gpu.py meets its precondition -- all
without a GPU."""
import pytest
import torch

import hash_ref as R
import oracle as O

U = R.U


def test_oracle_scatter_within_the_summation_bound():
    """oracle.hash_encode_bwd (fp32, sample order) vs scatter_ref64, at EVERY
    entry: |err| <= (cnt + 16) u mag, and bit-zero where mag == 0.  20 000
    points, 4 000 of them copies of one point (entries with thousands of
    terms), dL/denc spanning six decades."""
    scale = 0.5
    sp = R.spec(scale)
    mn, mx = R.box(scale)
    g = torch.Generator().manual_seed(41)
    x = R._uniform_points(20000, scale, g)
    x[16000:] = torch.tensor([0.1234, -0.2345, 0.3456])
    decade = 10.0 ** (-torch.randint(0, 7, (20000, 1), generator=g).float())
    denc = torch.randn(20000, 32, generator=g) * 1e-2 * decade
    ref, mag, cnt = R.scatter_ref64(sp, x, mn, mx, denc)
    got = O.hash_encode_bwd(sp, x, mn, mx, denc)
    err = (got.double() - ref).abs()
    bound = R.scatter_bound(sp, ref, mag, cnt)
    live = mag > 0
    ratio = float((err[live] / bound[live]).max())
    in_u = float((err[live] / (U * mag[live])).max())
    print(f"oracle scatter: worst err/bound {ratio:.3f}, {in_u:.2f} u mag, up to {int(cnt.max())} terms per entry")
    assert int(cnt.max()) >= 4000
    assert bool((err <= bound).all()), ratio
    assert bool((got[~live] == 0).all()) and not bool(torch.signbit(got[~live]).any())
    # the bound is tight enough to see one lost term: dropping the largest
    # term of a many-term entry moves it past its bound
    e = int(torch.argmax(cnt * live))
    assert float(mag[e]) / float(cnt[e]) > float(bound[e])


@pytest.mark.parametrize("step,grad_scale", [(1, 1.0), (1000, 0.5), (1, 0.5), (1000, 1.0)])
def test_oracle_adam_within_the_bounds(step, grad_scale):
    """or_adam (fp32 Adam in C) fed the fp32 bias corrections (as adam_bias
    forms them) vs adam_ref64 on the GPU tests' state, 2 M elements: m, v, p
    within dm, dv, dp; the update is resolved (dupd <= 0.1 |upd|) wherever the
    new m is not a cancellation; an element without gradient gets exactly
    fp32(b1 m0), fp32(b2 v0)."""
    n = 1 << 21
    p0, m0, v0 = R.adam_state(n, seed=7)
    gen = torch.Generator().manual_seed(8)
    g = (torch.randn(n, generator=gen) * 10.0 ** (-torch.randint(1, 7, (n,), generator=gen).float())).float()
    g[::3] = 0.0
    r = R.adam_ref64(p0, m0, v0, g.double(), 1e-2, step, grad_scale=grad_scale)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    gs = (g * grad_scale).contiguous()  # (x 0.5 / x 1: exact)
    O.lib().or_adam(n, O._p(p), O._p(gs), O._p(m), O._p(v), 1e-2, 0.9, 0.999, 1e-15, r.bc1, r.bc2)
    rm = float(((m.double() - r.m).abs() / r.dm).max())
    rv = float(((v.double() - r.v).abs() / r.dv).max())
    rp = float(((p.double() - r.p).abs() / r.dp).max())
    res = float((r.dupd / r.upd.abs())[~r.cancel].max())
    print(f"oracle adam step {step} x{grad_scale}: err/bound m {rm:.2f} v {rv:.2f} p {rp:.2f}; "
          f"dupd/|upd| <= {res:.1e} off cancellations ({float(r.cancel.float().mean()):.1e} of the elements)")
    assert rm <= 1 and rv <= 1 and rp <= 1
    assert res <= 0.1 and float(r.cancel.float().mean()) < 0.02
    z = g == 0
    assert torch.equal(m[z], (torch.tensor(0.9) * m0)[z]) and torch.equal(v[z], (torch.tensor(0.999) * v0)[z])
    # a skipped, doubled or unscaled update is far outside dp
    for wrong in (p0.double(), p0.double() - 2 * r.upd, p0.double() - r.upd / grad_scale if grad_scale != 1 else None):
        if wrong is not None:
            assert float((((wrong - r.p).abs() > r.dp) | r.cancel).float().mean()) > 0.6


def test_adam_bias_in_host_doubles_is_outside_the_fp32_bound():
    """Measured deviation: adam_bias raises the fp32 betas with
    powf; oracle.adam_ (as apex does) forms 1 - beta**step in host doubles.  At
    step 1000 the two bc2 differ by ~7.5e-6 relative, which puts the double
    form several times outside dp -- so the GPU checks use the fp32 form."""
    n = 1 << 18
    p0, m0, v0 = R.adam_state(n, seed=9)
    g = (torch.randn(n, generator=torch.Generator().manual_seed(10)) * 1e-3).float()
    r = R.adam_ref64(p0, m0, v0, g.double(), 1e-2, 1000)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    O.adam_(p, g, m, v, 1e-2, 1000)
    worst = float(((p.double() - r.p).abs() / r.dp).max())
    rel_bc2 = abs((1 - 0.999 ** 1000) / r.bc2 - 1)
    rel_upd = float(((p.double() - r.p).abs() / r.upd.abs())[~r.cancel].median())
    print(f"host-double bias at step 1000: bc2 differs by {rel_bc2:.2e} relative, the update by {rel_upd:.2e} "
          f"(median), worst err/dp {worst:.1f}")
    assert 1e-6 < rel_bc2 < 2e-5
    assert worst > 1.0


@pytest.mark.parametrize("name,scale", [("scattered", 0.5), ("rays", 0.5), ("rays", 16.0), ("pile", 0.5),
                                        ("sparse", 0.5), ("straddle", 0.5), ("straddle", 16.0), ("none", 0.5)])
def test_input_sets_meet_their_preconditions(name, scale):
    """input_set asserts what each set is built to reach (multi-chunk buckets,
    empty buckets, split pairs on dense and hashed levels, runs, a partial
    last tile); the reference of a set is finite and non-trivial."""
    s = R.input_set(name, scale)
    ref, mag, cnt = R.reference(name, scale)
    assert bool(torch.isfinite(ref).all())
    assert s.m <= 41000
    if name == "none":
        assert s.m == 0 and float(mag.max()) == 0
        return
    sp = R.spec(scale)
    for l in range(sp.L):
        assert float(mag[2 * int(sp.offsets[l]):2 * int(sp.offsets[l + 1])].max()) > 0
    if name == "straddle":  # the x+1 corners that get direct adds exist on the levels the set is for
        i0 = R.info(name, scale, 0, 0)
        lv = range(1, 6) if scale == 0.5 else (1, 2, 3, 13, 14, 15)
        for l in lv:
            assert int(i0.nstr[2 * int(sp.offsets[l]):2 * int(sp.offsets[l + 1])].sum()) >= 40, l
