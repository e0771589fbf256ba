"""tests/sg_shadow_ref.py (the per-pair fp64 restatement of the SSDF soft
shadows), sg_shadow.sg_shadow_torch (the torch formulation) and the CPU path of
sg_shadow.SGShadow held to tests/golden/sg_shadow.npz, which the reference's
own insert/sg_shadow.py produced in fp64 and fp32
(tests/golden/make_sg_shadow_golden.py); what that fixture's designed inputs
must hold for the GPU tests to mean anything; the blur-and-apply step; and the
new entry points' declarations and argument checks.  No GPU.

Bars.  fp64 against fp64: 1e-9 absolute -- values lie in [0,1] and sums have at
most 128 terms, so this is orders above fp64 rounding and orders below the
recorded fp32 deviations.  fp32: |x - ref64| <= 4 x the class's recorded
deviation (factor_dev / decay_dev: the reference's own fp32 runs against its
fp64 run, the maximum over three orders of the C axis).  Every point and every
pair is in exactly one class.  Recorded deviations (C = 128, no rotation):
factor inside 1.9e-7, outside 2.1e-7; decay low 0, saturated 0, deep 3.3e-3,
high 7.0e-8, mid 3.0e-6.
"""
import ctypes

import numpy as np
import pytest
import torch

import sg_shadow_ref as SR
from capi import C as CONSTS, FUNCS
from fixture_model import load

CS = (5, 67, 128)
FP64_BAR = 1e-9


@pytest.fixture(scope="module")
def fx():
    return load("sg_shadow")


@pytest.fixture(scope="module")
def restated(fx):
    """the fp64 restatement of every recorded case, computed once: (C, k) -> sg_shadow_ref's result (the decay call)"""
    return {(C, k): SR.sg_shadow_ref(**case(fx, C, k), rotate_lights=True) for C in CS for k in (0, 1)}


def case(fx, C, k, L=33):
    """the inputs of one recorded case as numpy arrays: the first C components, rotation k (0 none, 1 rot_inv),
    the first L lights"""
    return dict(coeff=np.ascontiguousarray(fx["coeff"][..., :C]), components=np.ascontiguousarray(fx["components"][:C]),
                mean=fx["mean"], fh_tab=fx["fh_tab"], vol_range=float(fx["vol_range"]), scale=float(fx["scale"]),
                pts=fx["pts"], model_pos=fx["model_pos"], lSGs=np.ascontiguousarray(fx["lSGs"][:L]),
                rot_inv=fx["rot_inv"] if k else None, angle_decay_fac=float(fx["angle_decay_fac"]),
                shadow_pow_fac=float(fx["shadow_pow_fac"]), self_shadow_pow_fac=float(fx["self_shadow_pow_fac"]))


def rotated(fx, k, L=33):
    """main.py:496-499: the lights the factor call is handed (axes rotated in fp32 when there is a rot_inv)"""
    return np.ascontiguousarray((fx["lSGs_rot"] if k else fx["lSGs"])[:L])


def assert_factor(fx, sfx, k, got, ref64, idx=None, what=""):
    """got (n) against ref64 (n) per point class; idx: the fixture point of every entry"""
    cls = fx[f"point_class_{sfx}"][k]
    cls = cls if idx is None else cls[idx]
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    seen = np.zeros(got.shape, dtype=bool)
    for i, name in enumerate(SR.POINT_CLASSES):
        m = cls == i
        seen |= m
        if not m.any():
            continue
        err, bar = np.abs(got[m] - ref64[m]).max(), 4 * fx[f"factor_dev_{sfx}"][k, i]
        print(f"{what} factor {name}: max err {err:.2e}, bar {bar:.2e}")
        assert err <= bar, (what, name, err, bar)
    assert seen.all()


def assert_decay(fx, sfx, k, got, ref64, idx=None, lights=None, what=""):
    """got (n,l) against ref64 (n,l) per pair class; idx / lights: the fixture point / light of every row / column"""
    cls = fx[f"pair_class_{sfx}"][k]
    cls = cls if idx is None else cls[idx]
    cls = cls if lights is None else cls[:, lights]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref64.shape == cls.shape and np.isfinite(got).all(), what
    seen = np.zeros(got.shape, dtype=bool)
    for i, name in enumerate(SR.PAIR_CLASSES):
        m = cls == i
        seen |= m
        if not m.any():
            continue
        err, bar = np.abs(got[m] - ref64[m]).max(), 4 * fx[f"decay_dev_{sfx}"][k, i]
        print(f"{what} decay {name}: max err {err:.2e}, bar {bar:.2e}")
        assert err <= bar, (what, name, err, bar)
    assert seen.all()


def _t(a, dtype=None):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dtype or torch.from_numpy(v).dtype)
                if isinstance(v, np.ndarray) else v) for k, v in a.items()}


# ------------------------------------------------------------------ the fixture
def test_fixture_is_the_designed_one(fx):
    assert fx["coeff"].shape == (5, 5, 5, 128) and fx["components"].shape == (128, 7, 14)
    assert fx["mean"].shape == (7, 14) and fx["fh_tab"].shape == (24, 32) and fx["lSGs"].shape == (33, 7)
    assert list(fx["Cs"]) == list(CS) and fx["pts"].shape == (70, 3)
    assert fx["factor64_l32"].shape == (2, 70) and np.all(fx["factor_dev_l32"] > 0)
    assert np.abs(fx["factor64_l32"] - fx["factor64_c128"]).max() > 1e-4          # light 32 shows
    for k in ("coeff", "components", "mean", "fh_tab", "pts", "model_pos", "lSGs", "rot_inv"):
        assert fx[k].dtype == np.float32, k
    tab = fx["fh_tab"]
    assert np.all(tab[:, 0] == 0) and np.all(tab >= 0) and np.all((tab == 0) | (tab >= 1e-30))   # fh(-pi/2) = 0
    assert tab[:, -1].min() > 0 and np.all(tab[:, -1] > tab[:, 8]) and np.all(tab[0] > tab[-1][None] - 1e-12)
    # asymmetric data: no axis of the volume, the env map or the table can be swapped unnoticed
    co = fx["coeff"].astype(np.float64)
    for perm in ((1, 0, 2, 3), (2, 1, 0, 3), (0, 2, 1, 3)):
        assert np.abs(co - co.transpose(perm)).max() > 0.5
    assert np.abs(co - co[::-1]).max() > 0.5 and np.abs(fx["mean"] - fx["mean"][::-1]).max() > 0.3
    assert np.abs(fx["mean"] - fx["mean"][:, ::-1]).max() > 0.3
    rot = fx["rot_inv"].astype(np.float64)
    assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-6 and np.abs(rot - np.eye(3)).max() > 0.3
    # lights
    l = fx["lSGs"]
    ax, lam = l[:, :3], l[:, 3]
    assert np.all(np.abs(np.linalg.norm(ax.astype(np.float64), axis=1) - 1) < 1e-6)
    assert any(np.array_equal(a, [0, 1, 0]) for a in ax) and any(np.array_equal(a, [0, -1, 0]) for a in ax)
    seam = (ax[:, 2] == 0) & (ax[:, 0] < 0)
    assert seam.sum() >= 3 and np.any(np.signbit(ax[seam, 2])) and np.any(~np.signbit(ax[seam, 2]))   # theta = +-pi
    assert (lam < 0.1).sum() >= 2 and (lam > 1e4).sum() >= 2 and ((lam > 1) & (lam < 1e3)).sum() >= 5
    assert np.sum(np.all(l[:, 4:] == 0, axis=1)) == 1 and np.all(l[0, 4:] > 0) and 1 < lam[0] < 100
    row = (np.log10(lam.astype(np.float64)) - 1.5) / 2.5
    assert row.min() < -1 and row.max() > 1                          # the row coordinate clamps at both ends
    # points: q = pts - model_pos (scale * vol_range = 1)
    assert float(fx["scale"]) * float(fx["vol_range"]) == 1.0
    dis = np.linalg.norm(fx["pts"].astype(np.float64) - fx["model_pos"].astype(np.float64), axis=1)
    assert (dis < 0.9).sum() >= 10 and dis.max() > 9.9
    assert np.any((dis > 1 - 1e-5) & (dis < 1)) and np.any((dis > 1) & (dis < 1 + 1e-5))
    q = fx["pts"] - fx["model_pos"]
    nodes = np.isin(q, np.float32([-1, -0.5, 0, 0.5, 1]))
    assert nodes.all(1).sum() >= 3 and (nodes.any(1) & ~nodes.all(1)).sum() >= 3   # grid nodes; cell boundaries
    assert np.any((np.abs(q).max(1) == 1) & (dis <= 1)) and np.any((np.abs(q).max(1) >= 1) & (dis > 1))   # faces


@pytest.mark.parametrize("C", CS)
def test_every_class_is_populated(fx, restated, C):
    sfx = f"c{C}"
    for k in (0, 1):
        pc, qc = fx[f"point_class_{sfx}"][k], fx[f"pair_class_{sfx}"][k]
        assert pc.shape == (70,) and qc.shape == (70, 33)
        for i, name in enumerate(SR.POINT_CLASSES):
            assert (pc == i).sum() >= 10, name
        for i, name in enumerate(SR.PAIR_CLASSES):
            assert (qc == i).sum() >= 20, name
        ssdf, ratio = restated[C, k]["ssdf"], restated[C, k]["ratio"]
        assert (ssdf < -SR.HALF_PI).sum() >= 20 and (ssdf > SR.HALF_PI).sum() >= 20        # clipped at both ends
        assert np.array_equal(SR.pair_class(ssdf, ratio), qc) and np.array_equal(SR.point_class(fx[f"dis64_{sfx}"][k]), pc)
        # exact classes: their recorded deviation is 0 and the reference's values are exactly 0 / 1
        dev = fx[f"decay_dev_{sfx}"][k]
        assert dev[SR.PAIR_CLASSES.index("low")] == 0 and dev[SR.PAIR_CLASSES.index("saturated")] == 0
        assert np.all(fx[f"decay64_{sfx}"][k][qc == SR.PAIR_CLASSES.index("low")] == 0)
        assert np.all(fx[f"decay64_{sfx}"][k][qc == SR.PAIR_CLASSES.index("saturated")] == 1)
        assert np.all(dev[2:] > 0) and np.all(fx[f"factor_dev_{sfx}"][k] > 0)
        # the recorded deviations cover the recorded fp32 run
        e = np.abs(fx[f"decay32_{sfx}"][k].astype(np.float64) - fx[f"decay64_{sfx}"][k])
        for i in range(len(SR.PAIR_CLASSES)):
            assert e[qc == i].max() <= dev[i]
        e = np.abs(fx[f"factor32_{sfx}"][k].astype(np.float64) - fx[f"factor64_{sfx}"][k])
        for i in range(len(SR.POINT_CLASSES)):
            assert e[pc == i].max() <= fx[f"factor_dev_{sfx}"][k, i]
        assert fx[f"factor64_{sfx}"][k].min() < 0.2 and fx[f"factor64_{sfx}"][k].max() > 0.8
    # the rotation matters
    assert np.abs(fx[f"factor64_{sfx}"][0] - fx[f"factor64_{sfx}"][1]).max() > 0.05


# ------------------------------------------------------------------ fp64 against fp64
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("k", (0, 1))
def test_restatement_matches_the_reference_fp64(fx, restated, C, k):
    a = case(fx, C, k)
    dec = restated[C, k]
    fac = SR.sg_shadow_ref(**dict(a, lSGs=rotated(fx, k)), rotate_lights=False)
    assert np.abs(dec["decay"] - fx[f"decay64_c{C}"][k]).max() <= FP64_BAR
    assert np.abs(fac["factor"] - fx[f"factor64_c{C}"][k]).max() <= FP64_BAR
    if C == 128:
        tile = SR.sg_shadow_ref(**dict(a, lSGs=rotated(fx, k, 32)), rotate_lights=False)
        assert np.abs(tile["factor"] - fx["factor64_l32"][k]).max() <= FP64_BAR
        one = SR.sg_shadow_ref(**dict(a, lSGs=a["lSGs"][:1]), rotate_lights=True)
        assert np.abs(one["decay"] - fx["decay64_l1"][k]).max() <= FP64_BAR
        assert np.array_equal(fx["decay64_l1"][k][:, 0], fx["decay64_c128"][k][:, 0])   # a pair's decay is its own


def test_a_transposed_volume_axis_shows(fx):
    a = case(fx, 67, 0)
    wrong = SR.sg_shadow_ref(**dict(a, coeff=np.ascontiguousarray(a["coeff"].transpose(2, 1, 0, 3))))
    assert np.abs(wrong["decay"] - fx["decay64_c67"][0]).max() > 0.1


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("k", (0, 1))
def test_torch_formulation_fp64(fx, C, k):
    import sg_shadow
    a = _t(case(fx, C, k), torch.float64)
    _, dec = sg_shadow.sg_shadow_torch(**a, rotate_lights=True, want=("decay",))
    assert dec.dtype == torch.float64 and np.abs(dec.numpy() - fx[f"decay64_c{C}"][k]).max() <= FP64_BAR
    lights = torch.from_numpy(rotated(fx, k)).double()
    fac, none = sg_shadow.sg_shadow_torch(**dict(a, lSGs=lights), rotate_lights=False, want=("factor",))
    assert none is None and np.abs(fac.numpy() - fx[f"factor64_c{C}"][k]).max() <= FP64_BAR


# ------------------------------------------------------------------ fp32 within the class bars
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("k", (0, 1))
def test_torch_formulation_and_cpu_path_fp32(fx, C, k):
    import sg_shadow
    a = case(fx, C, k)
    t = _t(a)
    sh = sg_shadow.SGShadow(t["coeff"], t["components"], t["mean"], t["fh_tab"], a["vol_range"], a["angle_decay_fac"],
                            a["shadow_pow_fac"], a["self_shadow_pow_fac"])
    assert not sh.is_cuda and (sh.grid_size, sh.ncomponents, sh.envH, sh.envW) == (5, C, 7, 14)
    dec = sh.self_shadow_decay(a["scale"], t["pts"], t["model_pos"], t["lSGs"], t["rot_inv"])
    assert dec.dtype == torch.float32 and dec.shape == (70, 33)
    assert torch.equal(dec, sg_shadow.sg_shadow_torch(**t, rotate_lights=True, want=("decay",))[1])
    assert_decay(fx, f"c{C}", k, dec.numpy(), fx[f"decay64_c{C}"][k], what=f"C={C} k={k}")
    lights = torch.from_numpy(rotated(fx, k))
    fac = sh.calc_shadow_factor(a["scale"], t["pts"], t["model_pos"], lights, t["rot_inv"])
    assert fac.dtype == torch.float32 and fac.shape == (70,)
    assert_factor(fx, f"c{C}", k, fac.numpy(), fx[f"factor64_c{C}"][k], what=f"C={C} k={k}")
    both = sh.factor_and_decay(a["scale"], t["pts"], t["model_pos"], lights, t["rot_inv"])
    assert torch.equal(both[0], fac)
    if C == 128:                                                     # L = 1
        one = sh.self_shadow_decay(a["scale"], t["pts"], t["model_pos"], t["lSGs"][:1], t["rot_inv"])
        assert_decay(fx, "l1", k, one.numpy(), fx["decay64_l1"][k], what="L=1")
        l1 = torch.from_numpy(rotated(fx, k, 1))
        f1 = sh.calc_shadow_factor(a["scale"], t["pts"], t["model_pos"], l1, t["rot_inv"])
        assert_factor(fx, "l1", k, f1.numpy(), fx["factor64_l1"][k], what="L=1")


def test_the_sliders_and_the_reference_spelling(fx):
    import sg_shadow
    a = case(fx, 5, 1)
    t = _t(a)
    sh = sg_shadow.SGShadow(t["coeff"], t["components"], t["mean"], t["fh_tab"], a["vol_range"])
    assert (sh.delta_angle_decay_fac, sh.delta_shadow_fac, sh.delta_self_shadow_fac) == (0.4, 2, 0.1)
    args = (a["scale"], t["pts"], t["model_pos"], t["lSGs"], t["rot_inv"])
    dec = sh.self_shadow_decay(*args)
    full = sh.calc_self_shadow_light_dacay(*args)
    assert full.shape == (70, 33, 7)
    assert torch.equal(full[:, :, :4], t["lSGs"][None, :, :4].expand(70, 33, 4))
    assert torch.equal(full[:, :, 4:], t["lSGs"][None, :, 4:] * dec[:, :, None])          # lights x decay
    f0 = sh.calc_shadow_factor(*args)
    sh.delta_shadow_fac = 1
    f1 = sh.calc_shadow_factor(*args)
    m = (f1 > 0) & (f1 < 1)
    assert bool(m.any()) and torch.allclose(f1 * f1, f0, atol=1e-6) and not torch.equal(f0, f1)
    sh.delta_self_shadow_fac = 1.0
    d1 = sh.self_shadow_decay(*args)
    assert not torch.equal(d1, dec) and bool((d1 <= dec + 1e-6).all())                     # x <= x^0.1 on [0,1]
    sh.delta_angle_decay_fac = 0.0
    assert not torch.equal(sh.self_shadow_decay(*args), d1)
    for bad in (dict(coeff=t["coeff"][:, :4]), dict(coeff=t["coeff"][:1, :1, :1]), dict(components=t["components"][:4]),
                dict(mean=t["mean"][:6]), dict(fh_tab=t["fh_tab"][0]), dict(vol_range=0.0),
                dict(coeff=torch.zeros(2, 2, 2, 129)), dict(coeff=t["coeff"].int())):
        kw = dict(coeff=t["coeff"], components=t["components"], mean=t["mean"], fh_tab=t["fh_tab"], vol_range=2.0)
        with pytest.raises(ValueError):
            sg_shadow.SGShadow(**dict(kw, **bad))
    with pytest.raises(ValueError):
        sh.self_shadow_decay(a["scale"], t["pts"], t["model_pos"], t["lSGs"][:, :6], None)
    # the CPU path checks its arguments like the device path: every failure a ValueError, before any work
    good = dict(scale=a["scale"], pts=t["pts"], model_pos=t["model_pos"], lSGs=t["lSGs"], rot_inv=t["rot_inv"])
    for over in (dict(pts=t["pts"][:, :2]), dict(pts=t["pts"].reshape(-1)), dict(pts=t["pts"].int()), dict(pts=None),
                 dict(model_pos=t["model_pos"][:2]), dict(rot_inv=t["rot_inv"][:2]), dict(scale=0.0),
                 dict(lSGs=t["lSGs"][:0]), dict(lSGs=t["lSGs"].int()), dict(out=torch.zeros(69))):
        for call in (sh.calc_shadow_factor, sh.self_shadow_decay):
            with pytest.raises(ValueError):
                call(**dict(good, **over))
    with pytest.raises(ValueError):
        sh.factor_and_decay(a["scale"], None, t["model_pos"], t["lSGs"])
    with pytest.raises(ValueError):
        sh.frame_decay(4, 4, None, None, (0, 0, 4, 4), None, 0.5, t["model_pos"], t["lSGs"], None)


# ------------------------------------------------------------------ blur and apply
def test_blur_weights_and_reflect_padding(fx):
    import sg_shadow
    w = sg_shadow.blur_weights().numpy()
    assert np.abs(w - SR.blur_weights()).max() < 1e-15 and abs(w.sum() - 1) < 1e-15
    assert np.allclose(w, [0.2390, 0.5220, 0.2390], atol=5e-5)
    for name, (h, wd) in (("apply", (6, 5)), ("apply2", (2, 2))):
        rgb, fac = torch.from_numpy(fx[f"{name}_rgb"]), torch.from_numpy(fx[f"{name}_factor"])
        assert np.abs(SR.shadow_apply_ref(fx[f"{name}_rgb"], fx[f"{name}_factor"]) - fx[f"{name}_out64"]).max() == 0
        out = sg_shadow.shadow_apply(rgb.double(), fac.double(), h, wd)
        assert out.shape == (h, wd, 3) and np.abs(out.numpy() - fx[f"{name}_out64"]).max() <= 1e-12
        out32 = sg_shadow.shadow_apply(rgb, fac, h, wd)
        assert out32.dtype == torch.float32 and np.abs(out32.numpy() - fx[f"{name}_out64"]).max() <= 1e-6
    # reflect, not replicate or zero: a factor that is 1 but for one border pixel
    f = np.ones((4, 4))
    f[0, 1] = 0.0
    got = SR.shadow_apply_ref(np.ones((4, 4, 3)), f)[..., 0]
    w0, w1 = SR.blur_weights()[1], SR.blur_weights()[0]
    assert abs(got[0, 1] - (1 - w0 * w0)) < 1e-15                     # the rows above (reflected: row 1) hold no 0
    assert abs(got[1, 1] - (1 - w0 * w1)) < 1e-15 and abs(got[0, 0] - (1 - 2 * w1 * w0)) < 1e-15   # column -1 is column 1
    with pytest.raises(ValueError):
        sg_shadow.shadow_apply(torch.ones(1, 4, 3), torch.ones(1, 4), 1, 4)
    for bad in ((torch.ones(4, 4, 3), torch.ones(4, 3), None), (torch.ones(4, 4, 2), torch.ones(4, 4), None),
                (torch.ones(4, 4, 3).int(), torch.ones(4, 4), None), (torch.ones(4, 4, 3), None, None),
                (torch.ones(4, 4, 3), torch.ones(4, 4), torch.ones(4, 4))):
        with pytest.raises(ValueError):
            sg_shadow.shadow_apply(bad[0], bad[1], 4, 4, out=bad[2])


# ------------------------------------------------------------------ the C ABI
def test_header_declares_the_shadow_entry_points():
    want = {"ngp_sg_shadow_lights": 10, "ngp_sg_shadow_points": 20, "ngp_sg_shadow_frame_decay": 22,
            "ngp_shadow_apply": 6}
    for name, n in want.items():
        assert name in FUNCS and FUNCS[name][0] is ctypes.c_int and len(FUNCS[name][1]) == n, name
    assert CONSTS["NGP_SSDF_MAX_COMPONENTS"] == 128 and CONSTS["NGP_SSDF_LIGHT_TILE"] == 32
    assert CONSTS["NGP_SSDF_LIGHT_WORDS"] >= 128 + 6


def test_argument_errors_return_before_any_launch():
    """Host-side checks of the entry points (no GPU needed): NGP_EINVAL (-1)."""
    import vren
    lib = vren.lib()
    for name in ("ngp_sg_shadow_lights", "ngp_sg_shadow_points", "ngp_sg_shadow_frame_decay", "ngp_shadow_apply"):
        assert hasattr(lib, name)
    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails its checks first
    f = ctypes.c_float

    def lights(ptrs=(p,) * 4, L=3, C=8, h=7, w=14):
        lsg, comp, mean, ws = ptrs
        return lib.ngp_sg_shadow_lights(lsg, L, None, comp, mean, C, h, w, ws, None)
    for k in range(4):
        assert lights(ptrs=(p,) * k + (None,) + (p,) * (3 - k)) == -1, k
    assert lights(L=0) == -1 and lights(C=0) == -1 and lights(C=129) == -1 and lights(h=0) == -1 and lights(w=0) == -1

    def points(pts=p, n=5, pos=p, coeff=p, G=5, C=8, ws=p, L=3, tab=p, nl=24, nt=32, factor=p, decay=p, scale=0.5,
               vol=2.0):
        return lib.ngp_sg_shadow_points(pts, n, pos, None, f(scale), coeff, G, C, f(vol), f(0.4), ws, L, tab, nl, nt,
                                        f(2.0), f(0.1), factor, decay, None)
    for over in (dict(pts=None), dict(pos=None), dict(coeff=None), dict(ws=None), dict(tab=None),
                 dict(factor=None, decay=None), dict(n=-1), dict(C=0), dict(C=129), dict(G=1), dict(L=0), dict(nl=0),
                 dict(nt=0), dict(scale=0.0), dict(vol=0.0)):
        assert points(**over) == -1, over
    assert points(n=0, pts=None) == 0                                 # no points: a no-op

    def frame(bbox=p, H=13, W=11, dirs=p, pose=p, depth=p, pos=p, coeff=p, G=5, C=8, ws=p, L=3, tab=p, decay=p):
        return lib.ngp_sg_shadow_frame_decay(bbox, H, W, dirs, pose, depth, pos, None, f(0.5), coeff, G, C, f(2.0),
                                             f(0.4), ws, L, tab, 24, 32, f(0.1), decay, None)
    for over in (dict(bbox=None), dict(dirs=None), dict(pose=None), dict(depth=None), dict(pos=None), dict(coeff=None),
                 dict(ws=None), dict(tab=None), dict(decay=None), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15),
                 dict(C=0), dict(C=129), dict(G=1), dict(L=0)):
        assert frame(**over) == -1, over

    def apply(rgb=p, fac=p, H=6, W=5, out=p):
        return lib.ngp_shadow_apply(rgb, fac, H, W, out, None)
    for over in (dict(rgb=None), dict(fac=None), dict(out=None), dict(H=1), dict(W=1), dict(H=0),
                 dict(H=1 << 16, W=1 << 15)):
        assert apply(**over) == -1, over
