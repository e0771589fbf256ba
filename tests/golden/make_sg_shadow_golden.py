"""Generate tests/golden/sg_shadow.npz: the SSDF soft shadows of the insertion
app through the REFERENCE's own insert/sg_shadow.py (read from the reference
checkout, never copied), on the CPU, in fp64 and in fp32 on the same fp32
inputs.

sg_shadow.py star-imports insert_utils and render_utils, which import open3d,
cv2, matplotlib, tqdm and torchvision at their tops and never reach them from
the two methods called here: stub modules stand in.  It also makes CUDA
tensors the default at import: torch.set_default_tensor_type is a no-op while
it loads.  SGShadow.__init__ reads asset files and calls .cuda(), so the object
is built with SGShadow.__new__ and its attributes are set here, in the layout
__init__ leaves them (coeff_volume = coeff.permute(3,2,1,0)[None], mean
(1,envH,envW), fh_tab (1,1,n_lambda,n_theta)).

Inputs are designed (tests/test_sg_shadow_ref_cpu.py states what they must
hold), not random where it matters:
  G = 5, C in {5, 67, 128} (the smaller volumes are the first C components of
  the largest), env 7 x 14, table 24 x 32, vol_range 2, scale 0.5 (so
  scale * vol_range = 1 and q = pts - model_pos exactly), model_pos with few
  mantissa bits.  Component 0 is constant 1 over the env map and its
  coefficient rises along x only, the volume's other components differ along
  every axis, the mean and the table are asymmetric: a transposed axis shows.
  fh_tab: a midpoint quadrature (256 x 256) of the reference's integrand
  exp(lam (sin z sin d - 1)) sin z over z in [pi/2 - theta_d, pi], d in
  [0, pi], rows lam = 10^linspace(-1, 4, 24), columns theta_d =
  linspace(-pi/2, pi/2, 32); column 0 is exactly 0 (an empty interval) and
  values below 1e-30 are stored as 0 (no subnormals).
  Points (P = 70): inside the unit range, |q| just either side of 1, |q| up to
  10, on cell boundaries and grid nodes, on the volume's faces, at both ends of
  x (ssdf clipped at both ends through component 0).
  Lights (L = 33, light 0 a middling one: the L = 1 case): axes exactly
  (0, +-1, 0), on the theta = +-pi seam, ordinary; sharpness below 0.1 and
  above 1e4 (the row coordinate clamps at both ends; above 1e4 the ratio
  fh / fh_n passes 1.05: saturated pairs); one light with zero amplitude.
  With and without rot_inv (a seeded rotation); lSGs_rot: the lights with
  fp32-rotated axes, which the factor call is handed then (main.py:496-499).

Recorded per C (suffix _c5, _c67, _c128) and per rotation (k = 0 none, 1 rot_inv):
  factor64 (2,P), decay64 (2,P,L) float64   the reference in fp64
  factor32 (2,P), decay32 (2,P,L) float32   the reference in fp32, C axis as is
  dis64 (2,P)                               |q| before the clip at 1 (tests/sg_shadow_ref.py)
  point_class (2,P), pair_class (2,P,L)     class indices (sg_shadow_ref.POINT_CLASSES / PAIR_CLASSES), read from
                                            sg_shadow_ref's fp64 ssdf and |fh / fh_n| (not stored: the CPU tests
                                            recompute them)
  factor_dev (2, point classes), decay_dev (2, pair classes)
      max |fp32 - fp64| over the class and over THREE fp32 runs that differ only in the order of the C axis
      (as is, reversed, one seeded permutation, applied to coeff and components alike): mathematically one
      result, so the deviation includes what another summation order costs.
  and for L = 1 (light 0 alone), C = 128: factor64_l1, decay64_l1, factor_dev_l1, decay_dev_l1,
  point_class_l1, pair_class_l1; for L = 32 (one light tile of the kernels), C = 128: factor64_l32,
  factor_dev_l32, point_class_l32 (the decay of a pair does not depend on the other lights).
The blur-and-apply case (torchvision is not needed: gaussian_blur(kernel (3,3))
is sigma 0.8, 1-D weights exp(-0.5 (x/0.8)^2) normalised = 0.23899 / 0.52201 /
0.23899, reflect padding, the 2-D kernel their outer product), fp64, from
sg_shadow_ref.shadow_apply_ref: apply_rgb (6,5,3) float32, apply_factor (6,5)
float32, apply_out64 (6,5,3); and a 2 x 2 frame apply2_*.

Run:  python tests/golden/make_sg_shadow_golden.py   (needs the reference; seconds)
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AR_NERF_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sg_shadow_ref as SR  # noqa: E402

SEED = 22
G, CS, ENV_H, ENV_W, N_LAMBDA, N_THETA = 5, (5, 67, 128), 7, 14, 24, 32
VOL_RANGE, SCALE, ANGLE_DECAY, SHADOW_POW, SELF_POW = 2.0, 0.5, 0.4, 2, 0.1
MODEL_POS = np.array([0.25, -0.5, 0.125], dtype=np.float32)
L = 33


class _Anything(types.ModuleType):
    """a module whose every attribute is another such module (import x.y.z and `from x import name` all work)"""
    __path__ = []
    __all__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        m = _Anything(self.__name__ + "." + name)
        sys.modules[m.__name__] = m
        setattr(self, name, m)
        return m

    def __call__(self, *a, **k):
        return self


def load_reference():
    for name in ("open3d", "cv2", "matplotlib", "matplotlib.pyplot", "tqdm", "torchvision", "torchvision.transforms",
                 "torchvision.transforms.functional", "kornia", "imageio", "scipy", "einops", "OpenEXR", "Imath",
                 "trimesh", "pyrender", "PIL", "PIL.Image", "skimage", "lpips"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Anything(name)
    sys.path.insert(0, os.path.join(REF, "insert"))
    keep = torch.set_default_tensor_type
    torch.set_default_tensor_type = lambda *_a, **_k: None
    try:
        spec = importlib.util.spec_from_file_location("ref_sg_shadow", os.path.join(REF, "insert", "sg_shadow.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        torch.set_default_tensor_type = keep
        sys.path.pop(0)
    return mod


def fh_table():
    n = 256
    lam = 10.0 ** np.linspace(-1, 4, N_LAMBDA)
    theta_d = np.linspace(-np.pi / 2, np.pi / 2, N_THETA)
    tab = np.zeros((N_LAMBDA, N_THETA))
    d = (np.arange(n) + 0.5) * (np.pi / n)
    for j, t in enumerate(theta_d):
        lo = np.pi / 2 - t
        hz = (np.pi - lo) / n
        z = lo + (np.arange(n) + 0.5) * hz
        for i, lm in enumerate(lam):
            f = np.exp(lm * (np.sin(z)[:, None] * np.sin(d)[None, :] - 1)) * np.sin(z)[:, None]
            tab[i, j] = f.sum() * hz * (np.pi / n)
    tab[:, 0] = 0.0
    tab[tab < 1e-30] = 0.0
    return tab.astype(np.float32)


def design(gen):
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64).numpy()  # noqa: E731
    randn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).numpy()  # noqa: E731
    C = max(CS)
    # the volume: component 0 rises along x from -2.4 to 2.4 (it meets a constant-1 component image: a per-point
    # offset that clips the ssdf at both ends near the x faces); the others: seeded values with a distinct
    # gradient along each axis
    ix, iy, iz = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij")
    coeff = 0.35 * randn(G, G, G, C)
    coeff += (0.10 * ix + 0.23 * iy - 0.17 * iz)[..., None] * np.linspace(-1, 1, C)[None, None, None, :]
    coeff[..., 0] = -2.4 + 1.2 * ix
    components = randn(C, ENV_H, ENV_W) * (1.2 / np.sqrt(np.arange(1, C + 1)))[:, None, None] * 0.3
    components[0] = 1.0
    v, u = np.meshgrid(np.linspace(-1, 1, ENV_H), np.linspace(-1, 1, ENV_W), indexing="ij")
    mean = 0.5 * v - 0.3 * u + 0.15 * u * v + 0.05 * randn(ENV_H, ENV_W)

    # points, as q = pts - model_pos (scale * vol_range = 1)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)  # noqa: E731
    q = []
    q += list(unit(randn(14, 3)) * rnd(14, 1) ** (1 / 3) * 0.98)                      # inside
    u3 = unit(randn(3, 3))
    q += [u3[0] * (1 - 1e-6), u3[1] * (1 + 1e-6), u3[2]]                              # |q| either side of 1
    q += list(unit(randn(8, 3)) * np.array([1.5, 2, 3, 4, 5, 7, 9, 10])[:, None])     # up to 10
    q += [[0.5, 0.0, -0.5], [0.0, 0.0, 0.0], [-0.5, 0.5, 0.25], [0.5, 0.1, 0.3], [0.2, -0.5, 0.7],
          [0.25, 0.25, 0.25], [-0.5, -0.5, -0.5]]                                     # cell boundaries and nodes
    q += [[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.6, 0.8, 0.0],
          [1.0, 0.5, -0.25], [-1.0, 1.0, 1.0], [0.3, -1.0, 0.9]]                      # faces (some pushed back on them)
    q += [[0.97, 0.05, -0.1], [-0.97, 0.1, 0.05], [0.9, -0.2, 0.2], [-0.9, 0.3, -0.1],
          [0.8, 0.1, 0.1], [-0.8, -0.1, 0.3]]                                         # both ends of x
    q = np.array(q, dtype=np.float64)
    q = np.concatenate([q, unit(randn(70 - len(q), 3)) * (0.2 + 1.6 * rnd(70 - len(q), 1))])
    pts = (q.astype(np.float32) + MODEL_POS[None]).astype(np.float32)

    # lights
    ax = unit(randn(L, 3))
    ax[1], ax[2] = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)
    ax[3], ax[4], ax[6] = (-1.0, 0.0, 0.0), (-0.8, 0.6, 0.0), (-0.6, -0.8, -0.0)       # the theta = +-pi seam
    lam = 10.0 ** np.linspace(-1, 4, L)[torch.randperm(L, generator=gen).numpy()]
    lam[0] = 20.0
    lam[7], lam[8], lam[9], lam[10] = 0.05, 0.08, 2e4, 5e4
    lam[1], lam[3] = 3.0, 150.0
    amp = (0.1 + 1.2 * rnd(L, 3)) * (lam / (2 * np.pi))[:, None]
    amp[5] = 0.0
    lSGs = np.concatenate([ax, lam[:, None], amp], 1).astype(np.float32)
    lSGs[6, 2] = -0.0
    rot, _ = np.linalg.qr(randn(3, 3))
    if np.linalg.det(rot) < 0:
        rot[:, 0] = -rot[:, 0]
    return dict(coeff=coeff.astype(np.float32), components=components.astype(np.float32),
                mean=mean.astype(np.float32), fh_tab=fh_table(), pts=pts, model_pos=MODEL_POS, lSGs=lSGs,
                rot_inv=rot.astype(np.float32))


def rotated(lights, rot):
    """the lights with their axes rotated in fp32, as the app hands them to calc_shadow_factor"""
    out = lights.copy()
    out[:, :3] = (lights[:, :3].astype(np.float32) @ rot.astype(np.float32).T).astype(np.float32)
    return out


def reference_run(mod, d, C, lights, rot, dtype, order=None):
    """the reference's two methods on the first C components, the C axis in `order` -> factor (P), decay (P,L)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    order = np.arange(C) if order is None else order
    torch.set_default_dtype(dtype)
    try:
        sh = mod.SGShadow.__new__(mod.SGShadow)
        sh.delta_angle_decay_fac, sh.delta_shadow_fac, sh.delta_self_shadow_fac = ANGLE_DECAY, SHADOW_POW, SELF_POW
        sh.vol_range = VOL_RANGE
        sh.raw_h_angle = torch.asin(torch.Tensor([1.0 / VOL_RANGE]))
        sh.ncomponents, sh.envH, sh.envW = C, ENV_H, ENV_W
        sh.fh_tab = t(d["fh_tab"])[None, None]
        sh.coeff_volume = t(d["coeff"][..., :C][..., order]).permute(3, 2, 1, 0).unsqueeze(0)
        sh.components = t(d["components"][:C][order])
        sh.mean = t(d["mean"])[None]
        pts, pos, lsg = t(d["pts"]), t(d["model_pos"]), t(lights)
        r = None if rot is None else t(rot)
        # main.py:496-499: the factor takes rotated lights; rotated once in fp32 (rotated()), the same for every run
        lrot = lsg if r is None else t(rotated(lights, rot))
        factor = sh.calc_shadow_factor(SCALE, pts, pos, lrot, r)
        # the decay does not depend on the amplitudes: with amplitudes of 1 the (P,L,7) result holds it exactly
        unit = lsg.clone()
        unit[:, 4:] = 1.0
        res = sh.calc_self_shadow_light_dacay(SCALE, pts, pos, unit, r)
        assert torch.equal(res[:, :, 4], res[:, :, 5]) and torch.equal(res[:, :, 4], res[:, :, 6])
        return factor.numpy(), res[:, :, 4].contiguous().numpy()
    finally:
        torch.set_default_dtype(torch.float32)


def record(mod, d, C, lights, perm_gen):
    """every array of one (C, lights) case, rotation k = 0 / 1"""
    orders = [None, np.arange(C)[::-1].copy(), torch.randperm(C, generator=perm_gen).numpy()]
    out = {k: [] for k in ("factor64", "decay64", "factor32", "decay32", "dis64", "point_class", "pair_class",
                           "factor_dev", "decay_dev", "_ssdf", "_ratio")}
    for rot in (None, d["rot_inv"]):
        f64, d64 = reference_run(mod, d, C, lights, rot, torch.float64)
        mine = SR.sg_shadow_ref(d["coeff"][..., :C], d["components"][:C], d["mean"], d["fh_tab"], VOL_RANGE, SCALE,
                                d["pts"], d["model_pos"], lights, rot, True, ANGLE_DECAY, SHADOW_POW, SELF_POW)
        mine_f = SR.sg_shadow_ref(d["coeff"][..., :C], d["components"][:C], d["mean"], d["fh_tab"], VOL_RANGE, SCALE,
                                  d["pts"], d["model_pos"], lights if rot is None else rotated(lights, rot), rot,
                                  False, ANGLE_DECAY, SHADOW_POW, SELF_POW)
        assert np.abs(d64 - mine["decay"]).max() < 1e-9 and np.abs(f64 - mine_f["factor"]).max() < 1e-9
        pc, qc = SR.point_class(mine["dis"]), SR.pair_class(mine["ssdf"], mine["ratio"])
        fdev, ddev = np.zeros(len(SR.POINT_CLASSES)), np.zeros(len(SR.PAIR_CLASSES))
        f32 = d32 = None
        for order in orders:
            f, dd = reference_run(mod, d, C, lights, rot, torch.float32, order)
            assert f.dtype == np.float32 and dd.dtype == np.float32
            if f32 is None:
                f32, d32 = f, dd
            for i in range(len(SR.POINT_CLASSES)):
                if (pc == i).any():
                    fdev[i] = max(fdev[i], np.abs(f.astype(np.float64) - f64)[pc == i].max())
            for i in range(len(SR.PAIR_CLASSES)):
                m = qc == i
                if m.any():
                    ddev[i] = max(ddev[i], np.abs(dd.astype(np.float64) - d64)[m].max())
        for k, v in (("factor64", f64), ("decay64", d64), ("factor32", f32), ("decay32", d32),
                     ("_ssdf", mine["ssdf"]), ("_ratio", mine["ratio"]), ("dis64", mine["dis"]),
                     ("point_class", pc), ("pair_class", qc), ("factor_dev", fdev), ("decay_dev", ddev)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def main():
    mod = load_reference()
    torch.set_num_threads(1)
    gen = torch.Generator().manual_seed(SEED)
    d = design(gen)
    out = dict(d, lSGs_rot=rotated(d["lSGs"], d["rot_inv"]), seed=SEED, vol_range=VOL_RANGE, scale=SCALE, angle_decay_fac=ANGLE_DECAY,
               shadow_pow_fac=SHADOW_POW, self_shadow_pow_fac=SELF_POW, Cs=np.array(CS, dtype=np.int32))
    for C in CS:
        rec = record(mod, d, C, d["lSGs"], torch.Generator().manual_seed(SEED + C))
        for k, v in rec.items():
            if not k.startswith("_"):
                out[f"{k}_c{C}"] = v
        counts = [[int((rec["pair_class"][r] == i).sum()) for i in range(len(SR.PAIR_CLASSES))] for r in (0, 1)]
        print(f"C={C}: pairs {dict(zip(SR.PAIR_CLASSES, counts[0]))} / {counts[1]}  points "
              f"{[int((rec['point_class'][0] == i).sum()) for i in (0, 1)]}")
        print(f"   factor_dev {rec['factor_dev']}\n   decay_dev {rec['decay_dev']}")
        edge = np.abs(np.abs(rec["_ssdf"]) - SR.HALF_PI).min()
        rat = rec["_ratio"]
        print(f"   nearest ssdf to a clip {edge:.2e}; ratios in [1, 1.05): {int(((rat >= 1) & (rat < 1.05)).sum())}, "
              f">= 1.05: {int((rat >= 1.05).sum())}")
    rec = record(mod, d, 128, d["lSGs"][:1], torch.Generator().manual_seed(SEED))
    for k in ("factor64", "decay64", "factor_dev", "decay_dev", "point_class", "pair_class"):
        out[f"{k}_l1"] = rec[k]
    print(f"L=1: factor_dev {rec['factor_dev']} decay_dev {rec['decay_dev']}")
    rec = record(mod, d, 128, d["lSGs"][:32], torch.Generator().manual_seed(SEED + 32))
    for k in ("factor64", "factor_dev", "point_class"):      # (a pair's decay is its own: the L = 33 columns serve)
        out[f"{k}_l32"] = rec[k]
    print(f"L=32: factor_dev {rec['factor_dev']}")

    g = np.random.default_rng(SEED)
    for name, (h, w) in (("apply", (6, 5)), ("apply2", (2, 2))):
        rgb = g.uniform(0, 1.5, size=(h, w, 3)).astype(np.float32)
        fac = g.uniform(0, 1, size=(h, w)).astype(np.float32)
        fac[0, 0], fac[-1, -1] = 0.0, 1.0
        out[f"{name}_rgb"], out[f"{name}_factor"] = rgb, fac
        out[f"{name}_out64"] = SR.shadow_apply_ref(rgb, fac)
    path = os.path.join(HERE, "sg_shadow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
