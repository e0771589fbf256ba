"""Generate tests/golden/sg_probe.npz: the SG light probes of the insertion
app through the REFERENCE's own insert/envfit.py (SG2Envmap, EnvOptim) and
insert/render_utils.py (cubemap_sample, cubemap2env_map), read from the
reference checkout and never copied, on the CPU, in fp64 and in fp32 on the
same fp32 inputs.

Both files import cv2, tqdm, matplotlib and torchvision at their tops and never
reach them from the functions called here: stub modules stand in.  envfit.py
makes CUDA tensors the default at import: torch.set_default_tensor_type is a
no-op while it loads.  EnvOptim.__init__ calls .cuda(), so the object is built
with EnvOptim.__new__ and lgtSGs, optimizer and N_iter are set here.  The
module globals `viewdirs` (envfit) and `env_vdirs` (render_utils) are assigned
here from the fp32 directions (tests/sg_probe_ref.env_dirs), so that an fp64
run sees the values an fp32 run sees.

Fit cases (name hHxW_lL): 9x14 L=1, 9x14 L=7 (126 pixels: less than one block
of the gradient kernel), 16x32 L=32 (whole blocks), 17x31 L=33 (527 pixels: a
ragged tail; one light more than the shade kernel's tile), 128x128 L=32 (the
app's shape: the draw of EnvOptim.__init__, the target the reference's fp32
cubemap2env_map of the stored 32-resolution cube map `cubemap32`).
  Lights (L >= 7): light 1 a raw sharpness of exactly 0; light 2 a negative
  sharpness and negative amplitudes; light 3 one amplitude channel exactly 0;
  light 4 a zero lobe vector (it moves: the gradient of x / (|x| + eps) at 0 is
  da / eps); light 5 a sharpness near 300 aimed just off a pixel (most of its
  pairs underflow in fp32); the rest ordinary.
  Targets of the designed cases: the env map of three broad lights plus seeded
  noise, non-negative, one pixel an HDR peak (40), one row all zero.
Recorded per case:
  init (L,7) f32, target (H,W,3) f32, fixed (L,7) bool: the entries whose
      gradient is exactly 0 (sharpness 0 and the lobe of that light, the zero
      amplitude channel) and which every run left bit-fixed
  params64 (6,L,7), loss64 (6): the raw parameters after, and the loss of,
      iterations CHECKPOINTS = 1, 2, 3, 5, 10, 25 of the fp64 run
  params_dev (6,3), loss_dev (6): max |fp32 - fp64| per checkpoint and per kind
      of parameter (lobe, sharpness, amplitude; fixed entries left out) over
      THREE fp32 runs that differ only in order -- pixels as they are; pixels
      reversed and lights reversed; a seeded pixel permutation -- applied to
      viewdirs and the target alike: mathematically one result
  gparams (2,L,7) f32: where the gradient is recorded -- the fp32 rounding of
      the fp64 run's parameters before iterations GRAD_CHECKPOINTS = 1, 10;
  grad64 (2,L,7), gloss64 (2): the reference's fp64 autograd gradient and loss
      there; A (2,L,7): sg_probe_ref's sum of absolute per-pixel contributions
      (its gradient is checked against grad64 within 1e-9 relative here);
      grad_dev (2,L,7), gloss_dev (2): max |fp32 - fp64| over the three orders
Lookup cases, res in {2, 5, 32} (cube maps cubemap2, cubemap5, cubemap32):
  look_dirs_rR (300,3) f32: directions on every face, with two and with three
  equal largest components, within half a texel of a face edge, with signed
  zeros, the zero vector; look64_rR (300,3), look_dev_rR (max |fp32 - fp64|),
  look_face_rR (300): the face the reference chose (-1: none; read off a cube
  map whose face f is constant f).  env64_5x8 (5,8,3) and env_dev_5x8 from
  cubemap5; env_dev_128 for the 128 x 128 map of cubemap32, whose fp32 result is
  the last fit case's target and whose fp64 result sg_probe_ref restates
  (checked here within 1e-12).  sg_env64 / sg_env_dev: SG2Envmap of the 17x31
  case's lights.

Run:  python tests/golden/make_sg_probe_golden.py   (needs the reference; about a minute)
"""
import importlib
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
import torch.nn.functional as F  # noqa: E402

import sg_probe_ref as PR  # noqa: E402

SEED = 24
CASES = ((9, 14, 1), (9, 14, 7), (16, 32, 32), (17, 31, 33), (128, 128, 32))
LOOK_RES = (2, 5, 32)
N_LOOK = 300


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
    for name in ("cv2", "matplotlib", "matplotlib.pyplot", "tqdm", "torchvision", "torchvision.transforms",
                 "torchvision.transforms.functional"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Anything(name)
    keep = torch.set_default_tensor_type
    torch.set_default_tensor_type = lambda *_a, **_k: None
    mods = []
    try:
        for fname in ("envfit", "render_utils"):
            spec = importlib.util.spec_from_file_location("ref_" + fname, os.path.join(REF, "insert", fname + ".py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            mods.append(mod)
    finally:
        torch.set_default_tensor_type = keep
    return mods


def name_of(H, W, L):
    return f"h{H}x{W}_l{L}"


# ------------------------------------------------------------------ designed inputs
def design_lights(gen, L, dirs, sharp_scale):
    x = torch.randn(L, 7, generator=gen, dtype=torch.float64).numpy()
    x[:, 3] *= sharp_scale
    x[:, 4:] *= 0.6
    if L >= 7:
        x[1, 3] = 0.0
        x[2, 3] = -abs(x[2, 3]) - 1.0
        x[2, 4:] = -np.abs(x[2, 4:]) - 0.1
        x[3, 5] = 0.0
        x[4, :3] = 0.0
        i = len(dirs) // 3 + 2                                            # just off a pixel: a well-conditioned gradient
        x[5, :3] = 1.7 * (0.9 * dirs[i].astype(np.float64) + 0.1 * dirs[i + 1].astype(np.float64))
        x[5, 3] = 300.0 + x[5, 3] / sharp_scale
    return x.astype(np.float32)


def design_target(gen, H, W, dirs):
    gt = np.array([[0.3, 0.9, 0.2, 2.0, 1.0, 0.8, 0.6], [-0.7, 0.1, 0.6, 6.0, 0.3, 0.5, 0.9],
                   [0.1, -0.8, -0.5, 1.0, 0.2, 0.2, 0.25]])
    t = PR.sg_envmap_ref(gt, dirs) + 0.05 * torch.rand(H * W, 3, generator=gen, dtype=torch.float64).numpy()
    t = t.reshape(H, W, 3)
    t[H // 2] = 0.0
    t[2, 3] = 40.0
    return t.astype(np.float32)


def design_cubemap(gen, res, peak):
    d = get_cubemap_dirs(res)
    sky = 0.4 + 0.5 * np.clip(d[:, 1:2], 0, 1) * np.array([[0.5, 0.7, 1.0]]) + 0.15 * np.sin(5 * d[:, 0:1] + 3 * d[:, 2:3])
    cm = np.clip(sky + 0.05 * torch.rand(len(d), 3, generator=gen, dtype=torch.float64).numpy(), 0, None)
    if peak:
        sun = np.array([0.5, 0.6, -0.62])
        sun /= np.linalg.norm(sun)
        cm += 60.0 * np.exp(400.0 * (d @ sun - 1.0))[:, None] * np.array([[1.0, 0.9, 0.7]])
    return cm.astype(np.float32)


def get_cubemap_dirs(res):
    """insert_utils.get_cubemap_rays's directions (faces +z, -z, +x, -x, +y, -y), float64"""
    x = np.linspace(0, 1, res) * 2 - 1
    X, Y = np.meshgrid(x, x, indexing="ij")
    one = np.ones_like(X)
    faces = [(X, Y, one), (X, Y, -one), (one, X, Y), (-one, X, Y), (X, one, Y), (X, -one, Y)]
    d = np.stack([np.stack(f, -1) for f in faces]).reshape(-1, 3)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def design_look_dirs(gen, res):
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64).numpy()  # noqa: E731
    d = [[0.3, -0.2, 0.9]]                                                        # (the list of length 1)
    for axis in range(3):                                                         # two equal largest components
        for s0 in (1, -1):
            for s1 in (1, -1):
                v = np.full(3, 0.37)
                v[axis] = 0.1
                o = [k for k in range(3) if k != axis]
                v[o[0]], v[o[1]] = s0 * 0.37, s1 * 0.37
                d.append(v)
    for s in ((1, 1, 1), (-1, 1, 1), (1, -1, -1), (-1, -1, -1), (-1, -1, 1)):     # three
        d.append(0.5 * np.array(s, dtype=np.float64))
    for axis in range(3):                                                         # within half a texel of an edge
        for sgn in (1, -1):
            for e0, e1 in ((1 - 0.3 / res, 0.2), (-(1 - 0.1 / res), -0.6), (0.4, 1 - 0.45 / res),
                           (1 - 0.2 / res, -(1 - 0.2 / res))):
                v = np.zeros(3)
                o = [k for k in range(3) if k != axis]
                v[axis], v[o[0]], v[o[1]] = sgn * 1.3, 1.3 * e0, 1.3 * e1
                d.append(v)
    d += [[1.0, -0.0, 0.0], [0.0, -0.0, -1.0], [-0.0, 2.0, 0.0], [-0.0, -3.0, -0.0], [0.0, 0.0, 0.5],
          [-1.0, 0.0, -0.0], [0.0, 0.0, 0.0], [-0.0, 0.0, -0.0]]                  # signed zeros; the zero vector
    d = np.array(d, dtype=np.float64)
    rest = torch.randn(N_LOOK - len(d), 3, generator=gen, dtype=torch.float64).numpy() * (0.2 + 2 * rnd(N_LOOK - len(d), 1))
    return np.concatenate([d, rest]).astype(np.float32)


# ------------------------------------------------------------------ reference runs
class Dtype:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        torch.set_default_dtype(self.dtype)

    def __exit__(self, *a):
        torch.set_default_dtype(torch.float32)


def T(a, dtype):
    return torch.from_numpy(np.array(a, order="C").reshape(np.shape(a))).to(dtype)


def ref_lookup(RU, cubemap, dirs, res, dtype):
    with Dtype(dtype):
        return RU.cubemap_sample(T(cubemap, dtype), T(dirs, dtype), res, None, False).numpy()


def ref_env_map(RU, cubemap, res, H, W, dtype):
    with Dtype(dtype):
        RU.env_vdirs = T(PR.env_dirs(H, W), dtype).reshape(H, W, 3)
        try:
            return RU.cubemap2env_map(T(cubemap, dtype), res, H, W).numpy()
        finally:
            RU.env_vdirs = None


class RefFit:
    """the reference's EnvOptim on one ordering of the pixels and lights"""

    def __init__(self, EF, init, dirs, target, dtype, pix=None, flip_lights=False):
        self.EF, self.dtype, self.flip = EF, dtype, flip_lights
        P = len(dirs)
        pix = np.arange(P) if pix is None else pix
        self.H, self.W = target.shape[:2]
        self.vd = T(dirs[pix], dtype).reshape(self.H, self.W, 1, 3)
        self.im = T(target.reshape(-1, 3)[pix], dtype).reshape(self.H, self.W, 3)
        self.start(init)

    def start(self, init):
        with Dtype(self.dtype):
            x = T(init[::-1] if self.flip else init, self.dtype)
            self.opt = self.EF.EnvOptim.__new__(self.EF.EnvOptim)
            self.opt.lgtSGs = torch.nn.Parameter(x.clone())
            self.opt.optimizer = torch.optim.Adam([self.opt.lgtSGs], lr=1e-1)
            self.opt.N_iter = 0

    def _out(self, a):
        a = a.detach().numpy().copy()
        return a[::-1].copy() if self.flip else a

    def run(self, n):
        with Dtype(self.dtype):
            self.EF.viewdirs = self.vd
            try:
                self.opt.N_iter = n
                return self._out(self.opt.eval(self.im))
            finally:
                self.EF.viewdirs = None

    def loss_grad(self):
        """the loss and its autograd gradient at the current parameters (no step)"""
        with Dtype(self.dtype):
            self.EF.viewdirs = self.vd
            try:
                p = self.opt.lgtSGs.detach().clone().requires_grad_(True)
                loss = F.mse_loss(self.EF.SG2Envmap(p, self.H, self.W), self.im)
                loss.backward()
                return float(loss), self._out(p.grad)
            finally:
                self.EF.viewdirs = None

    def params(self):
        return self._out(self.opt.lgtSGs)


def orders(P, gen):
    return [(None, False), (np.arange(P)[::-1].copy(), True), (torch.randperm(P, generator=gen).numpy(), False)]


def record_fit(EF, init, dirs, target, gen, designed):
    P, L = len(dirs), len(init)
    fixed = np.zeros((L, 7), dtype=bool)
    if designed and L >= 7:
        fixed[1, :4] = True
        fixed[3, 5] = True
    ords = orders(P, gen)
    runs = [RefFit(EF, init, dirs, target, torch.float64)] + \
           [RefFit(EF, init, dirs, target, torch.float32, pix, flip) for pix, flip in ords]
    n_ck = len(PR.CHECKPOINTS)
    params64, loss64 = np.zeros((n_ck, L, 7)), np.zeros(n_ck)
    params_dev, loss_dev = np.zeros((n_ck, 3)), np.zeros(n_ck)
    gparams = np.zeros((2, L, 7), dtype=np.float32)
    done = 0
    for ci, it in enumerate(PR.CHECKPOINTS):
        for r in runs:
            r.run(it - 1 - done)
        done = it - 1
        if it in PR.GRAD_CHECKPOINTS:
            gparams[PR.GRAD_CHECKPOINTS.index(it)] = runs[0].params().astype(np.float32)
        l64 = runs[0].loss_grad()[0]
        loss64[ci] = l64
        for r in runs[1:]:
            loss_dev[ci] = max(loss_dev[ci], abs(r.loss_grad()[0] - l64))
        for r in runs:
            r.run(1)
        done = it
        p64 = runs[0].params()
        params64[ci] = p64
        for r in runs[1:]:
            p32 = r.params()
            assert p32.dtype == np.float32
            assert np.array_equal(p32[fixed], init[fixed]), "a fixed parameter moved in an fp32 run"
            e = np.abs(p32.astype(np.float64) - p64)
            for k in range(3):
                m = (PR.KIND_OF_COLUMN[None, :] == k) & ~fixed
                params_dev[ci, k] = max(params_dev[ci, k], e[m].max())
        assert np.array_equal(p64[fixed], init.astype(np.float64)[fixed]), "a fixed parameter moved in the fp64 run"
    # the gradient where it is recorded: fresh objects at the fp32-rounded parameters
    grad64, A, grad_dev = np.zeros((2, L, 7)), np.zeros((2, L, 7)), np.zeros((2, L, 7))
    gloss64, gloss_dev = np.zeros(2), np.zeros(2)
    for gi in range(2):
        runs[0].start(gparams[gi])
        gloss64[gi], grad64[gi] = runs[0].loss_grad()
        loss, mine, A[gi] = PR.sg_grad_ref(gparams[gi], dirs, target)
        scale = np.abs(grad64[gi]).max()
        assert np.abs(mine - grad64[gi]).max() <= 1e-9 * scale and abs(loss - gloss64[gi]) <= 1e-9 * gloss64[gi], \
            (np.abs(mine - grad64[gi]).max(), scale)
        assert np.all(grad64[gi][fixed] == 0)
        for r in runs[1:]:
            r.start(gparams[gi])
            l32, g32 = r.loss_grad()
            assert g32.dtype == np.float32
            grad_dev[gi] = np.maximum(grad_dev[gi], np.abs(g32.astype(np.float64) - grad64[gi]))
            gloss_dev[gi] = max(gloss_dev[gi], abs(l32 - gloss64[gi]))
    return dict(init=init, target=target, fixed=fixed, params64=params64, loss64=loss64, params_dev=params_dev,
                loss_dev=loss_dev, gparams=gparams, grad64=grad64, gloss64=gloss64, A=A, grad_dev=grad_dev,
                gloss_dev=gloss_dev)


def main():
    EF, RU = load_reference()
    torch.set_num_threads(1)
    gen = torch.Generator().manual_seed(SEED)
    out = dict(seed=SEED, cases=np.array(CASES, dtype=np.int32), checkpoints=np.array(PR.CHECKPOINTS),
               grad_checkpoints=np.array(PR.GRAD_CHECKPOINTS))

    # ---- lookups
    cubemaps = {res: design_cubemap(gen, res, peak=(res == 32)) for res in LOOK_RES}
    for res in LOOK_RES:
        cm = cubemaps[res]
        out[f"cubemap{res}"] = cm
        dirs = design_look_dirs(gen, res)
        r64 = ref_lookup(RU, cm, dirs, res, torch.float64)
        r32 = ref_lookup(RU, cm, dirs, res, torch.float32)
        assert r32.dtype == np.float32
        ids = np.repeat(np.arange(6, dtype=np.float32), res * res)[:, None].repeat(3, 1) + 2.0   # face f holds f + 2
        face = np.rint(ref_lookup(RU, ids, dirs, res, torch.float64)[:, 0]).astype(np.int64) - 2  # (none: 1 -> -1)
        mine, mine_face = PR.cubemap_sample_ref(cm, dirs, res)
        assert np.array_equal(mine_face, face), "sg_probe_ref chooses another face than the reference"
        assert np.abs(mine - r64).max() <= 1e-12 * max(1.0, np.abs(r64).max())
        out[f"look_dirs_r{res}"], out[f"look64_r{res}"], out[f"look_face_r{res}"] = dirs, r64, face.astype(np.int8)
        out[f"look_dev_r{res}"] = np.abs(r32.astype(np.float64) - r64).max()
        print(f"lookup res {res}: dev {out[f'look_dev_r{res}']:.3e}, faces {np.bincount(face + 1, minlength=7)}")
    e64, e32 = (ref_env_map(RU, cubemaps[5], 5, 5, 8, dt) for dt in (torch.float64, torch.float32))
    out["env64_5x8"], out["env_dev_5x8"] = e64, np.abs(e32.astype(np.float64) - e64).max()
    e64, e32 = (ref_env_map(RU, cubemaps[32], 32, 128, 128, dt) for dt in (torch.float64, torch.float32))
    mine = PR.cubemap_sample_ref(cubemaps[32], PR.env_dirs(128, 128), 32)[0].reshape(128, 128, 3)
    assert np.abs(mine - e64).max() <= 1e-12 * np.abs(e64).max()
    out["env_dev_128"] = np.abs(e32.astype(np.float64) - e64).max()
    print(f"env map 5x8 dev {out['env_dev_5x8']:.3e}; 128x128 dev {out['env_dev_128']:.3e}, max {e64.max():.2f}")
    target128 = e32

    # ---- fits
    for H, W, L in CASES:
        dirs = PR.env_dirs(H, W)
        if (H, W) == (128, 128):
            init = torch.randn(L, 7, generator=gen)
            init[..., 3:4] *= 100.
            init, target = init.numpy(), target128
        else:
            init = design_lights(gen, L, dirs, 6.0 if L > 1 else 3.0)
            target = design_target(gen, H, W, dirs)
        rec = record_fit(EF, init, dirs, target, torch.Generator().manual_seed(SEED + H * W + L), (H, W) != (128, 128))
        for k, v in rec.items():
            out[f"{name_of(H, W, L)}_{k}"] = v
        print(f"{name_of(H, W, L)}: loss {rec['loss64'][0]:.4g} -> {rec['loss64'][-1]:.4g}; loss_dev {rec['loss_dev'].max():.2e}")
        print("   params_dev (checkpoint x lobe/sharpness/amplitude):\n", np.array2string(rec["params_dev"], precision=2))
        rel = rec["grad_dev"] / np.maximum(2.0 ** -24 * rec["A"], 1e-300)
        print(f"   grad_dev / (2^-24 A): median {np.median(rel[rel > 0]):.2f}, max {rel.max():.2f}")
    H, W, L = CASES[3]
    lights, dirs = out[f"{name_of(H, W, L)}_init"], PR.env_dirs(H, W)
    envs = []
    for dt in (torch.float64, torch.float32):
        with Dtype(dt):
            EF.viewdirs = T(dirs, dt).reshape(H, W, 1, 3)
            envs.append(EF.SG2Envmap(T(lights, dt), H, W).numpy())
            EF.viewdirs = None
    assert np.abs(PR.sg_envmap_ref(lights, dirs).reshape(H, W, 3) - envs[0]).max() <= 1e-12 * np.abs(envs[0]).max()
    out["sg_env64"], out["sg_env_dev"] = envs[0], np.abs(envs[1].astype(np.float64) - envs[0]).max()
    path = os.path.join(HERE, "sg_probe.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
