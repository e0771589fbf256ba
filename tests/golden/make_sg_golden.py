"""Generate tests/golden/sg_shade.npz: the insertion app's object shade under
SG lights (insert/main.py:521-594, Insertor.render_object with use_sg_base)
through the REFERENCE's own insert/render_utils.SG_render_core and
datasets/ray_utils.get_rays (read from the reference checkout, never copied),
on the CPU, once in fp32 and once in fp64.

render_utils imports torchvision at its top for the cubemap blur, which the SG
path never calls: stub modules stand in for it.  Insertor itself cannot be
imported (open3d, cv2), so the mask / material / scatter glue of main.py:
526-552 and 585-589 is restated here (render_object below), as
make_insert_golden.py does for its frame.  The app hands render_object box-
sized normals / depths / maps; here every per-pixel input is a whole-frame
array and the box slice is taken inside, which is the same gather.

One 13 x 11 frame (143 pixels), the model's box strictly inside it.  The
inputs are designed (tests/test_sg_shade_ref_cpu.py states what they must
hold): depth 0, 5e-7, float32(1e-6) and its two fp32 neighbours, ordinary
depths inside and outside the box; normals of non-unit length built per pixel
for a prescribed n.v -- facing (>= 0.3), middle, grazing (0 < n.v < 0.05),
back-facing (< 0); 33 lights with sharpness spread over 1e-1 .. 1e4, one with
zero amplitude; a decay map; metal / rough / albedo maps (rough below 0.2 and
above 1).  Five configurations of those (CONFIGS) are recorded.

Recorded:
  H, W, bbox (hs, ws, hl, wl), pose (3,4), directions (H*W,3), normals (H*W,3), obj_depth (H*W),
  lSGs (33,7), decay (H*W,33), metal_map, rough_map (H*W), albedo_row (1,3), albedo_map (H*W,3)
  config_names, and per configuration k:
  out64 (K,H,W,3) float64 / out32 (K,H,W,3) float32   the reference in fp64 / fp32 on the same fp32 inputs
  class_names, class_of (H*W) the class index of every pixel (sg_shade_ref.pixel_classes)
  ref32_abs (K,C)   max |out32 - out64| over the class's pixels and channels
  ref32_rel (K,C)   max |out32 - out64| / (1e-3 + |out64|)

Run:  python tests/golden/make_sg_golden.py   (needs the reference; seconds)
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

import sg_shade_ref as SR  # noqa: E402

H, W = 13, 11
BBOX = (2, 1, 11, 10)  # hs, ws, hl, wl: strictly inside the frame, 9 x 9
SEED = 21
L = 33
EPS32 = np.float32(1e-6)
CONFIGS = SR.CONFIGS


def load_reference():
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    fn = types.ModuleType("torchvision.transforms.functional")
    fn.gaussian_blur = None  # (the cubemap blur of the SH path: never reached from SG_render_core)
    tv.transforms, tr.functional = tr, fn
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.functional": fn})
    spec = importlib.util.spec_from_file_location("ref_render_utils", os.path.join(REF, "insert", "render_utils.py"))
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    # the reference's datasets/ without its __init__ (image loaders this host lacks); get_rays does not touch the
    # meshgrid helper its module imports from kornia
    kornia = sys.modules.setdefault("kornia", types.ModuleType("kornia"))
    kornia.__dict__.setdefault("create_meshgrid", None)
    pkg = types.ModuleType("datasets")
    pkg.__path__ = [os.path.join(REF, "datasets")]
    sys.modules["datasets"] = pkg
    from datasets.ray_utils import get_rays
    return ru, get_rays


def render_object(ru, get_rays, bbox, normals, depths, lSGs, pose, directions, metal, rough, albedo, decay, clamp01):
    """main.py:521-594 with use_sg_base; whole-frame inputs, sliced to the box here.  decay (H,W,L) or None:
    sg_shadow.py:143-152 (the amplitudes times the decay, the rest of each light repeated per pixel)."""
    hs, ws, hl, wl = bbox
    height, width = hl - hs, wl - ws
    box = lambda a: a[hs:hl, ws:wl]  # noqa: E731
    depths_b = box(depths)
    mask = (depths_b > 1e-6).flatten()
    normal_msk = box(normals).reshape(-1, 3)[mask]
    if albedo is None:
        albedo = torch.ones_like(normal_msk)
    elif albedo.shape[0] == 1:
        albedo = albedo.expand_as(normal_msk)
    else:
        albedo = box(albedo.reshape(H, W, 3)).reshape(-1, 3)[mask]
    if type(metal) == float:
        metal = torch.ones(normal_msk.shape[0], 1) * metal
    else:
        metal = box(metal.reshape(H, W)).reshape(-1, 1)[mask]
    if type(rough) == float:
        rough = torch.ones(normal_msk.shape[0], 1) * rough
    else:
        rough = box(rough.reshape(H, W)).reshape(-1, 1)[mask].clip(0.2, 1.0)
    rays_o, rays_d = get_rays(box(directions.reshape(H, W, 3)).reshape(-1, 3), pose)
    rays_d = rays_d.reshape(-1, 3)[mask]
    vdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)  # insert_utils.normalize
    self_shadow = decay is not None
    if self_shadow:
        dec = box(decay).reshape(height * width, -1)[mask].unsqueeze(-1)  # px,lx,1
        t = lSGs[:, :4].unsqueeze(0).expand(dec.shape[0], dec.shape[1], 4)
        lights = torch.concat([t, lSGs[:, -3:].unsqueeze(0) * dec], -1)  # px,lx,7
    else:
        lights = lSGs
    cols = ru.SG_render_core(albedo, metal, rough, normal_msk, vdirs, lights, clamp01, self_shadow, None)
    render_res_t = torch.zeros(height * width, 3)
    render_res_t[mask] = cols
    render_res = torch.zeros(H, W, 3)
    render_res[hs:hl, ws:wl, :] = render_res_t.reshape(height, width, 3)
    return render_res


def design(gen):
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    # a pinhole camera looking down its z axis, rotated by a seeded orthogonal matrix
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    directions = torch.stack([(u - W / 2 + 0.5) / 14.0, (v - H / 2 + 0.5) / 14.0, torch.ones_like(u)], -1)
    directions = directions.reshape(-1, 3).float()
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=gen, dtype=torch.float64))
    pose = torch.cat([q, torch.tensor([[0.3], [-0.2], [1.1]], dtype=torch.float64)], 1).float()

    n = H * W
    hs, ws, hl, wl = BBOX
    inbox = torch.zeros(H, W, dtype=torch.bool)
    inbox[hs:hl, ws:wl] = True
    inbox = inbox.reshape(-1)
    inside = torch.nonzero(inbox)[:, 0]
    inside = inside[torch.randperm(inside.numel(), generator=gen)]
    depth = np.zeros(n, dtype=np.float32)
    below, above = np.nextafter(EPS32, np.float32(0)), np.nextafter(EPS32, np.float32(1))
    k = 0
    for val in (0.0, 5e-7, EPS32, below, above):
        depth[inside[k:k + 3].numpy()] = val
        k += 3
    rest = inside[k:]
    depth[rest.numpy()] = (0.5 + 2.5 * rnd(rest.numel())).float().numpy()
    outside = torch.nonzero(~inbox)[:, 0]
    od = (0.5 + 2.5 * rnd(outside.numel())).float().numpy()
    od[::3] = 0.0  # every third pixel outside the box has no object either
    depth[outside.numpy()] = od

    # normals: a prescribed cosine c against the unit view direction, a seeded tangent, a length in [0.3, 3]
    view = torch.from_numpy(SR.view_dirs(directions.numpy(), pose.numpy()))
    covered = torch.nonzero(torch.from_numpy(SR.cover_mask(H, W, BBOX, depth)))[:, 0]
    covered = covered[torch.randperm(covered.numel(), generator=gen)]
    c = 0.3 + 0.7 * rnd(n)                                   # uncovered pixels: anything nonzero
    counts = (("facing", 30), ("middle", 10), ("grazing", 14))
    k = 0
    for name, m in counts:
        sel = covered[k:k + m]
        k += m
        if name == "facing":
            c[sel] = 0.3 + 0.7 * rnd(m)
            c[sel[0]] = 1.0                                  # head on
        elif name == "middle":
            c[sel] = 0.06 + 0.22 * rnd(m)
        else:
            c[sel] = 0.004 + 0.04 * rnd(m)
    sel = covered[k:]
    c[sel] = -(0.02 + 0.9 * rnd(sel.numel()))                # back-facing: the rest
    t = torch.linalg.cross(view, torch.randn(n, 3, generator=gen, dtype=torch.float64))
    t = t / torch.linalg.vector_norm(t, dim=-1, keepdim=True)
    normals = c[:, None] * view + torch.sqrt((1 - c * c).clamp(min=0))[:, None] * t
    normals = (normals * (0.3 + 2.7 * rnd(n))[:, None]).float()

    # lights: seeded axes, sharpness over 1e-1 .. 1e4 (light 0 a middling one: it is the L = 1 case), amplitudes
    # that give every light an energy of the same order whatever its sharpness, one light dark
    ax = torch.randn(L, 3, generator=gen, dtype=torch.float64)
    ax = ax / torch.linalg.vector_norm(ax, dim=-1, keepdim=True)
    lam = torch.logspace(-1, 4, L, dtype=torch.float64)[torch.randperm(L, generator=gen)]
    lam[0] = 20.0
    energy = 0.1 + 1.2 * rnd(L, 3)
    amp = energy * (lam / (2 * np.pi * (1 - torch.exp(-2 * lam))))[:, None]
    amp[0] *= 8.0
    amp[5] = 0.0
    lSGs = torch.cat([ax, lam[:, None], amp], 1).float()
    decay = rnd(n, L).float()
    decay[:, 7] = 1.0
    decay[::5, 3] = 0.0
    metal_map = rnd(n).float()
    rough_map = (0.05 + 1.2 * rnd(n)).float()                # below 0.2 and above 1: the clip shows
    albedo_row = torch.tensor([[0.8, 0.5, 0.3]])
    albedo_map = (0.05 + 0.95 * rnd(n, 3)).float()
    return dict(directions=directions, pose=pose, normals=normals, obj_depth=torch.from_numpy(depth), lSGs=lSGs,
                decay=decay, metal_map=metal_map, rough_map=rough_map, albedo_row=albedo_row, albedo_map=albedo_map)


def run(ru, get_rays, d, cfg, dtype):
    torch.set_default_dtype(dtype)  # (SG_render_core builds its lobes with torch.ones(...))
    try:
        c = lambda a: a.to(dtype)  # noqa: E731
        lights = c(d["lSGs"][:cfg["L"]])
        pick = lambda v, m, r=None: c(d[m]) if v == "map" else (c(d[r]) if v == "row" else v)  # noqa: E731
        decay = c(d["decay"][:, :cfg["L"]]).reshape(H, W, -1) if cfg["decay"] else None
        return render_object(ru, get_rays, BBOX, c(d["normals"]).reshape(H, W, 3), c(d["obj_depth"]).reshape(H, W),
                             lights, c(d["pose"]), c(d["directions"]), pick(cfg["metal"], "metal_map"),
                             pick(cfg["rough"], "rough_map"), pick(cfg["albedo"], "albedo_map", "albedo_row"),
                             decay, cfg["clamp01"])
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    ru, get_rays = load_reference()
    torch.set_num_threads(1)
    d = design(torch.Generator().manual_seed(SEED))
    np_in = {k: v.numpy() for k, v in d.items()}
    classes = SR.pixel_classes(H, W, np_in["directions"], np_in["pose"], BBOX, np_in["normals"], np_in["obj_depth"])
    class_of = np.full(H * W, -1, dtype=np.int32)
    for i, name in enumerate(SR.CLASSES):
        class_of[classes[name]] = i
    assert (class_of >= 0).all()
    print({name: int(classes[name].sum()) for name in SR.CLASSES})

    out64, out32 = [], []
    ref32_abs = np.zeros((len(CONFIGS), len(SR.CLASSES)))
    ref32_rel = np.zeros_like(ref32_abs)
    for k, (name, cfg) in enumerate(CONFIGS.items()):
        o64 = run(ru, get_rays, d, cfg, torch.float64).numpy()
        o32 = run(ru, get_rays, d, cfg, torch.float32).numpy()
        assert o64.dtype == np.float64 and o32.dtype == np.float32
        assert np.isfinite(o64).all() and np.isfinite(o32).all(), name   # the reference is finite on every pixel
        err = np.abs(o32.astype(np.float64) - o64).reshape(-1, 3)
        rel = err / (1e-3 + np.abs(o64).reshape(-1, 3))
        for i, cname in enumerate(SR.CLASSES):
            m = classes[cname]
            ref32_abs[k, i], ref32_rel[k, i] = err[m].max(), rel[m].max()
        out64.append(o64)
        out32.append(o32)
        print(f"{name:16s} max {o64.max():.3f}  >1: {int((o64 > 1).sum())}  ==1: {int((o64 == 1).sum())}  "
              f"abs {ref32_abs[k]}  rel {ref32_rel[k]}")
    out = dict(np_in, H=H, W=W, bbox=np.array(BBOX, dtype=np.int32), seed=SEED,
               config_names=np.array(list(CONFIGS)), class_names=np.array(SR.CLASSES), class_of=class_of,
               out64=np.stack(out64), out32=np.stack(out32), ref32_abs=ref32_abs, ref32_rel=ref32_rel)
    path = os.path.join(HERE, "sg_shade.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
