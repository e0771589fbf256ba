"""Generate tests/golden/insert_frame.npz: one frame of the insertion app's
per-frame call (insert/main.py:620-684, Insertor.render_insert_object) through
the REFERENCE's own models.rendering.render and datasets.ray_utils.get_rays
(read from the reference checkout, never copied), with this repo's CPU oracle
plugged in as `vren` / `tinycudann` (make_golden.install_stubs).

The frame is 16 x 16 with the model and camera of lego_test (make_golden.
test_render_case; table amplitude 0.5, see AMP), the rectangle rows 5..15, columns 0..12 (neither square nor
full; it holds the frame's one ray that misses the box), and the app's settings: render(test_time=True, T_threshold=1e-2,
max_samples=100, IM_bkg=<object colour, clipped>, mesh_depth_map=<object depth,
clipped>), then the write into the last_rgb / last_depth canvases (main.py:
652-654) and pts = rays_o + rays_d * depth (main.py:429).

The object depth map is designed (tests/test_insert_ref_cpu.py states what it
must contain): pixels of the rectangle are given, by class, depth 0, a depth in
(0, 1e-6), float32(1e-6) and its two fp32 neighbours, a depth <= t1, one in
(t1, t2) and one >= t2 of their own ray; the rest get a seeded mix of those.

Recorded (arrays only; parameters are regenerated from seeds as for lego_test):
  H, W, rect (hs, ws, hl, wl), scale, seed, amp, pose (3,4), directions (H*W,3)
  pix (n)                 the rectangle's pixel indices, row-major, as the app slices them
  rays_o, rays_d (n,3)    get_rays(directions[hs:hl, ws:wl], pose)
  hits_raw (n,2)          AABB + near clamp, before the mesh clip
  hits_clip (n,2)         what the loop was handed (the clone of hits_t at its first march)
  obj_rgb (H,W,3), obj_depth (H,W)
  rgb, opacity, depth (n), total_samples        render(...)'s results
  rgb_pre (n,3)           the same call with blend_bkg=False (the loop's rgb before the blend)
  alive_after (iters)     rays still alive after each iteration's composite
  n_samples (iters)       N_samples of each iteration
  t_margin                the least |T / T_threshold - 1| over every sample the composites took (>= T_MARGIN)
  total_samples_full_n, opacity_full_n (n)
                          the same rays rendered in a batch padded to H*W rays with rays that miss the box
                          (N_rays = H*W in the N_samples rule; the padding dies in iteration 1 without a sample)
  canvas0_rgb (H,W,3), canvas0_depth (H,W,1)    the canvases before the frame (junk)
  canvas_rgb, canvas_depth                      after last_rgb[hs:hl, ws:wl] = rgb etc.
  pts (n,3)               rays_o + rays_d * depth

Run:  python tests/golden/make_insert_golden.py   (needs the reference; ~1 min)
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import install_stubs, table_override  # noqa: E402

import oracle as O  # noqa: E402
import synthetic as S  # noqa: E402

# lego_test's model (make_golden.main: scale, table seed, bitfield, camera) with the table amplitude halved: at
# amplitude 1 every ray of this camera is opaque or out of occupied cells before the app's 100-sample budget ends,
# so N_rays would not show in any pixel; at 0.5 some rays are cut short by the budget and others still end on T
SCALE, SEED, AMP = 0.5, 3, 0.5
H = W = 16
RECT = (5, 0, 16, 13)            # hs, ws, hl, wl: holds the one pixel (15, 0) whose ray misses the box
DESIGN_SEED = 11
SETTINGS = dict(test_time=True, T_threshold=1e-2, max_samples=100)
EPS = np.float32(1e-6)
# No transmittance the composite sees may lie within this relative distance of T_threshold: the product's fp16
# field differs from the oracle's by ~1e-3 relative in sigma, and a ray that ends one sample earlier or later
# changes the alive count, with it the whole N_samples schedule, and the pixels of every ray the budget cuts.
T_MARGIN = 0.02


def design_depth(t1, t2, pix, gen):
    """obj_depth (H*W): by class over the rectangle's rays (t1, t2: their near-clamped box interval, -1 on a miss)"""
    depth = torch.zeros(H * W)
    hit = torch.nonzero(t1 >= 0)[:, 0]
    order = hit[torch.randperm(hit.numel(), generator=gen)]
    below, above = np.nextafter(EPS, np.float32(0)), np.nextafter(EPS, np.float32(1))
    k = 0

    def take(m):
        nonlocal k
        sel = order[k:k + m]
        k += m
        return sel

    depth[pix[take(4)]] = 0.0
    depth[pix[take(4)]] = 5e-7
    depth[pix[take(3)]] = float(EPS)
    depth[pix[take(3)]] = float(below)
    depth[pix[take(3)]] = float(above)
    s = take(8)
    depth[pix[s]] = t1[s] * torch.rand(8, generator=gen)             # <= t1: zero length
    s = take(4)
    depth[pix[s]] = t1[s]                                            # == t1
    s = take(8)
    depth[pix[s]] = t2[s] * (1 + torch.rand(8, generator=gen))       # >= t2: no clip
    rest = order[k:]
    u = torch.rand(rest.numel(), generator=gen)
    between = t1[rest] + (t2[rest] - t1[rest]) * (0.05 + 0.9 * torch.rand(rest.numel(), generator=gen))
    depth[pix[rest]] = torch.where(u < 0.6, between, torch.zeros_like(between))  # in (t1, t2), or no object
    miss = torch.nonzero(t1 < 0)[:, 0]
    # a miss under the object (every other one): the clip leaves its -1 alone
    depth[pix[miss]] = (0.05 + 0.3 * torch.rand(miss.numel(), generator=gen)) * ((torch.arange(miss.numel()) + 1) % 2)
    return depth


def main():
    install_stubs()
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    import vren
    # the reference's datasets/ without its __init__ (image and EXR loaders this host lacks); kornia is an
    # empty stub here, and get_rays does not touch the meshgrid helper its module imports from it
    import types
    from make_golden import REF
    sys.modules["kornia"].__dict__.setdefault("create_meshgrid", None)
    pkg = types.ModuleType("datasets")
    pkg.__path__ = [os.path.join(REF, "datasets")]
    sys.modules["datasets"] = pkg
    from datasets.ray_utils import get_rays
    from models.networks import NGP
    from models.rendering import NEAR_DISTANCE, render

    log = {"hits": [], "alive": [], "ns": [], "margin": []}
    march, composite = vren.raymarching_test, vren.composite_test_fw

    def raymarching_test(*a):
        log["hits"].append(a[2].detach().clone())
        log["ns"].append(int(a[-1]))
        return march(*a)

    def composite_test_fw(*a):
        # the transmittance after every sample the composite takes (up to a ray's end): its distance from T_threshold
        sig, deltas, al, thr, n_eff = a[0].double(), a[2].double(), a[5].long(), float(a[6]), a[7].long()
        T = (1 - a[8].double()[al])[:, None] * torch.cumprod(torch.exp(-sig * deltas), 1)
        k = torch.arange(T.shape[1])[None, :]
        ended_before = torch.cat([torch.zeros_like(T[:, :1], dtype=torch.bool), (T <= thr)[:, :-1]], 1).cumsum(1) > 0
        taken = (k < n_eff[:, None]) & ~ended_before
        if taken.any():
            log["margin"].append(float((T[taken] / thr - 1).abs().min()))
        out = composite(*a)
        log["alive"].append(int((a[5] >= 0).sum()))
        return out

    vren.raymarching_test, vren.composite_test_fw = raymarching_test, composite_test_fw

    model = NGP(SCALE)
    table_override(model, 100 + SEED, AMP)
    model.density_bitfield.copy_(S.packbits_cpu(S.shell_density_grid(128, model.cascades, SCALE), 0.5))
    sc = S.AnalyticScene(W=W, H=H, n_images=2, scale=SCALE)
    pose, directions = sc.poses[0].contiguous(), sc.directions.contiguous()
    hs, ws, hl, wl = RECT
    h, w = hl - hs, wl - ws
    n = h * w
    # the app's slices (main.py:639-641)
    rays_o, rays_d = get_rays(directions.reshape(H, W, 3)[hs:hl, ws:wl, :].reshape(-1, 3), pose)
    rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
    pix = torch.arange(H * W).reshape(H, W)[hs:hl, ws:wl].reshape(-1)
    _, ht, _ = O.ray_aabb_intersect(rays_o, rays_d, model.center, model.half_size, 1)
    ht = ht[:, 0].clone()
    ht[(ht[:, 0] >= 0) & (ht[:, 0] < NEAR_DISTANCE), 0] = NEAR_DISTANCE

    # the design seed: the first from DESIGN_SEED on whose frame leaves a ray alive when the sample budget ends
    # (then the N_samples schedule, and with it N_rays, shows in the pixels)
    for design_seed in range(DESIGN_SEED, DESIGN_SEED + 32):
        gen = torch.Generator().manual_seed(design_seed)
        obj_depth = design_depth(ht[:, 0], ht[:, 1], pix, gen).reshape(H, W)
        obj_rgb = torch.rand(H, W, 3, generator=gen)
        rgb_clip = obj_rgb[hs:hl, ws:wl, :].reshape(-1, 3)
        depth_clip = obj_depth[hs:hl, ws:wl].flatten()
        for v in log.values():
            v.clear()
        with torch.no_grad():
            res = render(model, rays_o, rays_d, IM_bkg=rgb_clip, mesh_depth_map=depth_clip, **SETTINGS)
        hits_clip, alive_after, n_samples = log["hits"][0], list(log["alive"]), list(log["ns"])
        print("design seed", design_seed, "alive_after", alive_after, "n_samples", n_samples)
        t_margin = min(log["margin"])
        print("   T margin", t_margin)
        if alive_after[-1] > 0 and len(alive_after) == len(n_samples) and sum(n_samples) >= SETTINGS["max_samples"] \
                and t_margin >= T_MARGIN:
            break
    else:
        raise SystemExit("no design seed leaves a ray alive at the end of the budget")

    with torch.no_grad():
        pre = render(model, rays_o, rays_d, IM_bkg=rgb_clip, mesh_depth_map=depth_clip, blend_bkg=False, **SETTINGS)
        # the same rays in a batch of H*W: the padding looks away from the box
        pad = H * W - n
        o_full = torch.cat([rays_o, torch.full((pad, 3), 5.0)]).contiguous()
        d_full = torch.cat([rays_d, torch.ones(pad, 3) / 3 ** 0.5]).contiguous()
        full = render(model, o_full, d_full, IM_bkg=torch.cat([rgb_clip, torch.zeros(pad, 3)]),
                      mesh_depth_map=torch.cat([depth_clip, torch.zeros(pad)]), **SETTINGS)
    assert float(full["opacity"][n:].abs().max()) == 0.0
    assert not torch.equal(full["opacity"][:n], res["opacity"]), "the budget must cut a ray short"
    for k in ("opacity", "depth"):
        assert torch.equal(pre[k], res[k])

    # the canvases (main.py:650-654) and the surface points (main.py:429)
    canvas0_rgb, canvas0_depth = torch.rand(H, W, 3, generator=gen) + 2.0, torch.rand(H, W, 1, generator=gen) + 2.0
    last_rgb, last_depth = canvas0_rgb.clone(), canvas0_depth.clone()
    rgb = res["rgb"].reshape(h, w, 3)
    depth_sur = res["depth"].reshape(h, w, 1)
    last_rgb[hs:hl, ws:wl, :] = rgb
    last_depth[hs:hl, ws:wl, :] = depth_sur
    pts = rays_o + rays_d * res["depth"].reshape(-1, 1)

    out = {
        "H": H, "W": W, "rect": np.array(RECT, dtype=np.int32), "scale": SCALE, "seed": SEED, "amp": AMP,
        "design_seed": design_seed, "t_margin": t_margin,
        "pose": pose.numpy(), "directions": directions.numpy(), "pix": pix.numpy(),
        "rays_o": rays_o.numpy(), "rays_d": rays_d.numpy(), "hits_raw": ht.numpy(), "hits_clip": hits_clip.numpy(),
        "obj_rgb": obj_rgb.numpy(), "obj_depth": obj_depth.numpy(),
        "rgb": res["rgb"].numpy(), "opacity": res["opacity"].numpy(), "depth": res["depth"].numpy(),
        "total_samples": int(res["total_samples"]), "rgb_pre": pre["rgb"].numpy(),
        "alive_after": np.array(alive_after, dtype=np.int64), "n_samples": np.array(n_samples, dtype=np.int64),
        "total_samples_full_n": int(full["total_samples"]), "opacity_full_n": full["opacity"][:n].numpy(),
        "canvas0_rgb": canvas0_rgb.numpy(), "canvas0_depth": canvas0_depth.numpy(),
        "canvas_rgb": last_rgb.numpy(), "canvas_depth": last_depth.numpy(), "pts": pts.numpy(),
        "T_threshold": SETTINGS["T_threshold"], "max_samples": SETTINGS["max_samples"],
    }
    path = os.path.join(HERE, "insert_frame.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(path, os.path.getsize(path), "bytes")
    print("misses", int((ht[:, 0] < 0).sum()), "of", n, "alive_after", alive_after, "n_samples", n_samples,
          "total", out["total_samples"], "full-N total", out["total_samples_full_n"])


if __name__ == "__main__":
    main()
