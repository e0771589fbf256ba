#!/usr/bin/env python3
"""Timing of the insertion frame: models.rendering.render_insert (one cached
renderer.InsertRenderer: frame opening, device loop, closing launch; the
rectangle is a device value) against the composed path it replaces, which needs
none of the insertion kernels: vren.raygen_aabb on the rectangle's pixels,
render(test_time=True, IM_bkg=clip, mesh_depth_map=clip) and the torch scatter
into the canvases (the body of the reference's Insertor.render_insert_object,
insert/main.py:632-660).

Workload: an 800 x 800 frame on a seeded random NGP with a 2 % random occupancy
bitfield (scripts/probe_bench.py's model), the app's loop settings
(T_threshold 1e-2, max_samples 100), a synthetic object -- a disc of constant
depth with a colour ramp.  Two sequences of --frames frames:
  full   a whole-screen redraw on every frame (a moving camera)
  rect   a rectangle that drifts and changes size every frame (seeded sides
         between 150 and 300 pixels: a moving object)
Both paths first render every frame of both sequences and their canvases are
asserted equal, bit for bit.  Then the two paths are alternated frame by frame
in one process after a warm-up of both; the time of a frame is a host clock
around work that ends in a device synchronise.  Prints one JSON line (median and
min ms per frame and path, ratio composed / render_insert).  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ar-nerf_amd")]

import torch  # noqa: E402

import synthetic as S  # noqa: E402
import vren  # noqa: E402
from models.networks import NGP  # noqa: E402
from models.rendering import NEAR_DISTANCE, render, render_insert  # noqa: E402

DEV = "cuda"
H = W = 800
APP = dict(T_threshold=1e-2, max_samples=100)


def scene_model(scale=0.5, occ_frac=0.02, seed=5):
    m = NGP(scale)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.params.uniform_(-1, 1, generator=g)
        bits = (torch.rand(m.density_bitfield.numel() * 8, generator=g) < occ_frac).to(torch.uint8)
        m.density_bitfield.copy_((bits.view(-1, 8) << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8))
    return m.to(DEV)


def synthetic_object(pose):
    """A disc in the middle of the screen at the depth of the box centre, with a colour ramp"""
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    disc = ((yy - H / 2) ** 2 + (xx - W / 2) ** 2) < (0.2 * H) ** 2
    depth = torch.where(disc, pose[:, 3].norm(), torch.zeros((), device=DEV)).float().contiguous()
    rgb = torch.stack([xx / W, yy / H, 1 - xx / W], -1).float() * disc[..., None]
    return rgb.contiguous(), depth


def sequences(frames, seed=1):
    g = torch.Generator().manual_seed(seed)
    rects, y, x = [], 250, 250
    for _ in range(frames):
        h, w = (int(v) for v in torch.randint(150, 301, (2,), generator=g))
        dy, dx = (int(v) for v in torch.randint(-12, 13, (2,), generator=g))
        y, x = min(max(y + dy, 0), H - h), min(max(x + dx, 0), W - w)
        rects.append((y, x, y + h, x + w))
    return {"full": [(0, 0, H, W)] * frames, "rect": rects}


class Composed:
    """The parent path: ray generation, render() and the app's canvas writes"""

    def __init__(self, model, dirs, pose):
        self.model, self.dirs, self.pose = model, dirs, pose.reshape(1, 3, 4).contiguous()
        self.pix = torch.arange(H * W, device=DEV).view(H, W)
        self.img = torch.zeros(H * W, dtype=torch.int64, device=DEV)
        self.rgb = torch.zeros(H, W, 3, device=DEV)
        self.depth = torch.zeros(H, W, device=DEV)
        self.pts = torch.zeros(H, W, 3, device=DEV)

    @torch.no_grad()
    def frame(self, rect, obj_rgb, obj_depth):
        hs, ws, hl, wl = rect
        h, w = hl - hs, wl - ws
        pix = self.pix[hs:hl, ws:wl].reshape(-1)
        m = self.model
        o, d, _ = vren.raygen_aabb(self.dirs, self.pose, self.img[:h * w], pix, m.center, m.half_size, NEAR_DISTANCE)
        res = render(m, o, d, test_time=True, IM_bkg=obj_rgb[hs:hl, ws:wl].reshape(-1, 3),
                     mesh_depth_map=obj_depth[hs:hl, ws:wl].flatten(), **APP)
        self.rgb[hs:hl, ws:wl] = res["rgb"].reshape(h, w, 3)
        self.depth[hs:hl, ws:wl] = res["depth"].reshape(h, w)
        self.pts[hs:hl, ws:wl] = (o + d * res["depth"][:, None]).reshape(h, w, 3)
        return {"rgb": self.rgb, "depth": self.depth, "pts": self.pts}


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("insert_bench needs the GPU: a CPU run gives no time")
    model = scene_model()
    dirs = S.get_ray_directions(H, W, S.intrinsics(W, H)).reshape(-1, 3).to(DEV).contiguous()
    pose = S.make_poses(2, seed=0)[1].to(DEV).contiguous()
    obj_rgb, obj_depth = synthetic_object(pose)
    comp = Composed(model, dirs, pose)
    new = lambda rect: render_insert(model, pose, dirs, H, W, rect, obj_rgb, obj_depth, **APP)  # noqa: E731
    old = lambda rect: comp.frame(rect, obj_rgb, obj_depth)  # noqa: E731
    seqs = sequences(a.frames)
    for name, rects in seqs.items():  # equal canvases on every frame of both sequences
        for i, rect in enumerate(rects):
            got, ref = new(rect), old(rect)
            for k in ("rgb", "depth", "pts"):
                assert torch.equal(got[k], ref[k]), (name, i, rect, k)
    rr = next(iter(model._insert_renderers.values()))
    assert len(model._insert_renderers) == 1 and rr.n_captures == 2
    result = {}
    for name, rects in seqs.items():
        for rect in rects[:a.warmup]:
            old(rect)
            new(rect)
        t = {"render_insert": [], "composed": []}
        for i, rect in enumerate(rects):  # alternated, the order swapped every frame
            for which in (("composed", "render_insert") if i % 2 == 0 else ("render_insert", "composed")):
                t[which].append(timed(old if which == "composed" else new, rect))
        med = {k: statistics.median(v) for k, v in t.items()}
        result[name] = {"render_insert_ms": round(med["render_insert"], 4), "composed_ms": round(med["composed"], 4),
                        "render_insert_min_ms": round(min(t["render_insert"]), 4),
                        "composed_min_ms": round(min(t["composed"]), 4),
                        "ratio_composed_over_render_insert": round(med["composed"] / med["render_insert"], 3)}
    assert rr.n_captures == 2
    print(json.dumps({"insert_bench": result, "frames": a.frames, "warmup": a.warmup}), flush=True)


if __name__ == "__main__":
    main()
