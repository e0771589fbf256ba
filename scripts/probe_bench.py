#!/usr/bin/env python3
"""Timing of the light-probe path: probes.sh_probes (probe rays, device loop,
finish and SH9 projection on the device) against the composed path that needs
none of the probe kernels: expand the rays with torch, render(test_time=True,
blend_bkg=False), project the radiance and 1 - opacity with the reference's
torch get_SH_coeff expressions.

Workloads, on a seeded random NGP with a 2 % random occupancy bitfield:
  sphere  64 probes x 2048 random sphere rays (generate_SH_probes_for_precompute)
  cube    one 6 x 32^2 cube-map probe (generate_probe)
The two paths are alternated in one process after a warm-up of both; the time
of a call is a host clock around work that ends in a device synchronise.
Prints one JSON line (median and min ms per call, ratio composed / sh_probes,
and the largest difference of the coefficients).  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ar-nerf_amd")]

import torch  # noqa: E402

import probes  # noqa: E402
from models.networks import NGP  # noqa: E402
from models.rendering import render  # noqa: E402

DEV = "cuda"


def scene_model(scale=0.5, occ_frac=0.02, seed=5):
    m = NGP(scale)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.params.uniform_(-1, 1, generator=g)
        bits = (torch.rand(m.density_bitfield.numel() * 8, generator=g) < occ_frac).to(torch.uint8)
        m.density_bitfield.copy_((bits.view(-1, 8) << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8))
    return m.to(DEV)


def torch_sh_coeff(rays_d, vals):
    """get_SH_coeff as the reference writes it (insert_utils.py:132-136), in torch."""
    shs = probes.sh9_basis(rays_d)
    res = torch.matmul(shs.unsqueeze(-1), vals.unsqueeze(-2))
    return torch.sum(res, dim=1) * 4 * torch.pi / rays_d.shape[1]


@torch.no_grad()
def composed(model, pts, dirs):
    P, R = dirs.shape[:2]
    o = pts[:, None].expand(P, R, 3).reshape(-1, 3)
    out = render(model, o, dirs.reshape(-1, 3), test_time=True, blend_bkg=False)
    rgb = out["rgb"].reshape(P, R, 3)
    trans = 1.0 - out["opacity"].reshape(P, R, 1)
    return torch_sh_coeff(dirs, rgb), torch_sh_coeff(dirs, trans)


def fused(model, pts, dirs):
    out = probes.sh_probes(model, pts, dirs, blend_bkg=False, probes_per_batch=pts.shape[0])
    return out["rgb_sh"], out["trans_sh"]


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_bench needs the GPU: a CPU run gives no time")
    model = scene_model()
    g = torch.Generator().manual_seed(1)
    work = {
        "sphere_64x2048": ((torch.rand(64, 3, generator=g) - 0.5).mul(0.8).to(DEV),
                           probes.get_sphere_rays(64, 2048, generator=g, device=DEV).contiguous()),
        "cube_1x6144": (torch.tensor([[0.05, -0.1, 0.02]], device=DEV),
                        probes.get_cubemap_rays(1, 32).to(DEV).contiguous()),
    }
    result = {}
    for name, (pts, dirs) in work.items():
        for _ in range(a.warmup):
            ref = composed(model, pts, dirs)
            got = fused(model, pts, dirs)
        diff = max(float((x - y).abs().max()) for x, y in zip(got, ref))
        t = {"sh_probes": [], "composed": []}
        for _ in range(a.reps):
            t["composed"].append(timed(composed, model, pts, dirs))
            t["sh_probes"].append(timed(fused, model, pts, dirs))
        med = {k: statistics.median(v) for k, v in t.items()}
        result[name] = {"sh_probes_ms": round(med["sh_probes"], 4), "composed_ms": round(med["composed"], 4),
                        "sh_probes_min_ms": round(min(t["sh_probes"]), 4),
                        "composed_min_ms": round(min(t["composed"]), 4),
                        "ratio_composed_over_sh_probes": round(med["composed"] / med["sh_probes"], 3),
                        "max_coeff_diff": diff}
    print(json.dumps({"probe_bench": result, "reps": a.reps, "warmup": a.warmup}), flush=True)


if __name__ == "__main__":
    main()
