#!/usr/bin/env python3
"""Device time of the object shade on one frame:
  kernel  shading.sg_shade       (ngp_sg_shade: one launch, no temporaries)
  torch   shading.sg_shade_torch (the reference's formulation on the GPU:
          mask gather, (pixels, L, .) temporaries, masked scatter)
at 800 x 800 with L = 32 lights, for a 300 x 300 box and for a whole-frame box,
every pixel of the box covered, materials as maps.  Both paths are warmed up,
then timed in --rounds alternating rounds of --reps (kernel) / --torch-reps
(torch) calls between device events; per path the median of each round is
kept, and the result gives the median over rounds and their spread
(min .. max of the round medians).  The outputs of both paths at the timed
size are compared.  Prints one JSON line.
Usage: python scripts/bench_shade.py [--wh 800 800] [--lights 32]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ar-nerf_amd")]

import torch  # noqa: E402


def _round(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)


def _summary(meds):
    return {"median_us": round(statistics.median(meds), 1), "min_us": round(min(meds), 1),
            "max_us": round(max(meds), 1), "spread": round((max(meds) - min(meds)) / statistics.median(meds), 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--wh", type=int, nargs=2, default=(800, 800))
    ap.add_argument("--lights", type=int, default=32)
    ap.add_argument("--box", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--torch-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    import shading
    if not torch.cuda.is_available():
        raise SystemExit("bench_shade.py times the GPU: no device found")
    dev = torch.device("cuda", 0)
    W, H = a.wh
    L = a.lights
    g = torch.Generator().manual_seed(0)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    directions = torch.stack([(u - W / 2 + 0.5) / (1.2 * W), (v - H / 2 + 0.5) / (1.2 * W), torch.ones_like(u)], -1)
    directions = directions.reshape(-1, 3).contiguous().to(dev)
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 2.0]], device=dev)
    # normals: towards the camera, tilted
    normals = (torch.randn(H, W, 3, generator=g) * 0.6 + torch.tensor([0.0, 0.0, 1.0])).to(dev).contiguous()
    depth = (1.0 + torch.rand(H, W, generator=g)).to(dev)
    ax = torch.nn.functional.normalize(torch.randn(L, 3, generator=g), dim=-1)
    lam = 10 ** (torch.rand(L, 1, generator=g) * 5 - 1)
    amp = torch.rand(L, 3, generator=g) * lam / (2 * torch.pi * (1 - torch.exp(-2 * lam)))
    lSGs = torch.cat([ax, lam, amp], 1).to(dev).contiguous()
    mats = dict(metal=torch.rand(H * W, generator=g).to(dev), rough=(0.1 + torch.rand(H * W, generator=g)).to(dev),
                albedo=torch.rand(H * W, 3, generator=g).to(dev))
    out = torch.empty(H, W, 3, device=dev)
    res = {"wh": [W, H], "lights": L, "reps": a.reps, "torch_reps": a.torch_reps, "rounds": a.rounds, "device":
           torch.cuda.get_device_name(0)}
    b = min(a.box, H, W)
    hs, ws = (H - b) // 2, (W - b) // 2
    for name, box in (("box", (hs, ws, hs + b, ws + b)), ("whole", (0, 0, H, W))):
        bbox = torch.tensor(box, dtype=torch.int32, device=dev)
        args = (H, W, directions, c2w, bbox, normals, depth, lSGs)

        def kernel():
            return shading.sg_shade(*args, out=out, **mats)

        def torch_path():
            return shading.sg_shade_torch(*args[:4], box, *args[5:], **mats)
        for _ in range(a.warmup):
            kernel()
            torch_path()
        torch.cuda.synchronize()
        diff = float((kernel() - torch_path()).abs().max())
        k_meds, t_meds = [], []
        for _ in range(a.rounds):
            k_meds.append(_round(kernel, a.reps))
            t_meds.append(_round(torch_path, a.torch_reps))
        k, t = _summary(k_meds), _summary(t_meds)
        res[name] = {"bbox": list(box), "pixels": (box[2] - box[0]) * (box[3] - box[1]), "kernel": k, "torch": t,
                     "torch_over_kernel": round(t["median_us"] / k["median_us"], 2),
                     "max_abs_diff_kernel_vs_torch": diff}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
