#!/usr/bin/env python3
"""Device time of the test-set metrics on one 800x800 frame:
  update      metrics.ImageMetrics.update (MSE + SSIM, ngp_image_metrics)
  psnr_torch  the per-frame PSNR expression scripts/train_scene.py evaluated
              before: pred.clamp(0, 1), torch.mean((pred - gt) ** 2) (device
              time only; its .item() host sync is reported beside it as wall time)
  ssim_torch  an fp32 torch conv2d SSIM (tests/metrics_ref.ssim_torch_fp32)
Device events around every call, --reps calls after --warmup; the median.
Prints one JSON line.  Usage: python scripts/metrics_timing.py [--wh 800 800]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ar-nerf_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402


def _timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--wh", type=int, nargs=2, default=(800, 800))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--render-ms", type=float, default=8.0, help="a test frame's render time, for the share")
    a = ap.parse_args(argv)
    import metrics
    import metrics_ref as MR
    dev = torch.device("cuda", 0)
    w, h = a.wh
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(h * w, 3, generator=g).to(dev)
    pred = (gt + 0.05 * torch.randn(h * w, 3, generator=g).to(dev)).contiguous()
    im = metrics.ImageMetrics((w, h), 1, dev)

    def update():
        im.reset()
        im.update(pred, gt, clamp=True)

    def psnr_torch():
        return torch.mean((pred.clamp(0, 1) - gt) ** 2)

    def ssim_torch():
        return MR.ssim_torch_fp32(pred.clamp(0, 1), gt, h, w)[1]

    res = {"wh": [w, h], "reps": a.reps, "update": _timed(update, a.warmup, a.reps),
           "psnr_torch": _timed(psnr_torch, a.warmup, a.reps), "ssim_torch": _timed(ssim_torch, a.warmup, a.reps)}
    t0 = time.perf_counter()
    for _ in range(a.reps):
        psnr_torch().item()
    res["psnr_torch_with_item_wall_us"] = round((time.perf_counter() - t0) / a.reps * 1e6, 2)
    # what the kernel has to move: both frames once, plus the tile slots and the two results
    res["bytes_per_frame"] = 2 * h * w * 3 * 4 + 2 * int(im._ws.numel()) * 8 + 8
    res["update_share_of_render"] = round(res["update"]["median_us"] / (a.render_ms * 1e3), 4)
    res["kernel_vs_fp32_torch_ssim"] = abs(float(im.compute()["ssim"][0]) - float(ssim_torch()))
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
