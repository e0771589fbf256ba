#!/usr/bin/env python3
"""Train on a real scene and report test PSNR and SSIM -- the reference's
train.py flow (NeRFSystem: mark_invisible_cells, 8192-ray batches, occupancy
updates every 16 steps, Adam + cosine lr, test renders at the end) on the
native trainer.  Usage:
  python scripts/train_scene.py --dataset nsvf --root /data/Synthetic_NeRF/Lego --steps 30000
Prints one JSON line: rays/s of the training loop and the mean test PSNR and
SSIM over the test images (metrics.ImageMetrics: the reference's test/psnr and
test/ssim, train.py:208-249; render(test_time=True): device-resident loop,
black background -> the reference evaluates synthetic scenes on white GT, so
bg=1 like train.py's validation for esf == 0)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ar-nerf_amd")]

import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="nsvf")
    ap.add_argument("--root", required=True)
    ap.add_argument("--downsample", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=30000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--test-views", type=int, default=0, help="0 = all")
    ap.add_argument("--exact", action="store_true",
                    help="exact mode: every marched sample through the field (chunk_first=0) and the per-sample "
                         "atomic hash backward, instead of the chunked field + binned fine-level backward")
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--use_raw_HDR", action="store_true",
                    help="raw-HDR model (train.py:76-77 under --use_EXR): no colour activation, leaky_relu in "
                         "training, evaluated with output_radiance=True and without the [0,1] clamp; needs fp32 "
                         "ground truth")
    ap.add_argument("--use_exposure", action="store_true",
                    help="exposure-conditioned model on an HDR-NeRF folder (train.py:76-77 under --use_exposure; "
                         "NGPTrainer(use_exposure=True)): the rays' 4th channel is the image's exposure, test frames are "
                         "rendered at their own; --ckpt then also holds tonemapper_net_{0,1,2}.params")
    ap.add_argument("--optimize_ext", action="store_true",
                    help="refine the training cameras inside the fused step (opt.py:54; NGPTrainer(optimize_ext=True))")
    ap.add_argument("--pose_lr", type=float, default=1e-6, help="the reference hard-codes 1e-6 (train.py:149)")
    ap.add_argument("--ckpt", default=None,
                    help="write {'params'} here after training (torch.save); with --optimize_ext also 'dR' and 'dT', "
                         "the reference checkpoint's keys for the two pose parameters")
    ap.add_argument("--sync-every", type=int, default=0, help="(diagnostics) synchronize + report every N steps")
    a = ap.parse_args(argv)
    from datasets import dataset_dict
    from trainer import NGPTrainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    train = dataset_dict[a.dataset](a.root, split='train', downsample=a.downsample)
    test = dataset_dict[a.dataset](a.root, split='test', downsample=a.downsample)
    if a.use_raw_HDR and not torch.as_tensor(train.rays).is_floating_point():
        raise SystemExit(f"--use_raw_HDR needs floating-point (fp32) ground truth; dataset {a.dataset!r} at {a.root} "
                         f"holds {torch.as_tensor(train.rays).dtype} pixels only")
    expo = {}
    if a.use_exposure:
        rays = torch.as_tensor(train.rays)
        if rays.dim() != 3 or rays.shape[-1] != 4 or not bool((rays[..., 3] == rays[:, :1, 3]).all()):
            raise SystemExit(f"--use_exposure needs rays (n_img, hw, 4) with one exposure per image in the 4th channel "
                             f"(an HDR-NeRF folder); dataset {a.dataset!r} at {a.root} holds {tuple(rays.shape)}")
        gt = rays[..., :3].float().contiguous().to(dev)
        expo = {"exposure": rays[:, 0, 3].float().contiguous().to(dev)}  # one value per training image
    else:
        gt = train.gt_f32().to(dev)  # float targets, as the reference's loss sees them
    dirs, poses = train.directions.to(dev).contiguous(), train.poses.to(dev).contiguous()
    # erode for COLMAP scenes, as train.py:176-178 passes erode=dataset_name=='colmap'
    mode = dict(chunk_first=0, hash_backward="atomic") if a.exact else {}
    tr = NGPTrainer(scale=a.scale, batch_size=a.batch, device=dev, num_epochs=max(1, a.steps // 1000),
                    erode=a.dataset == "colmap", seed=a.seed, use_raw_HDR=a.use_raw_HDR,
                    optimize_ext=a.optimize_ext, pose_lr=a.pose_lr, use_exposure=a.use_exposure,
                    unit_exposure_rgb=getattr(train, "unit_exposure_rgb", None) if a.use_exposure else None, **mode)
    tr.mark_invisible_cells(train.K.to(dev), poses, train.img_wh)  # train.py:169-172
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(a.steps):
        tr.train_step(gt, dirs, poses, **expo)
        if a.sync_every and (it + 1) % a.sync_every == 0:
            torch.cuda.synchronize()
            print(f"[train_scene] step {it + 1} ok, samples {int(tr.n_samples.item())}, occupied-cell count "
                  f"{int(tr._occ_count.item())}", file=sys.stderr, flush=True)
    tr.drain()
    torch.cuda.synchronize()
    t_train = time.perf_counter() - t0
    n = len(test.poses) if a.test_views <= 0 else min(a.test_views, len(test.poses))
    tdirs = test.directions.to(dev)
    from metrics import ImageMetrics
    im = ImageMetrics(test.img_wh, max(1, n), dev)  # per-frame MSE and SSIM stay on the device: one sync after the loop
    for i in range(n):
        P = test.poses[i].to(dev)
        d = (tdirs @ P[:, :3].t()).contiguous()
        o = P[:, 3].expand_as(d).contiguous()
        at = {"exposure": torch.as_tensor(test.rays[i])[0, 3].reshape(1).float().to(dev)} if a.use_exposure else {}
        out = tr.render(o, d, bg=1.0 if tr.esf == 0 else 0.0, output_radiance=a.use_raw_HDR, **at)
        # sigmoid models are scored clamped to [0,1]; radiance is not clamped
        im.update(out["rgb"], test.rays[i].to(dev)[..., :3].float().contiguous(), clamp=not a.use_raw_HDR)
    scores = im.compute()
    if a.ckpt:
        ck = {"params": tr.full_params().detach().cpu()}
        if tr.pose_refiner is not None:
            ck.update({k: v.cpu() for k, v in tr.pose_refiner.state_dict_reference().items()})
        if a.use_exposure:
            ck.update({k: v.cpu() for k, v in tr.tone_state().items()})
        torch.save(ck, a.ckpt)
    import vren
    res = {"dataset": a.dataset, "root": a.root, "steps": a.steps, "mode": "exact" if a.exact else "default",
           "use_raw_HDR": bool(a.use_raw_HDR), "optimize_ext": bool(a.optimize_ext), "use_exposure": bool(a.use_exposure),
           "guard_hits": int(vren.lib().ngp_guard_hits()),
           "train_rays_per_s": round(a.steps * a.batch / t_train, 1),
           "test_psnr": round(scores["mean_psnr"], 3), "test_ssim": round(scores["mean_ssim"], 4), "test_views": n}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
