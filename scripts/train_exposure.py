#!/usr/bin/env python3
"""Exposure-conditioned training on the drop-in surface: the reference's loop
under --use_exposure (train.py:76-77, 84-109, 174-200) -- models.rendering.render
with the per-ray exposure, losses.NeRFLoss, the unit-exposure term, and one
FusedAdam over the field's `params` and the tonemappers' `tone_params`, with
update_density_grid every 16 steps -- on NGP(scale, 'None', False,
use_exposure=True).  Data: an HDR-NeRF folder read by datasets.colmap
(--root_dir .../HDR-NeRF/...), or, by default, the analytic scene of
synthetic.py as a multi-exposure set: radiance = 4 x its colour, imaged through
a fixed smooth response curve at exposures {1/4, 1, 4}, with {1/2, 2} held out.
Prints one JSON line with the test PSNR per held-out exposure.  Usage:
  python scripts/train_exposure.py --steps 1000
  python scripts/train_exposure.py --root_dir data/HDR-NeRF/syndata/sponza --downsample 0.5 --steps 5000
"""
import argparse
import json
import math
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ar-nerf_amd")]

import torch  # noqa: E402

TRAIN_EXPOSURES, TEST_EXPOSURES = (0.25, 1.0, 4.0), (0.5, 2.0)
RADIANCE_SCALE = 4.0


def response(v):
    """The synthetic camera's response curve, radiance x exposure -> [0, 1): s / (1 + s), s = e^0.4 v^1.1
    (a logistic curve in log exposure, like a film's characteristic curve)."""
    s = math.exp(0.4) * v.clamp(min=0) ** 1.1
    return s / (1 + s)


def synthetic_data(res=64, n_train=12, n_test=2, seed=0, device="cuda"):
    """The analytic scene as multi-exposure data: rays (N, h*w, 4) = the LDR colour at the image's exposure and
    the exposure, one image per (pose, exposure); the background stays white (what render() composites
    behind a synthetic scene)."""
    import synthetic as S
    sc = S.AnalyticScene(W=res, H=res, n_images=n_train + n_test, seed=seed)
    col = sc.gt_images(device=device).float() / 255  # (n, hw, 3)
    miss = (col == 1).all(-1, keepdim=True)

    def images(views, exposures):
        rays = []
        for v in views:
            for e in exposures:
                ldr = torch.where(miss[v], torch.ones_like(col[v]), response(RADIANCE_SCALE * col[v] * e))
                rays.append(torch.cat([ldr, torch.full_like(ldr[:, :1], e)], 1))
        return torch.stack(rays), sc.poses[list(views)].repeat_interleave(len(exposures), 0).to(device)

    train_rays, train_poses = images(range(n_train), TRAIN_EXPOSURES)
    test_rays, test_poses = images(range(n_train, n_train + n_test), TEST_EXPOSURES)
    return SimpleNamespace(K=sc.K, img_wh=(res, res), directions=sc.directions.to(device), scale=sc.scale,
                           train_rays=train_rays, train_poses=train_poses, test_rays=test_rays, test_poses=test_poses,
                           unit_exposure_rgb=float(response(torch.tensor(1.0))), erode=False)


def hdr_nerf_data(root_dir, downsample, scale, device="cuda"):
    from datasets import dataset_dict
    train = dataset_dict['colmap'](root_dir, split='train', downsample=downsample)
    test = dataset_dict['colmap'](root_dir, split='test', downsample=downsample)
    return SimpleNamespace(K=train.K, img_wh=train.img_wh, directions=train.directions.to(device), scale=scale,
                           train_rays=train.rays.to(device), train_poses=train.poses.to(device),
                           test_rays=test.rays.to(device), test_poses=test.poses.to(device),
                           unit_exposure_rgb=train.unit_exposure_rgb, erode=True)


def torch_tonemap(log_rad, exposure, tone_params):
    """DESIGN.md §18 in torch ops (fp32 on the fp16-rounded weights, the rounding passed straight through):
    the restatement the kernel path is trained against (use_torch_tonemapper)."""
    w = tone_params + (tone_params.detach().half().float() - tone_params.detach())
    w = w.view(3, 2048)
    A, B0 = w[:, :1024].view(3, 64, 16), w[:, 1024:1024 + 64]
    u = log_rad if exposure is None else log_rad + torch.log(exposure.reshape(-1, 1).float())
    a = u[:, :, None] * A[None, :, :, 0] + A[:, :, 1:].sum(-1)[None]
    return torch.sigmoid((torch.relu(a) * B0[None]).sum(-1))


def use_torch_tonemapper(model):
    """Replace the model's tonemap kernels by torch_tonemap on the same parameters."""
    model.log_radiance_to_rgb = lambda log_rad, **kw: torch_tonemap(log_rad, kw.get('exposure', None), model.tone_params)
    return model


class ExposureLoop:
    """bench.DropinLoop from scratch with the reference's use_exposure branch.  zero_exposure: every ray is
    rendered at exposure 1 (log exposure 0) in training and testing -- the model without its conditioning."""

    def __init__(self, data, batch=1024, lr=1e-2, seed=4, torch_ops=False, zero_exposure=False):
        from datasets.ray_utils import get_rays
        from losses import NeRFLoss
        from models.networks import NGP
        from models.rendering import render
        from optimizers import FusedAdam
        dev = data.directions.device
        self.get_rays, self.render, self.data, self.batch = get_rays, render, data, batch
        m = NGP(data.scale, 'None', False, seed=seed, use_exposure=True).to(dev)
        G = m.grid_size
        m.register_buffer('density_grid', torch.zeros(m.cascades, G ** 3, device=dev))  # train.py:78-82
        ax = torch.arange(G, dtype=torch.int32, device=dev)
        m.register_buffer('grid_coords', torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3))
        m.mark_invisible_cells(data.K.to(dev), data.train_poses, data.img_wh)
        self.model = use_torch_tonemapper(m) if torch_ops else m
        self.opt = FusedAdam([m.params, m.tone_params], lr, eps=1e-15)
        self.loss = NeRFLoss(30, "raw", data.scale, 0.0, lambda_distortion=0.0)
        self.kw = {"exp_step_factor": 1 / 256} if data.scale > 0.5 else {}
        self.zero_exposure = zero_exposure
        self.global_step = 0
        self.gen = torch.Generator(device=dev).manual_seed(seed)

    def _exposure(self, e):
        return torch.ones_like(e) if self.zero_exposure else e

    def step(self):
        m, B, d = self.model, self.batch, self.data
        if self.global_step % 16 == 0:
            m.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=self.global_step < 256, erode=d.erode)
        img = torch.randint(d.train_rays.shape[0], (B,), device=d.directions.device, generator=self.gen)
        pix = torch.randint(d.train_rays.shape[1], (B,), device=d.directions.device, generator=self.gen)
        rays_o, rays_d = self.get_rays(d.directions[pix], d.train_poses[img])
        picked = d.train_rays[img, pix]
        results = self.render(m, rays_o, rays_d, test_time=False, random_bg=False,
                              exposure=self._exposure(picked[:, 3:]), **self.kw)
        loss_d = self.loss(results, {"rgb": picked[:, :3]}, step=self.global_step)
        unit = m.log_radiance_to_rgb(torch.zeros(1, 3, device=picked.device),
                                     exposure=torch.ones(1, 1, device=picked.device))  # train.py:182-187
        loss_d['unit_exposure'] = 0.5 * (unit - d.unit_exposure_rgb) ** 2
        loss = sum(lo.mean() for lo in loss_d.values())
        loss.backward()
        self.opt.step()
        self.opt.zero_grad()
        self.global_step += 1
        return loss, results

    @torch.no_grad()
    def test_psnr(self):
        """{exposure: mean PSNR over the test frames taken at it}"""
        d, out = self.data, {}
        for i in range(d.test_rays.shape[0]):
            e = d.test_rays[i, 0, 3]
            rays_o, rays_d = self.get_rays(d.directions, d.test_poses[i])
            res = self.render(self.model, rays_o, rays_d, test_time=True, exposure=self._exposure(e.reshape(1)), **self.kw)
            # (render(test_time=True) composites on black; the training background -- white without an
            # exp_step_factor, rendering.py:179-185 -- goes behind the rays here)
            rgb = res['rgb'] + (0.0 if self.kw else 1.0) * (1 - res['opacity'])[:, None]
            mse = ((rgb.clamp(0, 1) - d.test_rays[i, :, :3]) ** 2).mean()
            out.setdefault(round(float(e), 6), []).append(float(-10 * torch.log10(mse)))
        return {e: sum(v) / len(v) for e, v in sorted(out.items())}


class FusedLoop:
    """The same data and hyper-parameters through the fused step, NGPTrainer(use_exposure=True,
    unit_exposure_rgb=...): batches drawn on the device, the exposure one value per
    training image (rays[:, 0, 3]), steady-state steps replayed as captured graphs."""

    def __init__(self, data, batch=1024, lr=1e-2, seed=4, **kw):
        from datasets.ray_utils import get_rays
        from trainer import NGPTrainer
        dev = data.directions.device
        self.get_rays, self.data = get_rays, data
        self.gt = data.train_rays[..., :3].contiguous()
        self.table = data.train_rays[:, 0, 3].contiguous()
        assert bool((data.train_rays[..., 3] == self.table[:, None]).all()), "one exposure per training image"
        self.dirs, self.poses = data.directions.contiguous(), data.train_poses.contiguous()
        self.tr = NGPTrainer(scale=data.scale, batch_size=batch, lr=lr, seed=seed, device=dev, erode=data.erode,
                             use_exposure=True, unit_exposure_rgb=data.unit_exposure_rgb, **kw)
        self.tr.mark_invisible_cells(data.K.to(dev), data.train_poses, data.img_wh)

    def step(self, allow_pair=True):
        """-> (the per-ray losses, None): on the device, not waited for; the unit-exposure term's value is
        tr.out_loss_unit"""
        return self.tr.train_step(self.gt, self.dirs, self.poses, allow_pair=allow_pair, exposure=self.table), None

    def last_loss(self):
        return float(self.tr.out_loss.sum() + self.tr.out_loss_unit[0])

    @torch.no_grad()
    def test_psnr(self):
        """{exposure: mean PSNR over the test frames taken at it} (ExposureLoop.test_psnr on NGPTrainer.render)"""
        d, tr, out = self.data, self.tr, {}
        tr.drain()
        for i in range(d.test_rays.shape[0]):
            e = d.test_rays[i, 0, 3]
            rays_o, rays_d = self.get_rays(d.directions, d.test_poses[i])
            res = tr.render(rays_o.contiguous(), rays_d.contiguous(), bg=1.0 if tr.esf == 0 else 0.0, exposure=e.reshape(1))
            mse = ((res['rgb'].clamp(0, 1) - d.test_rays[i, :, :3]) ** 2).mean()
            out.setdefault(round(float(e), 6), []).append(float(-10 * torch.log10(mse)))
        return {e: sum(v) / len(v) for e, v in sorted(out.items())}


def fused_compare(data, a):
    """--fused-compare N: ms/step of the drop-in loop and of the fused step on the same data, alternated
    for N rounds of `--window` steps each (both warmed up past the occupancy warm-up first), and the
    composited samples per step of each, the mean over each window (the work per step moves with the
    model's state)."""
    import time
    loops = {"dropin": ExposureLoop(data, a.batch, a.lr, a.seed), "fused": FusedLoop(data, a.batch, a.lr, a.seed)}
    for lp in loops.values():
        for _ in range(a.steps):
            lp.step()
    tr = loops["fused"].tr
    ms = {k: [] for k in loops}
    samples = {k: [] for k in loops}
    for _ in range(a.fused_compare):
        for name, lp in loops.items():
            torch.cuda.synchronize()
            if name == "fused":
                tr.reset_stats()
            t0 = time.perf_counter()
            vr = []  # (the drop-in loop's per-step counts, device tensors: read after the window)
            for _ in range(a.window):
                _, res = lp.step()
                if res is not None:
                    vr.append(res['vr_samples'])
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.window * 1e3)
            samples[name].append(tr.stat_totals()[1] / a.window if name == "fused"
                                 else sum(float(v) for v in vr) / a.window)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    return {"rounds": a.fused_compare, "window": a.window, "warm_steps": a.steps,
            "ms_per_step_dropin": round(med(ms["dropin"]), 4), "ms_per_step_fused": round(med(ms["fused"]), 4),
            "ms_range_dropin": [round(min(ms["dropin"]), 4), round(max(ms["dropin"]), 4)],
            "ms_range_fused": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
            "dropin_over_fused": round(med(ms["dropin"]) / med(ms["fused"]), 2),
            "composited_per_step_dropin": round(med(samples["dropin"])),
            "composited_per_step_fused": round(med(samples["fused"]))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", default=None, help="an HDR-NeRF scene folder; default: the synthetic multi-exposure scene")
    ap.add_argument("--downsample", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=0.5, help="scene scale of the HDR-NeRF folder")
    ap.add_argument("--res", type=int, default=100, help="synthetic scene: image side")
    ap.add_argument("--images", type=int, default=24, help="synthetic scene: training poses (x 3 exposures)")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--torch-ops", action="store_true", help="the tonemappers restated in torch ops, not the kernels")
    ap.add_argument("--zero-exposure", action="store_true", help="ignore the exposure (the unconditioned model)")
    ap.add_argument("--fused", action="store_true",
                    help="train through the fused step, NGPTrainer(use_exposure=True, unit_exposure_rgb=...)")
    ap.add_argument("--fused-compare", type=int, default=0, metavar="N",
                    help="ms/step of the drop-in loop and of the fused step, alternated for N rounds after --steps "
                         "warm-up steps of each")
    ap.add_argument("--window", type=int, default=50, help="--fused-compare: steps per timed window")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    data = hdr_nerf_data(a.root_dir, a.downsample, a.scale, dev) if a.root_dir else \
        synthetic_data(a.res, a.images, 2, device=dev)
    name = a.root_dir or f"synthetic multi-exposure {a.res}x{a.res}x{a.images}x{len(TRAIN_EXPOSURES)}"
    if a.fused_compare:
        print(json.dumps({"data": name, "batch": a.batch, **fused_compare(data, a)}))
        return
    if a.fused:
        if a.torch_ops or a.zero_exposure:
            raise SystemExit("--fused runs the kernels at the data's exposures: no --torch-ops, no --zero-exposure")
        loop = FusedLoop(data, a.batch, a.lr, a.seed, num_epochs=max(1, a.steps // 1000))
    else:
        loop = ExposureLoop(data, a.batch, a.lr, a.seed, a.torch_ops, a.zero_exposure)
    loss = None
    for _ in range(a.steps):
        loss, _ = loop.step()
    torch.cuda.synchronize()
    psnr = loop.test_psnr()
    if a.fused and loss is not None:
        loss = torch.tensor(loop.last_loss())
    print(json.dumps({"data": name, "loop": "fused" if a.fused else "dropin",
                      "steps": a.steps, "batch": a.batch, "tonemapper": "torch ops" if a.torch_ops else "kernels",
                      "zero_exposure": a.zero_exposure, "last_loss": round(float(loss.detach()), 5) if loss is not None else None,
                      "test_psnr_per_exposure": {str(e): round(v, 2) for e, v in psnr.items()},
                      "test_psnr": round(sum(psnr.values()) / len(psnr), 2)}))


if __name__ == "__main__":
    main()
