#!/usr/bin/env python3
"""Camera pose refinement on the drop-in surface: the reference's training
loop with --optimize_ext (train.py:84-108, 132-152, 158-200) -- PoseRefiner's
rays, models.rendering.render, losses.NeRFLoss, and the two FusedAdams (the
net's at the trainer's lr, dR / dT's at the reference's hard-coded 1e-6) -- on
the analytic scene, starting from an NGPTrainer state the way bench.DropinLoop
does.  The cameras are perturbed (--perturb-deg / --perturb-t) so that there is
something to refine; the refined poses are written with --out.  Usage:
  python scripts/refine_poses.py --steps 200 --out refined_poses.pt
  python scripts/refine_poses.py --compare 30      # ms/step with / without refinement, alternated
  python scripts/refine_poses.py --fused 30        # the same scene through NGPTrainer(optimize_ext=True):
                                                   # ms/step of this loop and of the fused step with and without
                                                   # refinement (alternated, all warmed), pose error before / after
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ar-nerf_amd")]

import torch  # noqa: E402


class RefineLoop:
    """bench.DropinLoop with the reference's optimize_ext branch: rays from PoseRefiner (refine=True) or
    straight from the poses; both share the model, its optimizer and the batch draw."""

    def __init__(self, trainer, gt_images, directions, poses, batch, pose_lr=1e-6, seed=7):
        from datasets.ray_utils import get_rays
        from losses import NeRFLoss
        from models.networks import NGP
        from models.rendering import render
        from optimizers import FusedAdam
        from pose_refine import PoseRefiner
        dev = trainer.dev
        self.get_rays, self.render = get_rays, render
        m = NGP(trainer.scale).to(dev)
        with torch.no_grad():
            m.params.copy_(trainer.params)
        m.density_bitfield.copy_(trainer.density_bitfield)
        m.register_buffer("density_grid", trainer.density_grid.clone())  # train.py:78-80
        m.register_buffer("grid_coords", trainer.grid_coords.clone())
        self.model = m
        self.opt = FusedAdam([m.params], trainer.lr(), eps=1e-15)
        st = self.opt.state[m.params]
        st["step"] = int(trainer.dctr[0].item())
        st["exp_avg"], st["exp_avg_sq"] = trainer.exp_avg.clone(), trainer.exp_avg_sq.clone()
        self.refiner = PoseRefiner(poses.shape[0], device=dev)
        self.pose_opt = self.refiner.optimizer(pose_lr)
        self.loss = NeRFLoss(30, "raw", trainer.scale, 0.0, lambda_distortion=0.0)
        self.gt, self.directions, self.poses, self.batch = gt_images, directions, poses, batch
        self.global_step = trainer.global_step
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        self.kw = {"exp_step_factor": 1 / 256} if trainer.scale > 0.5 else {}

    def step(self, refine=True):
        m, B = self.model, self.batch
        if self.global_step % 16 == 0:
            m.update_density_grid(0.01 * 1024 / 3 ** 0.5, warmup=False)
        img = torch.randint(self.gt.shape[0], (B,), device=self.gt.device, generator=self.gen)
        pix = torch.randint(self.gt.shape[1], (B,), device=self.gt.device, generator=self.gen)
        if refine:
            rays_o, rays_d = self.refiner.rays(img, pix, self.directions, self.poses)
        else:
            rays_o, rays_d = self.get_rays(self.directions[pix], self.poses[img])
        results = self.render(m, rays_o, rays_d, test_time=False, random_bg=False, **self.kw)
        rgb = self.gt[img, pix].float() / 255
        loss = sum(lo.mean() for lo in self.loss(results, {"rgb": rgb}, step=self.global_step).values())
        loss.backward()
        self.opt.step()
        self.opt.zero_grad()
        if refine:
            self.pose_opt.step()
            self.pose_opt.zero_grad()
        self.global_step += 1
        return loss, results


def pose_error(a, b):
    """mean rotation angle (deg) and mean translation distance between two (n,3,4) pose sets"""
    Rr = a[:, :, :3] @ b[:, :, :3].transpose(1, 2)
    cos = ((Rr.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2).clamp(-1, 1)
    return float(torch.rad2deg(torch.acos(cos)).mean()), float((a[:, :, 3] - b[:, :, 3]).norm(dim=1).mean())


def fused_compare(a, tr, loop, gt, dirs, poses, true_poses):
    """--fused: two more trainers from tr's state (parameters, Adam moments, occupancy grid, step counters), one
    refining the poses inside the step; rounds of [drop-in loop with refinement, fused + refinement, fused] on
    one device, each step timed between synchronisations, then 64-step windows back to back; the pose kernels'
    times inside the step; a fresh refining trainer's pose error over --steps steps."""
    from ktimer import KernelTimer
    from trainer import NGPTrainer

    def clone(**kw):
        t = NGPTrainer(scale=tr.scale, batch_size=a.batch, device=tr.dev, **kw)
        t.load_params(tr.params, tr.params16)
        t.exp_avg.copy_(tr.exp_avg)
        t.exp_avg_sq.copy_(tr.exp_avg_sq)
        t.density_grid.copy_(tr.density_grid)
        t.density_bitfield.copy_(tr.density_bitfield)
        t.dctr.copy_(tr.dctr)
        t.global_step = tr.global_step
        return t

    fused, plain = clone(optimize_ext=True, pose_lr=a.pose_lr), clone()
    for _ in range(40):  # warm: the plain trainer's graph variants (with and without the occupancy update) captured
        loop.step(True)
        fused.train_step(gt, dirs, poses)
        plain.train_step(gt, dirs, poses, allow_pair=False)
    ms = {"dropin_refine": [], "fused_refine": [], "fused_plain": []}
    runs = {"dropin_refine": lambda: loop.step(True), "fused_refine": lambda: fused.train_step(gt, dirs, poses),
            "fused_plain": lambda: plain.train_step(gt, dirs, poses, allow_pair=False)}
    for _ in range(a.fused):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {f"ms_per_step_{k}": round(statistics.median(v), 3) for k, v in ms.items()}
    res["rounds"] = a.fused
    res["dropin_over_fused_refine"] = round(res["ms_per_step_dropin_refine"] / res["ms_per_step_fused_refine"], 2)
    # training throughput: windows of 64 steps back to back (4 occupancy updates each), one synchronisation per
    # window, the three paths alternated
    bb = {k: [] for k in runs}
    for _ in range(5):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(64):
                fn()
            torch.cuda.synchronize()
            bb[k].append((time.perf_counter() - t0) * 1e3 / 64)
    for k, v in bb.items():
        res[f"ms_per_step_back_to_back_{k}"] = round(statistics.median(v), 3)
    res["back_to_back_dropin_over_fused_refine"] = round(
        res["ms_per_step_back_to_back_dropin_refine"] / res["ms_per_step_back_to_back_fused_refine"], 2)
    # the pose kernels inside the (eager) refining step: stamp kernels around their launches
    names = ["input_grad", "ray_segment_sum", "pose_compose", "pose_grad"]
    timer = KernelTimer(fused.dctr, rows=64, names=names, device=tr.dev)
    timer.arm()
    for _ in range(32):
        fused.train_step(gt, dirs, poses)
    torch.cuda.synchronize()
    timer.disarm()
    for k, v in timer.read().items():
        res[f"{k}_us"] = round(statistics.median(v) * 1e3, 2)
    # convergence from the perturbed cameras: a fresh refining trainer, exactly --steps steps
    conv = clone(optimize_ext=True, pose_lr=a.pose_lr)
    e0 = pose_error(poses, true_poses)
    for _ in range(a.steps):
        conv.train_step(gt, dirs, poses)
    torch.cuda.synchronize()
    e1 = pose_error(conv.refined_poses(poses), true_poses)
    res.update(steps=a.steps, rot_err_deg=[round(e0[0], 5), round(e1[0], 5)],
               trans_err=[round(e0[1], 6), round(e1[1], 6)],
               dR_abs_max=float(conv.pose_refiner.dR.detach().abs().max()),
               dT_abs_max=float(conv.pose_refiner.dT.detach().abs().max()))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=100)
    ap.add_argument("--images", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pretrain", type=int, default=500, help="NGPTrainer steps on the true poses before the loop")
    ap.add_argument("--steps", type=int, default=200, help="refining steps")
    ap.add_argument("--pose-lr", type=float, default=1e-6, help="the reference hard-codes 1e-6 (train.py:149)")
    ap.add_argument("--perturb-deg", type=float, default=0.5)
    ap.add_argument("--perturb-t", type=float, default=0.005)
    ap.add_argument("--compare", type=int, default=0, metavar="N",
                    help="instead: N warmed step pairs, with and without refinement alternated -> median ms/step each")
    ap.add_argument("--ktimer", action="store_true", help="with --compare: the two new kernels' time per launch")
    ap.add_argument("--fused", type=int, default=0, metavar="N",
                    help="instead: the perturbed scene through NGPTrainer(optimize_ext=True); N alternated rounds of "
                         "the drop-in loop with refinement, the fused step with it and the fused step without -> "
                         "median ms/step each, the pose kernels' time inside the step, and the pose error before "
                         "and after --steps fused steps")
    ap.add_argument("--out", default=None, help="write {'poses', 'dR', 'dT'} here (torch.save)")
    a = ap.parse_args(argv)
    import synthetic as S
    from datasets.ray_utils import axisangle_to_R
    from trainer import NGPTrainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sc = S.AnalyticScene(W=a.res, H=a.res, n_images=a.images)
    gt = sc.gt_images(device=dev)
    dirs, true_poses = sc.directions.to(dev).contiguous(), sc.poses.to(dev).contiguous()
    tr = NGPTrainer(scale=sc.scale, batch_size=a.batch, device=dev)
    for i in range(a.pretrain):
        tr.train_step(gt, dirs, true_poses, allow_pair=i < a.pretrain - 1)
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(11)
    w = torch.nn.functional.normalize(torch.randn(a.images, 3, generator=g), dim=1) * torch.deg2rad(
        torch.tensor(a.perturb_deg))
    poses = torch.cat([axisangle_to_R(w).to(dev) @ true_poses[:, :, :3],
                       (true_poses[:, :, 3] + torch.randn(a.images, 3, generator=g).to(dev) * a.perturb_t)[..., None]], -1)
    loop = RefineLoop(tr, gt, dirs, poses.contiguous(), a.batch, pose_lr=a.pose_lr)
    out = {"scene": f"analytic {a.res}x{a.res}x{a.images}", "batch": a.batch, "pretrain": a.pretrain,
           "pose_lr": a.pose_lr}
    if a.fused:
        out.update(fused_compare(a, tr, loop, gt, dirs, poses.contiguous(), true_poses))
    elif a.compare:
        for _ in range(5):
            loop.step(True)
            loop.step(False)
        timer = None
        if a.ktimer:
            from ktimer import KernelTimer
            ctr = torch.zeros(1, dtype=torch.int64, device=dev)
            timer = KernelTimer(ctr, rows=a.compare + 1, names=["input_grad", "ray_segment_sum"], device=dev)
            timer.arm()
        ms = {True: [], False: []}
        rows = []
        for _ in range(a.compare):
            for refine in (True, False):
                hook = None
                if refine and timer is not None:  # rows with a nonzero dL/dxyzs: the gradient-carrying samples
                    def pre(mod, args):
                        if args[0].requires_grad:
                            args[0].register_hook(lambda gr: rows.append((gr != 0).any(1).sum()))
                    hook = loop.model.register_forward_pre_hook(pre)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loop.step(refine)
                torch.cuda.synchronize()
                ms[refine].append((time.perf_counter() - t0) * 1e3)
                if hook is not None:
                    hook.remove()
                    ctr += 1
        out["ms_per_step_refine"] = round(statistics.median(ms[True]), 3)
        out["ms_per_step_plain"] = round(statistics.median(ms[False]), 3)
        out["pairs"] = a.compare
        if timer is not None:
            timer.disarm()
            n_rows = float(torch.stack(rows).double().mean())
            out["gradient_rows_per_step"] = round(n_rows)
            for k, v in timer.read().items():
                out[f"{k}_us"] = round(statistics.median(v) * 1e3, 2)
                out[f"{k}_ns_per_row"] = round(statistics.median(v) * 1e6 / max(n_rows, 1), 3)
    else:
        e0 = pose_error(poses, true_poses)
        loss = None
        for _ in range(a.steps):
            loss, _ = loop.step(True)
        torch.cuda.synchronize()
        refined = loop.refiner.refined_poses(poses)
        e1 = pose_error(refined, true_poses)
        out.update(steps=a.steps, last_loss=round(float(loss.detach()), 5) if loss is not None else None,
                   rot_err_deg=[round(e0[0], 5), round(e1[0], 5)], trans_err=[round(e0[1], 6), round(e1[1], 6)],
                   dR_abs_max=float(loop.refiner.dR.detach().abs().max()),
                   dT_abs_max=float(loop.refiner.dT.detach().abs().max()))
        if a.out:
            torch.save({"poses": refined.cpu(), **{k: v.cpu() for k, v in loop.refiner.state_dict_reference().items()}},
                       a.out)
            out["out"] = a.out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
