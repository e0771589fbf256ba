#!/usr/bin/env python3
"""Device time of the SG fit of one light probe:
  kernel        sg_probe.EnvOptim.eval (ngp_sg_fit: two launches per iteration,
                no (pixels, L, 3) temporaries), launched eagerly
  kernel_graph  the same launches replayed from one captured graph
  torch         sg_probe.sg_fit_torch (the reference's formulation on the GPU:
                autograd over (pixels, L, 3) tensors, torch.optim.Adam)
at the app's shape: a 128 x 128 env map, L = 32 lights, 25 iterations (every
placement of the object) and 450 (the app's decomposition comparison).  The
target is the env map of a synthetic cube map (a sky gradient and a sun); the
lights are EnvOptim's seeded draw.  Every timed call starts from the same
parameters and a zero Adam state (restored outside the timed window).  All
paths are warmed up, then timed in --rounds alternating rounds of --reps
(kernel) / --torch-reps (torch) calls between device events; per path the
median of each round is kept, and the result gives the median over rounds and
their spread (min .. max of the round medians).  The lights of the kernel and
torch paths are compared.  The cube-map lookup (32-resolution cube map to the
128 x 128 map) is timed separately.  Prints one JSON line.
Usage: python scripts/bench_sg_probe.py [--hw 128 128] [--lights 32]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ar-nerf_amd")]

import torch  # noqa: E402


def _round(fn, reps, before=None):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        if before is not None:
            before()
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)


def _summary(meds, n_iter=None):
    out = {"median_us": round(statistics.median(meds), 1), "min_us": round(min(meds), 1),
           "max_us": round(max(meds), 1), "spread": round((max(meds) - min(meds)) / statistics.median(meds), 3)}
    if n_iter:
        out["per_iteration_us"] = round(statistics.median(meds) / n_iter, 2)
    return out


def _cubemap(res, dev):
    import probes
    d = probes.get_cubemap_rays(1, res)[0]
    sky = 0.4 + 0.5 * d[:, 1:2].clamp(0, 1) * torch.tensor([[0.5, 0.7, 1.0]]) + 0.15 * torch.sin(5 * d[:, 0:1] + 3 * d[:, 2:3])
    sun = torch.nn.functional.normalize(torch.tensor([0.5, 0.6, -0.62]), dim=0)
    cm = sky.clamp_min(0) + 60.0 * torch.exp(400.0 * (d @ sun - 1.0))[:, None] * torch.tensor([[1.0, 0.9, 0.7]])
    return cm.contiguous().to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, nargs=2, default=(128, 128))
    ap.add_argument("--lights", type=int, default=32)
    ap.add_argument("--iters", type=int, nargs="+", default=(25, 450))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    import sg_probe
    import vren
    if not torch.cuda.is_available():
        raise SystemExit("bench_sg_probe.py times the GPU: no device found")
    dev = torch.device("cuda", 0)
    H, W = a.hw
    L = a.lights
    cm = _cubemap(32, dev)
    target = sg_probe.cubemap2env_map(cm, 32, H, W).contiguous()
    dirs = sg_probe.env_dirs(H, W, dev)
    opt = sg_probe.EnvOptim(L, generator=torch.Generator().manual_seed(0), device=dev)
    init = opt.lgtSGs.clone()
    res = {"hw": [H, W], "lights": L, "reps": a.reps, "torch_reps": a.torch_reps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}

    def restore():
        opt.lgtSGs.copy_(init)
        opt.exp_avg.zero_()
        opt.exp_avg_sq.zero_()
        opt.step.zero_()

    lookup = lambda: sg_probe.cubemap2env_map(cm, 32, H, W)  # noqa: E731
    for _ in range(a.warmup):
        lookup()
    res["cubemap2env_map"] = _summary([_round(lookup, a.reps) for _ in range(a.rounds)])

    for n_iter in a.iters:
        opt.N_iter = n_iter
        state = {}

        def kernel():
            return opt.eval(target)

        def torch_setup():
            state["p"] = init.clone().requires_grad_(True)

        def torch_path():
            return sg_fit(state["p"], target, dirs, n_iter)[0]
        sg_fit = sg_probe.sg_fit_torch
        for _ in range(a.warmup):
            restore()
            kernel()
            torch_setup()
            torch_path()
        restore()
        graph = torch.cuda.CUDAGraph()
        with vren.graph_capture(graph):
            opt.eval(target)
        restore()
        graph.replay()
        torch.cuda.synchronize()
        replayed = opt.lgtSGs.clone()
        restore()
        k_out = kernel().clone()
        torch_setup()
        t_out = torch_path()
        k_meds, g_meds, t_meds = [], [], []
        for _ in range(a.rounds):
            k_meds.append(_round(kernel, a.reps, restore))
            g_meds.append(_round(graph.replay, a.reps, restore))
            t_meds.append(_round(torch_path, a.torch_reps, torch_setup))
        k, g, t = _summary(k_meds, n_iter), _summary(g_meds, n_iter), _summary(t_meds, n_iter)
        res[f"fit_{n_iter}"] = {"kernel": k, "kernel_graph": g, "torch": t,
                                "torch_over_kernel": round(t["median_us"] / k["median_us"], 2),
                                "torch_over_kernel_graph": round(t["median_us"] / g["median_us"], 2),
                                "graph_equals_eager": bool(torch.equal(replayed, k_out)),
                                "final_loss_kernel": float(opt.losses[-1]),
                                "max_abs_diff_kernel_vs_torch": float((k_out - t_out).abs().max())}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
