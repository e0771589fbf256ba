"""The reference's training step (train.py NeRFSystem, Lightning + apex +
tcnn + vren) as a chain of libngp_amd.so kernels on one MI355X per process.

One step (train.py:174-200), all on the current HIP stream, no host sync:
  raygen_aabb (ray_utils.get_rays + RayAABBIntersector + near clamp)
  -> march_train_count / scan / write (RayMarcher; sample count stays on device)
  -> field_forward (hash grid + density MLP + SH + colour MLP)
  -> composite_loss (VolumeRenderer fw + bg blend + NeRFLoss + VolumeRenderer bw)
  -> field_backward (MLP backward + hash scatter)
  -> [all_reduce(grad) over RCCL when world_size > 1]  (DDP, train.py:288)
  -> adam_step (FusedAdam + fp16 shadow + grad zeroing)
and every `update_interval` steps the occupancy update
(models/networks.py:252-281) before the batch (train.py:175-178).

Per-sample buffers are allocated once at capacity n_rays * max_samples; the
kernels read the live sample count from device memory.

optimize_ext (train.py:92-95, 132-137, 148-149; off by default): the poses are
composed with the per-image dR / dT on the device before the batch is drawn
(pose_compose), and after the MLP backward the field's input gradients, their
per-ray sums, the per-image chain rule (pose_grad) and a second Adam step the
corrections -- step N's rays use ext_N, step N + 1's ext_{N+1}, so no batch is
marched ahead of the pose Adam and its steps run eagerly: use_graphs has no
effect under it (_pose_state, _pose_backward, _step).

use_exposure (train.py:76-77, 106-107, 182-187 under --use_exposure; off by
default): the field gives log radiance (`rgbs`), the three
tonemapper nets turn it and each sample's exposure into the composited colour
(`ldr`) right after every field launch, over exactly the samples it evaluated;
after the compositing their backward turns dL/dldr into dL/dlog-radiance in
place over the gradient-carrying samples and adds into `tone_grad`, the
unit-exposure term follows, and one more Adam launch steps `tone_params`.  The
exposure comes per training image (train_step) or per ray (step) and is spread
to the samples when the batch is marched (_expose).
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.distributed as dist

import ddp
import hashgrid as HG
import vren
from capi import C

MAX_SAMPLES = 1024  # models/rendering.py:9
NEAR_DISTANCE = 0.01  # models/rendering.py:10
LOSS_TYPES = {"raw": 0, "mse": 1, "log": 2, "tanh": 3}


_p = HG._ptr  # (diagnostics import it; the trainer passes tensors)


STAT_STRIPES, STAT_STRIDE = C["NGP_STAT_STRIPES"], C["NGP_STAT_STRIDE"]
THROTTLE_EVERY, THROTTLE_DEPTH = 32, 4  # host run-ahead bound: <= 160 steps enqueued
COARSE_REP, COARSE_REP_LEVELS = 8, 4  # gradient replicas of the coarsest atomic levels


def rng_keys(seed):
    """The trainer's three Philox keys (64 bits each) from its seed:
    (sample_seed: the batch draw, ngp_sample_batch; its random-background key,
    ngp_random_bg; occ_seed: the occupancy draws, ngp_occupancy_samples*).
    Pairwise different for every seed: they differ by the xor constants."""
    base = (1000003 * (seed + 1)) & 0xFFFFFFFFFFFFFFFF
    return base, base ^ 0x6267, (base ^ 0x5DEECE66D) & 0xFFFFFFFFFFFFFFFF


class NGPTrainer:
    def __init__(self, scale=0.5, batch_size=8192, lr=1e-2, num_epochs=30, steps_per_epoch=1000, loss="raw",
                 lambda_opacity=1e-3, lambda_depth=0.0, random_bg=False, exp_step_factor=None, grid_size=128,
                 update_interval=16, warmup_steps=256, max_samples=MAX_SAMPLES, sample_capacity=None, seed=4,
                 device="cuda", process_group=None, hash_backward="hybrid", bin_samples_per_ray=None, bin_level_lo=None,
                 chunk_first=64, erode=False, lambda_distortion=0.0, bin_merge_hi=None, fused_adam=True, use_graphs=True,
                 pair_steps=False, emulate_dp=False, dp_fine_buckets=2, use_raw_HDR=False, optimize_ext=False,
                 pose_lr=1e-6, use_exposure=False, unit_exposure_rgb=None):
        self.dev = torch.device(device)
        # raw-HDR model (train.py:76-77: NGP(rgb_act='None', use_raw_HDR=True) under --use_EXR): no
        # colour activation but leaky_relu in training, relu for output_radiance
        # (networks.py:152-157); fp32 ground truth may exceed 1
        self.use_raw_HDR = bool(use_raw_HDR)
        self.rgb_act = HG.RGB_LEAKY_RELU if self.use_raw_HDR else HG.RGB_SIGMOID
        # exposure-conditioned model (train.py:76-77 under --use_exposure: NGP(rgb_act='None',
        # use_raw_HDR=False)): the colour net gives log radiance, the three tonemapper nets turn log
        # radiance + log exposure into the LDR colour that is composited;
        # unit_exposure_rgb: the target of the unit-exposure term (train.py:182-187), None: no such term
        self.use_exposure = bool(use_exposure)
        self.unit_exposure_rgb = None if unit_exposure_rgb is None else float(unit_exposure_rgb)
        self.tone_params = None
        if self.use_exposure:
            if self.use_raw_HDR:
                raise ValueError("use_exposure=True is the reference's NGP(scale, rgb_act='None', use_raw_HDR=False): "
                                 "it has no raw-HDR variant (the tonemappers' output is an LDR colour)")
            self.rgb_act = HG.RGB_NONE
        self.scale = float(scale)
        self.batch_size = batch_size
        self.lr0, self.num_epochs, self.steps_per_epoch = lr, num_epochs, steps_per_epoch
        self.loss_type = LOSS_TYPES[loss]
        self.lambda_opacity, self.lambda_depth = lambda_opacity, lambda_depth
        self.lambda_distortion = float(lambda_distortion)  # losses.py:77-80 (opt.py:25 default 0)
        self.random_bg = random_bg
        # train.py:104-105
        self.esf = exp_step_factor if exp_step_factor is not None else (1 / 256 if scale > 0.5 else 0.0)
        self.G = grid_size
        # erode (networks.py:270-272): per-cell decay from mark_invisible_cells'
        # count_grid; train.py:178 turns it on for COLMAP scenes
        self.erode = bool(erode)
        self.count_grid = None
        self.decay_cells = None
        self._decay_for = None
        self.cascades = max(1 + int(np.ceil(np.log2(2 * scale))), 1)  # models/networks.py:27
        self.update_interval, self.warmup_steps, self.max_samples = update_interval, warmup_steps, max_samples
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if self.world > 1 else 0
        # the data-parallel (ZeRO-1, graph-segmented) step; emulate_dp = N runs it in one process
        # with the shards of a world of N (this process = rank 0) and the collectives replaced by
        # local copies of its shard -- one rank's compute at world N without the xGMI transfers
        # (bench --emulate-dp N; only shard 0 of each bucket is stepped, so N > 1 is for timing)
        self.dp = self.world > 1 or bool(emulate_dp)
        self.dp_world = self.world if self.world > 1 else max(1, int(emulate_dp))
        # camera pose refinement inside the step (train.py:92-95, 132-137, 148-149; _pose_state)
        self.optimize_ext = bool(optimize_ext)
        self.pose_lr = float(pose_lr)  # constant: the reference's cosine schedule is the net optimizer's alone
        self.pose_refiner = None
        self._ps = None
        if self.optimize_ext and self.dp:
            raise NotImplementedError("NGPTrainer(optimize_ext=True) runs the single-process step only: the pose "
                                      "gradient is not reduced across ranks (no process group of more than one "
                                      "rank, no emulate_dp)")
        if self.use_exposure and self.optimize_ext:
            raise NotImplementedError("NGPTrainer(use_exposure=True, optimize_ext=True): the pose gradient does not "
                                      "pass through the tonemappers yet (the field's input gradients would need "
                                      "dL/dlog-radiance kept beside the pose chain)")
        if self.use_exposure and self.dp:
            raise NotImplementedError("NGPTrainer(use_exposure=True) runs the single-process step only: the "
                                      "tonemappers' gradient has no ZeRO-1 bucket and is not reduced across ranks "
                                      "(no process group of more than one rank, no emulate_dp)")
        dev = self.dev
        # ---- field parameters: fp32 master, fp16 shadow, Adam state, grad
        self.grid = HG.HashGrid(scale)
        init = HG.init_params(self.grid, seed=seed, device=dev)
        self.n_params = n = init.numel()
        # hash backward: "atomic": per-sample fp32 atomics (ngp_hash_backward); "binned": all
        # levels through the counting-sort path; "hybrid" (default): coarse levels
        # [0, bin_level_lo) atomic -- their in-wave run merge keeps the requests few --
        # fine levels binned (DESIGN.md "hash backward").  Defaults by scene size (measured,
        # DESIGN.md §9): one cascade (object scenes, ~70 samples/ray) 8 atomic levels + 128
        # binned samples/ray; cascaded (unbounded) scenes have ~2x the gradient-carrying
        # samples and 4 more hashed levels: all levels binned (+17 % at scale 16) with room
        # for 512 samples/ray.  Resolved before the ZeRO-1 buckets, which split at it.
        assert hash_backward in ("atomic", "binned", "hybrid")
        big = self.cascades > 1
        if bin_level_lo is None:
            bin_level_lo = 0 if big else 8
        if bin_samples_per_ray is None:
            bin_samples_per_ray = 512 if big else 128
        self.hash_backward = hash_backward
        self.bin_level_lo = 0 if hash_backward == "binned" else min(max(int(bin_level_lo), 0), self.grid.n_levels)
        # ZeRO-1 layout (ddp.zero_buckets): buffers padded to n_pad; bucket 0 =
        # [MLP | coarse levels], then the binned levels in dp_fine_buckets level
        # ranges (bin_cuts: [lo, c_1), [c_1, c_2), ...), each split where its
        # gradient is complete -- the world > 1 step accumulates the ranges in
        # turn and reduce-scatters / steps / all-gathers each range's bucket
        # on the comm stream while the next range accumulates, so only the
        # last range's chain is exposed after the backward; rank r owns shard
        # r of each bucket.  All levels binned (bin_level_lo 0): bucket 0 is
        # the MLP alone.
        self.bin_cuts = ddp.level_cuts(self.bin_level_lo, self.grid.n_levels, dp_fine_buckets)
        splits = [HG.MLP_PARAMS + 2 * int(self.grid.offsets[lv]) for lv in self.bin_cuts[:-1]] or \
            [HG.MLP_PARAMS + 2 * int(self.grid.offsets[self.grid.n_levels])]
        self.n_pad, self.buckets = ddp.zero_buckets(n, splits, self.dp_world)
        pb = torch.zeros(self.n_pad, device=dev)
        pb[:n] = init
        self._pbuf = pb
        self.params = pb[:n]  # fp32 master (a rank updates its shards only when world > 1)
        self._p16buf = pb.half()
        self.params16 = self._p16buf[:n]
        self._gbuf = torch.zeros(self.n_pad, device=dev)
        self.grad = self._gbuf[:n]
        self.exp_avg = torch.zeros(self.n_pad, device=dev)
        self.exp_avg_sq = torch.zeros(self.n_pad, device=dev)
        self.shards = [(a + (b - a) * self.rank // self.dp_world, a + (b - a) * (self.rank + 1) // self.dp_world)
                       for a, b in self.buckets]
        self._gshard = [torch.zeros(hi - lo, device=dev) for lo, hi in self.shards] if self.dp else None
        self._bk = None  # (_bucket_host)
        self.global_step = 0
        # ---- occupancy (models/networks.py:20-30, train.py:78-82)
        self.center = torch.zeros(1, 3, device=dev)
        self.half_size = torch.ones(1, 3, device=dev) * scale
        self.density_grid = torch.zeros(self.cascades, self.G ** 3, device=dev)
        self.density_bitfield = torch.zeros(self.cascades * self.G ** 3 // 8, dtype=torch.uint8, device=dev)
        ax = torch.arange(self.G, dtype=torch.int32, device=dev)
        self.grid_coords = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).contiguous()
        self.all_indices = vren.morton3D(self.grid_coords).long()
        self._sum_cnt = torch.zeros(2, dtype=torch.float64, device=dev)
        # device-side occupancy sampling buffers (update_density_grid)
        M2 = 2 * (self.G ** 3 // 4)
        # density_grid_tmp as 64-bit (list position, sigma) keys: last writer wins (ngp_density_scatter_last)
        self._occ_key = torch.zeros(self.density_grid.shape, dtype=torch.int64, device=dev)
        self._occ_list = torch.empty(self.G ** 3, dtype=torch.int32, device=dev)
        self._occ_count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.L = K = vren.kernels()  # the checked view: tensors and numbers as they are, a failed status raises
        self._occ_list_ws = torch.empty((K.ngp_occupied_cells_workspace(self.G ** 3) + 3) // 4, dtype=torch.int32,
                                        device=dev)
        self._occ_xyz = torch.empty(M2, 3, device=dev)
        self._occ_flat = torch.empty(M2, dtype=torch.int64, device=dev)
        self._occ_sig = torch.empty(M2, device=dev)
        # only the samples whose sigma the update keeps are evaluated (ngp_occupancy_keep:
        # a cell's last draw; bit-identical grid, 362 -> 302 us per update; occ_keep = False
        # (tests): all 2M, as the reference evaluates them)
        self.occ_keep = True
        self._occ_mark = torch.empty((self.G ** 3 + 15) // 16, 4, dtype=torch.int32, device=dev)
        self._occ_kept = torch.empty(M2, dtype=torch.int32, device=dev)
        self._occ_kept_n = torch.zeros(1, dtype=torch.int64, device=dev)
        self._occ_ws = torch.empty((K.ngp_occupancy_sorted_workspace(M2 // 2) + 7) // 8, dtype=torch.float64,
                                   device=dev)
        self.threshold = torch.zeros(2, device=dev)
        # ---- per-step buffers
        R = batch_size
        if sample_capacity is not None:  # never let a ray overflow the sample buffers
            self.max_samples = max_samples = max(1, min(max_samples, sample_capacity // R))
        cap = R * max_samples
        self.cap = cap
        f = dict(device=dev, dtype=torch.float32)
        # Two sets of ray / march buffers: the next batch is marched on a side
        # stream while the current batch's field, loss, backward and Adam run.
        self.msets = [self._march_buffers(R, cap, f, self.density_bitfield.numel()) for _ in range(2)]
        if self.use_exposure:
            self._tone_buffers(seed, R, cap, f)
        self.cur = 0
        self.march_stream = torch.cuda.Stream(device=dev)
        self._pending = None  # (set index, event) of a batch marched ahead
        self.n_prefetched = 0
        self.no_prefetch = False  # (diagnostics) march every batch inline
        # pair_steps: two consecutive steady-state steps per graph replay (_replay_pair)
        # (not under optimize_ext: the second step's rays depend on the first step's pose update)
        self.pair_steps = bool(pair_steps) and not self.optimize_ext
        self._ran_ahead = False
        self._pair_key = None
        self._bind(self.msets[0])
        self.sigmas, self.rgbs = torch.zeros(cap, **f), torch.zeros(cap, 3, **f)  # (finite where never evaluated)
        # saved encoding: pair-major (8, cap, 4) for the split forward, else row-major (cap, 32)
        # hybrid hash backward: the atomic coarse levels run on their own
        # stream beside the binned fine levels (disjoint gradient ranges;
        # memory-side atomics vs LDS-bound passes overlap)
        # (Single process) the Adam of the MLP + coarse levels runs on that side stream
        # right after the coarse levels' backward, beside the binned levels'
        # accumulation, whose own FusedAdam is fused into it (+5 %,
        # profiles/r02/ab/fused_adam.txt; bit-identical to one FusedAdam launch after the
        # backward, which fused_adam=False restores).
        # (its own stream: sharing the march's side stream -- their work never overlaps in time --
        # measured 6 % slower, the graph's branches then map onto fewer hardware queues)
        self.bwd_stream = torch.cuda.Stream(device=dev)
        self.fused_adam = bool(fused_adam)
        self._adam_hi = None
        # the training forward: encode + MLPs in one launch (ngp_field_encode_mlp), the
        # pair-major encoding kept for the backward (+1.8 %, profiles/r02/ab/fused_field.txt)
        self.enc = torch.empty(8 * cap * 4, dtype=torch.float16, device=dev)
        self.dsig, self.drgb = torch.empty(cap, **f), torch.empty(cap, 3, **f)
        self.denc = torch.empty(cap, 32, **f)
        self.out_rgb, self.out_op = torch.empty(R, 3, **f), torch.empty(R, **f)
        self.out_depth, self.out_loss = torch.empty(R, **f), torch.empty(R, **f)
        # running totals: [0] marched, [1] composited (vr_samples), [2] gradient-carrying,
        # [3] field-evaluated samples
        # striped counters (ngp_composite_loss: NGP_STAT_STRIPES x NGP_STAT_STRIDE), written by the
        # compositing kernel only; field-evaluated samples in their own 128-B line (eval_stats[0],
        # main stream only: the list launches of the step that evaluates them add both rounds'
        # totals, device-scope atomics) -- no counter word shares a cache line with a writer on
        # another stream
        self.stats = torch.zeros(STAT_STRIPES * STAT_STRIDE, dtype=torch.int64, device=dev)
        self.eval_stats = torch.zeros(STAT_STRIDE, dtype=torch.int64, device=dev)
        # chunked field evaluation (ngp_chunk_counts): first `chunk_first` samples of
        # every row, then the rest of the rows not yet terminated (0 = every sample).
        # (More rounds evaluate 22 % fewer samples, but each extra encode launch costs
        # more than it saves: profiles/r02/ab/chunk_rounds.txt)
        self.chunk_first = int(chunk_first)
        self.eval_counts = torch.empty(R, dtype=torch.int32, device=dev)
        # round-2 list in one launch (counts + look-back scan + map): its look-back workspace, zeroed once
        self._cs_ws = torch.zeros((K.ngp_chunk_segments_workspace(R) + 7) // 8, dtype=torch.int64, device=dev)
        # row forward (the default since round 4: +2 %, 9 of 9 alternating pairs,
        # profiles/r04/ab/row_forward_variants.txt): round 1 one wave per non-empty row with the
        # row's transmittance in its epilogue, which appends the row's round-2 samples to the
        # round-2 list itself (ngp_field_forward_first: no list launch); row_forward = 0 (tests)
        # or chunk_first != 64: the two-round lists below
        self.row_forward = 1
        assert self.row_forward in (0, 1)
        # where the next batch's march forks off the step: after the row forward's round 1 on the
        # single-cascade (Lego-shaped) scenes (round 1 runs alone, the march beside round 2 /
        # composite / MLP backward: +2.1 %, 6 of 6 pairs, profiles/r04/ab/march_fork_position.txt);
        # at the step's start on cascaded scenes, whose march is 3/4 of a forward-sized step and
        # beside the MLP backward slows it 1.7x (garden-shaped: -6 %, profiles/r04/ab/garden_r4.txt);
        # (march_at = start | r1 | fwd | mlp: diagnostics, scripts/diag/skip_cost.py)
        self.march_at = "r1" if self.cascades == 1 else "start"
        # round 1's coarse levels 0-7 encoded ahead (the next batch's first chunks, once the MLP + coarse
        # levels' Adam of this step has run, beside the binned levels' accumulation): round 1 then gathers
        # only levels 8-15 (pre_coarse = False, tests: off)
        # (nor under optimize_ext, where no batch is marched before the pose Adam: pre_ready stays false)
        self.pre_coarse = not self.optimize_ext
        self.pre_levels = 8  # (the kernel's PRE_LEVELS: levels 0-7, final once the side stream's Adam has run)
        assert self.march_at in ("start", "r1", "fwd", "mlp")
        self.eval_total = torch.zeros(1, dtype=torch.int64, device=dev)
        self.eval_idx = torch.empty(cap, dtype=torch.int32, device=dev)
        self.act_start = torch.empty(R, dtype=torch.int64, device=dev)
        # gradient-carrying samples (up to each ray's termination): index map
        self.n_active = torch.empty(R, dtype=torch.int32, device=dev)
        self.n_active_total = torch.zeros(1, dtype=torch.int64, device=dev)
        self.sample_idx = torch.empty(cap, dtype=torch.int32, device=dev)
        # binned hash backward: workspace for bin_samples_per_ray gradient-
        # carrying samples per ray on average (1 KiB each; the rest take the
        # atomic path, still exact)
        # binned levels [bin_level_lo, bin_merge_hi) merge runs of equal corner pairs along a ray
        # in the record write (one single-entry record per corner for a whole run: fewer records
        # written and accumulated).  Default for one-cascade scenes: levels 8-10 (consecutive
        # samples share a level-10 cell ~3 times on Lego; +1.2 % mean of 5 alternating pairs, 4 of 5,
        # profiles/r03/ab/bin_merge_hi.txt); cascaded scenes, whose every level is binned: all 16
        # (garden-shaped step 7.0 -> 8.3 M rays/s, profiles/r03/ab/garden_bin_merge_hi.txt).
        if bin_merge_hi is None:
            bin_merge_hi = 16 if big else 11
        self.bin_merge_hi = int(bin_merge_hi)
        if hash_backward != "atomic":
            self.bin_max_samples = R * bin_samples_per_ray
            nbytes = K.ngp_hash_backward_binned_workspace(self.bin_max_samples)
            self.bin_ws = torch.empty((nbytes + 255) // 256, 64, dtype=torch.int32, device=dev)
        # coarse atomic levels [0, coarse_rep_levels) add into coarse_rep replicas of their
        # gradient range, folded afterwards (ngp_hash_backward_levels_rep): the coarsest
        # levels are a few hundred KB every sample touches (levels 0-3 x 8 measured best,
        # profiles/r02/ab/coarse_replicas.txt); single process: folded by the MLP + coarse
        # levels' Adam launch
        self.coarse_rep = COARSE_REP
        self.coarse_rep_levels = min(COARSE_REP_LEVELS, self.bin_level_lo) if hash_backward != "atomic" else 0
        self.rep_buf = None
        if self.coarse_rep > 0 and self.coarse_rep_levels > 0:
            nrep = K.ngp_hash_backward_rep_floats(self.grid.desc, self.coarse_rep_levels, self.coarse_rep)
            self.rep_buf = torch.zeros(nrep, **f)
        self.bg = torch.ones(3, **f) if self.esf == 0 else torch.zeros(3, **f)  # models/rendering.py:287-296
        self._bg_rand = torch.zeros(3, **f)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(1000 + seed + self.rank)
        # ngp_sample_batch key: one seed for all ranks, rank r draws rays [r*R, (r+1)*R) of the global
        # batch (independent uniform draws per ray, as the reference's per-rank DataLoaders)
        # occupancy draws: rank-independent (every rank draws the same cells and
        # jitter; each evaluates its shard), so any world size builds one grid
        self.sample_seed, self.bg_seed, self.occ_seed = rng_keys(seed)
        self.occ_gen = torch.Generator(device=dev)
        self.occ_gen.manual_seed(2000 + seed)
        # device step counters: [0] Adam steps taken, [1] batches drawn (RNG
        # counter), [2] device-sampled occupancy updates (their RNG counter)
        self.dctr = torch.zeros(3, dtype=torch.int64, device=dev)
        # (Measured and removed in round 5's clean-up, DESIGN.md §9: a completion ticket by which
        # the step's Adam launches advanced dctr themselves, -2..-4 %; the coarse levels scattered
        # by the MLP backward launch, -4 %.)
        self._updated_for = -1  # global step whose occupancy update already ran (end of the previous graph)
        self.lr_dev = torch.full((1,), float(lr), device=dev)
        self._lr_set = float(lr)
        # HIP graphs of the steady-state step, one per buffer set (see train_step)
        self.use_graphs = bool(use_graphs)
        self._graphs = {}
        self._graph_post = {}
        # {"field_fwd"|"mlp_bwd"|"hash_bwd"|stage: (start, end) torch.cuda.Event} (eager diagnostics)
        self.kernel_events = None
        # ktimer.KernelTimer (bench): graph replays carry HIP events around every kernel
        self.timer = None
        # world > 1 graph replays run as segments with the collectives between them
        self._segmented = False
        self.comm_stream = torch.cuda.Stream(device=dev) if torch.cuda.is_available() else None
        self._throttle_q = []  # events of every THROTTLE_EVERY-th step (train_step)

    @staticmethod
    def _march_buffers(R, cap, f, cap_bits):
        dev = f["device"]
        return dict(rays_o=torch.empty(R, 3, **f), rays_d=torch.empty(R, 3, **f), hits_t=torch.empty(R, 2, **f),
                    noise=torch.empty(R, **f), counts=torch.empty(R, dtype=torch.int32, device=dev),
                    img_idxs=torch.empty(R, dtype=torch.int64, device=dev),
                    pix_idxs=torch.empty(R, dtype=torch.int64, device=dev), rgb_gt=torch.empty(R, 3, **f),
                    occ_summary=torch.empty(2 * ((cap_bits + 255) // 256), dtype=torch.int32, device=dev),
                    rays_a=torch.empty(R, 3, dtype=torch.int64, device=dev),
                    n_samples=torch.zeros(1, dtype=torch.int64, device=dev),
                    xyzs=torch.empty(cap, 3, **f), dirs=torch.empty(cap, 3, **f), deltas=torch.empty(cap, **f),
                    ts=torch.empty(cap, **f), slot_t=torch.empty(cap, **f), slot_dt=torch.empty(cap, **f),
                    # the chunked forward's round-1 list (first chunk_first samples of every row),
                    # built by the march itself (_march): off the step's critical path
                    eval_idx1=torch.empty(cap, dtype=torch.int32, device=dev),
                    eval_total1=torch.zeros(1, dtype=torch.int64, device=dev),
                    act_start1=torch.empty(R, dtype=torch.int64, device=dev), eval1_K=0,
                    # row-forward round 1: the non-empty rows (built by the march), the round-2 counts
                    rows_ne=torch.empty(R, dtype=torch.int32, device=dev),
                    n_rows_ne=torch.zeros(1, dtype=torch.int64, device=dev),
                    eval_total2=torch.zeros(1, dtype=torch.int64, device=dev),
                    # round 1's coarse levels 0-7 already in self.enc for this set's first chunks
                    # (ngp_field_encode_first_coarse, run by the previous step beside its accumulation)
                    pre_ready=False)

    def _tone_buffers(self, seed, R, cap, f):
        """use_exposure: the tonemappers' fp32 master (drawn as NGP draws it: a generator of its own at
        seed + 1), fp16 shadow, gradient, Adam moments and the backward's workspace; the tonemapped
        colours `ldr` beside `rgbs`, which keeps the log radiance (the backward recomputes the hidden
        layer from it); per march set the exposure of every sample (1 where no row owns the slot) and
        the table it was filled from (exp_key: host-side, None = not from a table)."""
        dev = self.dev
        self.tone_params = HG.init_tone_params(torch.Generator().manual_seed(seed + 1)).to(dev)
        self.tone16 = self.tone_params.half()
        self.tone_grad = torch.zeros(HG.TONE_PARAMS, **f)
        self.tone_exp_avg, self.tone_exp_avg_sq = torch.zeros(HG.TONE_PARAMS, **f), torch.zeros(HG.TONE_PARAMS, **f)
        self._tone_ws = torch.empty((self.L.ngp_tonemap_backward_indexed_workspace(cap) + 3) // 4, **f)
        self.ldr = torch.zeros(cap, 3, **f)  # (finite where never evaluated, as rgbs)
        self.out_loss_unit = torch.zeros(1, **f)
        self._exp_table = self._ray_exposure = None
        for m in self.msets:
            m["sample_exposure"] = torch.ones(cap, **f)
            m["exp_key"] = None

    def _bind(self, m):
        for k, v in m.items():
            setattr(self, k, v)

    # ------------------------------------------------------- exposure (use_exposure)
    def _exp_key(self):
        """What identifies the per-image exposure table of train_step, appended to the graph keys next
        to gt's: (address, length); nothing with the mode off"""
        if not self.use_exposure:
            return ()
        t = self._exp_table
        return (None,) if t is None else ((t.data_ptr(), int(t.shape[0])),)

    def _check_exposure(self, exposure, n, what):
        if not self.use_exposure:
            if exposure is not None:
                raise ValueError("exposure= needs a trainer built with use_exposure=True")
            return None
        if exposure is None:
            raise ValueError(f"NGPTrainer(use_exposure=True): pass exposure=, {what}")
        if (not isinstance(exposure, torch.Tensor) or exposure.dtype != torch.float32 or not exposure.is_contiguous()
                or exposure.device.type != self.dev.type or tuple(exposure.shape) != (n,)):
            raise ValueError(f"exposure must be a contiguous f32 tensor of shape ({n},) on the device: {what}")
        return exposure

    def _expose(self, k, s):
        """sample_exposure of buffer set k from the per-image table and the set's img_idxs (stream s)"""
        m, t = self.msets[k], self._exp_table
        self.L.ngp_sample_exposure(m["rays_a"], self.batch_size, m["img_idxs"], t, t.shape[0], self.cap,
                                   m["sample_exposure"], s)
        m["exp_key"] = self._exp_key()

    def _tonemap(self, s, total, idx):
        """LDR colours of the samples a field launch just evaluated: the listed samples idx[:total]
        (idx None: the range [0, total)), rgbs (log radiance) -> ldr"""
        self.L.ngp_tonemap_forward(self.rgbs, self.sample_exposure, self.cap, self.cap, total, idx, self.tone16,
                                   HG.TONE_LDR, self.ldr, s)

    # ---- argument groups the launches below share, in the header's order
    @property
    def _field(self):
        """(grid, hash table, MLP weights): the field as every kernel that evaluates it takes it"""
        return self.grid.desc, self.params16[HG.MLP_PARAMS:], self.params16

    @property
    def _listed(self):
        """The hash backward's leading arguments: the bound set's gradient-carrying
        samples (xyzs, capacity, count, list), the grid, dL/denc, the table's gradient"""
        return (self.xyzs, self.cap, self.n_active_total, self.sample_idx, self.grid.desc, self.denc,
                self.grad[HG.MLP_PARAMS:])

    @property
    def _bin(self):
        """... and the binned levels' (workspace, its sample capacity, level_lo, merge_hi) after them"""
        return self.bin_ws, self.bin_max_samples, self.bin_level_lo, self.bin_merge_hi

    @property
    def _adam_hp(self):
        """FusedAdam's (lr, beta1, beta2, eps, step count, gradient scale 1 / world); lr and the count on the device"""
        return self.lr_dev, 0.9, 0.999, 1e-15, self.dctr, 1.0 / self.world

    # ------------------------------------------------------- pose refinement
    def _pose_state(self, poses):
        """optimize_ext: the trainer's PoseRefiner and its device state, created
        on the first step from poses.shape[0]: fp32 Adam moments and the fp16
        shadow the Adam launch writes (unused), the optimizer's own device step
        count, the dense gradient, poses_eff
        (n_img,3,4) = the poses the rays are formed from, the constant learning
        rate, and the per-sample / per-ray gradient buffers of the chain."""
        n = int(poses.shape[0])
        assert poses.dtype == torch.float32 and poses.is_contiguous() and tuple(poses.shape[1:]) == (3, 4)
        ps = self._ps
        if ps is not None and ps["n_img"] != n:
            raise RuntimeError(f"optimize_ext: {n} poses, the trainer refines {ps['n_img']}")
        if ps is None:
            from pose_refine import PoseRefiner
            dev, R = self.dev, self.batch_size
            f = dict(device=dev, dtype=torch.float32)
            self.pose_refiner = PoseRefiner(n, device=dev)
            ext = self.pose_refiner.ext.data
            ps = self._ps = dict(
                n_img=n, ext=ext, m=torch.zeros_like(ext), v=torch.zeros_like(ext), ext16=torch.zeros_like(ext).half(),
                grad=torch.zeros_like(ext), poses_eff=torch.empty(n, 3, 4, **f),
                lr=torch.full((1,), self.pose_lr, **f),
                # the pose optimizer's own step count (its bias correction starts at 1 when the refiner is
                # created, as the reference's second FusedAdam, whatever the trainer's step count is then)
                step=torch.zeros(1, dtype=torch.int64, device=dev),
                # only the gradient-carrying samples are written and read (rays_act: rays_a with each row's
                # count cut to its n_active), so the per-sample buffers are never zeroed
                dxyz=torch.empty(self.cap, 3, **f), ddir=torch.empty(self.cap, 3, **f),
                rays_act=torch.zeros(R, 3, dtype=torch.int64, device=dev),
                d_rays_o=torch.zeros(R, 3, **f), d_rays_d=torch.zeros(R, 3, **f))
        return ps

    def _pose_compose(self, poses):
        """poses_eff = [Rod(dR) R | t + dT] on the current stream (train.py:92-95); `poses` is not modified"""
        ps = self._pose_state(poses)
        self.L.ngp_pose_compose(poses, ps["ext"], ps["n_img"], ps["poses_eff"], vren._stream())
        return ps["poses_eff"]

    def _pose_backward(self, directions, poses, apply_adam):
        """After the MLP backward, on the current stream and before any Adam of
        this step touches params16 (the input gradients gather the hash table
        and read the MLP weights): field input gradients over the step's own
        list -> per-ray sums over each row's gradient-carrying samples -> the
        chain rule to ext's dense gradient -> FusedAdam on ext (apex defaults
        as PoseRefiner.optimizer: betas (0.9, 0.999), eps 1e-8; dense, so an
        image absent from the batch still moves by its momentum).  The step's
        dL/dsigma, dL/drgb carry no loss scale beyond the parameter Adam's 1 /
        world, and the world is 1 here."""
        ps, L, s, R = self._ps, self.L, vren._stream(), self.batch_size
        self._ev("pose_bwd", 0)
        L.ngp_field_input_grad_pm(self.xyzs, self.dirs, self.cap, self.n_active_total, self.sample_idx, *self._field,
                                  self.enc, self.cap, self.drgb, self.denc, self.rgb_act, ps["dxyz"], ps["ddir"], s)
        ra = ps["rays_act"]
        ra.copy_(self.rays_a)
        ra[:, 2].copy_(self.n_active)
        L.ngp_ray_segment_sum(ps["dxyz"], ps["ddir"], self.ts, self.cap, ra, R, ps["d_rays_o"], ps["d_rays_d"], s)
        L.ngp_pose_grad(ps["d_rays_o"], ps["d_rays_d"], self.img_idxs, self.pix_idxs, R, directions, poses, ps["ext"],
                        ps["n_img"], ps["grad"], s)
        if apply_adam:
            L.ngp_adam_step_dev(ps["ext"], ps["grad"], ps["m"], ps["v"], ps["ext16"], ps["ext"].numel(), ps["lr"], 0.9,
                                0.999, 1e-8, ps["step"], 1.0, 0, s)
            L.ngp_counters_inc(ps["step"], 1, s)
        self._ev("pose_bwd", 1)

    @torch.no_grad()
    def refined_poses(self, poses):
        """(n_img,3,4): every image's pose with its current correction applied
        (the poses as given while optimize_ext is off or no step has run)"""
        if self.pose_refiner is None:
            return poses.clone()
        return self.pose_refiner.refined_poses(poses)

    # ------------------------------------------------------------ schedule
    def lr(self):
        """CosineAnnealingLR(T_max=num_epochs, eta_min=lr/30), stepped per epoch (train.py:149-151)."""
        e = self.global_step // self.steps_per_epoch
        eta_min = self.lr0 / 30
        return eta_min + (self.lr0 - eta_min) * (1 + math.cos(math.pi * e / self.num_epochs)) / 2

    # ------------------------------------------------------ occupancy grid
    @torch.no_grad()
    def mark_invisible_cells(self, K, poses, img_wh, chunk=64 ** 3):
        """models/networks.py:209-250 (once, before training): density -1 for
        cells no camera sees (or too near one), and count_grid = the fraction
        of cameras that see each cell, from which the erode decay is derived."""
        K, poses = K.to(self.dev), poses.to(self.dev)
        N_cams = poses.shape[0]
        self.count_grid = torch.zeros_like(self.density_grid)
        w2c_R = poses[:, :3, :3].transpose(1, 2)
        w2c_T = -w2c_R @ poses[:, :3, 3:]
        for c in range(self.cascades):
            indices, coords = self.all_indices, self.grid_coords
            for i in range(0, len(indices), chunk):
                xyzs = coords[i:i + chunk] / (self.G - 1) * 2 - 1
                s = min(2 ** (c - 1), self.scale)
                half_grid_size = s / self.G
                xyzs_w = (xyzs * (s - half_grid_size)).T
                xyzs_c = w2c_R @ xyzs_w + w2c_T
                uvd = K @ xyzs_c
                uv = uvd[:, :2] / uvd[:, 2:]
                in_image = (uvd[:, 2] >= 0) & (uv[:, 0] >= 0) & (uv[:, 0] < img_wh[0]) & (uv[:, 1] >= 0) & \
                           (uv[:, 1] < img_wh[1])
                covered_by_cam = (uvd[:, 2] >= NEAR_DISTANCE) & in_image
                count = covered_by_cam.sum(0) / N_cams
                self.count_grid[c, indices[i:i + chunk]] = count
                too_near_to_any_cam = ((uvd[:, 2] < NEAR_DISTANCE) & in_image).any(0)
                valid_mask = (count > 0) & (~too_near_to_any_cam)
                self.density_grid[c, indices[i:i + chunk]] = torch.where(valid_mask, 0., -1.)
        self.decay_cells = vren.erode_decay(self.count_grid).to(self.dev)
        self._decay_for = 0.95

    @torch.no_grad()
    def _occ_draw(self, c, density_threshold, s):
        """The parameter-independent head of a past-warmup update of cascade c:
        the occupied-cell list from density_grid, the sorted draws, and (keep)
        the kept draws -- launched on stream s.  Returns (lo, hi, M)."""
        L, G = self.L, self.G
        sc = min(2 ** (c - 1), self.scale)
        half_grid_size = sc / G
        M = G ** 3 // 4
        L.ngp_occupied_cells(self.density_grid[c], G ** 3, density_threshold, self._occ_list, self._occ_count,
                             self._occ_list_ws, s)
        lo, hi = ddp.shard_range(2 * M, self.rank, self.world)
        # (keep: every rank draws the whole list, positions = list positions, so that
        # the kept ones -- a cell's last draw -- are found over the whole list)
        glo, ghi = (0, 2 * M) if self.occ_keep else (lo, hi)
        # each half's cells drawn in ascending order: the density forward's waves
        # stay cache-local (1.8x faster than draw order, scripts/diag/density_order.py)
        L.ngp_occupancy_samples_sorted(self.occ_seed, self.dctr[2:], c, G, M, sc - half_grid_size, half_grid_size,
                                       self._occ_list, self._occ_count, glo, ghi, self._occ_ws, self._occ_xyz,
                                       self._occ_flat, s)
        if self.occ_keep:
            L.ngp_occupancy_keep(self._occ_flat, M, c * G ** 3, G ** 3, lo, hi, self._occ_mark, self._occ_kept,
                                 self._occ_kept_n, s)
        return lo, hi, M

    def update_density_grid(self, density_threshold, warmup=False, decay=0.95, erode=None, jitter=None,
                            drawn=False):
        """models/networks.py:252-281.  Past warmup the cells are drawn on device
        (ngp_occupied_cells + ngp_occupancy_samples: no host sync, so the update
        can sit inside a captured graph).  Multi-GPU: each rank evaluates its
        1/world share of the (identically drawn) cells and the cell maxima are
        combined with one MAX all-reduce, so every rank packs an identical
        bitfield.  erode (default: the trainer's setting) decays each cell by
        clamp(decay**(1/count_grid), 0.1, 0.95) (networks.py:270-272).
        jitter (tests): the warm-up's U[0,1) jitter per cell (C, G^3, 3) in
        grid_coords order instead of the trainer's own draw.  drawn (one
        cascade, past warmup): _occ_draw already ran for this update (the
        captured step launches it beside the step before the update)."""
        C, G = self.cascades, self.G
        erode = self.erode if erode is None else erode
        if erode and self.decay_cells is None:
            raise RuntimeError("update_density_grid(erode=True) needs count_grid: call mark_invisible_cells first")
        if erode and decay != self._decay_for:  # (host evaluation: not inside a graph capture)
            self.decay_cells = vren.erode_decay(self.count_grid, decay).to(self.dev)
            self._decay_for = decay
        L, s = self.L, vren._stream()
        key = self._occ_key  # zero on entry; the EMA consumes (re-zeroes) it
        for c in range(C):
            sc = min(2 ** (c - 1), self.scale)
            half_grid_size = sc / G
            if warmup:  # get_all_cells (networks.py:167-179)
                # the jitter is drawn for every cell from a rank-independent
                # generator, then each rank evaluates its share of the cells:
                # any world size builds the same grid
                jit = (torch.rand(self.grid_coords.shape, device=self.dev, generator=self.occ_gen) if jitter is None
                       else jitter[c].to(self.dev))
                lo, hi = ddp.shard_range(self.grid_coords.shape[0], self.rank, self.world)
                indices, coords = self.all_indices[lo:hi], self.grid_coords[lo:hi]
                xyzs_w = (coords / (G - 1) * 2 - 1) * (sc - half_grid_size)
                xyzs_w += (jit[lo:hi] * 2 - 1) * half_grid_size
                sig, _ = HG.density_forward(xyzs_w.float().contiguous(), self.grid, self.params16)
                flat = (indices + c * G ** 3).contiguous()
                n = flat.shape[0]
            else:  # sample_uniform_and_occupied_cells (networks.py:181-207), on device
                if drawn:
                    assert C == 1, "update_density_grid(drawn=True) needs one cascade"
                    M = G ** 3 // 4
                    lo, hi = ddp.shard_range(2 * M, self.rank, self.world)
                else:
                    lo, hi, M = self._occ_draw(c, density_threshold, s)
                n = hi - lo
                if self.occ_keep:
                    # encode + density net of the kept samples only (sigma written at their position)
                    L.ngp_field_encode_mlp(self._occ_xyz, None, n, self._occ_kept_n, self._occ_kept, *self._field, None,
                                           self._occ_sig, None, None, s)
                    L.ngp_density_scatter_kept(self._occ_kept, self._occ_kept_n, n, self._occ_flat, self._occ_sig, 0,
                                               key, s)
                    continue
                # encode + density net in one launch (no encoding kept)
                L.ngp_field_encode_mlp(self._occ_xyz, None, n, None, None, *self._field, None, self._occ_sig, None,
                                       None, s)
                sig, flat = self._occ_sig, self._occ_flat
            # density_grid_tmp[c, indices] = sigma, list positions lo + i (rank shards)
            L.ngp_density_scatter_last(flat, sig, n, lo, key, s)
        if not warmup:
            L.ngp_counters_inc(self.dctr[2:], 1, s)
        ddp.combine_density_tmp_(key, self.pg)
        L.ngp_density_grid_ema(self.density_grid, key, self.density_grid.numel(), decay,
                               self.decay_cells if erode else None, density_threshold, self._sum_cnt, self.threshold, s)
        ddp.sync_threshold_(self.threshold, self.pg)  # identical threshold on every rank
        vren.packbits(self.density_grid, self.threshold[:1], self.density_bitfield)

    def _march(self, k, src, directions, poses, stream):
        """Ray generation + AABB + single-pass march of one batch into buffer
        set k.  src = ("idx", img_idxs, pix_idxs, noise | None): rays of the
        given pixels (noise drawn from self.gen when None); or ("sample", add,
        gt_u8): the whole batch drawn on device (ngp_sample_batch_dev: pixels,
        ground truth, noise from Philox keyed by (seed, batch counter + add),
        the counter in device memory so a replayed graph draws fresh batches)."""
        m = self.msets[k]
        m["pre_ready"] = False  # (the set's coarse-level round-1 encoding is stale from here on)
        L, R = self.L, self.batch_size
        side = stream is self.march_stream
        with torch.cuda.stream(stream):
            if side:
                self._ev("march_side", 0, stream)
            s = stream.cuda_stream
            rays = (m["rays_o"], m["rays_d"], m["hits_t"])
            if src[0] == "sample":
                _, add, gt = src
                n_img, hw = gt.shape[0], gt.shape[1]
                assert gt.dtype in (torch.uint8, torch.float32) and gt.is_contiguous()
                L.ngp_sample_batch_dev(self.sample_seed, self.dctr[1:], add, self.rank * R, gt,
                                       int(gt.dtype == torch.float32), n_img, hw, directions, poses, R, self.center,
                                       self.half_size, NEAR_DISTANCE, m["img_idxs"], m["pix_idxs"], m["rgb_gt"],
                                       m["noise"], *rays, s)
            else:
                _, img_idxs, pix_idxs, noise = src
                assert img_idxs.shape[0] == R
                if self.optimize_ext or self.use_exposure:  # (the pose gradient / the exposure lookup read the set's indices)
                    m["img_idxs"].copy_(img_idxs)
                    m["pix_idxs"].copy_(pix_idxs)
                L.ngp_raygen_aabb(directions, poses, img_idxs, pix_idxs, R, self.center, self.half_size, NEAR_DISTANCE,
                                  *rays, s)
                if noise is None:
                    torch.rand(R, out=m["noise"], generator=self.gen)  # custom_functions.py:83
                else:
                    m["noise"].copy_(noise)
            # the bitfield's block summary, rebuilt per march: any writer of
            # density_bitfield (update_density_grid, tests, tools) stays valid
            vren.bitfield_summary(self.density_bitfield, self.G, out=m["occ_summary"])
            L.ngp_march_train_slots(*rays, R, self.density_bitfield, self.cascades, self.G, self.scale, self.esf,
                                    m["noise"], self.max_samples, m["counts"], m["rays_a"], m["n_samples"], m["slot_t"],
                                    m["slot_dt"], m["occ_summary"], s)
            L.ngp_march_train_compact(m["rays_o"], m["rays_d"], m["rays_a"], R, m["slot_t"], m["slot_dt"],
                                      self.max_samples, m["xyzs"], m["dirs"], m["deltas"], m["ts"], s)
            # round 1 of the chunked forward: the list of each row's first chunk_first samples
            # (counts min(N_r, K) + scan + list in one launch), here beside the previous step
            # instead of at the head of this batch's step; its length eval_total1 is counted
            # into eval_stats by the round-2 list launch of the step that evaluates it
            K = self.chunk_first
            rows = self._rows_fwd(K)
            m["eval1_K"] = K if (K > 0 and R <= 65536 and not rows) else 0
            if m["eval1_K"]:
                L.ngp_ray_segments_capped(m["rays_a"], R, K, m["act_start1"], m["eval_total1"], None, m["eval_idx1"], s)
            elif rows:
                L.ngp_rays_nonempty(m["rays_a"], R, m["rows_ne"], m["n_rows_ne"], None, m["eval_total2"], s)
            if self.use_exposure:
                # every sample's exposure from the per-image table, here beside the previous step; a batch
                # given per-ray exposures (step) gets them once it is bound (_step)
                if src[0] == "sample":
                    self._expose(k, s)
                else:
                    m["exp_key"] = None
            if side:
                self._ev("march_side", 1, stream)

    def _rows_fwd(self, K):
        """The row forward runs the chunked evaluation (its first chunk is one
        wave: chunk_first 64; other chunk sizes take the two-round lists)."""
        return bool(self.row_forward) and K == 64

    def march_fork_point(self):
        """Where the next batch's march forks off the step (march_at; "r1"
        needs the row forward's own round-1 launch, else the step's start)."""
        if self.march_at == "r1" and not (self._rows_fwd(self.chunk_first) and self.row_forward == 1):
            return "start"
        return self.march_at

    def _can_prefetch(self):
        """The next batch may be marched ahead unless the next step begins with
        an occupancy update (that batch must see the new bitfield)."""
        return (self._pending is None and (self.global_step + 1) % self.update_interval != 0
                and not self.no_prefetch and not self.optimize_ext)

    def prefetch(self, src, directions, poses):
        """March the NEXT batch into the idle buffer set on the side stream so
        it overlaps the current step's field / loss / backward / Adam.  Called
        by step() once the current set is bound: everything the side stream
        needs (the next batch's indices, the bitfield, the idle set's last
        readers = the previous step's backward) is already enqueued on the
        main stream, which one event captures.  (Callers that edit
        density_bitfield between steps must not pass next_batch; callers that
        edit params / params16 between steps call invalidate_pre_encode, or
        use load_params.)"""
        if not self._can_prefetch():
            return False
        k = 1 - self.cur
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())
        self.march_stream.wait_event(ready)
        self._march(k, src, directions, poses, self.march_stream)
        ev = torch.cuda.Event()
        ev.record(self.march_stream)
        self._pending = (k, ev)
        self.n_prefetched += 1
        return True

    def invalidate_pre_encode(self):
        """Forget every buffer set's round-1 coarse-level encoding done ahead
        (pre_ready): it was encoded from the parameters of its time, so any
        write to params / params16 between steps (checkpoint load, state
        transplant, hand edits) must call this (load_params does) -- the next
        round 1 then gathers all 16 levels itself instead of mixing levels 0-7
        of the old parameters with 8-15 of the new."""
        for m in self.msets:
            m["pre_ready"] = False

    @torch.no_grad()
    def load_params(self, params, params16=None):
        """Overwrite the fp32 master (and the fp16 shadow: params16, or the
        master rounded) between steps, invalidating the pre-encoded round 1."""
        n = self.n_params
        self.params.copy_(params[:n].to(self.params))
        self.params16.copy_(params[:n].half() if params16 is None else params16[:n].to(self.params16))
        self.invalidate_pre_encode()

    def drain(self):
        """Order the current stream after a batch marched ahead on the side
        stream (the batch stays pending for the next train_step)."""
        if self._pending is not None and self._pending[1] is not None:
            torch.cuda.current_stream().wait_event(self._pending[1])

    def _ev(self, name, i, stream=None):
        """Breakdown instrumentation (eager steps only): i = 0 opens a new
        (start, end) HIP-event pair for `name` on `stream` (default: the
        current one), i = 1 closes the last one.  kernel_events maps a name to
        the list of its pairs (a kernel launched twice per step has two)."""
        ev = self.kernel_events
        if ev is None:
            return
        st = stream if stream is not None else torch.cuda.current_stream()
        if i == 0:
            pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            pair[0].record(st)
            ev.setdefault(name, []).append(pair)
        else:
            ev[name][-1][1].record(st)

    # ---------------------------------------------------------------- step
    def reset_stats(self):
        """Zero the sample counters (stat_totals) on the current stream."""
        self.stats.zero_()
        self.eval_stats.zero_()

    def stat_totals(self):
        """(marched, composited, active, evaluated) samples of the steps run
        since reset_stats() (sum over the stripes; evaluated = both chunked
        rounds, 0 when chunk_first == 0: every marched sample is evaluated)."""
        t = [int(v) for v in self.stats.view(STAT_STRIPES, STAT_STRIDE)[:, :3].sum(0).tolist()]
        return t + [int(self.eval_stats[0])]

    def step(self, img_idxs, pix_idxs, rgb_gt, directions, poses, noise=None, apply_adam=True, next_batch=None,
             exposure=None):
        """One training step on a batch (train.py:174-200).  img/pix (R) i64,
        rgb_gt (R,3) f32, directions (HW,3), poses (n_img,3,4), all on device.
        next_batch = (img, pix) of the following step: marched ahead on the
        side stream.  exposure (use_exposure): the exposure of every ray (R) f32."""
        self._ray_exposure = self._check_exposure(exposure, self.batch_size, "one value per ray of the batch")
        nxt = None if next_batch is None else ("idx", next_batch[0], next_batch[1], None)
        return self._step(("idx", img_idxs, pix_idxs, noise), rgb_gt, directions, poses, apply_adam, nxt)

    def train_step(self, gt, directions, poses, allow_pair=True, exposure=None):
        """One training step on a batch drawn on device from the training set
        (gt (n_img, HW, 3) u8 images -- or f32 colours, e.g. alpha-blended
        data -- directions (HW,3), poses (n_img,3,4)):
        the reference's DataLoader + training_step with nothing on the host.
        The next step's batch is drawn and marched ahead on the side stream.
        Steady-state steps (batch already marched ahead, no occupancy update
        now or next step) replay a captured HIP graph of the whole step
        (NGP_GRAPHS=0: always eager).  pair_steps: a call may run this step
        AND the next in one replay (the next call then only advances the
        count); allow_pair=False keeps this call to one step, e.g. the last
        step of a measured window.  exposure (use_exposure): one exposure per
        training image (n_img) f32 on the device, e.g. rays[:, 0, 3] of an
        HDR-NeRF set; read when the kernels run, its address part of the graph
        key like gt's."""
        gs, ui = self.global_step, self.update_interval
        self._throttle()
        if self.use_exposure or exposure is not None:
            self._exp_table = self._check_exposure(exposure, gt.shape[0], "one value per training image")
        if self._ran_ahead:  # this step was the second half of the previous call's two-step graph
            if self._pair_key != (gt.data_ptr(), directions.data_ptr(), poses.data_ptr(), gt.shape,
                                  gt.dtype) + self._exp_key():
                raise RuntimeError("pair_steps: the second step of a two-step graph replay must be given the same "
                                   "gt / directions / poses (/ exposure) as the first (it already ran on them)")
            self._ran_ahead = False
            self.global_step += 1
            return self.out_loss
        # (optimize_ext steps are eager: nothing is marched ahead of a pose Adam, so _pending stays None
        # and use_graphs has no effect under it)
        if (self.use_graphs and self._pending is not None and (gs % ui != 0 or self._updated_for == gs)
                and gs >= self.warmup_steps and self.kernel_events is None and not self.no_prefetch):
            if (allow_pair and self.pair_steps and not self.dp and self.timer is None and (gs + 1) % ui != 0
                    and (gs + 2) % ui != 0 and gs // self.steps_per_epoch == (gs + 1) // self.steps_per_epoch):
                return self._replay_pair(gt, directions, poses)
            return self._replay(gt, directions, poses, (gs + 1) % ui == 0)
        return self._step(("sample", 0, gt), None, directions, poses, True, ("sample", 1, gt))

    def _throttle(self):
        """Back-pressure on the host: an event every THROTTLE_EVERY steps, and
        before enqueueing more the host waits for the one THROTTLE_DEPTH events
        back, so at most ~160 steps are ever enqueued ahead of the GPU (that
        step finished long ago when the GPU is the bottleneck: the queue never
        drains, measured no slower).  It bounds the host's lead -- a caller
        that stops, reads out_loss or edits the scene waits for at most that
        many steps, and the runtime's command queue stays bounded -- and is not
        a fault fix.  (The memory faults once seen in long graph-replayed runs
        had another cause, found and fixed in d87e59d: a captured
        hipMemsetAsync of the occupancy-list counter was not ordered before the
        list kernel, which then read stale counts and wrote past the list;
        counters are now zeroed by a kernel node, and the list is built from
        per-block counts with no counter to zero at all.)"""
        if self.global_step % THROTTLE_EVERY:
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._throttle_q.append(ev)
        if len(self._throttle_q) > THROTTLE_DEPTH:
            self._throttle_q.pop(0).synchronize()

    def _set_lr(self):
        lr = self.lr()
        if lr != self._lr_set:
            self.lr_dev.fill_(lr)
            self._lr_set = lr

    def _replay(self, gt, directions, poses, update_after):
        """Graph-replayed steady-state step for the batch pending in set k.
        Plain variant: the step's kernels on the capture stream, the next
        batch's march forked onto the side stream and joined before the end,
        the device counters advanced last.  update_after (the next step opens
        with an occupancy update): no fork; after the step the update
        (networks.py:252-281, cells drawn on device) and then the next batch's
        march against the new bitfield, all inside the graph."""
        k, ev = self._pending
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)
        self._set_lr()
        key = (k, bool(update_after), gt.data_ptr(), directions.data_ptr(), poses.data_ptr(), gt.shape, gt.dtype,
               self.msets[k]["pre_ready"]) + self._exp_key()
        self._expose_pending(k)
        if not self.dp:
            self._run_graph(key, lambda: self._graph_body(k, gt, directions, poses, update_after))
        else:
            if self._capture_comm():  # the whole step, its collectives included, in ONE graph
                self._run_graph(key + ("whole",), lambda: self._dp_sequence(k, gt, directions, poses, update_after,
                                                                          lambda sub, fn: fn()))
            else:  # collectives between graph segments
                self._dp_sequence(k, gt, directions, poses, update_after,
                                  lambda sub, fn: self._run_graph(key + sub, fn))
            if update_after:  # (every 16 steps) eager: the update has its own collectives
                self.update_density_grid(0.01 * MAX_SAMPLES / 3 ** 0.5, warmup=False)
                self._march(1 - k, ("sample", 0, gt), directions, poses, torch.cuda.current_stream())
        self.cur = k
        self._bind(self.msets[k])
        self._pending = (1 - k, None)  # marched (and joined) inside the graph
        if self.use_exposure:
            self.msets[1 - k]["exp_key"] = self._exp_key()  # (a replay does not run _march)
        self.n_prefetched += 1
        self.global_step += 1
        if update_after:
            self._updated_for = self.global_step
        return self.out_loss

    def _capture_comm(self):
        """The data-parallel step's collectives captured into the step's graph
        (one replay per step, no segment boundaries): emulated worlds (local
        copies) and a world-1 RCCL group (tests) by default.  A real world > 1
        keeps the graph segments with eager RCCL calls between them unless
        NGP_DP_CAPTURE=1 opts in (captured multi-rank RCCL
        collectives, with the occupancy update's eager ones between the
        replays, have not run on a multi-GPU node; the segmented step measured
        ~4 % slower emulated).  gloo stages device tensors
        through the host and cannot be captured.  NGP_DP_CAPTURE=0: segments
        always."""
        opt = os.environ.get("NGP_DP_CAPTURE", "")
        if opt == "0":
            return False
        if not ddp.comm_active(self.pg):
            return True
        if dist.get_backend(self.pg) != "nccl":
            return False
        return self.world == 1 or opt == "1"

    def _dp_sequence(self, k, gt, directions, poses, update_after, run):
        """The data-parallel step (ZeRO-1, per-bucket pipeline): run(sub, fn)
        executes one graph segment -- its own graph (segmented replay,
        collectives between the segments) or inline (the whole step captured
        as one graph).  Compute segment; coarse levels on the side stream ->
        bucket 0's reduce-scatter, Adam, all-gather on the comm stream while
        the binned levels run range by range (bin_cuts), each range's bucket
        following it on the comm stream while the next range accumulates;
        joined; device counters advanced."""
        cs, comm = torch.cuda.current_stream(), self.comm_stream
        run(("compute",), lambda: self._segment_compute(k, gt, directions, poses, update_after))
        if self.hash_backward != "atomic":
            self.bwd_stream.wait_stream(cs)
            with torch.cuda.stream(self.bwd_stream):
                run(("coarse",), self._coarse_levels)  # (graph segment on the side stream)
            comm.wait_stream(self.bwd_stream)
            self._bucket_update(0)
            nr = len(self.bin_cuts) - 1
            if nr <= 0:  # every level atomic (bin_level_lo == n_levels): the buckets past the
                # alignment cut hold the last params, complete once the coarse segment is
                for j in range(1, len(self.buckets)):
                    self._bucket_update(j)
            for r in range(nr):
                run(("apply", r), lambda r=r: self._segment_apply(r))
                comm.wait_stream(cs)
                # (a range's bucket; a bucket emptied by the alignment was dropped: the rest
                # follow the last range)
                for j in ([1 + r] if r < nr - 1 else range(1 + r, len(self.buckets))):
                    if j < len(self.buckets):
                        self._bucket_update(j)
        else:
            comm.wait_stream(cs)
            for i in range(len(self.buckets)):
                self._bucket_update(i)
        cs.wait_stream(comm)
        self.L.ngp_counters_inc(self.dctr, 2, vren._stream())

    def _replay_pair(self, gt, directions, poses):
        """Two consecutive steady-state steps (no occupancy update at, between
        or right after them; one epoch, so one learning rate) as ONE graph
        replay: the replay boundary (the GPU finishing one graph before it
        starts the next) is paid once per two steps.  The second step's
        train_step call then only advances the host step count
        (self._ran_ahead); out_loss holds the second step's losses."""
        k, ev = self._pending
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)
        self._set_lr()
        key = ("pair", k, gt.data_ptr(), directions.data_ptr(), poses.data_ptr(), gt.shape, gt.dtype,
               self.msets[k]["pre_ready"]) + self._exp_key()
        self._expose_pending(k)

        def body():
            self._graph_body(k, gt, directions, poses, False)
            self._graph_body(1 - k, gt, directions, poses, False)
        self._run_graph(key, body)
        self.cur = 1 - k
        self._bind(self.msets[1 - k])
        self._pending = (k, None)  # the batch after both, marched inside the graph
        if self.use_exposure:
            self.msets[k]["exp_key"] = self.msets[1 - k]["exp_key"] = self._exp_key()
        self.n_prefetched += 2
        self.global_step += 1
        self._ran_ahead = True
        self._pair_key = key[2:7] + self._exp_key()
        return self.out_loss

    def _expose_pending(self, k):
        """use_exposure: the batch marched ahead into set k took its exposures from the table of the call
        that marched it; a call with another table fills them again (current stream, outside the graph)"""
        if self.use_exposure and self.msets[k]["exp_key"] != self._exp_key():
            self._expose(k, vren._stream())

    def _run_graph(self, key, body):
        """Replay the graph captured for `key` (capturing body() first if new;
        with a measurement timer set, one with its stamps)."""
        tm = self.timer  # (measurement) graphs with wall-clock stamp kernels around every kernel
        if tm is not None:
            key = key + (tm.uid,)
        if key not in self._graphs:
            g = torch.cuda.CUDAGraph()
            # capture on a side stream, ordered after everything enqueued so far
            torch.cuda.current_stream().synchronize()
            if tm is not None:
                tm.arm()
            try:
                with vren.graph_capture(g):
                    body()
            finally:
                if tm is not None:
                    tm.disarm()
            # host-side state the body leaves (which buffer set has its round-1 coarse levels
            # encoded ahead): a replay does not run the body, so it restores this instead
            self._graph_post[key] = tuple(m["pre_ready"] for m in self.msets)
            self._graphs[key] = g
        self._graphs[key].replay()
        for m, f in zip(self.msets, self._graph_post[key]):
            m["pre_ready"] = f

    def _segment_compute(self, k, gt, directions, poses, update_after):
        """world > 1, first segment: the step up to the gradient (and the next
        batch's march on the side stream, joined, unless an update follows)."""
        self.cur = k
        self._bind(self.msets[k])
        cs = torch.cuda.current_stream()
        fork = None
        if not update_after:
            def fork():
                self.march_stream.wait_stream(cs)
                self._march(1 - k, ("sample", 1, gt), directions, poses, self.march_stream)
                return True
        self._segmented = True
        try:
            self._compute(self.rgb_gt, True, fork)
        finally:
            self._segmented = False
        if fork is not None:
            cs.wait_stream(self.march_stream)

    def _coarse_levels(self, fold=True):
        """The atomic coarse hash levels [0, bin_level_lo) on the current stream
        (fold=False: their replicated part stays in rep_buf for the accumulation)."""
        self.L.ngp_hash_backward_levels_rep(*self._listed, 0, self.bin_level_lo, self.rep_buf,
                                            self.coarse_rep_levels if self.rep_buf is not None else 0,
                                            max(1, self.coarse_rep), int(fold), vren._stream())

    def _segment_apply(self, r):
        """world > 1 graph segment r (main stream): accumulation of the binned
        level range [bin_cuts[r], bin_cuts[r + 1]) (beside the previous
        range's bucket chain on the comm stream); segment 0 first writes the
        binned levels' records."""
        if r == 0:
            self.L.ngp_hash_binned_write(*self._listed, *self._bin, vren._stream())
        self._accum_levels(self.bin_cuts[r], self.bin_cuts[r + 1])

    def _accum_levels(self, lo, hi):
        self.L.ngp_hash_binned_accum_levels(self.grid.desc, self.grad[HG.MLP_PARAMS:], *self._bin, lo, hi,
                                            vren._stream())

    def _bucket_update(self, i):
        """On the comm stream: reduce-scatter of gradient bucket i into this
        rank's shard, FusedAdam on the shard (the same launch clears the
        bucket's local gradient), all-gather of the shard's fp16 shadow.  The
        step runs this for every bucket, so its host path is lean: views and
        launch arguments built once (_bucket_host)."""
        cs = self.comm_stream
        with torch.cuda.stream(cs):
            self._reduce_bucket(i)
            self._adam_shard(i, cs.cuda_stream, zero=True)
            self._gather_bucket(i)

    def _bucket_host(self):
        """per bucket: the tensors its collectives take and the argument tuple
        of its Adam launch (ngp_adam_step_dev_zero minus the stream)"""
        if getattr(self, "_bk", None) is None:
            self._bk = []
            for i, ((a, b), (lo, hi)) in enumerate(zip(self.buckets, self.shards)):
                h = {"full": self._gbuf[a:b], "src": self._gbuf[lo:hi], "shard": self._gshard[i],
                     "p16full": self._p16buf[a:b], "p16shard": self._p16buf[lo:hi]}
                h["adam"] = (self._pbuf[lo:hi], h["shard"], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], h["p16shard"],
                             hi - lo, *self._adam_hp, 1, h["full"], b - a)
                self._bk.append(h)
        return self._bk

    def _reduce_bucket(self, i):
        """reduce-scatter (SUM) of gradient bucket i into this rank's shard buffer"""
        h = self._bucket_host()[i]
        if not ddp.comm_active(self.pg):  # (emulation: this rank's shard of the local gradient)
            h["shard"].copy_(h["src"])
        else:
            ddp.reduce_scatter_(h["full"], h["shard"], self.pg)

    def _gather_bucket(self, i):
        """all-gather of bucket i's fp16 shadow from every rank's shard"""
        h = self._bucket_host()[i]
        if ddp.comm_active(self.pg):  # (emulation: the shard's shadow is in place already)
            ddp.all_gather_(h["p16full"], h["p16shard"], self.pg)

    def _graph_body(self, k, gt, directions, poses, update_after=False):
        self.cur = k
        self._bind(self.msets[k])
        cs = torch.cuda.current_stream()
        if not update_after:
            def fork():
                self.march_stream.wait_stream(cs)
                self._march(1 - k, ("sample", 1, gt), directions, poses, self.march_stream)
                return True

            self._compute(self.rgb_gt, True, fork)
            cs.wait_stream(self.march_stream)
            self.L.ngp_counters_inc(self.dctr, 2, vren._stream())
        else:
            thr = 0.01 * MAX_SAMPLES / 3 ** 0.5
            drawn = self.cascades == 1
            if drawn:
                # the update's parameter-independent head (occupied cells, draws, kept draws: they
                # read density_grid and the occupancy counter only) beside this step, on the march
                # stream (idle: no prefetch before an update)
                self.march_stream.wait_stream(cs)
                with torch.cuda.stream(self.march_stream):
                    self._occ_draw(0, thr, vren._stream())
            self._compute(self.rgb_gt, True, None)
            self.L.ngp_counters_inc(self.dctr, 2, vren._stream())
            if drawn:
                cs.wait_stream(self.march_stream)
            self.update_density_grid(thr, warmup=False, drawn=drawn)
            self._march(1 - k, ("sample", 0, gt), directions, poses, cs)

    def _step(self, src, rgb_gt, directions, poses, apply_adam, next_src):
        self._ev("occupancy_update", 0)
        if self.global_step % self.update_interval == 0 and self._updated_for != self.global_step:
            self.update_density_grid(0.01 * MAX_SAMPLES / 3 ** 0.5, warmup=self.global_step < self.warmup_steps)
        self._ev("occupancy_update", 1)
        self._ev("raygen_march", 0)
        if self._pending is not None:  # this batch was marched ahead on the side stream
            k, ev = self._pending
            self._pending = None
            self.cur = k
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
        else:
            # optimize_ext: the rays of step N are those of ext_N (train.py:92-95), composed on the device
            mp = self._pose_compose(poses) if self.optimize_ext else poses
            self._march(self.cur, src, directions, mp, torch.cuda.current_stream())
        if self.optimize_ext:
            self._pose_state(poses)
            self._pose_args = (directions, poses)
        self._bind(self.msets[self.cur])
        if self.use_exposure:
            if src[0] == "sample":
                self._expose_pending(self.cur)
            else:
                self.L.ngp_sample_exposure_rays(self.rays_a, self.batch_size, self._ray_exposure, self.cap,
                                                self.sample_exposure, vren._stream())
                self.msets[self.cur]["exp_key"] = None
        if rgb_gt is None:
            rgb_gt = self.rgb_gt
        self._ev("raygen_march", 1)
        fork = None
        if next_src is not None and apply_adam and not self.optimize_ext:
            fork = lambda: self.prefetch(next_src, directions, poses)  # noqa: E731
        if apply_adam:
            self._set_lr()
        out = self._compute(rgb_gt, apply_adam, fork)
        if apply_adam:
            self.L.ngp_counters_inc(self.dctr, 2, vren._stream())
            self.global_step += 1
        return out

    def _compute(self, rgb_gt, apply_adam, fork):
        """Field forward (chunked), compositing + loss + its backward, field
        backward, [all-reduce], Adam -- on the current stream, no host sync.
        fork() (nullable) launches the next batch's march on the side stream
        and returns whether it did (prefetch() declines before an occupancy
        update or with no_prefetch), where self.march_at says: by default right after the row forward's
        round 1 (which then has the chip to itself; the march overlaps round
        2, the composite and the MLP backward: +2.1 %,
        profiles/r04/ab/march_fork_position.txt); before the row forward, at
        the step's start (round 2: +1.5 % against after the composite,
        profiles/r02/ab/prefetch_at.txt)."""
        L, s, R = self.L, vren._stream(), self.batch_size
        at = self.march_fork_point()
        marched = False  # the next batch marched beside this step (fork() said so)
        if fork is not None and at == "start":
            marched = bool(fork())
        self._ev("field_fwd", 0)
        if self._rows_fwd(self.chunk_first):
            # round 1: a wave per non-empty row (the list built by the march), its transmittance
            # deciding the row's round 2, whose samples it appends to the round-2 list itself (no
            # list pass); round 2: the field over that list
            self._ev("hash_encode", 0)
            m = self.msets[self.cur]
            pre = 8 if m["pre_ready"] else 0
            m["pre_ready"] = False
            L.ngp_field_forward_first_pre_act(self.xyzs, self.dirs, self.deltas, self.rays_a, self.rows_ne,
                                              self.n_rows_ne, R, self.cap, 1e-4, *self._field, self.enc, self.sigmas,
                                              self.rgbs, None, self.eval_idx, self.eval_total2, self.eval_stats, pre,
                                              self.rgb_act, s)
            self._ev("hash_encode", 1)
            if fork is not None and at == "r1":
                # (captured before round 2: round 2 captured first and the march forked from an event
                # recorded after round 1 -- the same dependencies -- ran 27 % slower: the graph's
                # queue assignment follows the capture order, profiles/r06/ab/capture_order.txt)
                marched = bool(fork())
            self._field_indexed(s, self.eval_idx, self.eval_total2, tone=False)
            if self.use_exposure:
                # exactly the samples the two rounds evaluated: round 1's rows (their first chunk_first
                # samples: the chunk _rows_fwd admits), then round 2's list.  Both
                # after round 2, so that round 1, the fork and round 2 are captured in the order above
                # (the march then runs beside these as well)
                L.ngp_tonemap_forward_rows(self.rgbs, self.cap, self.rays_a, self.rows_ne, self.n_rows_ne, R,
                                           self.chunk_first, self.sample_exposure, self.tone16, self.ldr, s)
                self._tonemap(s, self.eval_total2, self.eval_idx)
        elif self.chunk_first > 0:  # two rounds: first K samples per row, then the rest of unterminated rows
            K = self.chunk_first
            if self.eval1_K == K:  # built by this batch's march
                self._field_indexed(s, self.eval_idx1, self.eval_total1)
            else:
                L.ngp_chunk_counts(self.rays_a, R, K, None, None, 1e-4, self.eval_counts, s)
                L.ngp_ray_segments(self.eval_counts, self.rays_a, R, 0, self.act_start, self.eval_total,
                                   self.eval_stats, self.eval_idx, s)
                self._field_indexed(s)
            # second round [K, N_r) of the rows still transparent after K samples: counts, scan
            # and list in one launch (ngp_chunk_segments; the two launches it replaces cost a
            # launch gap and a second pass over rays_a)
            L.ngp_chunk_segments(self.sigmas, self.deltas, self.rays_a, R, K, 0, 1e-4, self._cs_ws, self.act_start,
                                 self.eval_total, self.eval_stats, self.eval_total1 if self.eval1_K == K else None,
                                 self.eval_idx, s)
            self._field_indexed(s)
        else:  # encode + MLPs in one launch over every marched sample
            self._ev("hash_encode", 0)
            L.ngp_field_encode_mlp_act(self.xyzs, self.dirs, self.cap, self.n_samples, None, *self._field, self.enc,
                                       self.sigmas, self.rgbs, None, self.rgb_act, s)
            self._ev("hash_encode", 1)
            if self.use_exposure:
                self._tonemap(s, self.n_samples, None)
        self._ev("field_fwd", 1)
        if fork is not None and at == "fwd":
            marched = bool(fork())
        bg = self.bg
        if self.random_bg:  # rendering.py:287-288, one colour per batch, drawn on device (graph-safe)
            bg = self._bg_rand
            L.ngp_random_bg(self.bg_seed, self.dctr[1:], 0, bg, s)
        self._ev("composite_loss", 0)
        self._ev("composite", 0)
        L.ngp_composite_loss(self.sigmas, self.ldr if self.use_exposure else self.rgbs, self.deltas, self.ts,
                             self.rays_a, R, rgb_gt, bg, self.loss_type,
                             self.lambda_opacity, self.lambda_depth, self.lambda_distortion, self.scale, 1e-4,
                             self.dsig, self.drgb, self.out_rgb, self.out_op, self.out_depth, self.out_loss,
                             self.n_active, None, None, None, self.stats, s)
        self._ev("composite", 1)
        # compacted gradient-carrying samples: scan + map (a per-block atomic reservation inside
        # composite_loss serialises on one address, and an ordered decoupled look-back across its
        # 2048 four-row blocks made the launch 5x longer: both measured slower)
        L.ngp_active_samples(self.n_active, self.rays_a, R, self.act_start, self.n_active_total, self.sample_idx, s)
        self._ev("composite_loss", 1)
        cs = torch.cuda.current_stream()
        hybrid = self.hash_backward != "atomic"
        binned = hybrid and self.bin_level_lo < self.grid.n_levels  # (hybrid at bin_level_lo == L: all atomic)
        bs = self.bwd_stream
        def plan(after=None):  # bucket plan of the binned fine levels (xyzs / sample_idx only) beside the MLP backward
            if after is None:
                bs.wait_stream(cs)
            else:
                bs.wait_event(after)
            with torch.cuda.stream(bs):
                L.ngp_hash_binned_plan(*self._listed[:5], *self._bin, vren._stream())  # (no dL/denc, no gradient)
                ev = torch.cuda.Event()
                ev.record(bs)
            return ev

        # capture order (the graph's queue assignment follows it; dependencies unchanged): the MLP
        # backward, then the plan forked from an event recorded before it; the binned accumulation, then
        # the coarse branch forked from an event after the MLP backward -- +0.8 % against the reverse
        # order (5 of 7 alternating pairs, profiles/r06/ab/capture_order.txt)
        planned = seg_done = None
        if binned:
            seg_done = torch.cuda.Event()
            seg_done.record(cs)
        if self.use_exposure:
            # dL/dldr -> dL/dlog-radiance in place over the gradient-carrying samples, the tonemappers'
            # gradient added into tone_grad; then the unit-exposure term (train.py:182-187).  After
            # seg_done: the bucket plan (sample_idx only) may run beside these too
            self._ev("tone_bwd", 0)
            L.ngp_tonemap_backward_indexed(self.rgbs, self.sample_exposure, self.cap, self.n_active_total,
                                           self.sample_idx, self.tone16, self.drgb, self.drgb, self.tone_grad,
                                           self._tone_ws, s)
            if self.unit_exposure_rgb is not None:
                L.ngp_unit_exposure_term(self.tone16, self.unit_exposure_rgb, self.tone_grad, self.out_loss_unit, s)
            self._ev("tone_bwd", 1)
        self._ev("mlp_bwd", 0)
        L.ngp_field_backward_mlp_act(self.dirs, self.cap, self.n_active_total, self.sample_idx, self.enc, self.cap,
                                     self.params16, self.dsig, self.drgb, self.denc, self.grad, self.rgb_act, s)
        self._ev("mlp_bwd", 1)
        if seg_done is not None:
            planned = plan(seg_done)
        if self.use_exposure and apply_adam:
            # the tonemappers' FusedAdam (one optimizer, one schedule with the field: train.py:139-151), on
            # this stream after their last reader of the step; it clears tone_grad
            L.ngp_adam_step_dev(self.tone_params, self.tone_grad, self.tone_exp_avg, self.tone_exp_avg_sq, self.tone16,
                                HG.TONE_PARAMS, *self._adam_hp, 1, s)
        if self.optimize_ext:
            self._pose_backward(*self._pose_args, apply_adam)
        if fork is not None and at == "mlp":
            marched = bool(fork())
        if self._segmented and hybrid:
            # (world > 1 graph segments: the hash backward runs as two more
            # graphs -- coarse levels on the side stream, binned levels here --
            # so the reduce-scatter of the [MLP | coarse] bucket overlaps the
            # binned levels; _replay / _dp_sequence / _segment_apply)
            cs.wait_stream(bs)
            return self.out_loss
        self._ev("hash_bwd", 0)
        if hybrid:
            # atomic coarse levels on the side stream and binned fine levels
            # (after the plan) here, side by side: disjoint gradient ranges
            split = HG.MLP_PARAMS + 2 * self.grid.offsets[self.bin_level_lo]
            # single process: the MLP + coarse levels' Adam right after them on the side stream
            # (no all-reduce orders it after the whole gradient), folding the coarse gradient
            # replicas itself; the binned levels' Adam inside their accumulation (fused_adam)
            adam_split = apply_adam and not self.dp
            fused = self.fused_adam and adam_split
            self._adam_hi = split if fused else self.n_params
            fold_in_adam = adam_split and self.rep_buf is not None

            # the next batch's round-1 pre-encode after the Adam below (only while levels 0-7 are all
            # stepped by that Adam: the binned levels' parameters change inside the accumulation)
            # (any fork point: the next batch's march is captured before this point)
            pre = (adam_split and self.pre_coarse and marched
                   and self._rows_fwd(self.chunk_first) and self.bin_level_lo >= self.pre_levels)
            def side(after=None):
                if after is None:
                    bs.wait_stream(cs)
                else:
                    bs.wait_event(after)
                if pre:
                    # its dependency on the next batch's march (done long before) taken by the coarse
                    # kernel, which waits on the main stream anyway (a second cross-queue wait on the
                    # pre-encode itself started it ~12 us after the Adam's end instead of ~7: r5tl / r5ii)
                    bs.wait_stream(self.march_stream)
                with torch.cuda.stream(bs):
                    self._ev("hash_bwd_coarse", 0)
                    self._coarse_levels(fold=not fold_in_adam)
                    self._ev("hash_bwd_coarse", 1)
                    if adam_split:
                        self._adam(0, split, vren._stream(), rep=fold_in_adam)
                        if pre:
                            # the next batch (marched beside this step) gets its round-1 coarse levels now
                            nx = self.msets[1 - self.cur]
                            L.ngp_field_encode_first_coarse(nx["xyzs"], nx["rays_a"], nx["rows_ne"], nx["n_rows_ne"], R,
                                                            self.cap, *self._field[:2], self.enc, vren._stream())
                            nx["pre_ready"] = True

            mlp_done = None
            if binned:
                mlp_done = torch.cuda.Event()
                mlp_done.record(cs)
            else:
                side()
            self._ev("hash_binned_apply", 0)
            t = HG.MLP_PARAMS
            if binned:  # (none at bin_level_lo == L: the side stream took every level and its Adam)
                cs.wait_event(planned)
                if fused:  # + FusedAdam of the binned levels inside the accumulation
                    L.ngp_hash_binned_apply_adam(*self._listed, *self._bin, self.params[t:], self.exp_avg[t:],
                                                 self.exp_avg_sq[t:], self.params16[t:], *self._adam_hp, s)
                else:
                    L.ngp_hash_binned_apply(*self._listed, *self._bin, s)
                    if adam_split:
                        self._adam(split, self.n_params, s)
            self._ev("hash_binned_apply", 1)
            if mlp_done is not None:
                side(mlp_done)
            cs.wait_stream(bs)
            if adam_split:
                self._ev("hash_bwd", 1)
                return self.out_loss
        else:
            L.ngp_hash_backward(*self._listed, s)
        self._ev("hash_bwd", 1)
        if not self.dp and apply_adam:
            self._ev("adam", 0)
            self._adam(0, self.n_params, s)
            self._ev("adam", 1)
        elif self.dp and not self._segmented:
            self._reduce_grads()
            if apply_adam:
                self._adam_shards()
                self._gather_params16()
        return self.out_loss

    # ------------------------------------------------- data parallel (ZeRO-1)
    def _reduce_grads(self):
        """Reduce-scatter (SUM) of each gradient bucket into this rank's shard
        buffers, then the local gradient is zeroed for the next step (RCCL over
        xGMI; outside graph captures).  apply_adam=False callers (tests) find
        the summed shards in _gshard."""
        for i in range(len(self.buckets)):
            self._reduce_bucket(i)
        self._gbuf.zero_()

    def _adam_shards(self):
        for i in range(len(self.buckets)):
            self._adam_shard(i, vren._stream())

    def _adam_shard(self, i, s, zero=False):
        """FusedAdam on this rank's shard of bucket i: fp32 master, moments
        and fp16 shadow of the shard, from the reduced gradient shard (the
        1/world mean folded in; the shard buffer zeroed).  zero: the launch
        also clears the bucket's local gradient."""
        args = self._bucket_host()[i]["adam"]
        if not zero:
            args = args[:-2] + (None, 0)
        self.L.ngp_adam_step_dev_zero(*args, s)

    def _gather_params16(self):
        """All-gather of the updated fp16 shadow the kernels read."""
        for i in range(len(self.buckets)):
            self._gather_bucket(i)

    def full_params(self):
        """The fp32 master vector, complete on every rank (world > 1: each rank
        updates only its shards; this all-gathers them -- checkpoints, tests)."""
        if self.world > 1:
            for (a, b), (lo, hi) in zip(self.buckets, self.shards):
                ddp.all_gather_(self._pbuf[a:b], self._pbuf[lo:hi].clone(), self.pg)
        return self.params

    def fused_params(self):
        """Parameters whose Adam runs inside the binned accumulation (the binned
        hash levels; single process, hybrid/binned backward), 0 otherwise."""
        if not (self.fused_adam and not self.dp and self.hash_backward != "atomic"):
            return 0
        return self.n_params - (HG.MLP_PARAMS + 2 * self.grid.offsets[self.bin_level_lo])

    def _adam(self, lo, hi, s, rep=False):
        """FusedAdam over params[lo:hi] (16-byte aligned bounds).  lr and the
        step count from device memory (graph replays); dctr[0] = steps taken
        so far, advanced after the step by ngp_counters_inc.  rep: the coarse
        levels' gradient replicas (unfolded, fold=False) are folded here
        (lo <= MLP_PARAMS, hi past the replicated levels)."""
        args = (*(t[lo:hi] for t in (self.params, self.grad, self.exp_avg, self.exp_avg_sq, self.params16)), hi - lo,
                *self._adam_hp, 1)
        if rep:
            self.L.ngp_adam_step_dev_rep(*args, self.rep_buf, HG.MLP_PARAMS - lo,
                                         2 * self.grid.offsets[self.coarse_rep_levels], self.coarse_rep, s)
        else:
            self.L.ngp_adam_step_dev(*args, s)

    def _field_indexed(self, s, idx=None, total=None, tone=True):
        """Field forward (encode + MLPs in one launch) over the listed samples
        idx[:total] (default eval_idx[:eval_total]); the pair-major encoding
        kept for the backward.  use_exposure: followed by the tonemappers over
        the same list (tone=False: the caller launches them)."""
        idx = self.eval_idx if idx is None else idx
        total = self.eval_total if total is None else total
        self._ev("hash_encode", 0)
        self.L.ngp_field_encode_mlp_act(self.xyzs, self.dirs, self.cap, total, idx, *self._field, self.enc, self.sigmas,
                                        self.rgbs, None, self.rgb_act, s)
        self._ev("hash_encode", 1)
        if self.use_exposure and tone:
            self._tonemap(s, total, idx)

    # ------------------------------------------------- tonemappers' state (use_exposure)
    def tone_state(self):
        """{'tonemapper_net_{0,1,2}.params': (2048) f32}: the tonemappers in the reference
        checkpoint's key layout (utils.tcnn_state_dict's entries for them), clones."""
        if not self.use_exposure:
            raise RuntimeError("tone_state needs a trainer built with use_exposure=True")
        from utils import TONE_KEYS
        n = HG.TONE_NET
        return {k: self.tone_params[n * i:n * (i + 1)].detach().clone() for i, k in enumerate(TONE_KEYS)}

    @torch.no_grad()
    def load_tone_params(self, tone):
        """Overwrite the tonemappers' fp32 master and fp16 shadow between steps: a flat (6144) tensor
        ([T_0 | T_1 | T_2]) or tone_state()'s dict."""
        if not self.use_exposure:
            raise RuntimeError("load_tone_params needs a trainer built with use_exposure=True")
        if isinstance(tone, dict):
            from utils import TONE_KEYS
            tone = torch.cat([tone[k].reshape(-1) for k in TONE_KEYS])
        if tone.numel() != HG.TONE_PARAMS:
            raise ValueError(f"the tonemappers hold {HG.TONE_PARAMS} values, got {tone.numel()}")
        self.tone_params.copy_(tone.reshape(-1).to(self.tone_params))
        self.tone16.copy_(self.tone_params.half())

    @torch.no_grad()
    def to_model(self):
        """The trainer's state as the drop-in model: an NGP of the trainer's mode holding params, the
        occupancy bitfield and, under use_exposure, tone_params (utils.tcnn_state_dict of it is the
        reference's checkpoint, tonemapper_net_i.params included)."""
        from models.networks import NGP
        if self.use_exposure:
            m = NGP(self.scale, 'None', False, use_exposure=True)
        else:
            m = NGP(self.scale, 'None' if self.use_raw_HDR else 'Sigmoid', self.use_raw_HDR)
        m = m.to(self.dev)
        m.params.copy_(self.full_params())
        m.density_bitfield.copy_(self.density_bitfield)
        if self.use_exposure:
            m.tone_params.copy_(self.tone_params)
        return m

    # ---------------------------------------------------- test-time render
    @torch.no_grad()
    def render(self, rays_o, rays_d, T_threshold=1e-4, max_samples=MAX_SAMPLES, bg=0.0, output_radiance=False,
               exposure=None):
        """__render_rays_test (models/rendering.py:162-253) on the native kernels.
        output_radiance: a raw-HDR trainer's relu radiance instead of the
        training-time leaky_relu (networks.py:152-157); no effect on a sigmoid one.
        use_exposure: the samples' log radiance tonemapped at `exposure` (None:
        1; one value; or one per ray (N_rays,) / (N_rays,1)), or with
        output_radiance exp(clamp(x, 0, 20)) (networks.py:158-163)."""
        act = HG.RGB_RELU if self.use_raw_HDR and output_radiance else self.rgb_act
        N_rays = rays_o.shape[0]
        dev = self.dev
        if exposure is not None and not self.use_exposure:
            raise ValueError("exposure= needs a trainer built with use_exposure=True")
        expo, n_expo = HG.tone_exposure(exposure, N_rays, rays_o.device) if self.use_exposure else (None, 0)
        _, hits_t, _ = vren.ray_aabb_intersect(rays_o, rays_d, self.center, self.half_size, 1)
        m = (hits_t[:, 0, 0] >= 0) & (hits_t[:, 0, 0] < NEAR_DISTANCE)
        hits_t[m, 0, 0] = NEAR_DISTANCE
        ht = hits_t[:, 0]
        opacity = torch.zeros(N_rays, device=dev)
        depth = torch.zeros(N_rays, device=dev)
        rgb = torch.zeros(N_rays, 3, device=dev)
        samples = total = 0
        alive = torch.arange(N_rays, device=dev)
        min_samples = 1 if self.esf == 0 else 4
        while samples < max_samples:
            N_alive = len(alive)
            if N_alive == 0:
                break
            Ns = max(min(N_rays // N_alive, 64), min_samples)
            samples += Ns
            xyzs, dirs, deltas, ts, neff = vren.raymarching_test(rays_o, rays_d, ht, alive, self.density_bitfield,
                                                                 self.cascades, self.scale, self.esf, self.G,
                                                                 MAX_SAMPLES, Ns)
            total += int(neff.sum())
            xyzs = xyzs.reshape(-1, 3)
            dirs = dirs.reshape(-1, 3)
            valid = ~torch.all(dirs == 0, dim=1)
            if valid.sum() == 0:
                break
            sig = torch.zeros(len(xyzs), device=dev)
            rgbs = torch.zeros(len(xyzs), 3, device=dev)
            sv, rv, _, _ = HG.field_forward(xyzs[valid].contiguous(), dirs[valid].contiguous(), self.grid,
                                            self.params16, save_enc=False, rgb_act=act)
            if self.use_exposure and output_radiance:
                rv = HG.tonemap_forward(rv, None, 0, None, HG.TONE_RADIANCE)
            elif self.use_exposure and n_expo > 1:  # each ray's exposure on its Ns samples
                e = expo[alive].repeat_interleave(Ns)[valid].contiguous()
                rv = HG.tonemap_forward(rv, e, rv.shape[0], self.tone16)
            elif self.use_exposure:
                rv = HG.tonemap_forward(rv, expo, n_expo, self.tone16)
            sig[valid] = sv
            rgbs[valid] = rv
            vren.composite_test_fw(sig.view(-1, Ns), rgbs.view(-1, Ns, 3), deltas, ts, ht, alive, T_threshold, neff,
                                   opacity, depth, rgb)
            alive = alive[alive >= 0].contiguous()
        rgb = rgb + bg * (1 - opacity)[:, None]
        return {"rgb": rgb, "opacity": opacity, "depth": depth, "total_samples": total}


def ctypes_float(x):  # (diagnostics; the declared c_float argtype converts the trainer's own floats)
    return HG.c_float(float(x))

