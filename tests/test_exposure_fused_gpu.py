"""NGPTrainer(use_exposure=True): the fused training step of the
exposure-conditioned model against the drop-in surface (NGP(use_exposure=True),
VolumeRenderer, NeRFLoss, the unit-exposure term) on the trainer's own marched
samples, its forward paths against each other, graph replays against eager
steps, the tonemappers' Adam against FusedAdam, a short training run against
the drop-in loop, and the render / export surface."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import hashgrid as HG
import synthetic as S
import tonemap_ref as T
import tonemap_step_ref as TS
import vren
from trainer import NGPTrainer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT_RGB = 0.73
DENSE_GAIN = 8.0


def _setup(R=512, table_init=0.2, seed=3, **kw):
    """tests/test_hdr_gpu.py's _hdr_setup for this mode, on the 64 x 64 analytic scene: a seeded hash
    table, the scene's bitfield, no occupancy update inside the step; per-ray exposures from
    tonemap_ref.EXPOSURES.  At table_init 2.0 the density net's second layer is scaled by DENSE_GAIN:
    a Xavier-initialised net on features of that size gives sigma = exp(h) with h ~ N(0, 0.6), far
    from the sigma > 30 a row of this scene (at most 0.3 long) needs to fall under T = 1e-4, so
    without the gain no row terminates early; with it about a fifth of the samples are that dense.
    At table_init 0.2 the field stays thin and rows carry gradient past their 64th sample."""
    sc = S.AnalyticScene(W=64, H=64, n_images=10)
    kw.setdefault("unit_exposure_rgb", UNIT_RGB)
    tr = NGPTrainer(scale=0.5, batch_size=R, device=DEV, seed=seed, use_exposure=True, **kw)
    with torch.no_grad():
        g = torch.Generator().manual_seed(11)
        tr.params[10240:] = ((torch.rand(tr.params.numel() - 10240, generator=g) * 2 - 1) * table_init).to(DEV)
        if table_init >= 2.0:
            tr.params[2048:3072] *= DENSE_GAIN
        tr.params16.copy_(tr.params.half())
    tr.density_bitfield.copy_(sc.bitfield.to(DEV))
    tr.global_step = 1
    gen = torch.Generator().manual_seed(seed)
    img, pix = sc.sample_batch(R, gen)
    noise = torch.rand(R, generator=gen)
    expo = torch.tensor(T.EXPOSURES)[torch.randint(len(T.EXPOSURES), (R,), generator=gen)]
    o, d = sc.rays(img, pix)
    batch = dict(img=img.to(DEV), pix=pix.to(DEV), noise=noise.to(DEV), expo=expo.to(DEV).contiguous(),
                 gt=sc.gt_rgb_rays(o, d).to(DEV), dirs=sc.directions.to(DEV), poses=sc.poses.to(DEV))
    return sc, tr, batch


def _step(tr, b, **kw):
    out = tr.step(b["img"], b["pix"], b["gt"], b["dirs"], b["poses"], noise=b["noise"], exposure=b["expo"], **kw)
    torch.cuda.synchronize()
    return out


def _rel(a, b):
    return float((a - b).norm() / b.norm())


# The bars of the one-step test.  The project's training-step bars (test_hdr_training_step_matches_oracle) are
# loss 1e-5 relative, out_rgb / out_op 1e-5, params gradient 1e-3 relative L2 per block, and tone_params against
# the drop-in's never above 1e-3.  Measured on an MI355X, both table initialisations: loss equal
# to the last printed digit (the two sides run the same kernels on the same samples and differ only in how the
# per-ray losses are summed), out_rgb 5.1e-7, out_op 6.0e-7, params gradient 3.7e-6 / 3.3e-7 / 9.2e-6, tone_params
# 1.2e-7 -- all under a tenth of those bars, so the test holds 4 x the measurement; for the loss, whose
# measurement is 0, 4 x the fp32 resolution of the sum it is compared through.
LOSS_REL, OUT_ABS, GRAD_REL = 2.0 ** -21, 2.4e-6, 3.7e-5
TONE_REL = 4.9e-7


@pytest.mark.parametrize("table_init", [0.2, 2.0])
def test_one_step_matches_the_drop_in_surface(table_init):
    from losses import NeRFLoss
    from models.custom_functions import VolumeRenderer
    sc, tr, b = _setup(table_init=table_init)
    assert tr.rgb_act == HG.RGB_NONE and tr.tone_params.shape == (HG.TONE_PARAMS,)
    loss = _step(tr, b, apply_adam=False)
    n, R = int(tr.n_samples.item()), tr.batch_size
    rays_a = tr.rays_a.clone()
    N, n_act = rays_a[:, 2], tr.n_active.long()
    # preconditions: rows run past their first 64 samples / terminate early; both ReLU branches are taken
    print(f"table_init {table_init}: {n} samples, longest row {int(N.max())}, rows carrying gradient past 64 samples "
          f"{int((n_act > 64).sum())}, rows terminated early {int((n_act < N).sum())}")
    assert int(N.max()) > 64
    assert int((n_act > 64).sum()) > 0 if table_init == 0.2 else int((n_act < N).sum()) > 0
    e_np = TS.expand_exposure(rays_a.cpu().numpy(), np.ones(n, np.float32), ray_exposure=b["expo"].cpu().numpy())
    e_s = torch.from_numpy(e_np).to(DEV)
    own = torch.from_numpy(TS.owned(rays_a.cpu().numpy(), n)).to(DEV)
    assert torch.equal(tr.sample_exposure[:n][own], e_s[own])
    # ---- the drop-in surface on the trainer's own marched samples
    model = tr.to_model()
    assert torch.equal(model._tone_shadow.get(), tr.tone16) and torch.equal(model._shadow.get(), tr.params16)
    sig, rgb = model(tr.xyzs[:n].contiguous(), tr.dirs[:n].contiguous(), exposure=e_s[:, None])
    _, opacity, depth, comp, _ = VolumeRenderer.apply(sig, rgb.contiguous(), tr.deltas[:n].contiguous(),
                                                      tr.ts[:n].contiguous(), rays_a, 1e-4)
    comp = (comp + torch.ones(3, device=DEV) * (1 - opacity)[:, None]).contiguous()
    loss_d = NeRFLoss(30, "raw", 0.5, 0.0, lambda_distortion=0.0)({"rgb": comp, "opacity": opacity, "depth": depth},
                                                                 {"rgb": b["gt"]})
    unit = model.log_radiance_to_rgb(torch.zeros(1, 3, device=DEV), exposure=torch.ones(1, 1, device=DEV))
    loss_d["unit_exposure"] = 0.5 * (unit - UNIT_RGB) ** 2
    l_ref = sum(v.mean() for v in loss_d.values())
    l_ref.backward()
    l_ref, l_gpu = float(l_ref.detach()), float(loss.sum() + tr.out_loss_unit[0])
    d_rgb = float((tr.out_rgb - comp.detach()).abs().max())  # (both indexed by ray)
    d_op = float((tr.out_op - opacity.detach()).abs().max())
    g_ref = model.params.grad
    rels = [_rel(tr.grad[lo:hi], g_ref[lo:hi]) for lo, hi in ((0, 3072), (3072, 10240), (10240, g_ref.numel()))]
    tone_rel = _rel(tr.tone_grad, model.tone_params.grad)
    print(f"loss {l_gpu:.6e} vs the drop-in's {l_ref:.6e}, relative {abs(l_gpu - l_ref) / abs(l_ref):.2e}; rgb max |diff| "
          f"{d_rgb:.2e}, opacity {d_op:.2e}; params gradient per block " + " / ".join(f"{r:.1e}" for r in rels) +
          f"; tone_params gradient {tone_rel:.2e} (|g| {float(tr.tone_grad.norm()):.3e})")
    assert abs(l_gpu - l_ref) <= LOSS_REL * abs(l_ref)
    assert d_rgb <= OUT_ABS and d_op <= OUT_ABS
    assert max(rels) < GRAD_REL, rels
    assert tone_rel <= TONE_REL and float(tr.tone_grad.abs().max()) > 0
    # ---- tone_params gradient, elementwise, against the fp64 restatement on the device's own inputs.  The step
    # turns its dL/dldr into dL/dlog_rad in place, so the compositing launch is repeated here on the step's own
    # buffers into scratch outputs: the same kernel on the same inputs, no atomics in dL/drgb
    dldr_dev = torch.full_like(tr.drgb, float("nan"))
    scratch = [torch.empty_like(t) for t in (tr.dsig, tr.out_rgb, tr.out_op, tr.out_depth, tr.out_loss)]
    n_act2 = torch.empty_like(tr.n_active)
    tr.L.ngp_composite_loss(tr.sigmas, tr.ldr, tr.deltas, tr.ts, tr.rays_a, R, b["gt"], tr.bg, tr.loss_type,
                            tr.lambda_opacity, tr.lambda_depth, tr.lambda_distortion, tr.scale, 1e-4, scratch[0],
                            dldr_dev, scratch[1], scratch[2], scratch[3], scratch[4], n_act2, None, None, None,
                            tr.stats.clone(), vren._stream())
    torch.cuda.synchronize()
    assert torch.equal(n_act2, tr.n_active) and torch.equal(scratch[4], loss) and torch.equal(scratch[1], tr.out_rgb)
    n_list = int(tr.n_active_total.item())
    idx = tr.sample_idx[:n_list].cpu().numpy()
    assert n_list == int(n_act.sum()) and len(np.unique(idx)) == n_list and idx.max() < n
    w = tr.tone16.float().cpu().numpy()
    x, dldr = tr.rgbs[:n].cpu().numpy(), dldr_dev[:n].cpu().numpy()
    ref = TS.backward_indexed(w, x, e_np, dldr, idx)
    _, g_unit, bar_unit = TS.unit_exposure(w, UNIT_RGB)
    err = np.abs(tr.tone_grad.double().cpu().numpy() - (ref["grad"] + g_unit))
    bar = ref["grad_bar"] + bar_unit + 1e-9
    A, _ = T.split(w.astype(np.float64))
    a = (x[idx].astype(np.float64) + np.log(e_np[idx].astype(np.float64))[:, None])[:, :, None] * A[None, :, :, 0] \
        + T.beta_of(A)[None]
    print(f"tone_params gradient over {n_list} listed samples: max err {err.max():.3e}, largest share of its bar "
          f"{(err / bar).max():.4f}; {ref['n_amb']} ambiguous pairs; hidden units on {float((a > 0).mean()):.2f}")
    assert bool((a > 0).any()) and bool((a <= 0).any())
    assert ref["n_amb"] <= T.AMBIGUOUS_CAP * a.size
    assert np.all(err <= bar)
    # dL/dlog_rad on the listed rows is what the restatement derives from dL/dldr
    dx = tr.drgb[:n].double().cpu().numpy()
    assert np.all(np.abs(dx[idx] - ref["dx"][idx]) <= ref["dx_bar"][idx] + 1e-12)


@pytest.mark.parametrize("table_init", [0.2, 2.0])
def test_forward_paths_agree(table_init):
    """Full forward, two chunked rounds and the row forward: loss / out_rgb / out_op and the tonemappers'
    gradient bit-identical (the same list, the same sums), the params gradient within 1e-5 relative L2,
    a second step repeats the first."""
    runs = []
    for chunk, rows in ((0, 0), (64, 0), (64, 1)):
        sc, tr, b = _setup(table_init=table_init)
        tr.chunk_first, tr.row_forward = chunk, rows
        loss = _step(tr, b, apply_adam=False)
        out = (loss.clone(), tr.out_rgb.clone(), tr.out_op.clone(), tr.tone_grad.clone(), tr.out_loss_unit.clone(),
               tr.grad.clone())
        assert float(tr.tone_grad.abs().max()) > 0 and bool(torch.isfinite(tr.tone_grad).all())
        tr.grad.zero_()
        tr.tone_grad.zero_()
        loss2 = _step(tr, b, apply_adam=False)
        assert torch.equal(loss2, out[0]) and torch.equal(tr.out_rgb, out[1]) and torch.equal(tr.out_op, out[2])
        assert torch.equal(tr.tone_grad, out[3]) and torch.equal(tr.out_loss_unit, out[4])
        if rows:  # the row forward did cut rows at 64 (and, the thin field, left round 2 some of them)
            assert int(table_init == 0.2) <= int(tr.eval_total2.item()) < int(tr.n_samples.item())
        runs.append(out)
    for other in runs[1:]:
        for k in range(5):
            assert torch.equal(runs[0][k], other[k]), k
        assert _rel(other[5], runs[0][5]) < 1e-5


def test_fused_adam_steps_the_tonemappers_bit_for_bit():
    from optimizers import FusedAdam
    sc, tr, b = _setup(table_init=2.0)
    t0 = tr.tone_params.clone()
    _step(tr, b, apply_adam=False)
    g = tr.tone_grad.clone()
    assert float(g.abs().max()) > 0
    tr.grad.zero_()
    tr.tone_grad.zero_()
    _step(tr, b, apply_adam=True)
    p = torch.nn.Parameter(t0.clone())
    p.grad = g
    opt = FusedAdam([p], tr.lr0, eps=1e-15)
    opt.step()
    st = opt.state[p]
    assert not torch.equal(tr.tone_params, t0)
    assert torch.equal(tr.tone_params, p.detach()) and torch.equal(tr.tone16, st["half"])
    assert torch.equal(tr.tone_exp_avg, st["exp_avg"]) and torch.equal(tr.tone_exp_avg_sq, st["exp_avg_sq"])
    assert torch.equal(tr.tone16, tr.tone_params.half())
    assert bool((tr.tone_grad == 0).all()) and bool((tr.grad == 0).all())


# ------------------------------------------------------------ the data of scripts/train_exposure.py
def _train_exposure_module():
    spec = importlib.util.spec_from_file_location("train_exposure", os.path.join(ROOT, "scripts", "train_exposure.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def exposure_data():
    TE = _train_exposure_module()
    data = TE.synthetic_data(res=64, n_train=12, n_test=2, device=DEV)
    assert data.train_rays.shape == (36, 4096, 4) and data.test_rays.shape == (4, 4096, 4)
    return TE, data


def test_steady_state_steps_replay_graphs_and_follow_the_table(exposure_data):
    """Two eager trainers and a graph-replaying one (pair_steps on) from one seed: the replayed run is
    as close to an eager run as a second eager run is (test_trainer_gpu.py's bar for replayed pairs
    against single steps: float atomics make any two runs differ); the graphs stop growing; another
    table captures anew and is the one the step reads."""
    TE, data = exposure_data
    outs = []
    for graphs in (False, False, True):
        lp = TE.FusedLoop(data, batch=1024, seed=3, warmup_steps=16, use_graphs=graphs, pair_steps=graphs)
        tr = lp.tr
        losses = []
        for it in range(96):
            losses.append(float(lp.step()[0].mean()))
            if it == 79:
                n_graphs = len(tr._graphs)
        tr.drain()
        torch.cuda.synchronize()
        assert all(np.isfinite(losses)) and bool(torch.isfinite(tr.tone_params).all())
        outs.append((tr.params.clone(), tr.tone_params.clone(), sum(losses[-20:]) / 20))
        if not graphs:
            assert len(tr._graphs) == 0
            continue
        assert len(tr._graphs) == n_graphs >= 2 and any(k[0] == "pair" for k in tr._graphs)
        assert tr.global_step == 96 and int(tr.dctr[0]) == 96 + int(tr._ran_ahead)
        assert not torch.equal(tr.tone_params, HG.init_tone_params(torch.Generator().manual_seed(4)).to(DEV))
        # a second table at another address: captured anew, and read
        while tr._ran_ahead:
            lp.step()
        other = torch.full_like(lp.table, 8.0)
        before = len(tr._graphs)
        for _ in range(2):  # (the second of a pair, if the first call ran two steps)
            tr.train_step(lp.gt, lp.dirs, lp.poses, exposure=other)
        torch.cuda.synchronize()
        assert len(tr._graphs) > before
        rays_a = tr.rays_a.cpu().numpy()
        own = torch.from_numpy(TS.owned(rays_a, int(tr.n_samples.item()))).to(DEV)
        assert int(own.sum()) > 0 and bool((tr.sample_exposure[:own.numel()][own] == 8.0).all())
        if tr._ran_ahead:
            with pytest.raises(RuntimeError, match="pair_steps"):
                tr.train_step(lp.gt, lp.dirs, lp.poses, exposure=lp.table)
    (pa, ta, la), (pb, tb, lb), (pg, tg, lg) = outs
    noise, tnoise = float((pb - pa).norm()), float((tb - ta).norm())
    print(f"replayed vs eager {float((pg - pa).norm()):.3f} (tone {float((tg - ta).norm()):.4f}), eager vs eager "
          f"{noise:.3f} (tone {tnoise:.4f}); losses {la:.5f} {lb:.5f} {lg:.5f}")
    assert float((pg - pa).norm()) <= 3 * noise + 1e-3 * float(pa.norm())
    assert float((tg - ta).norm()) <= 3 * tnoise + 1e-3 * float(ta.norm())
    assert abs(lg - la) <= 0.1 * abs(la) + 3 * abs(lb - la)


# Seed-to-seed spread of the drop-in loop's held-out PSNR on this very run (0.62 dB over three
# seeds); the fused step may sit at most twice that below the drop-in loop, and at least 5 dB above the 20.7 dB
# §18 measured with the exposure held at 1.
MARGIN_DB = 1.25
BLIND_DB = 20.7
TRAIN_STEPS = 300


def test_short_training_run_matches_the_drop_in_loop(exposure_data):
    TE, data = exposure_data
    psnr = {}
    for name, make in (("dropin", lambda: TE.ExposureLoop(data, batch=1024, seed=4)),
                       ("fused", lambda: TE.FusedLoop(data, batch=1024, seed=4))):
        loop = make()
        for _ in range(TRAIN_STEPS):
            loss, _ = loop.step()
        assert bool(torch.isfinite(loss).all())
        per = loop.test_psnr()
        assert sorted(per) == [0.5, 2.0]
        psnr[name] = sum(per.values()) / len(per)
        if name == "fused":
            assert len(loop.tr._graphs) >= 1 and loop.tr.global_step == TRAIN_STEPS
    print(f"held-out PSNR after {TRAIN_STEPS} steps: fused {psnr['fused']:.2f} dB, drop-in loop {psnr['dropin']:.2f} dB "
          f"(margin {MARGIN_DB:.2f} dB); exposure-blind (DESIGN.md §18) {BLIND_DB:.1f} dB")
    assert psnr["fused"] >= psnr["dropin"] - MARGIN_DB
    assert psnr["fused"] >= BLIND_DB + 5


# ------------------------------------------------------------ the surface around the step
def test_render_and_export_agree_with_the_drop_in_model(exposure_data, tmp_path):
    from models.networks import NGP
    from models.rendering import render
    from utils import load_ckpt, tcnn_state_dict
    TE, data = exposure_data
    lp = TE.FusedLoop(data, batch=1024, seed=5, warmup_steps=16)
    for _ in range(40):
        lp.step()
    tr = lp.tr
    tr.drain()
    rays_o, rays_d = lp.get_rays(data.directions, data.test_poses[0])
    rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
    model = tr.to_model()
    n = rays_o.shape[0]
    with torch.no_grad():
        for e in (0.5, 4.0):
            ex = torch.tensor([e], device=DEV)
            mine = tr.render(rays_o, rays_d, exposure=ex)
            ref = render(model, rays_o, rays_d, test_time=True, exposure=ex)
            assert float(mine["opacity"].max()) > 0.05
            assert float((mine["rgb"] - ref["rgb"]).abs().max()) <= 1e-5
            assert float((mine["opacity"] - ref["opacity"]).abs().max()) <= 1e-5
            per_ray = tr.render(rays_o, rays_d, exposure=torch.full((n,), e, device=DEV))
            assert torch.equal(per_ray["rgb"], mine["rgb"])
        half = torch.where(torch.arange(n, device=DEV) % 2 == 0, 0.5, 4.0)
        mixed = tr.render(rays_o, rays_d, exposure=half)["rgb"]
        lo, hi = tr.render(rays_o, rays_d, exposure=0.5)["rgb"], tr.render(rays_o, rays_d, exposure=4.0)["rgb"]
        assert torch.equal(mixed[0::2], lo[0::2]) and torch.equal(mixed[1::2], hi[1::2]) and not torch.equal(lo, hi)
        rad = tr.render(rays_o, rays_d, output_radiance=True)
        rad_ref = render(model, rays_o, rays_d, test_time=True, output_radiance=True)
        scale = float(rad_ref["rgb"].abs().max())
        assert float((rad["rgb"] - rad_ref["rgb"]).abs().max()) <= 1e-5 * max(scale, 1.0)
        assert torch.equal(tr.render(rays_o, rays_d)["rgb"], tr.render(rays_o, rays_d, exposure=1.0)["rgb"])
    # export: the reference checkpoint's keys, and the way back
    state = tr.tone_state()
    sd = tcnn_state_dict(model)
    assert sorted(state) == [f"tonemapper_net_{i}.params" for i in range(3)]
    for k, v in state.items():
        assert v.shape == (2048,) and torch.equal(sd[k], v)
    path = str(tmp_path / "fused_exposure.ckpt")
    torch.save({"state_dict": {"model." + k: v.cpu() for k, v in sd.items()}}, path)
    dst = NGP(0.5, 'None', False, seed=9, use_exposure=True)
    load_ckpt(dst, path)
    assert torch.equal(dst.tone_params.detach().to(DEV), tr.tone_params)
    assert torch.equal(dst.params.detach().to(DEV), tr.params)
    tr2 = NGPTrainer(scale=0.5, batch_size=256, sample_capacity=256 * 64, device=DEV, seed=1, use_exposure=True)
    assert not torch.equal(tr2.tone_params, tr.tone_params)
    tr2.load_tone_params(state)
    assert torch.equal(tr2.tone_params, tr.tone_params) and torch.equal(tr2.tone16, tr.tone16)
    tr2.load_tone_params(torch.zeros(HG.TONE_PARAMS))
    assert bool((tr2.tone_params == 0).all()) and bool((tr2.tone16 == 0).all())
    with pytest.raises(ValueError, match="6144"):
        tr2.load_tone_params(torch.zeros(5))


def test_refusals_and_the_off_state():
    with pytest.raises(ValueError, match="raw-HDR"):
        NGPTrainer(use_exposure=True, use_raw_HDR=True, device=DEV)
    with pytest.raises(NotImplementedError, match="pose gradient"):
        NGPTrainer(use_exposure=True, optimize_ext=True, device=DEV)
    with pytest.raises(NotImplementedError, match="ZeRO-1 bucket"):
        NGPTrainer(use_exposure=True, emulate_dp=2, device=DEV)
    off = NGPTrainer(scale=0.5, batch_size=256, sample_capacity=256 * 64, device=DEV)
    assert off.use_exposure is False and off.tone_params is None and off.unit_exposure_rgb is None
    for name in ("ldr", "tone16", "tone_grad", "sample_exposure", "out_loss_unit"):
        assert not hasattr(off, name), name
    assert "sample_exposure" not in off.msets[0]
    for fn in (off.tone_state, lambda: off.load_tone_params(torch.zeros(HG.TONE_PARAMS))):
        with pytest.raises(RuntimeError, match="use_exposure"):
            fn()
    sc, tr, b = _setup(R=256, sample_capacity=256 * 64)
    with pytest.raises(ValueError, match="exposure"):
        off.step(b["img"], b["pix"], b["gt"], b["dirs"], b["poses"], exposure=b["expo"])
    with pytest.raises(ValueError, match="exposure"):
        tr.step(b["img"], b["pix"], b["gt"], b["dirs"], b["poses"])  # the mode needs one
    with pytest.raises(ValueError, match="exposure"):
        tr.step(b["img"], b["pix"], b["gt"], b["dirs"], b["poses"], exposure=b["expo"][:-1].contiguous())
    with pytest.raises(ValueError, match="exposure"):
        tr.train_step(sc.gt_images(device=DEV), b["dirs"], b["poses"], exposure=torch.ones(3, device=DEV))
    with pytest.raises(ValueError, match="exposure"):
        off.render(torch.zeros(4, 3, device=DEV), torch.ones(4, 3, device=DEV), exposure=2.0)
