// Fused compositing + NeRF loss + compositing backward of the training step
// (one wave per ray), and the drop-in surface's NeRFLoss forward / backward.
// Replaces (train.py:174-200, losses.py:41-82, volumerendering.cu:5-150,
// losses.cu:8-140, models/rendering.py:287-296).
#pragma clang fp contract(off)

#include "common.h"
#include "transmittance.h"
#include "wave.h"

namespace ngp {

// ------------------------------------------------------ composite + loss
// One wave per ray.  Pass 1 = composite_train_fw (volumerendering.cu:5-44),
// the transmittance chain walked sample by sample in lane order (readlane)
// with the reference's early break;
// then the background blend (models/rendering.py:287-296) and NeRFLoss
// (losses.py:63-82: rgb loss of type `loss_type`, opacity entropy, depth
// term, distortion term when lambda_distortion > 0) with its analytic
// gradient; pass 2 = composite_train_bw (volumerendering.cu:86-150) with
// dL/dws from the distortion loss (DistortionLoss fw / bw, losses.cu:8-140,
// over the ray's composited samples: the others have ws = 0 and the
// compositing backward stops at the termination anyway).
// Per-ray outputs: rgb (after bg), opacity, depth, loss contribution
// (already divided by the batch means' denominators).
struct LossArgs {
    int loss_type;  // 0 raw (default, opt.py:34), 1 mse (upstream ngp_pl), 2 log, 3 tanh
    float lambda_opacity, lambda_depth, depth_scale, inv_n_rays, T_thr;
    float lambda_dist;  // losses.py:77-80 (0: off, the default)
};

__device__ __forceinline__ void rgb_loss(int type, float x, float y, float& l, float& dldx) {
    switch (type) {
        case 0: {  // (x - y)/(x.detach() + 1e-3), squared
            const float den = x + 1e-3f, d = (x - y) / den;
            l = d * d; dldx = 2.f * d / den; break;
        }
        case 1: { const float d = x - y; l = d * d; dldx = 2.f * d; break; }
        case 2: {
            const float u = logf((0.2935f + x) / (0.2935f + y)) * 0.7607f;
            l = u * u; dldx = 2.f * u * 0.7607f / (0.2935f + x); break;
        }
        default: {
            const float tx = tanhf(x), u = tx - tanhf(y);
            l = u * u; dldx = 2.f * u * (1.f - tx * tx); break;
        }
    }
}

// (wave_sum / wave_incl_scan: wave.h, the reference's per-ray serial sums in a fixed reassociated order;
// ChunkT / chunk_transmittance: transmittance.h, shared with the field forward)

// One row of rays_a on one wave; returns the composited sample count
// (vr_samples' share of this ray) and, in na_out, the samples that carry
// gradient (up to and including the terminating one).  DIST: the distortion
// loss is on (lambda_dist != 0; its code and registers are left out otherwise).
template <bool DIST>
__device__ __forceinline__ int64_t composite_loss_ray(
    int64_t n, const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ deltas,
    const float* __restrict__ ts, const int64_t* __restrict__ rays_a, const float* __restrict__ gt,
    const float* __restrict__ bg, const LossArgs& la, float* __restrict__ dL_dsig, float* __restrict__ dL_drgbs,
    float* __restrict__ out_rgb, float* __restrict__ out_op, float* __restrict__ out_depth,
    float* __restrict__ out_loss, int32_t* __restrict__ n_active, int64_t& na_out) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = rays_a[3 * n], start = rays_a[3 * n + 1], N = rays_a[3 * n + 2];
    // The first two 64-sample chunks (most rows terminate within them) are
    // loaded together up front and kept in registers for the backward: two
    // memory round trips per row instead of one per chunk and pass.
    struct Chunk {
        float sg, dl, cr, cg, cb, tt, w, Ta;
    };
    auto load = [&](int64_t k0, Chunk& c) {
        const int64_t s = start + k0 + lane;
        c.sg = c.dl = c.cr = c.cg = c.cb = c.tt = 0.f;
        if (k0 + lane < N) {
            c.sg = sigmas[s]; c.dl = deltas[s]; c.tt = ts[s];
            c.cr = rgbs[3 * s]; c.cg = rgbs[3 * s + 1]; c.cb = rgbs[3 * s + 2];
        }
    };
    Chunk c0, c1;
    load(0, c0);
    if (N > 64) load(64, c1);
    // ---- forward
    float T = 1.0f, R = 0.f, G = 0.f, B = 0.f, D = 0.f, O = 0.f;
    int64_t samples = 0, na = 0;
    bool done = false;
    auto fw_chunk = [&](int64_t k0, Chunk& c) {
        const int cnt = (int)(N - k0 < 64 ? N - k0 : 64);
        const float a = 1.0f - __expf(-c.sg * c.dl);
        const float om = 1.0f - a;
        const ChunkT ct = chunk_transmittance(om, cnt, T, la.T_thr, lane);
        const int stop = ct.stop;
        if (ct.hit) done = true;
        T = __shfl(ct.Tn, stop - 1, 64);
        const bool act = lane < stop;
        c.w = act ? a * ct.Tk : 0.f;
        c.Ta = ct.Tk * om;
        R += wave_sum(c.w * c.cr); G += wave_sum(c.w * c.cg); B += wave_sum(c.w * c.cb);
        D += wave_sum(c.w * c.tt); O += wave_sum(c.w);
        samples += done ? stop - 1 : stop;
        na += stop;
    };
    fw_chunk(0, c0);
    if (!done && N > 64) fw_chunk(64, c1);
    if (!done && N > 128) {  // long rows: the next chunk in flight while one is composited; w / T spilled
        Chunk c;
        load(128, c);
        for (int64_t k0 = 128; k0 < N && !done; k0 += 64) {
            Chunk nx;
            if (k0 + 64 < N) load(k0 + 64, nx);
            fw_chunk(k0, c);
            const int64_t s = start + k0 + lane;
            if (k0 + lane < N) { dL_drgbs[3 * s] = c.w; dL_drgbs[3 * s + 1] = c.Ta; }
            c = nx;
        }
    }
    // ---- background + loss (wave-uniform)
    const float bgc[3] = {bg[0], bg[1], bg[2]};
    const float xc[3] = {R + bgc[0] * (1 - O), G + bgc[1] * (1 - O), B + bgc[2] * (1 - O)};
    float loss = 0.f, g[3], gop = 0.f;
    const float inv3n = la.inv_n_rays / 3.0f;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        float l, d;
        rgb_loss(la.loss_type, xc[q], gt[3 * ray + q], l, d);
        loss += l * inv3n;
        g[q] = d * inv3n;
        gop -= g[q] * bgc[q];
    }
    const float o = O + 1e-10f;
    loss += la.lambda_opacity * (-o * logf(o)) * la.inv_n_rays;
    gop += la.lambda_opacity * (-(logf(o) + 1.f)) * la.inv_n_rays;
    float gdep = 0.f;
    if (la.lambda_depth != 0.f) {
        const float v = D / la.depth_scale + 1e-10f;
        loss += -la.lambda_depth * logf(fminf(v, 1.0f)) * la.inv_n_rays;
        // (torch's clip(max=1) passes the gradient at v == 1 too, as nerf_loss_bw_kernel does)
        if (v <= 1.0f) gdep = -la.lambda_depth / v / la.depth_scale * la.inv_n_rays;
    }
    // ---- distortion loss (losses.py:77-80): its forward over the composited
    // samples (W_tot = O, WT_tot = D are the ray's sums of ws and ws*ts) and
    // dL/dws per sample (losses.cu:110-140); the ray's sum of dL/dws * ws is
    // needed before the compositing backward's first sample: a pass of its own.
    // Rows longer than two chunks park dL/dws in dL_dsig[s] (overwritten by
    // pass 2 after it is read).
    float gws_c[2] = {0.f, 0.f}, S_ws = 0.f;
    if (DIST) {
        const float gd2 = (la.lambda_dist * la.inv_n_rays) * 2;
        float cw = 0.f, cwt = 0.f, ld = 0.f;
        auto dist_chunk = [&](int64_t k0, const Chunk& c) {
            const int cnt = (int)(na - k0 < 64 ? na - k0 : 64);
            const bool in = lane < cnt;
            const float w = in ? c.w : 0.f, wt = w * c.tt;
            const float a = cw + wave_incl_scan(w, lane), b = cwt + wave_incl_scan(wt, lane);
            const float we = a - w, wte = b - wt;  // exclusive sums (the reference's serial fold values)
            const float l = 2 * (b * we - a * wte) + ((w * (1.0f / 3)) * w) * c.dl;
            ld += wave_sum(in ? l : 0.f);
            const float A = c.tt * we - wte, Bv = (D - b) - c.tt * (O - a);
            const float gw = in ? gd2 * (A + Bv) + ((gd2 / 3.0f) * w) * c.dl : 0.f;
            S_ws += wave_sum(gw * w);
            cw = __shfl(a, 63, 64); cwt = __shfl(b, 63, 64);
            return gw;
        };
        if (na > 0) gws_c[0] = dist_chunk(0, c0);
        if (na > 64) gws_c[1] = dist_chunk(64, c1);
        for (int64_t k0 = 128; k0 < na; k0 += 64) {
            Chunk c;
            load(k0, c);
            const int64_t s = start + k0 + lane;
            c.w = 0.f;
            if (k0 + lane < na) c.w = dL_drgbs[3 * s];
            const float gw = dist_chunk(k0, c);
            if (k0 + lane < na) dL_dsig[s] = gw;
        }
        loss += la.lambda_dist * ld * la.inv_n_rays;
    }
    if (lane == 0) {
        out_rgb[3 * ray] = xc[0]; out_rgb[3 * ray + 1] = xc[1]; out_rgb[3 * ray + 2] = xc[2];
        out_op[ray] = O;
        out_depth[ray] = D;
        out_loss[ray] = loss;
        if (n_active) n_active[n] = (int32_t)na;
    }
    na_out = na;
    // ---- backward over the na composited samples
    const float gs = gop * (1 - O);
    float rc = 0.f, gc = 0.f, bc = 0.f, dc = 0.f, wc = 0.f;
    auto bw_chunk = [&](int64_t k0, const Chunk& c, float gw) {
        const int cnt = (int)(na - k0 < 64 ? na - k0 : 64);
        const bool in = lane < cnt;
        const int64_t s = start + k0 + lane;
        const float w = in ? c.w : 0.f, Ta = c.Ta;
        const float pr = rc + wave_incl_scan(w * c.cr, lane), pg = gc + wave_incl_scan(w * c.cg, lane);
        const float pb = bc + wave_incl_scan(w * c.cb, lane), pd = dc + wave_incl_scan(w * c.tt, lane);
        float ws_term = 0.f;
        if (DIST) {  // + T g_ws - (S - prefix(g_ws ws)) (volumerendering.cu:138-146)
            const float pw = wc + wave_incl_scan(in ? gw * w : 0.f, lane);
            ws_term = Ta * gw - (S_ws - pw);
            wc = __shfl(pw, 63, 64);
        }
        if (in) {
            dL_drgbs[3 * s] = g[0] * w; dL_drgbs[3 * s + 1] = g[1] * w; dL_drgbs[3 * s + 2] = g[2] * w;
            dL_dsig[s] = c.dl * (g[0] * (c.cr * Ta - (R - pr)) + g[1] * (c.cg * Ta - (G - pg)) +
                                 g[2] * (c.cb * Ta - (B - pb)) + gs + gdep * (c.tt * Ta - (D - pd)) + ws_term);
        }
        rc = __shfl(pr, 63, 64); gc = __shfl(pg, 63, 64); bc = __shfl(pb, 63, 64); dc = __shfl(pd, 63, 64);
    };
    if (na > 0) bw_chunk(0, c0, gws_c[0]);
    if (na > 64) bw_chunk(64, c1, gws_c[1]);
    for (int64_t k0 = 128; k0 < na; k0 += 64) {
        Chunk c;
        load(k0, c);
        const int64_t s = start + k0 + lane;
        c.w = 0.f; c.Ta = 0.f;
        float gw = 0.f;
        if (k0 + lane < na) {
            c.w = dL_drgbs[3 * s]; c.Ta = dL_drgbs[3 * s + 1];
            if (DIST) gw = dL_dsig[s];
        }
        bw_chunk(k0, c, gw);
    }
    return samples;
}

// Each block takes 4 rows per round (one per wave).  Per round the block
// sums its rows' gradient-carrying sample counts and reserves that many
// entries of sample_idx with ONE atomic on alloc[0]; each wave then writes
// its row's entries (start + k, k < na) -- a row's samples stay contiguous,
// which the hash backward's run merging relies on.  The last block to finish
// (alloc[1] ticket) publishes the total to *n_active_total and resets both
// counters, so the kernel needs no memset and no scan launch.  stats
// (nullable): [0] += marched samples, [1] += composited samples (vr_samples),
// [2] += gradient-carrying samples, summed per block in LDS, then one atomic
// per counter per block into stripe blockIdx % NGP_STAT_STRIPES (one address
// for all 2048 blocks serialised ~40 us of the kernel on the memory side).
template <bool DIST>
__global__ void __launch_bounds__(256) composite_loss_wave_kernel(
    const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ deltas,
    const float* __restrict__ ts, const int64_t* __restrict__ rays_a, int64_t n_rays, const float* __restrict__ gt,
    const float* __restrict__ bg, LossArgs la, float* __restrict__ dL_dsig, float* __restrict__ dL_drgbs,
    float* __restrict__ out_rgb, float* __restrict__ out_op, float* __restrict__ out_depth,
    float* __restrict__ out_loss, int32_t* __restrict__ n_active, int32_t* __restrict__ sample_idx,
    unsigned long long* __restrict__ alloc, int64_t* __restrict__ n_active_total, int64_t* __restrict__ stats) {
    __shared__ unsigned long long blk[3];
    __shared__ int64_t s_na[4];
    __shared__ unsigned long long s_base;
    NGP_PROBE_BEGIN(NGP_P_COMPOSITE);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x < 3) blk[threadIdx.x] = 0;
    __syncthreads();
    int64_t rm = 0, vr = 0, act = 0;
    for (int64_t r0 = (int64_t)blockIdx.x * 4; r0 < n_rays; r0 += (int64_t)gridDim.x * 4) {
        const int64_t n = r0 + wid;
        int64_t na = 0, start = 0;
        if (n < n_rays) {
            vr += composite_loss_ray<DIST>(n, sigmas, rgbs, deltas, ts, rays_a, gt, bg, la, dL_dsig, dL_drgbs, out_rgb,
                                     out_op, out_depth, out_loss, n_active, na);
            start = rays_a[3 * n + 1];
            rm += rays_a[3 * n + 2];
            act += na;
        }
        if (sample_idx) {
            if (lane == 0) s_na[wid] = na;
            __syncthreads();
            if (threadIdx.x == 0) {
                const int64_t tot = s_na[0] + s_na[1] + s_na[2] + s_na[3];
                s_base = tot ? atomicAdd(alloc, (unsigned long long)tot) : 0ull;
            }
            __syncthreads();
            int64_t off = (int64_t)s_base;
            for (int w = 0; w < wid; ++w) off += s_na[w];
            for (int64_t k = lane; k < na; k += 64) sample_idx[off + k] = (int32_t)(start + k);
            __syncthreads();  // s_na / s_base are rewritten next round
        }
    }
    if (lane == 0) {
        atomicAdd(&blk[0], (unsigned long long)rm);
        atomicAdd(&blk[1], (unsigned long long)vr);
        atomicAdd(&blk[2], (unsigned long long)act);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (stats) {
            unsigned long long* st = (unsigned long long*)stats + (blockIdx.x % NGP_STAT_STRIPES) * NGP_STAT_STRIDE;
            if (blk[0]) atomicAdd(st, blk[0]);
            if (blk[1]) atomicAdd(st + 1, blk[1]);
            if (blk[2]) atomicAdd(st + 2, blk[2]);
        }
        if (sample_idx) {
            __threadfence();
            const unsigned long long ticket = atomicAdd(alloc + 1, 1ull);
            if (ticket == gridDim.x - 1) {  // last block: every reservation is done
                const unsigned long long total = atomicExch(alloc, 0ull);
                atomicExch(alloc + 1, 0ull);
                *n_active_total = (int64_t)total;
            }
        }
    }
    NGP_PROBE_END();
}

}  // namespace ngp

using namespace ngp;

// NeRFLoss (losses.py:41-82) of the drop-in surface in one launch each way:
// the per-ray terms {rgb (3), opacity, depth} the reference builds from ~15
// elementwise torch ops, and their backward, one lane per ray, each op of the
// reference's expression rounded in fp32 in its order (x.detach() in the rgb
// denominator carries no gradient; division by the grid scale is torch's
// multiplication by its reciprocal; clip's gradient is 0 where it clips).
// One deliberate exception: the log loss's backward divides (g 0.7607) by a =
// 0.2935 + x once, where autograd divides by (a / b) and then by b -- the same
// value to within a few fp32 roundings (tests/composite_ref.py bounds both), not the
// same bits.
// loss_type 0 raw, 2 log, 3 tanh (the reference's set).
__device__ __forceinline__ float nerf_rgb_term(int type, float x, float y, float& dtdx) {
    if (type == 0) {
        const float den = x + 1e-3f;
        dtdx = 1.0f / den;  // (only used as grad / den below)
        return (x - y) / den;
    }
    if (type == 2) {
        const float a = 0.2935f + x;
        dtdx = a;
        return logf(a / (0.2935f + y)) * 0.7607f;
    }
    const float tx = tanhf(x);
    dtdx = tx;
    return tx - tanhf(y);
}

__global__ void __launch_bounds__(256) nerf_loss_fw_kernel(const float* __restrict__ rgb, const float* __restrict__ gt,
                                                           const float* __restrict__ opacity,
                                                           const float* __restrict__ depth, int64_t n, int type,
                                                           float lam_op, float neg_lam_depth, float inv_scale,
                                                           float* __restrict__ l_rgb, float* __restrict__ l_op,
                                                           float* __restrict__ l_dep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float dd;
        const float t = nerf_rgb_term(type, rgb[3 * i + c], gt[3 * i + c], dd);
        l_rgb[3 * i + c] = t * t;
    }
    const float o = opacity[i] + 1e-10f;
    l_op[i] = lam_op * (-o * logf(o));
    const float v = fminf(depth[i] * inv_scale + 1e-10f, 1.0f);
    l_dep[i] = neg_lam_depth * logf(v);
}

// (g_*: dL/d of each loss term; null = no gradient flows into that term)
__global__ void __launch_bounds__(256) nerf_loss_bw_kernel(const float* __restrict__ rgb, const float* __restrict__ gt,
                                                           const float* __restrict__ opacity,
                                                           const float* __restrict__ depth, int64_t n, int type,
                                                           float lam_op, float neg_lam_depth, float inv_scale,
                                                           const float* __restrict__ g_rgb,
                                                           const float* __restrict__ g_op,
                                                           const float* __restrict__ g_dep, float* __restrict__ d_rgb,
                                                           float* __restrict__ d_op, float* __restrict__ d_dep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float g = 0.f;
        if (g_rgb) {
            const float x = rgb[3 * i + c];
            float dd;
            const float t = nerf_rgb_term(type, x, gt[3 * i + c], dd);
            const float gt2 = g_rgb[3 * i + c] * (2.0f * t);  // PowBackward: grad * (2 t)
            if (type == 0) g = gt2 / (x + 1e-3f);              // DivBackward (the denominator detached)
            else if (type == 2) g = (gt2 * 0.7607f) / dd;       // MulBackward, LogBackward of (a / b): 1 / a
            else g = gt2 * (1.0f - dd * dd);                    // TanhBackward
        }
        d_rgb[3 * i + c] = g;
    }
    float go = 0.f;
    if (g_op) {
        const float o = opacity[i] + 1e-10f, lo = logf(o);
        const float gl = g_op[i] * lam_op;  // MulBackward of lam * f
        // f = (-o) * log(o): d/d(-o) = gl * log(o) -> d/do = -(gl * log(o)); d/dlog = gl * (-o) -> / o
        go = -(gl * lo) + (gl * (-o)) / o;
    }
    d_op[i] = go;
    float gd = 0.f;
    if (g_dep) {
        const float v = depth[i] * inv_scale + 1e-10f;
        if (v <= 1.0f) gd = ((g_dep[i] * neg_lam_depth) / fminf(v, 1.0f)) * inv_scale;
    }
    d_dep[i] = gd;
}

extern "C" {

int ngp_composite_loss(const float* sigmas, const float* rgbs, const float* deltas, const float* ts,
                       const int64_t* rays_a, int64_t n_rays, const float* rgb_gt, const float* bg, int loss_type,
                       float lambda_opacity, float lambda_depth, float lambda_distortion, float depth_scale,
                       float T_threshold,
                       float* dL_dsigmas, float* dL_drgbs, float* out_rgb, float* out_opacity, float* out_depth,
                       float* out_loss, int32_t* n_active, int32_t* sample_idx, void* alloc_ws,
                       int64_t* n_active_total, int64_t* stats, void* stream) {
    NGP_CHECK_ARG(n_rays >= 0 && loss_type >= 0 && loss_type <= 3 && depth_scale > 0);
    if (n_rays == 0) return NGP_OK;
    NGP_CHECK_ARG(rays_a && rgb_gt && bg && out_rgb && out_opacity && out_depth && out_loss);
    NGP_CHECK_ARG(!sample_idx || (alloc_ws && n_active_total && ((uintptr_t)alloc_ws & 7) == 0));
    LossArgs la{loss_type, lambda_opacity, lambda_depth, depth_scale, 1.0f / (float)n_rays, T_threshold,
                lambda_distortion};
    // one row per wave: every row's dependent load chain in flight at once
    // (a few rows per wave serialised their memory latencies)
    const unsigned nb = (unsigned)std::min<int64_t>((n_rays + 3) / 4, 1 << 20);
    if (la.lambda_dist != 0.f)
        NGP_TIMED(NGP_K_COMPOSITE, as_stream(stream), composite_loss_wave_kernel<true><<<nb, 256, 0, as_stream(stream)>>>(
            sigmas, rgbs, deltas, ts, rays_a, n_rays, rgb_gt, bg, la, dL_dsigmas, dL_drgbs, out_rgb, out_opacity,
            out_depth, out_loss, n_active, sample_idx, (unsigned long long*)alloc_ws, n_active_total, stats));
    else
        NGP_TIMED(NGP_K_COMPOSITE, as_stream(stream), composite_loss_wave_kernel<false><<<nb, 256, 0, as_stream(stream)>>>(
            sigmas, rgbs, deltas, ts, rays_a, n_rays, rgb_gt, bg, la, dL_dsigmas, dL_drgbs, out_rgb, out_opacity,
            out_depth, out_loss, n_active, sample_idx, (unsigned long long*)alloc_ws, n_active_total, stats));
    return ngp_launch_status();
}

int ngp_nerf_loss_fw(const float* rgb, const float* rgb_gt, const float* opacity, const float* depth, int64_t n,
                     int loss_type, float lambda_opacity, float lambda_depth, float grid_scale, float* loss_rgb,
                     float* loss_opacity, float* loss_depth, void* stream) {
    NGP_CHECK_ARG(n >= 0 && (loss_type == 0 || loss_type == 2 || loss_type == 3) && grid_scale > 0.f);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(rgb && rgb_gt && opacity && depth && loss_rgb && loss_opacity && loss_depth);
    nerf_loss_fw_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(
        rgb, rgb_gt, opacity, depth, n, loss_type, lambda_opacity, -lambda_depth, 1.0f / grid_scale, loss_rgb,
        loss_opacity, loss_depth);
    return ngp_launch_status();
}

int ngp_nerf_loss_bw(const float* rgb, const float* rgb_gt, const float* opacity, const float* depth, int64_t n,
                     int loss_type, float lambda_opacity, float lambda_depth, float grid_scale, const float* g_rgb,
                     const float* g_opacity, const float* g_depth, float* d_rgb, float* d_opacity, float* d_depth,
                     void* stream) {
    NGP_CHECK_ARG(n >= 0 && (loss_type == 0 || loss_type == 2 || loss_type == 3) && grid_scale > 0.f);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(rgb && rgb_gt && opacity && depth && d_rgb && d_opacity && d_depth);
    nerf_loss_bw_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(
        rgb, rgb_gt, opacity, depth, n, loss_type, lambda_opacity, -lambda_depth, 1.0f / grid_scale, g_rgb,
        g_opacity, g_depth, d_rgb, d_opacity, d_depth);
    return ngp_launch_status();
}

}  // extern "C"
