// Light probes for the insertion app (insert/main.py:306-407 of the
// reference): from each of P scene points R rays are rendered over the
// sphere, the global light is blended in behind them as a 9-coefficient
// spherical-harmonic background (models/rendering.py:240-250), and the
// radiance and 1 - opacity are projected onto the SH9 basis
// (insert/insert_utils.py:132-136).
//
//  * probe_rays_kernel: the P*R rays (origin = the probe point) with their
//    AABB interval and near clamp, as render() computes them;
//  * render_finish_sh_kernel: the frame's closing blend with the SH light;
//  * probe_sh9_project_kernel: one workgroup per probe, 36 partial sums per
//    lane in registers, a fixed-order reduction (xor butterflies inside a
//    wave, then the four waves through LDS): no atomics, so every run gives
//    the same bits.
#pragma clang fp contract(off)

#include "common.h"
#include "march.h"
#include "sh9.h"
#include "wave.h"

namespace ngp {

constexpr int PJ_THREADS = 256;            // 4 waves per probe
constexpr int PJ_WAVES = PJ_THREADS / 64;
constexpr int PJ_ACC = 36;                 // 9 coefficients x (r, g, b, 1 - opacity)

// rays_o[p*R+r] = pts[p]; rays_d = dirs[r] (shared) or dirs[p*R+r]; hits_t as
// ray_aabb_kernel with one box and max_hits = 1, then rendering.py:29-31.
__global__ void __launch_bounds__(256) probe_rays_kernel(const float* __restrict__ pts,
                                                         const float* __restrict__ dirs, int dirs_per_probe,
                                                         int64_t n, int64_t R, const float* __restrict__ center,
                                                         const float* __restrict__ half_size, float near,
                                                         float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                         float* __restrict__ hits_t) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t p = i / R;
    const float* dp = dirs + 3 * (dirs_per_probe ? i : i - p * R);
    const float o[3] = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
    const float d[3] = {dp[0], dp[1], dp[2]};
    const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
    float t1, t2;
    aabb_t1t2(o, inv, center, half_size, t1, t2);
    float h0 = -1.0f, h1 = -1.0f;
    if (t2 > 0) { h0 = fmaxf(t1, 0.0f); h1 = t2; }  // intersection.cu:44-51
    if (h0 >= 0 && h0 < near) h0 = near;
#pragma unroll
    for (int c = 0; c < 3; ++c) { rays_o[3 * i + c] = o[c]; rays_d[3 * i + c] = d[c]; }
    hits_t[2 * i] = h0;
    hits_t[2 * i + 1] = h1;
}

// rendering.py:241-250 with SH_bkg: rgb += relu(get_SH_val(shec, rays_d)) * (1 - opacity)
__global__ void __launch_bounds__(256) render_finish_sh_kernel(const float* __restrict__ opacity,
                                                               const float* __restrict__ rays_d, int64_t n_rays,
                                                               const float* __restrict__ shec,
                                                               float* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    float Y[9];
    sh9_basis(rays_d[3 * i], rays_d[3 * i + 1], rays_d[3 * i + 2], Y);
    const float m = 1 - opacity[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = Y[0] * shec[c];
#pragma unroll
        for (int k = 1; k < 9; ++k) v += Y[k] * shec[3 * k + c];
        rgb[3 * i + c] += fmaxf(v, 0.0f) * m;
    }
}

// get_SH_coeff (insert_utils.py:132-136) of the radiance and of 1 - opacity
// (main.py:399-406) for probe blockIdx.x.  Lane t of the block walks rays
// t, t + 256, ...; a lane with no ray adds exact zeros.
__global__ void __launch_bounds__(PJ_THREADS) probe_sh9_project_kernel(const float* __restrict__ rays_d,
                                                                      const float* __restrict__ rgb,
                                                                      const float* __restrict__ opacity, int R,
                                                                      float scale, float* __restrict__ rgb_sh,
                                                                      float* __restrict__ trans_sh) {
    const int64_t p = blockIdx.x;
    const int64_t base = p * R;
    float acc[PJ_ACC];
#pragma unroll
    for (int a = 0; a < PJ_ACC; ++a) acc[a] = 0.0f;
    for (int64_t r = threadIdx.x; r < R; r += PJ_THREADS) {
        const int64_t i = base + r;
        float Y[9];
        sh9_basis(rays_d[3 * i], rays_d[3 * i + 1], rays_d[3 * i + 2], Y);
        const float v[4] = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], trans_sh ? 1 - opacity[i] : 0.0f};
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[4 * k + c] += Y[k] * v[c];
    }
#pragma unroll
    for (int a = 0; a < PJ_ACC; ++a) acc[a] = wave_sum(acc[a]);
    __shared__ float part[PJ_WAVES][PJ_ACC];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < PJ_ACC; ++a) part[threadIdx.x >> 6][a] = acc[a];
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= PJ_ACC) return;
    float s = part[0][t];
#pragma unroll
    for (int w = 1; w < PJ_WAVES; ++w) s += part[w][t];
    const int k = t >> 2, c = t & 3;
    if (c < 3)
        rgb_sh[(p * 9 + k) * 3 + c] = s * scale;
    else if (trans_sh)
        trans_sh[p * 9 + k] = s * scale;
}

}  // namespace ngp

using namespace ngp;

static inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

extern "C" {

int ngp_probe_rays(const float* pts, const float* dirs, int dirs_per_probe, int64_t P, int64_t R,
                   const float* center, const float* half_size, float near_distance, float* rays_o, float* rays_d,
                   float* hits_t, void* stream) {
    NGP_CHECK_ARG(P >= 0 && R >= 0 && (dirs_per_probe == 0 || dirs_per_probe == 1));
    if (P == 0) return NGP_OK;
    NGP_CHECK_ARG(R >= 1 && R < ((int64_t)1 << 31) && P < ((int64_t)1 << 31) && P * R < ((int64_t)1 << 31));
    NGP_CHECK_ARG(pts && dirs && center && half_size && rays_o && rays_d && hits_t);
    const int64_t n = P * R;
    probe_rays_kernel<<<nblk(n, 256), 256, 0, as_stream(stream)>>>(pts, dirs, dirs_per_probe, n, R, center, half_size,
                                                                   near_distance, rays_o, rays_d, hits_t);
    return ngp_launch_status();
}

int ngp_render_test_finish_sh(const float* opacity, const float* rays_d, int64_t n_rays, const float* shec, float* rgb,
                              void* stream) {
    NGP_CHECK_ARG(n_rays >= 0 && shec);
    if (n_rays == 0) return NGP_OK;
    NGP_CHECK_ARG(opacity && rays_d && rgb);
    render_finish_sh_kernel<<<nblk(n_rays, 256), 256, 0, as_stream(stream)>>>(opacity, rays_d, n_rays, shec, rgb);
    return ngp_launch_status();
}

int ngp_probe_sh9_project(const float* rays_d, const float* rgb, const float* opacity, int64_t P, int64_t R,
                          float* rgb_sh, float* trans_sh, void* stream) {
    NGP_CHECK_ARG(P >= 0 && R >= 0);
    if (P == 0) return NGP_OK;
    NGP_CHECK_ARG(R >= 1 && R < ((int64_t)1 << 31) && P < ((int64_t)1 << 31) && P * R < ((int64_t)1 << 31));
    NGP_CHECK_ARG(rays_d && rgb && rgb_sh && (opacity || !trans_sh));
    const float scale = (float)(4.0 * 3.14159265358979323846 / (double)R);
    probe_sh9_project_kernel<<<(unsigned)P, PJ_THREADS, 0, as_stream(stream)>>>(rays_d, rgb, opacity, (int)R, scale,
                                                                               rgb_sh, trans_sh);
    return ngp_launch_status();
}

}  // extern "C"
