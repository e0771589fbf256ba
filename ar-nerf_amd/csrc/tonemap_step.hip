// The exposure tonemappers inside the fused training step (DESIGN.md §19;
// include/ngp_amd.h "exposure tonemappers in the training step").  The step
// evaluates the field over rows of rays_a (round 1) and over compacted sample
// lists (round 2, the backward), and knows the exposure per ray; the kernels
// here are tonemap.hip's forward and backward in those shapes, on tonemap.h's
// arithmetic, so a row's bits do not depend on which form walked it:
//  * sample_exposure_kernel: one wave per row of rays_a, the ray's exposure
//    copied to the row's samples (the exposure itself: logf stays in one place).
//  * tonemap_rows_kernel: one wave per listed row, lane per sample of the
//    row's first `first` samples; the weights as tonemap_forward_kernel holds
//    them (LDS, broadcast reads).
//  * tonemap_backward_indexed_kernel: tonemap_backward_kernel with row =
//    sample_idx[i] in phase 1 (an index outside [0, n) is a dead row: delta 0);
//    phase 2, the slots and the fold are the same code.
//  * unit_exposure_kernel: train.py:182-187, one workgroup: wave c is channel
//    c at x = 0, exposure 1, lane j its hidden unit.
#pragma clang fp contract(off)

#include "common.h"
#include "tonemap.h"

namespace ngp {

constexpr int TM_ROW_BLOCKS = 2048;

__global__ void __launch_bounds__(TM_THREADS) sample_exposure_kernel(const int64_t* __restrict__ rays_a, int64_t n_rays,
                                                                    const int64_t* __restrict__ img_idxs,
                                                                    const float* __restrict__ img_exposure,
                                                                    int64_t n_img,
                                                                    const float* __restrict__ ray_exposure, int64_t n,
                                                                    float* __restrict__ sample_exposure) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * TM_WAVES;
    for (int64_t r = (int64_t)blockIdx.x * TM_WAVES + (threadIdx.x >> 6); r < n_rays; r += stride) {
        const int64_t ray = rays_a[3 * r], start = rays_a[3 * r + 1], N = rays_a[3 * r + 2];
        if (ray < 0 || ray >= n_rays || start < 0 || N <= 0) continue;
        float e;
        if (ray_exposure) {
            e = ray_exposure[ray];
        } else {
            const int64_t img = img_idxs[ray];
            if (img < 0 || img >= n_img) continue;
            e = img_exposure[img];
        }
        const int64_t end = N < n - start ? start + N : n;  // (never past the buffer)
        for (int64_t i = start + lane; i < end; i += 64) sample_exposure[i] = e;
    }
}

__global__ void __launch_bounds__(TM_THREADS) tonemap_rows_kernel(const float* log_rad, int64_t n,
                                                                 const int64_t* __restrict__ rays_a,
                                                                 const int32_t* __restrict__ rows,
                                                                 const int64_t* __restrict__ n_rows_dev, int64_t n_rows,
                                                                 int first,
                                                                 const float* __restrict__ sample_exposure,
                                                                 const _Float16* __restrict__ tone, float* rgbs) {
    __shared__ float4 w[3][64];
    tm_load_weights(tone, w);
    const int lane = threadIdx.x & 63;
    const int64_t NR = ngp_capped_count(n_rows_dev, n_rows);
    const int64_t stride = (int64_t)gridDim.x * TM_WAVES;
    for (int64_t j = (int64_t)blockIdx.x * TM_WAVES + (threadIdx.x >> 6); j < NR; j += stride) {
        const int64_t r = rows ? (int64_t)rows[j] : j;
        if (r < 0 || r >= n_rows) continue;
        const int64_t start = rays_a[3 * r + 1], N = rays_a[3 * r + 2];
        if (start < 0) continue;
        int64_t end = start + (N < first ? N : (int64_t)first);
        end = end < n ? end : n;  // (never past the buffer)
        for (int64_t i = start + lane; i < end; i += 64) {
            float x[3], y[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = log_rad[3 * i + c];
            tm_forward_row(w, x, logf(sample_exposure[i]), y);
#pragma unroll
            for (int c = 0; c < 3; ++c) rgbs[3 * i + c] = y[c];
        }
    }
}

__global__ void __launch_bounds__(TM_THREADS) tonemap_backward_indexed_kernel(
    const float* __restrict__ log_rad, const float* __restrict__ sample_exposure, int64_t n,
    const int64_t* __restrict__ n_dev, const int32_t* __restrict__ sample_idx, const _Float16* __restrict__ tone,
    const float* dL_drgbs, float* dL_dlog_rad, float* __restrict__ slots) {
    __shared__ float4 w[3][64];
    __shared__ float2 ud[TM_WAVES][3][64];  // (u, delta) of each wave's 64 rows
    __shared__ float part[TM_WAVES][TM_SLOT];
    tm_load_weights(tone, w);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t count = n_dev ? *n_dev : n;
    count = count < n ? count : n;
    const int64_t n_tiles = (count + TM_THREADS - 1) / TM_THREADS;
    float a0[3], be[3], s0[3], s1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a0[c] = w[c][lane].x;
        be[c] = w[c][lane].y;
        s0[c] = s1[c] = 0.0f;
    }
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // (the same trips for the whole workgroup)
        // phase 1, lane per listed row
        const int64_t i = tile * TM_THREADS + tid;
        int64_t row = -1;
        if (i < count) row = sample_idx ? (int64_t)sample_idx[i] : i;
        const bool live = row >= 0 && row < n;
        const float le = live ? logf(sample_exposure[row]) : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float u = 0.0f, delta = 0.0f;
            if (live) {
                const float g = dL_drgbs[3 * row + c];
                u = log_rad[3 * row + c] + le;
                float dx;
                tm_backward_channel(w[c], u, g, delta, dx);
                dL_dlog_rad[3 * row + c] = dx;
                if (delta == 0.0f) u = 0.0f;  // (adds nothing whatever its input holds: 0 * NaN must not reach S1)
            }
            ud[wv][c][lane] = make_float2(u, delta);
        }
        __syncthreads();
        // phase 2, lane per hidden unit over this wave's rows (a dead row has delta 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) tm_accumulate(ud[wv][c], a0[c], be[c], s0[c], s1[c]);
        __syncthreads();
    }
    tm_store_slot(part, s0, s1, slots);
}

// wave c = channel c, lane j = hidden unit j.  Every lane of the wave runs the forward's own loop
// (y is tonemap_forward's bits at x = 0, exposure 1: u = 0 + logf(1)); the row's S0_j = m_j delta,
// S1_j = m_j delta u with u = 0 go through the fold's statement of the three gradients.
__global__ void __launch_bounds__(192) unit_exposure_kernel(const _Float16* __restrict__ tone, float target,
                                                           float* __restrict__ grad, float* __restrict__ out_loss) {
    __shared__ float4 w[3][64];
    __shared__ float half_sq[3];
    tm_load_weights<192>(tone, w);
    const int c = threadIdx.x >> 6, j = threadIdx.x & 63;
    const float u = 0.0f + logf(1.0f);
    const float y = tm_forward_channel(w[c], u);
    const float d = y - target;
    const float g = d / 3.0f;  // d/dy_c of mean_c 0.5 (y_c - target)^2
    const float delta = g == 0.0f ? 0.0f : g * (y * (1.0f - y));
    const float4 p = w[c][j];
    const float s0 = fmaf(p.x, u, p.y) > 0.0f ? delta : 0.0f;
    tm_add_unit_grad(tone + c * TM_NET, j, s0, s0 * u, grad + c * TM_NET);
    if (j == 0) half_sq[c] = 0.5f * (d * d);
    __syncthreads();
    if (threadIdx.x == 0) *out_loss = (half_sq[0] + half_sq[1] + half_sq[2]) / 3.0f;
}

}  // namespace ngp

using namespace ngp;

static unsigned tm_row_blocks(int64_t n_rows) {
    const int64_t blocks = (n_rows + TM_WAVES - 1) / TM_WAVES;
    return (unsigned)(blocks < TM_ROW_BLOCKS ? blocks : TM_ROW_BLOCKS);
}

extern "C" {

int ngp_sample_exposure(const int64_t* rays_a, int64_t n_rays, const int64_t* img_idxs, const float* img_exposure,
                        int64_t n_img, int64_t n, float* sample_exposure, void* stream) {
    NGP_CHECK_ARG(n_rays >= 0 && n >= 0 && n_img >= 0);
    if (n_rays == 0 || n == 0) return NGP_OK;
    NGP_CHECK_ARG(rays_a && img_idxs && img_exposure && sample_exposure);
    sample_exposure_kernel<<<tm_row_blocks(n_rays), TM_THREADS, 0, as_stream(stream)>>>(
        rays_a, n_rays, img_idxs, img_exposure, n_img, nullptr, n, sample_exposure);
    return ngp_launch_status();
}

int ngp_sample_exposure_rays(const int64_t* rays_a, int64_t n_rays, const float* ray_exposure, int64_t n,
                             float* sample_exposure, void* stream) {
    NGP_CHECK_ARG(n_rays >= 0 && n >= 0);
    if (n_rays == 0 || n == 0) return NGP_OK;
    NGP_CHECK_ARG(rays_a && ray_exposure && sample_exposure);
    sample_exposure_kernel<<<tm_row_blocks(n_rays), TM_THREADS, 0, as_stream(stream)>>>(
        rays_a, n_rays, nullptr, nullptr, 0, ray_exposure, n, sample_exposure);
    return ngp_launch_status();
}

int ngp_tonemap_forward_rows(const float* log_rad, int64_t n, const int64_t* rays_a, const int32_t* rows,
                             const int64_t* n_rows_dev, int64_t n_rows, int first, const float* sample_exposure,
                             const void* tone_f16, float* rgbs, void* stream) {
    NGP_CHECK_ARG(n >= 0 && n_rows >= 0 && first >= 0);
    if (n == 0 || n_rows == 0 || first == 0) return NGP_OK;
    NGP_CHECK_ARG(log_rad && rays_a && sample_exposure && tone_f16 && rgbs);
    tonemap_rows_kernel<<<tm_row_blocks(n_rows), TM_THREADS, 0, as_stream(stream)>>>(
        log_rad, n, rays_a, rows, n_rows_dev, n_rows, first, sample_exposure, static_cast<const _Float16*>(tone_f16),
        rgbs);
    return ngp_launch_status();
}

size_t ngp_tonemap_backward_indexed_workspace(int64_t n) {
    return n > 0 ? (size_t)tm_bwd_blocks(n) * TM_SLOT * sizeof(float) : 0;
}

int ngp_tonemap_backward_indexed(const float* log_rad, const float* sample_exposure, int64_t n, const int64_t* n_dev,
                                 const int32_t* sample_idx, const void* tone_f16, const float* dL_drgbs,
                                 float* dL_dlog_rad, float* grad_tone, void* workspace, void* stream) {
    NGP_CHECK_ARG(n >= 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(log_rad && sample_exposure && tone_f16 && dL_drgbs && dL_dlog_rad && grad_tone && workspace);
    NGP_CHECK_ARG(n_dev || !sample_idx);
    NGP_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
    const int64_t blocks = tm_bwd_blocks(n);
    float* slots = static_cast<float*>(workspace);
    const _Float16* tone = static_cast<const _Float16*>(tone_f16);
    tonemap_backward_indexed_kernel<<<(unsigned)blocks, TM_THREADS, 0, as_stream(stream)>>>(
        log_rad, sample_exposure, n, n_dev, sample_idx, tone, dL_drgbs, dL_dlog_rad, slots);
    const int rc = ngp_launch_status();
    if (rc != NGP_OK) return rc;
    tonemap_fold_kernel<<<1, 192, 0, as_stream(stream)>>>(slots, (int)blocks, tone, grad_tone);
    return ngp_launch_status();
}

int ngp_unit_exposure_term(const void* tone_f16, float target, float* grad_tone, float* out_loss, void* stream) {
    NGP_CHECK_ARG(tone_f16 && grad_tone && out_loss);
    unit_exposure_kernel<<<1, 192, 0, as_stream(stream)>>>(static_cast<const _Float16*>(tone_f16), target, grad_tone,
                                                          out_loss);
    return ngp_launch_status();
}

}  // extern "C"
