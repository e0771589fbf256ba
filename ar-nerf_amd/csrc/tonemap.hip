// Exposure tonemappers of the HDR-NeRF mode (networks.py:80-93, 110-131 of the
// reference: three tcnn 1 -> 64 -> 1 networks, ReLU / Sigmoid, one per colour
// channel, fed log radiance + log exposure).  DESIGN.md §18 defines the
// arithmetic; include/ngp_amd.h "exposure tonemappers" states the entry points.
//
// The hidden width is the wave width, and each kernel takes the layout that
// keeps its inner loop free of cross-lane traffic:
//  * tonemap_forward_kernel: one lane per row.  The 192 units' {A_j0, beta_j,
//    B_0j} sit in LDS and every lane reads the same address (a broadcast), so
//    a unit costs one LDS read and two FMAs and a compare per 64 rows.
//  * tonemap_backward_kernel: per 256-row tile, phase 1 is the forward's
//    layout (lane per row: z, delta, dL/dx = delta * sum_j m_j B_j A_j0) and
//    leaves (u, delta) of every row-channel in LDS; phase 2 turns the wave
//    round (lane per hidden unit) and each lane walks its wave's 64 rows,
//    adding m_j delta and m_j delta u into two registers per channel -- the
//    two masked sums every weight gradient of the unit is made of.  No wave
//    reductions, no atomics.  The workgroup's sums go to its slot of the
//    workspace; tonemap_fold_kernel adds the slots in workgroup order, forms
//    the three gradients per unit and adds them into grad_tone.
// The arithmetic itself is tonemap.h's, shared with the training step's row
// and list forms (tonemap_step.hip).
#pragma clang fp contract(off)

#include "common.h"
#include "tonemap.h"

namespace ngp {

__global__ void __launch_bounds__(TM_THREADS) tonemap_forward_kernel(const float* log_rad,
                                                                    const float* __restrict__ exposure,
                                                                    int64_t n_exposure, int64_t n,
                                                                    const int64_t* __restrict__ n_dev,
                                                                    const int32_t* __restrict__ sample_idx,
                                                                    const _Float16* __restrict__ tone, int mode,
                                                                    float* rgbs) {
    __shared__ float4 w[3][64];
    if (mode == NGP_TONE_LDR) tm_load_weights(tone, w);
    int64_t count = n_dev ? *n_dev : n;
    count = count < n ? count : n;
    for (int64_t i = (int64_t)blockIdx.x * TM_THREADS + threadIdx.x; i < count; i += (int64_t)gridDim.x * TM_THREADS) {
        int64_t row = i;
        if (sample_idx) {
            row = sample_idx[i];
            if (row < 0 || row >= n) continue;
        }
        float x[3], y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = log_rad[3 * row + c];
        if (mode == NGP_TONE_RADIANCE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) y[c] = expf(fminf(fmaxf(x[c], 0.0f), 20.0f));
        } else {
            tm_forward_row(w, x, tm_log_exposure(exposure, n_exposure, row), y);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) rgbs[3 * row + c] = y[c];
    }
}

__global__ void __launch_bounds__(TM_THREADS) tonemap_backward_kernel(const float* __restrict__ log_rad,
                                                                     const float* __restrict__ exposure,
                                                                     int64_t n_exposure, int64_t n,
                                                                     const int64_t* __restrict__ n_dev,
                                                                     const _Float16* __restrict__ tone,
                                                                     const float* dL_drgbs, float* dL_dlog_rad,
                                                                     float* __restrict__ slots) {
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
        // phase 1, lane per row
        const int64_t row = tile * TM_THREADS + tid;
        const bool live = row < count;
        const float le = live ? tm_log_exposure(exposure, n_exposure, row) : 0.0f;
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

}  // namespace ngp

using namespace ngp;

static bool tm_exposure_ok(const float* exposure, int64_t n_exposure, int64_t n) {
    if (n_exposure != 0 && n_exposure != 1 && n_exposure != n) return false;
    return n == 0 || n_exposure == 0 || exposure != nullptr;
}

extern "C" {

int ngp_tonemap_forward(const float* log_rad, const float* exposure, int64_t n_exposure, int64_t n,
                        const int64_t* n_dev, const int32_t* sample_idx, const void* tone_f16, int mode,
                        float* rgbs, void* stream) {
    NGP_CHECK_ARG(mode == NGP_TONE_LDR || mode == NGP_TONE_RADIANCE);
    NGP_CHECK_ARG(n >= 0 && tm_exposure_ok(exposure, n_exposure, n));
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(log_rad && rgbs && (tone_f16 || mode != NGP_TONE_LDR) && (n_dev || !sample_idx));
    const int64_t blocks = (n + TM_THREADS - 1) / TM_THREADS;
    tonemap_forward_kernel<<<(unsigned)(blocks < TM_FWD_BLOCKS ? blocks : TM_FWD_BLOCKS), TM_THREADS, 0,
                             as_stream(stream)>>>(log_rad, exposure, n_exposure, n, n_dev, sample_idx,
                                                  static_cast<const _Float16*>(tone_f16), mode, rgbs);
    return ngp_launch_status();
}

size_t ngp_tonemap_backward_workspace(int64_t n) {
    return n > 0 ? (size_t)tm_bwd_blocks(n) * TM_SLOT * sizeof(float) : 0;
}

int ngp_tonemap_backward(const float* log_rad, const float* exposure, int64_t n_exposure, int64_t n,
                         const int64_t* n_dev, const void* tone_f16, const float* dL_drgbs, float* dL_dlog_rad,
                         float* grad_tone, void* workspace, void* stream) {
    NGP_CHECK_ARG(n >= 0 && tm_exposure_ok(exposure, n_exposure, n));
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(log_rad && tone_f16 && dL_drgbs && dL_dlog_rad && grad_tone && workspace);
    NGP_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
    const int64_t blocks = tm_bwd_blocks(n);
    float* slots = static_cast<float*>(workspace);
    const _Float16* tone = static_cast<const _Float16*>(tone_f16);
    tonemap_backward_kernel<<<(unsigned)blocks, TM_THREADS, 0, as_stream(stream)>>>(
        log_rad, exposure, n_exposure, n, n_dev, tone, dL_drgbs, dL_dlog_rad, slots);
    const int rc = ngp_launch_status();
    if (rc != NGP_OK) return rc;
    tonemap_fold_kernel<<<1, 192, 0, as_stream(stream)>>>(slots, (int)blocks, tone, grad_tone);
    return ngp_launch_status();
}

}  // extern "C"
