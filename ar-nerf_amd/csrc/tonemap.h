// The exposure tonemappers' arithmetic, stated once for
// tonemap.hip (whole buffers, the model surface) and tonemap_step.hip (the
// fused training step's row / list forms): the LDS weight image, one channel
// of one row forward and backward, a wave's masked sums, a workgroup's slot
// and the fold of the slots into the weight gradients.  A row's value depends
// on its inputs and the weights alone, never on which kernel walks it: the
// forms agree bit for bit because they run these same statements.
//
// Meant for exactly those two files.  It sets `fp contract(off)` for whatever
// follows it, and tonemap_fold_kernel is `static`: every translation unit that
// includes this header gets its own copy of that kernel (each of the two
// launches it).  A third user should move the fold's launch behind a function
// of one of them rather than include this.
#pragma once
#pragma clang fp contract(off)

#include "common.h"

namespace ngp {

constexpr int TM_THREADS = 256;
constexpr int TM_WAVES = TM_THREADS / 64;
constexpr int TM_NET = 2048;           // one channel's parameters: A 64x16 | B 16x64
constexpr int TM_B = 1024;             // offset of B in a channel
constexpr int TM_SLOT = 3 * 2 * 64;    // one workgroup's partial sums: [channel][S0, S1][unit]
constexpr int TM_FWD_BLOCKS = 2048;    // grid caps: the grids do not grow with n
constexpr int TM_BWD_BLOCKS = 512;

// beta_j: the fifteen padded inputs are 1 (ascending k, fp32)
__device__ __forceinline__ float tm_beta(const _Float16* __restrict__ A, int j) {
    float beta = (float)A[j * 16 + 1];
#pragma unroll
    for (int k = 2; k < 16; ++k) beta += (float)A[j * 16 + k];
    return beta;
}

// LDS image of the three networks: per (channel, unit) {A_j0, beta_j, B_0j, B_0j * A_j0}
// (THREADS: the workgroup's size)
template <int THREADS = TM_THREADS>
__device__ __forceinline__ void tm_load_weights(const _Float16* __restrict__ tone, float4 (*w)[64]) {
    for (int t = threadIdx.x; t < 192; t += THREADS) {
        const int c = t >> 6, j = t & 63;
        const _Float16* T = tone + c * TM_NET;
        const float a0 = (float)T[j * 16], b = (float)T[TM_B + j];
        w[c][j] = make_float4(a0, tm_beta(T, j), b, b * a0);
    }
    __syncthreads();
}

__device__ __forceinline__ float tm_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// log of the row's exposure (n_exposure: 0 none, 1 one value, else one per row)
__device__ __forceinline__ float tm_log_exposure(const float* __restrict__ exposure, int64_t n_exposure, int64_t row) {
    if (n_exposure == 0) return 0.0f;
    return logf(exposure[n_exposure == 1 ? 0 : row]);
}

// one channel of one row, forward: y = sigmoid(sum_j B_0j relu(A_j0 u + beta_j)), ascending j
__device__ __forceinline__ float tm_forward_channel(const float4* w, float u) {
    float z = 0.0f;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
        const float4 p = w[j];
        const float a = fmaf(p.x, u, p.y);
        z = fmaf(p.z, a > 0.0f ? a : 0.0f, z);
    }
    return tm_sigmoid(z);
}

// one row, forward (NGP_TONE_LDR): x (3) at log exposure le -> y (3)
__device__ __forceinline__ void tm_forward_row(const float4 (*w)[64], const float* x, float le, float* y) {
#pragma unroll
    for (int c = 0; c < 3; ++c) y[c] = tm_forward_channel(w[c], x[c] + le);
}

// one channel of one row, backward phase 1: the hidden layer recomputed at u, delta = g y (1 - y)
// (exactly 0 for g == 0) and dL/dx = delta sum_j m_j B_0j A_j0
__device__ __forceinline__ void tm_backward_channel(const float4* w, float u, float g, float& delta, float& dx) {
    float z = 0.0f, ba = 0.0f;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
        const float4 p = w[j];
        const float a = fmaf(p.x, u, p.y);
        const bool on = a > 0.0f;
        z = fmaf(p.z, on ? a : 0.0f, z);
        ba += on ? p.w : 0.0f;
    }
    const float y = tm_sigmoid(z);
    delta = g == 0.0f ? 0.0f : g * (y * (1.0f - y));
    dx = delta * ba;
}

// backward phase 2, lane = hidden unit j of one channel: the wave's 64 rows' (u, delta) from LDS
// added into S0 = sum m_j delta, S1 = sum m_j delta u (a dead row has delta 0)
__device__ __forceinline__ void tm_accumulate(const float2* ud, float a0, float be, float& s0, float& s1) {
#pragma unroll 8
    for (int r = 0; r < 64; ++r) {
        const float2 p = ud[r];
        const float d = fmaf(a0, p.x, be) > 0.0f ? p.y : 0.0f;
        s0 += d;
        s1 = fmaf(d, p.x, s1);
    }
}

// the workgroup's sums (its waves in order) to its slot of the workspace
__device__ __forceinline__ void tm_store_slot(float (*part)[TM_SLOT], const float* s0, const float* s1,
                                              float* __restrict__ slots) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        part[wv][(2 * c) * 64 + lane] = s0[c];
        part[wv][(2 * c + 1) * 64 + lane] = s1[c];
    }
    __syncthreads();
    for (int t = tid; t < TM_SLOT; t += TM_THREADS) {
        float s = part[0][t];
#pragma unroll
        for (int v = 1; v < TM_WAVES; ++v) s += part[v][t];
        slots[(int64_t)blockIdx.x * TM_SLOT + t] = s;
    }
}

// dB_0j = A_j0 S1 + beta_j S0, dA_j0 = B_0j S1, dA_jk = B_0j S0 (k = 1..15), added into one channel's gradient G
__device__ __forceinline__ void tm_add_unit_grad(const _Float16* __restrict__ T, int j, float s0, float s1,
                                                 float* __restrict__ G) {
    const float a0 = (float)T[j * 16], beta = tm_beta(T, j), bj = (float)T[TM_B + j];
    G[TM_B + j] += fmaf(a0, s1, beta * s0);
    G[j * 16] += bj * s1;
    const float db = bj * s0;
#pragma unroll
    for (int k = 1; k < 16; ++k) G[j * 16 + k] += db;
}

// One thread per (channel, unit): S0, S1 over the slots in workgroup order, then the three
// gradients of the unit added into grad.  (static: one copy per translation unit that launches it)
static __global__ void __launch_bounds__(192) tonemap_fold_kernel(const float* __restrict__ slots, int n_slots,
                                                                 const _Float16* __restrict__ tone,
                                                                 float* __restrict__ grad) {
    const int c = threadIdx.x >> 6, j = threadIdx.x & 63;
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll 8
    for (int b = 0; b < n_slots; ++b) {
        s0 += slots[(int64_t)b * TM_SLOT + (2 * c) * 64 + j];
        s1 += slots[(int64_t)b * TM_SLOT + (2 * c + 1) * 64 + j];
    }
    tm_add_unit_grad(tone + c * TM_NET, j, s0, s1, grad + c * TM_NET);
}

}  // namespace ngp

static inline int64_t tm_bwd_blocks(int64_t n) {
    const int64_t tiles = (n + ngp::TM_THREADS - 1) / ngp::TM_THREADS;
    return tiles < ngp::TM_BWD_BLOCKS ? tiles : ngp::TM_BWD_BLOCKS;
}
