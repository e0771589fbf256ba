// Input gradients of NGP.forward (models/networks.py:133-146): dL/dxyzs and
// dL/ddirs of the gradient-carrying samples, and their per-ray sums -- what
// RayMarcher.backward (custom_functions.py:102-112) hands to the rays, and
// through them to the reference's pose refinement (--optimize_ext,
// train.py:92-95, 132-137).  tcnn computes these as the input gradients of
// its grid encoding, SH encoding and both networks; tcnn's own arithmetic is
// not available here, so the restatement below is the specification (parity
// unpinned, as for normal.hip; checked against an fp64 restatement,
// tests/input_grad_ref.py).
//
// field_input_grad_kernel, one 64-lane wave = one 16-sample column block
// like the forward (lane -> sample s = lane & 15, lane group g = lane >> 4):
//   position   lane (s, g) takes hash levels 4g..4g+3 of sample s: per level
//              the 8 corner entries are gathered at once (a wave issues the
//              128 gathers of its 16 samples' level together), then
//                acc_d = sum_c dw_c/dpos_d * (denc[2l] t_c[0] + denc[2l+1] t_c[1])
//              (fmaf over the corners in tcnn's corner order) and
//              gx_d = fmaf(scale_l, acc_d, gx_d) over the lane's four levels;
//              the four lane groups' partial sums are added by two xor
//              shuffles, (g0 + g1) + (g2 + g3): a fixed order, no atomics.
//              denc is dL/d(encoding) as the MLP backward wrote it (it
//              already carries the colour path through h); the encoding's
//              fp16 rounding is straight-through.
//              dL/dx_d = gx_d / (xyz_max_d - xyz_min_d).
//   direction  (dL_ddirs given) the forward is recomputed through the forward
//              kernels' own device functions (density_net on the saved
//              encoding, sh4_select, color_net: field_net.h), so the ReLU
//              masks are the forward's; then, all in fp32 (the fp16 weights
//              are exact in fp32; no fp16 gradient storage):
//                dout = rgb_out_grad(o, dL/drgb, act)
//                da4 = relu'(h4) * W5^T dout;  da3 = relu'(h3) * W4^T da4
//                dSH = (W3^T da3)[0..15]
//                dL/du = sum_j dSH_j dSH_j/du, u = d/|d|  (the (u+1)/2 and
//                        *2-1 of the encoding cancel)
//                dL/dd = (dL/du - u <u, dL/du>) / |d|
//              Lane (s, g) owns the hidden units 16t + 4g + r of every tile t
//              (the accumulator layout of the forward); a layer's 64 input
//              gradients reach every lane group by shuffles, in unit order.
// Weights sit in LDS (the forward's image); no scratch.
//
// ray_segment_sum_kernel: one wave per ray; lanes walk the ray's samples with
// stride 64 and combine in a fixed xor butterfly, so the sums are bit-identical
// from run to run (custom_functions._segment_sum's index_add_ is atomic).
//
// This file is compiled twice: as itself, and from inputgrad_pm.hip with
// NGP_ENC_PAIR_MAJOR defined, which builds field_input_grad_pm_kernel alone --
// the same kernel reading the saved encoding in the training step's pair-major
// layout (field.hip: enc[p][i][0..3] = row i's features 4p..4p+3, row stride
// enc_pm_stride) behind ngp_field_input_grad_pm.  Two translation units, so the
// row-major kernel's code is what it was before the second one existed.
#pragma clang fp contract(off)
#include "field_net.h"
#include "grid.h"
#include "wave.h"

#ifdef NGP_ENC_PAIR_MAJOR
#define NGP_INPUT_GRAD_KERNEL field_input_grad_pm_kernel
#define NGP_ENC_STRIDE_PARAM , int64_t enc_pm_stride
#define NGP_ENC_ROW(enc, i, g) \
    pack(*reinterpret_cast<const h4*>((enc) + ((2 * (g)) * enc_pm_stride + (i)) * 4), \
         *reinterpret_cast<const h4*>((enc) + ((2 * (g) + 1) * enc_pm_stride + (i)) * 4))
#else
#define NGP_INPUT_GRAD_KERNEL field_input_grad_kernel
#define NGP_ENC_STRIDE_PARAM
#define NGP_ENC_ROW(enc, i, g) *reinterpret_cast<const h8*>((enc) + (i) * 32 + 8 * (g))
#endif

namespace ngp {

__device__ __forceinline__ h4 lds4h(const _Float16* p) { return *reinterpret_cast<const h4*>(p); }
// Ends one unit's weight reads and arithmetic before the next unit's begin.  The loops over a layer's
// 64 units are fully unrolled (the gradient registers are indexed statically); left free, the compiler
// issues every unit's reads first and sinks the arithmetic below them, which takes all 512 registers and
// spills (over 120 VGPRs).  The accumulators pass through the (empty) statement so the arithmetic cannot
// sink past it.
__device__ __forceinline__ void unit_fence(float (&a)[4]) {
    asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// One level's contribution to dL/dx01 of one sample: gx_d = fmaf(scale, acc_d, gx_d)
__device__ __forceinline__ void level_pos_grad(const float in[3], int l, const LevelLds& lv,
                                               const uint32_t* __restrict__ table, float d0, float d1, float gx[3]) {
    const float sc = lv.scale[l];
    const uint32_t res = lv.res[l], size = lv.size[l], off = lv.off[l];
    const bool dense = (lv.dense >> l) & 1u, pow2 = (lv.pow2 >> l) & 1u;
    float pos[3];
    uint32_t pg[3];
    level_cell(sc, in, pg, pos);
    uint32_t v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c)
        v[c] = table[off + corner_index(pg[0] + (c & 1), pg[1] + ((c >> 1) & 1), pg[2] + ((c >> 2) & 1), res, size,
                                        dense, pow2)];
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float t0 = (float)__builtin_bit_cast(_Float16, (uint16_t)(v[c] & 0xffffu));
        const float t1 = (float)__builtin_bit_cast(_Float16, (uint16_t)(v[c] >> 16));
        corner_pos_grad(pos, c, d0 * t0 + d1 * t1, acc);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) gx[d] = fmaf(sc, acc[d], gx[d]);
}

// dL/du of the 16 SH4 values (sh4_select's polynomials, differentiated by hand)
__device__ __forceinline__ void sh4_grad(float x, float y, float z, const float g[16], float gu[3]) {
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    const float c1 = 0.48860251190291987f, c2 = 1.0925484305920792f, c3 = 0.94617469575755997f,
                c4 = 0.54627421529603959f, c5 = 0.59004358992664352f, c6 = 2.8906114426405538f,
                c7 = 0.45704579946446572f, c8 = 0.3731763325901154f, c9 = 1.4453057213202769f;
    const float q = 1.0f - 5.0f * z2, e = 3.0f * (y2 - x2);
    float ax = 0.f, ay = 0.f, az = 0.f;
    ay = fmaf(g[1], -c1, ay);
    az = fmaf(g[2], c1, az);
    ax = fmaf(g[3], -c1, ax);
    ax = fmaf(g[4], c2 * y, ax); ay = fmaf(g[4], c2 * x, ay);
    ay = fmaf(g[5], -c2 * z, ay); az = fmaf(g[5], -c2 * y, az);
    az = fmaf(g[6], 2.0f * c3 * z, az);
    ax = fmaf(g[7], -c2 * z, ax); az = fmaf(g[7], -c2 * x, az);
    ax = fmaf(g[8], 2.0f * c4 * x, ax); ay = fmaf(g[8], -2.0f * c4 * y, ay);
    ax = fmaf(g[9], -6.0f * c5 * xy, ax); ay = fmaf(g[9], c5 * e, ay);
    ax = fmaf(g[10], c6 * yz, ax); ay = fmaf(g[10], c6 * xz, ay); az = fmaf(g[10], c6 * xy, az);
    ay = fmaf(g[11], c7 * q, ay); az = fmaf(g[11], -10.0f * c7 * yz, az);
    az = fmaf(g[12], c8 * (15.0f * z2 - 3.0f), az);
    ax = fmaf(g[13], c7 * q, ax); az = fmaf(g[13], -10.0f * c7 * xz, az);
    ax = fmaf(g[14], 2.0f * c9 * xz, ax); ay = fmaf(g[14], -2.0f * c9 * yz, ay); az = fmaf(g[14], c9 * (x2 - y2), az);
    ax = fmaf(g[15], c5 * e, ax); ay = fmaf(g[15], 6.0f * c5 * xy, ay);
    gu[0] = ax; gu[1] = ay; gu[2] = az;
}

__global__ void __launch_bounds__(256) NGP_INPUT_GRAD_KERNEL(
    const float* __restrict__ xyzs, const float* __restrict__ dirs, int64_t n, const int64_t* __restrict__ n_dev,
    const int32_t* __restrict__ sidx, GridArgs ga, const uint32_t* __restrict__ table,
    const _Float16* __restrict__ mlp, const _Float16* __restrict__ enc, const float* __restrict__ dL_drgb,
    const float* __restrict__ denc, int act, float* __restrict__ dL_dx, float* __restrict__ dL_dd NGP_ENC_STRIDE_PARAM) {
    __shared__ __attribute__((aligned(16))) _Float16 sw[SWF];
    __shared__ LevelLds lv;
    const bool want_d = dL_dd != nullptr;  // (block-uniform)
    if (want_d) load_fwd_weights_direct(mlp, sw, true);
    load_levels(ga, lv);
    __syncthreads();
    const int64_t N = ngp_capped_count(n_dev, n);
    const int lane = threadIdx.x & 63, s = lane & 15, g = lane >> 4;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t base = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16; base < N; base += nw * 16) {
        const int64_t j = base + s;  // row of the list (denc row); sample i
        const bool valid = j < N;
        const int64_t i = valid && sidx ? (int64_t)sidx[j] : j;
        // ---- position: levels 4g..4g+3 of sample s
        float in[3];
        load_x01(xyzs, i, valid, ga, in);
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 da = valid ? *reinterpret_cast<const float4*>(denc + j * 32 + 8 * g) : z4;
        const float4 db = valid ? *reinterpret_cast<const float4*>(denc + j * 32 + 8 * g + 4) : z4;
        float gx[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
        for (int jl = 0; jl < 4; ++jl) {  // (rolled: one copy of the index code; the pair by selects, not by indexing)
            const float d0 = jl == 0 ? da.x : jl == 1 ? da.z : jl == 2 ? db.x : db.z;
            const float d1 = jl == 0 ? da.y : jl == 1 ? da.w : jl == 2 ? db.y : db.w;
            level_pos_grad(in, 4 * g + jl, lv, table, d0, d1, gx);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float v = wave_xor_add(wave_xor_add(gx[d], 16), 32);  // (g0 + g1) + (g2 + g3)
            if (valid && g == 0) dL_dx[3 * i + d] = v / (ga.g.xyz_max[d] - ga.g.xyz_min[d]);
        }
        if (!want_d) continue;
        // ---- direction: the forward again, through the forward's functions
        const h8 e = valid ? NGP_ENC_ROW(enc, i, g) : h8{0, 0, 0, 0, 0, 0, 0, 0};
        h4 h1[4];
        const h4 hh = density_net(e, sw, s, g, h1);
        const float dx = valid ? dirs[3 * i] : 0.f, dy = valid ? dirs[3 * i + 1] : 0.f, dz = valid ? dirs[3 * i + 2] : 1.f;
        float sh[4];
        sh4_select(dx, dy, dz, g, sh);
        const h8 cin = {(_Float16)sh[0], (_Float16)sh[1], (_Float16)sh[2], (_Float16)sh[3], hh[0], hh[1], hh[2], hh[3]};
        h4 h3[4], h4v[4];
        const h4 o = color_net(cin, sw, s, g, h3, h4v);
        float dout[3];  // rows 0..2 of the output sit in lane group 0
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float gr = valid ? dL_drgb[3 * i + r] : 0.f;
            dout[r] = __shfl(rgb_out_grad(o[r], gr, act), s, 64);
        }
        // da4 of the lane's units 16t + 4g + r: W5^T dout, masked (W5 rows r', permuted columns)
        float a4[4][4], a3[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = 32 * (t >> 1) + 8 * g + 4 * (t & 1);  // P64inv(16t + 4g + r) = col + r
#pragma unroll
            for (int r = 0; r < 4; ++r) a4[t][r] = 0.f;
#pragma unroll
            for (int rr = 0; rr < 3; ++rr) {
                const h4 w = lds4h(sw + SW5 + rr * R64 + col);
#pragma unroll
                for (int r = 0; r < 4; ++r) a4[t][r] = fmaf((float)w[r], dout[rr], a4[t][r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                a4[t][r] = (float)h4v[t][r] > 0.f ? a4[t][r] : 0.f;
                a3[t][r] = 0.f;
            }
        }
        // da3 = relu'(h3) * W4^T da4: input gradient k = 16t + 4g' + r comes from lane (s, g'), k ascending;
        // row k of W4's image holds this lane's units of tiles 2q, 2q+1 at columns 32q + 8g .. + 7
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int gs = 0; gs < 4; ++gs)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * t + 4 * gs + r;
                    const float gk = __shfl(a4[t][r], s + 16 * gs, 64);
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const h8 w = lds8(sw + SW4 + k * R64 + 32 * q + 8 * g);
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            a3[2 * q][c] = fmaf((float)w[c], gk, a3[2 * q][c]);
                            a3[2 * q + 1][c] = fmaf((float)w[4 + c], gk, a3[2 * q + 1][c]);
                        }
                    }
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) unit_fence(a3[tt]);
                }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) a3[t][r] = (float)h3[t][r] > 0.f ? a3[t][r] : 0.f;
        // dSH[4g + c] = sum_k W3[k][4g + c] da3[k] (the SH columns of W3's image: 8g + c)
        float ds[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int gs = 0; gs < 4; ++gs)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * t + 4 * gs + r;
                    const float gk = __shfl(a3[t][r], s + 16 * gs, 64);
                    const h4 w = lds4h(sw + SW3 + k * R32 + 8 * g);
#pragma unroll
                    for (int c = 0; c < 4; ++c) ds[c] = fmaf((float)w[c], gk, ds[c]);
                    unit_fence(ds);
                }
        float dsh[16];
#pragma unroll
        for (int gs = 0; gs < 4; ++gs)
#pragma unroll
            for (int c = 0; c < 4; ++c) dsh[4 * gs + c] = __shfl(ds[c], s + 16 * gs, 64);
        // through SH4 and the normalisation (x, y, z as sh4_select forms them)
        const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
        const float x = ((dx / nrm + 1) / 2) * 2.f - 1.f;
        const float y = ((dy / nrm + 1) / 2) * 2.f - 1.f;
        const float z = ((dz / nrm + 1) / 2) * 2.f - 1.f;
        float gu[3];
        sh4_grad(x, y, z, dsh, gu);
        const float dot = x * gu[0] + y * gu[1] + z * gu[2];
        if (valid && g == 0) {
            dL_dd[3 * i] = (gu[0] - x * dot) / nrm;
            dL_dd[3 * i + 1] = (gu[1] - y * dot) / nrm;
            dL_dd[3 * i + 2] = (gu[2] - z * dot) / nrm;
        }
    }
}

#ifndef NGP_ENC_PAIR_MAJOR
// Per ray r of rays_a (ray index, start, N): sums over its samples [start, start + N).
__global__ void __launch_bounds__(256) ray_segment_sum_kernel(const float* __restrict__ dL_dx,
                                                              const float* __restrict__ dL_dd,
                                                              const float* __restrict__ ts, int64_t n_samples,
                                                              const int64_t* __restrict__ rays_a, int64_t n_rays,
                                                              float* __restrict__ dL_do, float* __restrict__ dL_drd) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n_rays) return;
    const int64_t ray = rays_a[3 * row], start = rays_a[3 * row + 1];
    int64_t cnt = rays_a[3 * row + 2];
    if (ray < 0 || ray >= n_rays) return;
    if (start < 0 || cnt < 0 || start > n_samples || cnt > n_samples - start) {  // a segment outside the samples: none of it
        if (lane == 0) ngp_guard_hit();
        cnt = 0;
    }
    float so[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f};
    for (int64_t k = lane; k < cnt; k += 64) {
        const int64_t i = start + k;
        const float t = ts[i];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float gxd = dL_dx[3 * i + d];
            so[d] += gxd;
            float term = t * gxd;
            if (dL_dd) term += dL_dd[3 * i + d];
            sd[d] += term;
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        so[d] = wave_sum(so[d]);
        sd[d] = wave_sum(sd[d]);
    }
    if (lane < 3) {
        dL_do[3 * ray + lane] = lane == 0 ? so[0] : lane == 1 ? so[1] : so[2];
        dL_drd[3 * ray + lane] = lane == 0 ? sd[0] : lane == 1 ? sd[1] : sd[2];
    }
}

#endif  // NGP_ENC_PAIR_MAJOR

}  // namespace ngp

using namespace ngp;

#ifdef NGP_ENC_PAIR_MAJOR
extern "C" int ngp_field_input_grad_pm(const float* xyzs, const float* dirs, int64_t n, const int64_t* n_dev,
                                       const int32_t* sample_idx, const ngp_hashgrid_t* grid, const void* table_f16,
                                       const void* mlp_f16, const void* enc_f16, int64_t enc_pm_stride,
                                       const float* dL_drgbs, const float* denc, int rgb_act, float* dL_dxyzs,
                                       float* dL_ddirs, void* stream) {
    NGP_CHECK_ARG(rgb_act >= NGP_RGB_SIGMOID && rgb_act <= NGP_RGB_RELU);
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n >= 0 && enc_pm_stride > 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(n <= INT32_MAX);  // rows are listed as int32
    NGP_CHECK_ARG(xyzs && table_f16 && denc && dL_dxyzs && ((uintptr_t)denc & 15) == 0);
    if (dL_ddirs) {
        NGP_CHECK_ARG(dirs && mlp_f16 && enc_f16 && dL_drgbs);
        NGP_CHECK_ARG(((uintptr_t)mlp_f16 & 15) == 0 && ((uintptr_t)enc_f16 & 7) == 0);
    }
    hipStream_t s = as_stream(stream);
    static const unsigned cap = resident_blocks(field_input_grad_pm_kernel, 256, 0);
    NGP_TIMED(NGP_K_INPUT_GRAD, s, field_input_grad_pm_kernel<<<persistent_blocks(n, 64, cap), 256, 0, s>>>(
        xyzs, dirs, n, n_dev, sample_idx, ga, (const uint32_t*)table_f16, (const _Float16*)mlp_f16,
        (const _Float16*)enc_f16, dL_drgbs, denc, rgb_act, dL_dxyzs, dL_ddirs, enc_pm_stride));
    return ngp_launch_status();
}
#else
extern "C" int ngp_field_input_grad(const float* xyzs, const float* dirs, int64_t n, const int64_t* n_dev,
                                    const int32_t* sample_idx, const ngp_hashgrid_t* grid, const void* table_f16,
                                    const void* mlp_f16, const void* enc_f16, const float* dL_drgbs,
                                    const float* denc, int rgb_act, float* dL_dxyzs, float* dL_ddirs, void* stream) {
    NGP_CHECK_ARG(rgb_act >= NGP_RGB_SIGMOID && rgb_act <= NGP_RGB_RELU);
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n >= 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(n <= INT32_MAX);  // rows are listed as int32
    NGP_CHECK_ARG(xyzs && table_f16 && denc && dL_dxyzs && ((uintptr_t)denc & 15) == 0);
    if (dL_ddirs) {
        NGP_CHECK_ARG(dirs && mlp_f16 && enc_f16 && dL_drgbs);
        NGP_CHECK_ARG(((uintptr_t)mlp_f16 & 15) == 0 && ((uintptr_t)enc_f16 & 15) == 0);
    }
    hipStream_t s = as_stream(stream);
    static const unsigned cap = resident_blocks(field_input_grad_kernel, 256, 0);
    NGP_TIMED(NGP_K_INPUT_GRAD, s, field_input_grad_kernel<<<persistent_blocks(n, 64, cap), 256, 0, s>>>(
        xyzs, dirs, n, n_dev, sample_idx, ga, (const uint32_t*)table_f16, (const _Float16*)mlp_f16,
        (const _Float16*)enc_f16, dL_drgbs, denc, rgb_act, dL_dxyzs, dL_ddirs));
    return ngp_launch_status();
}

extern "C" int ngp_ray_segment_sum(const float* dL_dxyzs, const float* dL_ddirs, const float* ts, int64_t n_samples,
                                   const int64_t* rays_a, int64_t n_rays, float* dL_drays_o, float* dL_drays_d,
                                   void* stream) {
    NGP_CHECK_ARG(n_rays >= 0 && n_samples >= 0);
    if (n_rays == 0) return NGP_OK;
    NGP_CHECK_ARG(rays_a && dL_drays_o && dL_drays_d && (n_samples == 0 || (dL_dxyzs && ts)));
    NGP_CHECK_ARG((n_rays + 3) / 4 <= 0x7fffffffLL);
    hipStream_t s = as_stream(stream);
    NGP_TIMED(NGP_K_RAY_SEGSUM, s, ray_segment_sum_kernel<<<(unsigned)((n_rays + 3) / 4), 256, 0, s>>>(
        dL_dxyzs, dL_ddirs, ts, n_samples, rays_a, n_rays, dL_drays_o, dL_drays_d));
    return ngp_launch_status();
}
#endif  // NGP_ENC_PAIR_MAJOR
