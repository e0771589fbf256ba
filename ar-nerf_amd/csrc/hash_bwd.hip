// The atomic hash-table backward over grid.h's level arithmetic: all levels for the API path (also called by
// field_bwd.hip's composed backward), the coarse levels of the training step (the fine ones: hashbin.hip), with
// the coarsest levels' gradient replicas and their fold.
#pragma clang fp contract(off)

#include <algorithm>

#include "common.h"
#include "grid.h"

namespace ngp {

// One level of the coarse (atomic) hash backward for the wave's 16 consecutive
// samples, lane = 4 s + 2 cx + f: corner c = cx | cy << 1 | cz << 2 of sample s
// receives w_c * gd (gd = dL/denc[s][2 l + f]); runs of equal corners along the
// 16 samples (lanes 4 apart) are merged by segmented suffix sums, and each
// run's head adds its sum with one memory-side fp32 atomic into dst.
// coarse_level_runs: the corner indices (idx[yz], level-offset included), the
// run sums v[yz] and the run-head masks of one level; coarse_scatter_level
// then adds each head's sum with a memory-side atomic.
__device__ __forceinline__ void coarse_level_runs(const float in[3], bool valid, float gd, int l, const LevelLds& lv,
                                                  int lane, int cx, uint32_t idx[4], float v[4], uint64_t heads[4]) {
    const float sc = lv.scale[l];
    const uint32_t res = lv.res[l], size = lv.size[l], off = lv.off[l];
    const bool dense = (lv.dense >> l) & 1u, pow2 = (lv.pow2 >> l) & 1u;
    float pos[3];
    uint32_t pg[3];
    level_cell(sc, in, pg, pos);
    // corner c = cx | (cy<<1) | (cz<<2); weight product in tcnn's d order.
    // The four y/z corners are independent: their shuffles are issued
    // together (one LDS round trip per scan step, not four).
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) {
        const int cy = yz & 1, cz = yz >> 1;
        float wt = 1.0f;
        wt *= cx ? pos[0] : 1 - pos[0];
        wt *= cy ? pos[1] : 1 - pos[1];
        wt *= cz ? pos[2] : 1 - pos[2];
        idx[yz] = valid ? off + corner_index(pg[0] + cx, pg[1] + cy, pg[2] + cz, res, size, dense, pow2)
                        : 0xffffffffu;
        v[yz] = wt * gd;
    }
    uint32_t prev[4];
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) prev[yz] = __shfl_up(idx[yz], 4, 64);
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) heads[yz] = __ballot(lane < 4 || prev[yz] != idx[yz]);
    if ((heads[0] & heads[1] & heads[2] & heads[3]) != ~0ull) {
        // some runs: segmented suffix sums at lane stride 4
#pragma unroll
        for (int o4 = 4; o4 < 64; o4 <<= 1) {
            float ov[4];
#pragma unroll
            for (int yz = 0; yz < 4; ++yz) ov[yz] = __shfl_down(v[yz], o4, 64);
            // lanes lane+4, lane+8, ..., lane+o4 must all continue the run
            const uint64_t span = ((0x1111111111111111ull & ((2ull << o4) - 1ull)) & ~1ull) << lane;
#pragma unroll
            for (int yz = 0; yz < 4; ++yz)
                if (lane + o4 < 64 && (heads[yz] & span) == 0) v[yz] += ov[yz];
        }
    }
}

__device__ __forceinline__ void coarse_scatter_level(const float in[3], bool valid, float gd, int l, const LevelLds& lv,
                                                     float* __restrict__ dst, int lane, int cx, int f) {
    uint32_t idx[4];
    float v[4];
    uint64_t heads[4];
    coarse_level_runs(in, valid, gd, l, lv, lane, cx, idx, v, heads);
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) {
        const bool head = (heads[yz] >> lane) & 1ull;
        if (head && valid) atomicAdd(&dst[2 * (size_t)idx[yz] + f], v[yz]);
    }
}

// Kernel B: hash-table gradient scatter, dL/dtable[e][f] += w_c * dL/denc[2l+f].
// Lane map: 16 consecutive samples per wave, 4 lanes per sample:
//   lane = 4*s + 2*cx + f  (cx = the corner's x bit, f = feature).
// One wave instruction then carries, per sample, the x-adjacent corner pair
// x both features: 4 floats that sit in 16 contiguous bytes whenever the two
// entries are neighbours (dense levels; hashed levels when px is even, since
// the x term of the hash is px*1), so the atomics leave as one request per
// sample instead of four scattered ones.  Samples of one ray are consecutive,
// so equal indices of the same (cx, f) at lane stride 4 are first summed by a
// segmented suffix scan; only each run's head issues its fp32 atomic.
// Levels [lo, hi) (the hybrid backward's atomic coarse levels; [0, L) for
// the all-atomic API path).
__global__ void __launch_bounds__(256) hash_bwd_kernel(const float* __restrict__ xyzs, int64_t n,
                                                       const int64_t* __restrict__ n_dev,
                                                       const int32_t* __restrict__ sidx, GridArgs ga,
                                                       const float* __restrict__ denc, float* __restrict__ grad,
                                                       int lo, int hi, float* __restrict__ rep = nullptr,
                                                       int rep_hi = 0, uint32_t rep_stride = 0, int nrep = 1) {
    // levels below rep_hi add into this block's replica of their gradient
    // range (ngp_hash_backward_levels_rep): the coarsest levels are a few
    // hundred KB that every sample touches, so their memory-side atomics
    // queue on few lines; nrep copies spread them (summed afterwards)
    float* const grep = rep ? rep + (size_t)(blockIdx.x % nrep) * rep_stride : grad;
    __shared__ LevelLds lv;
    // the wave's 16 denc rows, staged once per iteration with coalesced 16-B
    // loads (one global round trip instead of one per level)
    __shared__ __attribute__((aligned(16))) float drow[4][16][36];
    NGP_PROBE_BEGIN(NGP_P_HASH_BWD_COARSE);
    load_levels(ga, lv);
    __syncthreads();
    const int64_t N = ngp_capped_count(n_dev, n);  // (a device count never past the capacity: a guard hit)
    const int lane = threadIdx.x & 63, s = lane >> 2, cx = (lane >> 1) & 1, f = lane & 1, wv = threadIdx.x >> 6;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t base = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wv) * 16; base < N; base += nw * 16) {
        const int64_t j = base + s;  // compact position (denc row)
        const bool valid = j < N;
        const int64_t i = valid && sidx ? (int64_t)sidx[j] : j;  // sample
        {
            // lane (s, q = lane & 3) copies floats [8q, 8q+8) of row j
            const int q = lane & 3;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (valid && 8 * q + 8 > 2 * lo && 8 * q < 2 * hi) {
                a = *reinterpret_cast<const float4*>(denc + j * 32 + 8 * q);
                b = *reinterpret_cast<const float4*>(denc + j * 32 + 8 * q + 4);
            }
            __builtin_amdgcn_wave_barrier();  // previous iteration's reads of drow are done (in order per wave)
            *reinterpret_cast<float4*>(&drow[wv][s][8 * q]) = a;
            *reinterpret_cast<float4*>(&drow[wv][s][8 * q + 4]) = b;
        }
        float in[3];
        load_x01(xyzs, i, valid, ga, in);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 1
        for (int l = lo; l < hi; ++l)
            coarse_scatter_level(in, valid, drow[wv][s][2 * l + f], l, lv, l < rep_hi ? grep : grad, lane, cx, f);
    }
    NGP_PROBE_END();
}

constexpr unsigned HASH_BWD_BLOCKS = 8192;  // grid cap of hash_bwd_kernel, all-level API path (2048 measured slower)
// grid cap of the training step's coarse levels (launch_coarse): 2048 waves, two per SIMD.  Round 5: its
// atomics spread over a longer span beside the record write, now that the coarse levels' Adam runs beside
// the accumulation and no longer waits on it -- with the prefetch-free accumulation +1.2-1.3 %; round 6
// re-check: 256 / 1024 / 2048 blocks -3.2 / -0.5 / -1.2 %, profiles/r06/ab/coarse_grid.txt;
// profiles/r05/ab/round5_ab.txt r5ee / r5ff (rounds 2-4: 8192, when a longer coarse kernel delayed that Adam)
constexpr unsigned COARSE_BLOCKS = 512;

// grad[i] += sum_r rep[r][i]; rep[r][i] = 0 (i < n4 float4 groups), replicas
// summed in order r = 0..nrep-1; all of a lane's loads are issued first
template <int MAXR>
__global__ void __launch_bounds__(256) rep_reduce_kernel(float* __restrict__ grad, float* __restrict__ rep,
                                                         uint32_t n4, uint32_t stride4, int nrep) {
    float4* g4 = reinterpret_cast<float4*>(grad);
    float4* r4 = reinterpret_cast<float4*>(rep);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
        float4 b[MAXR];
#pragma unroll
        for (int r = 0; r < MAXR; ++r)
            if (r < nrep) b[r] = r4[(size_t)r * stride4 + i];
        float4 a = g4[i];
#pragma unroll
        for (int r = 0; r < MAXR; ++r)
            if (r < nrep) {
                a.x += b[r].x; a.y += b[r].y; a.z += b[r].z; a.w += b[r].w;
                r4[(size_t)r * stride4 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        g4[i] = a;
    }
}

}  // namespace ngp

using namespace ngp;

static void launch_coarse(const float* xyzs, int64_t n, const int64_t* n_dev, const int32_t* sample_idx,
                          const GridArgs& ga, const float* denc, float* grad_table, int lo, int hi, float* rep,
                          int rep_hi, uint32_t rep_stride, int nrep, hipStream_t s) {
    NGP_TIMED(NGP_K_HASH_BWD_COARSE, s, hash_bwd_kernel<<<persistent_blocks(n, 64, COARSE_BLOCKS), 256, 0, s>>>(
        xyzs, n, n_dev, sample_idx, ga, denc, grad_table, lo, hi, rep, rep_hi, rep_stride, nrep));
}

extern "C" {

int ngp_hash_backward(const float* xyzs, int64_t n, const int64_t* n_dev, const int32_t* sample_idx,
                      const ngp_hashgrid_t* grid, const float* denc, float* grad_table, void* stream) {
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n >= 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(xyzs && denc && grad_table && ((uintptr_t)denc & 15) == 0);
    NGP_TIMED(NGP_K_HASH_BWD_COARSE, as_stream(stream), hash_bwd_kernel<<<persistent_blocks(n, 64, HASH_BWD_BLOCKS), 256, 0, as_stream(stream)>>>(xyzs, n, n_dev, sample_idx,
                                                                                     ga, denc, grad_table, 0, L));
    return ngp_launch_status();
}

int ngp_hash_backward_levels(const float* xyzs, int64_t n, const int64_t* n_dev, const int32_t* sample_idx,
                             const ngp_hashgrid_t* grid, const float* denc, float* grad_table, int level_lo,
                             int level_hi, void* stream) {
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n >= 0 && 0 <= level_lo && level_lo <= level_hi && level_hi <= L);
    if (n == 0 || level_lo == level_hi) return NGP_OK;
    NGP_CHECK_ARG(xyzs && denc && grad_table && ((uintptr_t)denc & 15) == 0);
    launch_coarse(xyzs, n, n_dev, sample_idx, ga, denc, grad_table, level_lo, level_hi, nullptr, 0, 0, 1,
                  as_stream(stream));
    return ngp_launch_status();
}

int ngp_hash_backward_levels_rep(const float* xyzs, int64_t n, const int64_t* n_dev, const int32_t* sample_idx,
                                 const ngp_hashgrid_t* grid, const float* denc, float* grad_table, int level_lo,
                                 int level_hi, float* rep, int rep_levels, int n_rep, int fold, void* stream) {
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n >= 0 && 0 <= level_lo && level_lo <= level_hi && level_hi <= L);
    NGP_CHECK_ARG(0 <= rep_levels && rep_levels <= level_hi && n_rep >= 1 && n_rep <= 64);
    if (rep_levels == 0 || !rep)
        return ngp_hash_backward_levels(xyzs, n, n_dev, sample_idx, grid, denc, grad_table, level_lo, level_hi,
                                        stream);
    if (n == 0 || level_lo == level_hi) return NGP_OK;
    NGP_CHECK_ARG(xyzs && denc && grad_table && ((uintptr_t)denc & 15) == 0);
    NGP_CHECK_ARG(((uintptr_t)grad_table & 15) == 0 && ((uintptr_t)rep & 15) == 0);
    // replicas cover table entries [0, offsets[rep_levels]) (x 2 features)
    const uint32_t nfl = 2u * grid->offsets[rep_levels];
    NGP_CHECK_ARG(nfl % 4 == 0);
    hipStream_t s = as_stream(stream);
    launch_coarse(xyzs, n, n_dev, sample_idx, ga, denc, grad_table, level_lo, level_hi, rep, rep_levels, nfl, n_rep, s);
    if (!fold) return ngp_launch_status();  // the caller folds them (ngp_adam_step_dev_rep)
    const uint32_t n4 = nfl / 4;
    const unsigned rb = std::min(2048u, (n4 + 255) / 256);
    if (n_rep <= 8)
        NGP_TIMED(NGP_K_HASH_BWD_COARSE, s, rep_reduce_kernel<8><<<rb, 256, 0, s>>>(grad_table, rep, n4, n4, n_rep));
    else if (n_rep <= 16)
        NGP_TIMED(NGP_K_HASH_BWD_COARSE, s, rep_reduce_kernel<16><<<rb, 256, 0, s>>>(grad_table, rep, n4, n4, n_rep));
    else
        NGP_TIMED(NGP_K_HASH_BWD_COARSE, s, rep_reduce_kernel<64><<<rb, 256, 0, s>>>(grad_table, rep, n4, n4, n_rep));
    return ngp_launch_status();
}

size_t ngp_hash_backward_rep_floats(const ngp_hashgrid_t* grid, int rep_levels, int n_rep) {
    if (!grid || rep_levels < 0 || rep_levels > L || n_rep < 1) return 0;
    return (size_t)n_rep * 2u * grid->offsets[rep_levels];
}

}  // extern "C"
