// The occupancy-grid update: last-write-wins scatter of the sampled sigmas,
// the occupied-cell list and the cell sampling on the device, the kept
// positions of the sorted sample list, and the EMA / threshold of the density
// grid.  Replaces (models/networks.py:181-207, 252-281).
#pragma clang fp contract(off)

#include "common.h"
#include "wave.h"
#include "zero_words.h"

namespace ngp {

// --------------------------------------------------- occupancy grid update
// density_grid_tmp[c, idx] = sigma (models/networks.py:268) as a torch
// index_put_ over the cell list: with duplicate cells the LAST write in list
// order wins (torch's sequential semantics; sample_uniform_and_occupied_cells
// draws i.i.d., so a duplicated cell keeps its last draw's sigma, and a cell
// drawn in both halves keeps the occupied-half draw).  Each sample i at list
// position pos_base + i leaves the 64-bit key ((pos + 1) << 32 | sigma bits)
// with a 64-bit atomicMax, so the largest position wins independently of
// execution order; ranks sharding the list combine their key grids with a MAX
// all-reduce, the same rule across ranks.  Negative indices are skipped
// (occupancy samples that do not exist: no occupied cell to resample).
__global__ void scatter_last_kernel(const int64_t* __restrict__ idx, const float* __restrict__ sig, int64_t n,
                                    int64_t pos_base, unsigned long long* __restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t j = idx[i];
    if (j < 0) return;
    const unsigned long long k = ((unsigned long long)(pos_base + i + 1) << 32) | __float_as_uint(fmaxf(sig[i], 0.f));
    atomicMax(key + j, k);
}

// ---------------------------------------- occupancy cell sampling on device
// sample_uniform_and_occupied_cells (models/networks.py:181-207) without the
// host sync of torch.nonzero: occ_count_kernel + occ_list_kernel list the
// cells of one cascade with density > threshold in ascending cell order, as
// torch.nonzero does (two launches: per-block counts, then each block sums
// the counts of the blocks before it and writes its run -- deterministic, so
// every rank of a data-parallel job builds the same list);
// occ_sample_kernel draws M uniform cells and M cells uniformly from that
// list (none if it is empty, as the reference's empty nonzero gives none)
// and their jittered world positions (networks.py:262-266).
constexpr int OCC_T = 1024, OCC_PER = 8, OCC_CHUNK = OCC_T * OCC_PER;  // cells per block

__device__ __forceinline__ uint32_t occ_hits(const float* __restrict__ grid_c, int64_t n_cells, float thr, int64_t c0,
                                             bool hit[OCC_PER]) {
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < OCC_PER; ++k) {
        hit[k] = c0 + k < n_cells && grid_c[c0 + k] > thr;
        mine += hit[k];
    }
    return mine;
}

__global__ void __launch_bounds__(OCC_T) occ_count_kernel(const float* __restrict__ grid_c, int64_t n_cells, float thr,
                                                          uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t wcnt[OCC_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    bool hit[OCC_PER];
    const uint32_t v = wave_sum(occ_hits(grid_c, n_cells, thr, ((int64_t)blockIdx.x * OCC_T + tid) * OCC_PER, hit));
    if (lane == 0) wcnt[wid] = v;
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < OCC_T / 64; ++w) tot += wcnt[w];
        block_counts[blockIdx.x] = tot;
    }
}

__global__ void __launch_bounds__(OCC_T) occ_list_kernel(const float* __restrict__ grid_c, int64_t n_cells, float thr,
                                                         const uint32_t* __restrict__ block_counts,
                                                         int32_t* __restrict__ list,
                                                         unsigned long long* __restrict__ count) {
    __shared__ uint32_t wcnt[OCC_T / 64];
    __shared__ unsigned long long wbase[OCC_T / 64];
    __shared__ unsigned long long base;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // this block's base: the counts of the blocks before it, summed by every
    // wave over a strided share (a few hundred words, L2-resident)
    unsigned long long before = 0ull;
    for (int64_t b = tid; b < (int64_t)blockIdx.x; b += OCC_T) before += block_counts[b];
    before = wave_sum(before);
    if (lane == 0) wbase[wid] = before;
    bool hit[OCC_PER];
    const int64_t c0 = ((int64_t)blockIdx.x * OCC_T + tid) * OCC_PER;
    const uint32_t mine = occ_hits(grid_c, n_cells, thr, c0, hit);
    const uint32_t incl = wave_incl_scan(mine, lane);
    if (lane == 63) wcnt[wid] = incl;
    __syncthreads();
    if (tid == 0) {
        unsigned long long b = 0ull;
        for (int w = 0; w < OCC_T / 64; ++w) b += wbase[w];
        uint32_t tot = 0;
        for (int w = 0; w < OCC_T / 64; ++w) { const uint32_t v = wcnt[w]; wcnt[w] = tot; tot += v; }
        base = b;
        if (blockIdx.x == gridDim.x - 1) *count = b + tot;
    }
    __syncthreads();
    // (the list holds at most n_cells entries: a base past that can only come
    // from corrupted counts -- dropped instead of written)
    if (base > (unsigned long long)n_cells) {
        if (tid == 0) ngp_guard_hit();
        return;
    }
    int64_t pos = (int64_t)base + wcnt[wid] + incl - mine;
#pragma unroll
    for (int k = 0; k < OCC_PER; ++k)
        if (hit[k] && pos < n_cells) list[pos++] = (int32_t)(c0 + k);
}

__global__ void __launch_bounds__(256) occ_sample_kernel(uint64_t seed, const int64_t* __restrict__ ctr, int cascade,
                                                         int G, int64_t M, float s_minus_hgs, float hgs,
                                                         const int32_t* __restrict__ list,
                                                         const unsigned long long* __restrict__ count, int64_t lo,
                                                         int64_t hi, float* __restrict__ xyzs,
                                                         int64_t* __restrict__ flat) {
    const int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hi) return;
    const int64_t o = i - lo;
    const uint64_t step = (uint64_t)*ctr;
    const uint4 u = philox4x32(make_uint4((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)step, (uint32_t)cascade),
                               make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    int32_t idx;
    if (i < M) {  // uniform cell: torch.randint(G, (M, 3)) then morton3D
        const uint4 v = philox4x32(make_uint4((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)step, 0x9E3779B9u ^ cascade),
                                   make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
        idx = (int32_t)morton3((uint32_t)uniform_index(v.x, G), (uint32_t)uniform_index(v.y, G),
                               (uint32_t)uniform_index(v.z, G));
    } else {  // a cell drawn from the occupied list
        const unsigned long long cnt0 = *count, cnt = min(cnt0, (unsigned long long)G * G * G);  // (guard: list capacity)
        if (cnt0 != cnt && i == (lo > M ? lo : M)) ngp_guard_hit();
        if (cnt == 0) {
            flat[o] = -1;
            xyzs[3 * o] = 0.f; xyzs[3 * o + 1] = 0.f; xyzs[3 * o + 2] = 0.f;
            return;
        }
        idx = list[uniform_index(u.w, (int64_t)cnt)];
    }
    const uint32_t cx = compact3((uint32_t)idx), cy = compact3((uint32_t)idx >> 1), cz = compact3((uint32_t)idx >> 2);
    // xyzs_w = (coords / (G-1) * 2 - 1) * (s - hgs) + (rand * 2 - 1) * hgs, fp32 as torch evaluates it
    const float gm1 = (float)(G - 1);
    const float jr[3] = {(float)(u.x >> 8) * (1.0f / 16777216.0f), (float)(u.y >> 8) * (1.0f / 16777216.0f),
                         (float)(u.z >> 8) * (1.0f / 16777216.0f)};
    const uint32_t cc[3] = {cx, cy, cz};
#pragma unroll
    for (int d = 0; d < 3; ++d) xyzs[3 * o + d] = ((float)cc[d] / gm1 * 2.0f - 1.0f) * s_minus_hgs + (jr[d] * 2.0f - 1.0f) * hgs;
    flat[o] = (int64_t)cascade * G * G * G + idx;
}

// Sorted variant: the same two multisets of cells (M i.i.d. uniform cells, M
// i.i.d. uniform picks from the occupied list) emitted in ascending order, so
// that a wave's points share cache lines on the coarse hash levels (the
// density forward of the 1M points runs ~1.8x faster Morton-sorted than in
// draw order: scripts/diag/density_order.py).  Ascending i.i.d. uniforms are
// drawn directly as order statistics, U_(k) = S_k / S_M with S the running
// sum of M+1 i.i.d. Exp(1) variates (fp64), so no sort is needed: three
// launches -- block sums, one scan of the block sums, then each block
// regenerates its exponentials, scans them and writes its samples.
constexpr int OSC_T = 256, OSC_PER = 16, OSC_CH = OSC_T * OSC_PER;  // exponentials per block

__device__ __forceinline__ double occ_exp(uint64_t seed, uint64_t step, int cascade, int half, int64_t k) {
    const uint4 v = philox4x32(make_uint4((uint32_t)k, (uint32_t)(k >> 32), (uint32_t)step,
                                          0x7F4A7C15u ^ (uint32_t)(cascade << 1) ^ (uint32_t)half),
                               make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    const double u = ((double)(v.x >> 11) + 1.0) * (1.0 / 2097152.0);  // (0, 1], 21 bits
    const double u2 = u + (double)(v.y >> 11) * (1.0 / 2097152.0 / 2097152.0);  // 42-bit uniform
    return -log(fmin(u2, 1.0));
}

__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(OSC_T) occ_exp_sums_kernel(uint64_t seed, const int64_t* __restrict__ ctr,
                                                             int cascade, int64_t M, int64_t nb,
                                                             double* __restrict__ sums) {
    __shared__ double red[OSC_T / 64];
    const int half = (int)(blockIdx.x / nb);
    const int64_t c = blockIdx.x % nb;
    const uint64_t step = (uint64_t)*ctr;
    double v = 0.0;
#pragma unroll 4
    for (int j = 0; j < OSC_PER; ++j) {
        const int64_t k = c * OSC_CH + (int64_t)j * OSC_T + threadIdx.x;
        if (k <= M) v += occ_exp(seed, step, cascade, half, k);
    }
    v = block_sum_d(v, red);
    if (threadIdx.x == 0) sums[blockIdx.x] = v;
}

// exclusive prefix of the block sums within each half (in place), totals
// after; one workgroup per half, 1024 sums per round
__global__ void __launch_bounds__(1024) occ_exp_scan_kernel(int64_t nb, double* __restrict__ sums) {
    __shared__ double wsum[16];
    __shared__ double carry_s;
    double* p = sums + blockIdx.x * nb;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) carry_s = 0.0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
        const int64_t b = b0 + t;
        const double v = b < nb ? p[b] : 0.0;
        const double incl = wave_incl_scan(v, lane);
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        double before = carry_s;
        for (int q = 0; q < w; ++q) before += wsum[q];
        if (b < nb) p[b] = before + incl - v;
        __syncthreads();
        if (t == 1023) carry_s = before + incl;
        __syncthreads();
    }
    if (t == 0) sums[2 * nb + blockIdx.x] = carry_s;
}

__global__ void __launch_bounds__(OSC_T) occ_sample_sorted_kernel(
    uint64_t seed, const int64_t* __restrict__ ctr, int cascade, int G, int64_t M, int64_t nb, float s_minus_hgs,
    float hgs, const int32_t* __restrict__ list, const unsigned long long* __restrict__ count,
    const double* __restrict__ sums, int64_t lo, int64_t hi, float* __restrict__ xyzs, int64_t* __restrict__ flat) {
    __shared__ double wsum[OSC_T / 64];
    const int half = (int)(blockIdx.x / nb);
    const int64_t c = blockIdx.x % nb;
    const int64_t i0 = half * M + c * OSC_CH;  // sample index of this block's first exponential
    if (i0 >= hi || i0 + OSC_CH <= lo) return;  // (block-uniform)
    const uint64_t step = (uint64_t)*ctr;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    // thread t takes the OSC_PER consecutive exponentials k0 + t*OSC_PER + j
    const int64_t k0 = c * OSC_CH + (int64_t)t * OSC_PER;
    double e[OSC_PER], loc = 0.0;
#pragma unroll
    for (int j = 0; j < OSC_PER; ++j) {
        e[j] = k0 + j <= M ? occ_exp(seed, step, cascade, half, k0 + j) : 0.0;
        loc += e[j];
    }
    const double incl = wave_incl_scan(loc, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    double run = sums[blockIdx.x];
    for (int q = 0; q < w; ++q) run += wsum[q];
    run += incl - loc;
    const double inv_tot = 1.0 / sums[2 * nb + half];
    const int64_t n_cells = (int64_t)G * G * G;
    const unsigned long long cnt0 = half ? *count : 0ull, cnt = min(cnt0, (unsigned long long)n_cells);  // (guard: capacity)
    if (cnt0 != cnt && threadIdx.x == 0) ngp_guard_hit();
    const float gm1 = (float)(G - 1);
#pragma unroll 1
    for (int j = 0; j < OSC_PER; ++j) {
        run += e[j];
        const int64_t k = k0 + j, i = half * M + k;
        if (k >= M || i < lo || i >= hi) continue;
        const int64_t o = i - lo;
        const double u = run * inv_tot;  // U_(k), ascending in k
        int32_t idx;
        if (!half) {
            idx = (int32_t)min((int64_t)(u * (double)n_cells), n_cells - 1);
        } else {
            if (cnt == 0) {
                flat[o] = -1;
                xyzs[3 * o] = 0.f; xyzs[3 * o + 1] = 0.f; xyzs[3 * o + 2] = 0.f;
                continue;
            }
            idx = list[min((int64_t)(u * (double)cnt), (int64_t)cnt - 1)];
        }
        const uint4 r = philox4x32(make_uint4((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)step, (uint32_t)cascade),
                                   make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
        const uint32_t cc[3] = {compact3((uint32_t)idx), compact3((uint32_t)idx >> 1), compact3((uint32_t)idx >> 2)};
        const float jr[3] = {(float)(r.x >> 8) * (1.0f / 16777216.0f), (float)(r.y >> 8) * (1.0f / 16777216.0f),
                             (float)(r.z >> 8) * (1.0f / 16777216.0f)};
#pragma unroll
        for (int d = 0; d < 3; ++d)
            xyzs[3 * o + d] = ((float)cc[d] / gm1 * 2.0f - 1.0f) * s_minus_hgs + (jr[d] * 2.0f - 1.0f) * hgs;
        flat[o] = (int64_t)cascade * n_cells + idx;
    }
}

// The occupancy samples whose sigma survives density_grid_tmp[c, idx] =
// sigma's last-write-wins (networks.py:268): of the sorted 2M-sample list
// (each half ascending, ngp_occupancy_samples_sorted), position i is kept iff
// no later position holds its cell -- the last of its run within its half
// (duplicates are adjacent there), and, in the uniform half, only if the
// occupied half does not draw the cell at all.  Only kept positions need a
// density evaluation: the others' sigmas would be overwritten.
// occ_mark_kernel: byte per cell, set for every occupied-half cell (plain
// byte stores of one value: no atomics); occ_keep_kernel: the kept positions
// of [lo, hi), compacted per 8192-position block (one reservation per block).
__global__ void __launch_bounds__(256) zero_u4_kernel(uint4* __restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = make_uint4(0u, 0u, 0u, 0u);
}
__global__ void __launch_bounds__(256) occ_mark_kernel(const int64_t* __restrict__ flat, int64_t M, int64_t cell_base,
                                                       int64_t n_cells, uint8_t* __restrict__ mark) {
    const int64_t i = M + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * M) return;
    const int64_t c = flat[i] - cell_base;
    if (c >= 0 && c < n_cells) mark[c] = 1;
}

constexpr int KEEP_T = 1024, KEEP_PER = 8;
__global__ void __launch_bounds__(KEEP_T) occ_keep_kernel(const int64_t* __restrict__ flat, int64_t M,
                                                          int64_t cell_base, int64_t n_cells,
                                                          const uint8_t* __restrict__ mark, int64_t lo, int64_t hi,
                                                          int32_t* __restrict__ list,
                                                          unsigned long long* __restrict__ count) {
    __shared__ uint32_t wcnt[KEEP_T / 64];
    __shared__ unsigned long long base;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t i0 = lo + ((int64_t)blockIdx.x * KEEP_T + tid) * KEEP_PER;
    bool keep[KEEP_PER];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < KEEP_PER; ++k) {
        const int64_t i = i0 + k;
        bool kp = false;
        if (i < hi) {
            const int64_t f = flat[i];
            const int64_t end = i < M ? M : 2 * M;  // the end of i's half
            kp = f >= 0 && (i + 1 == end || flat[i + 1] != f);
            if (kp && i < M) {
                const int64_t c = f - cell_base;
                kp = !(c >= 0 && c < n_cells && mark[c]);
            }
        }
        keep[k] = kp;
        mine += kp;
    }
    const uint32_t incl = wave_incl_scan(mine, lane);
    if (lane == 63) wcnt[wid] = incl;
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < KEEP_T / 64; ++w) { const uint32_t v = wcnt[w]; wcnt[w] = tot; tot += v; }
        base = tot ? atomicAdd(count, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    int64_t pos = (int64_t)base + wcnt[wid] + incl - mine;
#pragma unroll
    for (int k = 0; k < KEEP_PER; ++k)
        if (keep[k]) list[pos++] = (int32_t)(i0 + k);
}

// scatter_last_kernel over the kept positions list[j], j < *count: sample i =
// list[j] (list position pos_base + i) with its cell flat[i] and sigma sig[i]
__global__ void __launch_bounds__(256) scatter_kept_kernel(const int32_t* __restrict__ list,
                                                           const int64_t* __restrict__ count, int64_t n_max,
                                                           const int64_t* __restrict__ flat,
                                                           const float* __restrict__ sig, int64_t pos_base,
                                                           unsigned long long* __restrict__ key) {
    const int64_t nk = ngp_capped_count(count, n_max);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nk; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = list[j];
        const int64_t c = flat[i];
        if (c < 0) continue;
        const unsigned long long k = ((unsigned long long)(pos_base + i + 1) << 32) | __float_as_uint(fmaxf(sig[i], 0.f));
        atomicMax(key + c, k);
    }
}

// models/networks.py:270-278: grid = where(grid<0, grid, max(grid*decay, tmp)),
// decay per cell when decay_cells != nullptr (erode, networks.py:270-272:
// clamp(decay**(1/count_grid), 0.1, 0.95), evaluated once per count grid by the
// caller);
// accumulates sum and count of grid > 0 for the mean, in fp64 so the mean is
// the correctly rounded one whatever the summation order: at initialisation
// every cell holds sigma ~= 1 and the threshold (= that mean) splits them, so
// a last-digit difference in an fp32 sum flips thousands of cells and sends
// training down a different trajectory.
__global__ void __launch_bounds__(256) grid_ema_kernel(float* __restrict__ grid, unsigned long long* __restrict__ key,
                                                       int64_t n, float decay, const float* __restrict__ decay_cells,
                                                       double* __restrict__ sum_cnt) {
    double s = 0.0, c = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float gv = grid[i];
        const float dc = decay_cells ? decay_cells[i] : decay;
        const unsigned long long kv = key[i];
        const float tv = kv ? __uint_as_float((uint32_t)kv) : 0.f;  // density_grid_tmp (zeros where unsampled)
        const float nv = gv < 0 ? gv : fmaxf(gv * dc, tv);
        grid[i] = nv;
        if (kv) key[i] = 0ull;  // consumed: left zeroed for the next update
        if (nv > 0) { s += (double)nv; c += 1.0; }
    }
    s = wave_sum(s);
    c = wave_sum(c);
    __shared__ double ws[2][4];  // one global add pair per block, not per wave
    if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = s; ws[1][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(sum_cnt, (ws[0][0] + ws[0][1]) + (ws[0][2] + ws[0][3]));
        atomicAdd(sum_cnt + 1, (ws[1][0] + ws[1][1]) + (ws[1][2] + ws[1][3]));
    }
}

// threshold = min(mean(grid[grid>0]), thr_max)  (models/networks.py:278-281)
__global__ void grid_threshold_kernel(const double* __restrict__ sum_cnt, float thr_max, float* __restrict__ thr) {
    // Python's min(nan, x) is nan (mean of an empty selection), and packbits
    // against a NaN threshold clears every bit -- reproduce that exactly.
    const float nan = __int_as_float(0x7fc00000);
    const float mean = sum_cnt[1] > 0 ? (float)(sum_cnt[0] / sum_cnt[1]) : nan;
    thr[0] = sum_cnt[1] > 0 ? fminf(mean, thr_max) : nan;
    thr[1] = mean;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_density_scatter_last(const int64_t* indices, const float* sigmas, int64_t n, int64_t pos_base,
                             uint64_t* grid_key, void* stream) {
    NGP_CHECK_ARG(n >= 0 && pos_base >= 0 && pos_base + n < (1ll << 31));
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(indices && sigmas && grid_key && ((uintptr_t)grid_key & 7) == 0);
    scatter_last_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(
        indices, sigmas, n, pos_base, reinterpret_cast<unsigned long long*>(grid_key));
    return ngp_launch_status();
}

size_t ngp_occupied_cells_workspace(int64_t n_cells) {
    return n_cells > 0 ? (size_t)((n_cells + OCC_CHUNK - 1) / OCC_CHUNK) * sizeof(uint32_t) : 0;
}

int ngp_occupied_cells(const float* grid_cascade, int64_t n_cells, float threshold, int32_t* list, int64_t* count,
                       void* workspace, void* stream) {
    NGP_CHECK_ARG(n_cells > 0 && n_cells < (1ll << 31) && grid_cascade && list && count && workspace &&
                  ((uintptr_t)count & 7) == 0 && ((uintptr_t)workspace & 3) == 0);
    hipStream_t s = as_stream(stream);
    const unsigned nb = (unsigned)((n_cells + OCC_CHUNK - 1) / OCC_CHUNK);
    uint32_t* bc = reinterpret_cast<uint32_t*>(workspace);
    occ_count_kernel<<<nb, OCC_T, 0, s>>>(grid_cascade, n_cells, threshold, bc);
    occ_list_kernel<<<nb, OCC_T, 0, s>>>(grid_cascade, n_cells, threshold, bc, list, (unsigned long long*)count);
    return ngp_launch_status();
}

int ngp_occupancy_samples(uint64_t seed, const int64_t* counter_dev, int cascade, int grid_size, int64_t M,
                          float s_minus_hgs, float hgs, const int32_t* occ_list, const int64_t* occ_count, int64_t lo,
                          int64_t hi, float* xyzs, int64_t* flat_idx, void* stream) {
    NGP_CHECK_ARG(counter_dev && occ_list && occ_count && xyzs && flat_idx && grid_size >= 2 && M >= 0 && lo >= 0 &&
                  lo <= hi && hi <= 2 * M && cascade >= 0);
    if (hi == lo) return NGP_OK;
    occ_sample_kernel<<<(unsigned)((hi - lo + 255) / 256), 256, 0, as_stream(stream)>>>(
        seed, counter_dev, cascade, grid_size, M, s_minus_hgs, hgs, occ_list, (const unsigned long long*)occ_count, lo,
        hi, xyzs, flat_idx);
    return ngp_launch_status();
}

size_t ngp_occupancy_sorted_workspace(int64_t M) {
    const int64_t nb = (M + 1 + OSC_CH - 1) / OSC_CH;
    return (size_t)(2 * nb + 2) * sizeof(double);
}

int ngp_occupancy_samples_sorted(uint64_t seed, const int64_t* counter_dev, int cascade, int grid_size, int64_t M,
                                 float s_minus_hgs, float hgs, const int32_t* occ_list, const int64_t* occ_count,
                                 int64_t lo, int64_t hi, void* workspace, float* xyzs, int64_t* flat_idx,
                                 void* stream) {
    NGP_CHECK_ARG(counter_dev && occ_list && occ_count && xyzs && flat_idx && workspace && grid_size >= 2 &&
                  M >= 0 && lo >= 0 && lo <= hi && hi <= 2 * M && cascade >= 0 && ((uintptr_t)workspace & 7) == 0);
    if (hi == lo) return NGP_OK;
    NGP_CHECK_ARG((int64_t)grid_size * grid_size * grid_size <= (1ll << 31));
    hipStream_t s = as_stream(stream);
    const int64_t nb = (M + 1 + OSC_CH - 1) / OSC_CH;
    double* sums = reinterpret_cast<double*>(workspace);
    occ_exp_sums_kernel<<<(unsigned)(2 * nb), OSC_T, 0, s>>>(seed, counter_dev, cascade, M, nb, sums);
    occ_exp_scan_kernel<<<2, 1024, 0, s>>>(nb, sums);
    occ_sample_sorted_kernel<<<(unsigned)(2 * nb), OSC_T, 0, s>>>(seed, counter_dev, cascade, grid_size, M, nb,
                                                                 s_minus_hgs, hgs, occ_list,
                                                                 (const unsigned long long*)occ_count, sums, lo, hi,
                                                                 xyzs, flat_idx);
    return ngp_launch_status();
}

int ngp_occupancy_keep(const int64_t* flat_idx, int64_t M, int64_t cell_base, int64_t n_cells, int64_t lo, int64_t hi,
                       void* mark_ws, int32_t* list, int64_t* count, void* stream) {
    NGP_CHECK_ARG(M >= 0 && n_cells > 0 && cell_base >= 0 && lo >= 0 && lo <= hi && hi <= 2 * M &&
                  hi < (1ll << 31) && flat_idx && mark_ws && list && count && ((uintptr_t)count & 7) == 0);
    NGP_CHECK_ARG(((uintptr_t)mark_ws & 15) == 0);
    hipStream_t s = as_stream(stream);
    zero_words_kernel<<<1, 64, 0, s>>>((unsigned long long*)count, 1);  // (kernel nodes, not memsets: zero_words.h)
    if (hi == lo) return ngp_launch_status();
    const int64_t n16 = (n_cells + 15) / 16;
    zero_u4_kernel<<<(unsigned)((n16 + 255) / 256), 256, 0, s>>>((uint4*)mark_ws, n16);
    if (M > 0)
        occ_mark_kernel<<<(unsigned)((M + 255) / 256), 256, 0, s>>>(flat_idx, M, cell_base, n_cells, (uint8_t*)mark_ws);
    const int64_t per_blk = (int64_t)KEEP_T * KEEP_PER;
    occ_keep_kernel<<<(unsigned)((hi - lo + per_blk - 1) / per_blk), KEEP_T, 0, s>>>(
        flat_idx, M, cell_base, n_cells, (const uint8_t*)mark_ws, lo, hi, list, (unsigned long long*)count);
    return ngp_launch_status();
}

int ngp_density_scatter_kept(const int32_t* list, const int64_t* count, int64_t n_max, const int64_t* indices,
                             const float* sigmas, int64_t pos_base, uint64_t* grid_key, void* stream) {
    NGP_CHECK_ARG(n_max >= 0 && pos_base >= 0 && pos_base + n_max < (1ll << 31));
    if (n_max == 0) return NGP_OK;
    NGP_CHECK_ARG(list && count && indices && sigmas && grid_key && ((uintptr_t)grid_key & 7) == 0);
    static const unsigned cap = resident_blocks(scatter_kept_kernel, 256, 0);
    const unsigned blocks = std::max(1u, std::min(cap, (unsigned)((n_max + 255) / 256)));
    scatter_kept_kernel<<<blocks, 256, 0, as_stream(stream)>>>(list, count, n_max, indices, sigmas, pos_base,
                                                              reinterpret_cast<unsigned long long*>(grid_key));
    return ngp_launch_status();
}

int ngp_density_grid_ema(float* density_grid, uint64_t* grid_key, int64_t n, float decay, const float* decay_cells,
                         float thr_max, void* sum_cnt_ws, float* threshold_out, void* stream) {
    NGP_CHECK_ARG(n > 0 && density_grid && grid_key && sum_cnt_ws && threshold_out && ((uintptr_t)grid_key & 7) == 0);
    NGP_CHECK_ARG(((uintptr_t)sum_cnt_ws & 7) == 0);
    hipStream_t s = as_stream(stream);
    zero_words_kernel<<<1, 64, 0, s>>>(reinterpret_cast<unsigned long long*>(sum_cnt_ws), 2);
    int64_t blocks = (n + 255) / 256;
    if (blocks > 512) blocks = 512;
    grid_ema_kernel<<<(unsigned)blocks, 256, 0, s>>>(density_grid, reinterpret_cast<unsigned long long*>(grid_key), n,
                                                     decay, decay_cells,
                                                     (double*)sum_cnt_ws);
    grid_threshold_kernel<<<1, 1, 0, s>>>((const double*)sum_cnt_ws, thr_max, threshold_out);
    return ngp_launch_status();
}

}  // extern "C"
