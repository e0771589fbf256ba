// Row and sample list builders of the training step: ray segments and the
// active-sample map, the chunked forward's round counts and round-2 list
// (decoupled look-back), the non-empty rows, the rows that carry gradient.
// No counterpart in the reference, which evaluates every marched sample
// (train.py:174-200, volumerendering.cu:5-44 for where a row terminates).
#pragma clang fp contract(off)

#include "common.h"
#include "transmittance.h"
#include "wave.h"
#include "zero_words.h"

namespace ngp {

// ---- decoupled look-back (ordered compaction across blocks in one launch)
// Workspace {ticket, done, generation, pad, status[blocks]}, zeroed once by
// the caller.  A block takes a ticket (its position in dispatch order: it
// only ever waits on blocks that started before it), publishes its
// aggregate, and one wave walks back over the status words 64 at a time,
// summing aggregates until the closest inclusive prefix; the last block to
// finish resets the ticket and advances the generation, so the words of the
// previous launch never match.  A status word carries its own value, so the
// hand-off is one 8-byte agent-scope atomic each way (sc1 store / sc1 poll,
// MI355X_MICROARCH.md "Valid forms"): no release / acquire fences -- an
// acquire poll or a release per block (L2 write-back of the whole XCD) made
// the step 60 % slower.  The lists themselves are read by later launches.
struct LookbackWs {
    uint32_t tick, done, gen, pad;
    unsigned long long status[1];  // [blocks]
};
constexpr unsigned long long LB_AGG = 1ull << 40, LB_INCL = 2ull << 40, LB_VAL = (1ull << 40) - 1;
__device__ __forceinline__ unsigned long long lb_word(uint32_t gen, unsigned long long flag, int64_t v) {
    return ((unsigned long long)(gen & 0x3fffffu) << 42) | flag | ((unsigned long long)v & LB_VAL);
}
// whole wave: publishes aggregate A of block b, returns the exclusive prefix
// of the blocks before it, publishes b's inclusive prefix
__device__ __forceinline__ int64_t lookback_prefix(LookbackWs* __restrict__ lb, uint32_t b, uint32_t gen, int64_t A,
                                                   int lane) {
    if (lane == 0)
        __hip_atomic_store(&lb->status[b], lb_word(gen, b == 0 ? LB_INCL : LB_AGG, A), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    int64_t P = 0;
    for (int64_t j = (int64_t)b - 1; j >= 0; j -= 64) {
        const int64_t q = j - lane;
        unsigned long long wv = LB_INCL;  // (q < 0: before block 0, an inclusive 0)
        // bounded: a predecessor publishes its aggregate without waiting on anyone, so this
        // ends in microseconds; the bound only keeps a corrupted workspace from hanging the
        // GPU (counted as a guard hit, ngp_guard_hits: the result is then wrong)
        for (uint32_t spin = 0;; ++spin) {
            if (q >= 0) wv = __hip_atomic_load(&lb->status[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool ok = q < 0 || ((uint32_t)(wv >> 42) == (gen & 0x3fffffu) && (wv & (3ull << 40)) != 0);
            if (__all(ok)) break;
            if (spin == (1u << 22)) {
                if (lane == 0) ngp_guard_hit();
                wv = LB_INCL;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        const bool incl = (wv & (3ull << 40)) == LB_INCL;
        const uint64_t m = __ballot(incl);
        const int k = m ? __ffsll((unsigned long long)m) - 1 : 63;
        P += wave_sum(lane <= k ? (int64_t)(wv & LB_VAL) : (int64_t)0);
        if (m) break;
    }
    if (lane == 0 && b > 0)
        __hip_atomic_store(&lb->status[b], lb_word(gen, LB_INCL, P + A), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return P;
}
// one thread per block, after the block's last use of its ticket
__device__ __forceinline__ void lookback_finish(LookbackWs* __restrict__ lb, uint32_t gen, uint32_t nb) {
    if (__hip_atomic_fetch_add(&lb->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nb - 1) {
        __hip_atomic_store(&lb->tick, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&lb->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&lb->gen, gen + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------- active-sample map
// Exclusive scan of the per-row active counts (one 1024-lane workgroup) and
// the compacted index map sample_idx[j] = rays_a[row].start + k for the
// first n_active[row] samples of every row (one wave per row).
__global__ void __launch_bounds__(1024) active_scan_kernel(const int32_t* __restrict__ n_active, int64_t n_rows,
                                                           int64_t* __restrict__ act_start,
                                                           int64_t* __restrict__ total,
                                                           int64_t* __restrict__ total_acc = nullptr) {
    __shared__ int64_t wave_sums[16];
    __shared__ int64_t carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    constexpr int PER = 8;
    for (int64_t base = 0; base < n_rows; base += 1024 * PER) {
        int64_t v[PER], local = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int64_t i = base + (int64_t)tid * PER + k;
            v[k] = i < n_rows ? n_active[i] : 0;
            local += v[k];
        }
        int64_t run = block_excl_scan_1024(local, wave_sums, &carry_s, lane, wid);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int64_t i = base + (int64_t)tid * PER + k;
            if (i < n_rows) act_start[i] = run;
            run += v[k];
        }
        block_scan_carry_1024(wave_sums, &carry_s);
    }
    if (tid == 0) {
        *total = carry_s;
        if (total_acc) atomicAdd((unsigned long long*)total_acc, (unsigned long long)carry_s);
    }
}

__global__ void __launch_bounds__(256) active_map_kernel(const int32_t* __restrict__ n_active,
                                                         const int64_t* __restrict__ rays_a,
                                                         const int64_t* __restrict__ act_start, int64_t n_rows,
                                                         int32_t* __restrict__ sample_idx, int first) {
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const int na = n_active[r];
    const int64_t src = rays_a[3 * r + 1] + first, dst = act_start[r];
    for (int k = lane; k < na; k += 64) sample_idx[dst + k] = (int32_t)(src + k);
}

// Fused scan + map for batch-sized row counts (one launch instead of a
// one-block scan and a map launch, both latency-bound on the step's critical
// path).  Block b owns rows [b*SEG_ROWS, (b+1)*SEG_ROWS): it first sums the
// counts of every row before its range itself (a redundant reduction over
// L2-resident counts, so no block waits on another), then scans its own rows
// in LDS and writes their sample indices.  CAP > 0: counts[r] = min(N_r, CAP)
// read from rays_a (counts unused).  The last block publishes the total.
constexpr int SEG_ROWS = 64, SEG_THREADS = 512;
constexpr int64_t SEG_MAX_ROWS = 65536;  // beyond: scan + map launches (O(rows^2 / SEG_ROWS) reads here)

template <bool CAPPED>
__global__ void __launch_bounds__(SEG_THREADS) segments_kernel(const int32_t* __restrict__ counts,
                                                               const int64_t* __restrict__ rays_a, int64_t n_rows,
                                                               int cap, int first, int64_t* __restrict__ start_ws,
                                                               int64_t* __restrict__ total,
                                                               int64_t* __restrict__ total_acc,
                                                               int32_t* __restrict__ sample_idx) {
    __shared__ int64_t red[SEG_THREADS / 64];
    __shared__ int32_t lofs[SEG_ROWS + 1];
    __shared__ int64_t src[SEG_ROWS];
    NGP_PROBE_BEGIN(NGP_P_SEGMENTS);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * SEG_ROWS, r1 = min(r0 + SEG_ROWS, n_rows);
    auto count = [&](int64_t r) -> int64_t {
        return CAPPED ? min(rays_a[3 * r + 2], (int64_t)cap) : (int64_t)counts[r];
    };
    // 1) prefix of the rows before this block: 8 independent loads in flight
    // per thread (the L2 round trips overlap instead of chaining)
    int64_t acc = 0;
    int64_t r = t;
    for (; r + 7 * SEG_THREADS < r0; r += 8 * SEG_THREADS) {
        int64_t c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = count(r + k * SEG_THREADS);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += c[k];
    }
    for (; r < r0; r += SEG_THREADS) acc += count(r);
    acc = wave_sum(acc);
    if (lane == 0) red[w] = acc;
    // 2) own rows: exclusive scan in wave 0 (SEG_ROWS = 64 = one wave)
    if (w == 0) {
        const int64_t r = r0 + lane;
        const int32_t c = r < r1 ? (int32_t)count(r) : 0;
        const int32_t x = wave_incl_scan(c, lane);
        lofs[lane] = x - c;
        if (lane == 63) lofs[SEG_ROWS] = x;
        src[lane] = r < r1 ? rays_a[3 * r + 1] + first : 0;
    }
    __syncthreads();
    int64_t prefix = 0;
#pragma unroll
    for (int i = 0; i < SEG_THREADS / 64; ++i) prefix += red[i];
    if (t < r1 - r0) start_ws[r0 + t] = prefix + lofs[t];
    const int32_t nb = lofs[SEG_ROWS];
    if (blockIdx.x == gridDim.x - 1 && t == 0) {
        *total = prefix + nb;
        if (total_acc) atomicAdd((unsigned long long*)total_acc, (unsigned long long)(prefix + nb));
    }
    // 3) map: entry q of this block belongs to the row whose [lofs, lofs+c) holds it
    for (int32_t q = t; q < nb; q += SEG_THREADS) {
        int lo = 0, hi = SEG_ROWS;  // lofs[lo] <= q < lofs[hi]
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int mid = (lo + hi) >> 1;
            if (lofs[mid] <= q) lo = mid; else hi = mid;
        }
        sample_idx[prefix + q] = (int32_t)(src[lo] + (q - lofs[lo]));
    }
    NGP_PROBE_END();
}

static void launch_segments(const int32_t* counts, const int64_t* rays_a, int64_t n_rows, int cap, int first,
                            int64_t* start_ws, int64_t* total, int64_t* total_acc, int32_t* sample_idx,
                            hipStream_t s) {
    const unsigned blocks = (unsigned)((n_rows + SEG_ROWS - 1) / SEG_ROWS);
    if (cap > 0)
        NGP_TIMED(NGP_K_SEGMENTS, s, segments_kernel<true><<<blocks, SEG_THREADS, 0, s>>>(nullptr, rays_a, n_rows, cap, first, start_ws, total,
                                                             total_acc, sample_idx));
    else
        NGP_TIMED(NGP_K_SEGMENTS, s, segments_kernel<false><<<blocks, SEG_THREADS, 0, s>>>(counts, rays_a, n_rows, 0, first, start_ws, total,
                                                              total_acc, sample_idx));
}

// ------------------------------------------- chunked forward (training)
// The training step only ever reads a row's samples up to its termination
// (composite_train_fw breaks there, the backward stops there), so the field
// is evaluated in two rounds: the first `first` samples of every row, then --
// only for rows still not terminated after them -- the rest.  Same outputs as
// evaluating every marched sample.
// Round-1 counts: min(N_r, first).
__global__ void __launch_bounds__(256) chunk_first_kernel(const int64_t* __restrict__ rays_a, int64_t n_rows, int first,
                                                          int32_t* __restrict__ counts) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    counts[r] = (int32_t)min(rays_a[3 * r + 2], (int64_t)first);
}

// Later-round counts: one wave per row computes the transmittance of its
// first min(N_r, first) samples exactly as composite_loss_ray's forward does
// (same expressions, chunk_transmittance); a row that has not terminated there
// and has more samples needs min(N_r, last) - first more (last <= 0: N_r).
__global__ void __launch_bounds__(256) chunk_rest_kernel(const float* __restrict__ sigmas,
                                                         const float* __restrict__ deltas,
                                                         const int64_t* __restrict__ rays_a, int64_t n_rows, int first,
                                                         int last, float T_thr, int32_t* __restrict__ counts) {
    const int64_t n = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const int64_t start = rays_a[3 * n + 1], N = rays_a[3 * n + 2];
    const int64_t M = min(N, (int64_t)first);
    float T = 1.0f;
    bool done = false;
    for (int64_t k0 = 0; k0 < M && !done; k0 += 64) {
        const int cnt = (int)(M - k0 < 64 ? M - k0 : 64);
        float sg = 0.f, dl = 0.f;
        if (lane < cnt) { sg = sigmas[start + k0 + lane]; dl = deltas[start + k0 + lane]; }
        const float om = 1.0f - (1.0f - __expf(-sg * dl));
        const ChunkT ct = chunk_transmittance(om, cnt, T, T_thr, lane);
        done = ct.hit;
        T = __shfl(ct.Tn, ct.stop - 1, 64);
    }
    const int64_t end = last > 0 ? min(N, (int64_t)last) : N;
    if (lane == 0) counts[n] = (!done && N > first) ? (int32_t)(end - first) : 0;
}

// The non-empty rows of rays_a in row order (rows[0..*n_rows)) for
// field_first_chunk_kernel's one-wave-per-row round 1, and rest[r] = 0 for the
// empty ones (that kernel writes the others).  One 1024-thread block, 8 rows
// per thread per tile; runs on the march's side stream right after the
// compaction, off the step's critical path.
__global__ void __launch_bounds__(1024) rays_nonempty_kernel(const int64_t* __restrict__ rays_a, int64_t n_rays,
                                                             int32_t* __restrict__ rows, int64_t* __restrict__ n_out,
                                                             int32_t* __restrict__ rest, int64_t* __restrict__ zero) {
    __shared__ int32_t wave_sums[16];
    __shared__ int64_t carry_s;
    NGP_PROBE_BEGIN(NGP_P_NONEMPTY);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    constexpr int PER = 8;
    for (int64_t base = 0; base < n_rays; base += 1024 * PER) {
        uint32_t f = 0;  // bit k: row base + 8 tid + k is non-empty
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int64_t i = base + (int64_t)tid * PER + k;
            if (i < n_rays && rays_a[3 * i + 2] > 0) f |= 1u << k;
        }
        int64_t o = block_excl_scan_1024((int32_t)__popc(f), wave_sums, &carry_s, lane, wid);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int64_t i = base + (int64_t)tid * PER + k;
            if (i >= n_rays) break;
            if (f >> k & 1u) rows[o++] = (int32_t)i;
            else if (rest) rest[i] = 0;
        }
        block_scan_carry_1024(wave_sums, &carry_s);
    }
    if (tid == 0) {
        *n_out = carry_s;
        if (zero) *zero = 0;
    }
    NGP_PROBE_END();
}

// Round-2 list in one launch: chunk_rest_kernel's counts + the exclusive scan
// across rows + the map of ray_segments.  Block b owns rows [64b, 64b + 64):
// its waves compute the counts of 8 rows each (first-chunk loads of all 8
// rows issued before any transmittance), wave 0 scans them, and the prefix
// over earlier blocks comes from a decoupled look-back: each block publishes
// its aggregate, then its inclusive prefix, as one 64-bit status word
// {generation, flag, value}; wave 0 reads the 64 predecessors before it at a
// time and stops at the closest inclusive one.  Block ids come from an atomic
// ticket (dispatch order), so a block only ever waits on blocks that started
// before it and publish their aggregate without waiting -- no deadlock at any
// grid size.  The last block to finish resets the ticket and advances the
// generation (stale status words of the previous launch never match).
// (64 rows per block: 32 / 16 measured slower, profiles/r03/ab/chunk_segments_rows.txt)
constexpr int CS_ROWS = 64, CS_THREADS = 512, CS_RPW = CS_ROWS / (CS_THREADS / 64);
constexpr int CS_LOG = CS_ROWS == 64 ? 6 : CS_ROWS == 32 ? 5 : 4;
static_assert(CS_ROWS == 64 || CS_ROWS == 32 || CS_ROWS == 16, "row block");

__global__ void __launch_bounds__(CS_THREADS) chunk_segments_kernel(
    const float* __restrict__ sigmas, const float* __restrict__ deltas, const int64_t* __restrict__ rays_a,
    int64_t n_rows, int first, int last, float T_thr, LookbackWs* __restrict__ lb, int64_t* __restrict__ start_ws,
    int64_t* __restrict__ total, int64_t* __restrict__ total_acc, const int64_t* __restrict__ total_acc_add,
    int32_t* __restrict__ sample_idx) {
    __shared__ int32_t cnt_s[CS_ROWS];
    __shared__ int32_t lofs[65];  // (wave 0 writes all 64 lanes' entries; [CS_ROWS] = the block's total)
    __shared__ int64_t src[64];
    __shared__ uint32_t sh_b;
    __shared__ int64_t sh_prefix;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t nb = gridDim.x;
    const uint32_t gen = __hip_atomic_load(&lb->gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0) sh_b = __hip_atomic_fetch_add(&lb->tick, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint32_t b = sh_b;
    const int64_t r0 = (int64_t)b * CS_ROWS, r1 = min(r0 + CS_ROWS, n_rows);
    // ---- counts (chunk_rest_kernel's arithmetic)
    int64_t st[CS_RPW], Nr[CS_RPW];
    float sg0[CS_RPW], dl0[CS_RPW];
#pragma unroll
    for (int i = 0; i < CS_RPW; ++i) {
        const int64_t r = r0 + w * CS_RPW + i;
        st[i] = r < r1 ? rays_a[3 * r + 1] : 0;
        Nr[i] = r < r1 ? rays_a[3 * r + 2] : 0;
    }
#pragma unroll
    for (int i = 0; i < CS_RPW; ++i) {
        const int64_t M = min(Nr[i], (int64_t)first);
        sg0[i] = dl0[i] = 0.f;
        if (lane < M) { sg0[i] = sigmas[st[i] + lane]; dl0[i] = deltas[st[i] + lane]; }
    }
#pragma unroll
    for (int i = 0; i < CS_RPW; ++i) {
        const int64_t M = min(Nr[i], (int64_t)first);
        float T = 1.0f;
        bool done = false;
        for (int64_t k0 = 0; k0 < M && !done; k0 += 64) {
            const int cnt = (int)(M - k0 < 64 ? M - k0 : 64);
            float sg = sg0[i], dl = dl0[i];
            if (k0 > 0) {
                sg = dl = 0.f;
                if (lane < cnt) { sg = sigmas[st[i] + k0 + lane]; dl = deltas[st[i] + k0 + lane]; }
            }
            const float om = 1.0f - (1.0f - __expf(-sg * dl));
            const ChunkT ct = chunk_transmittance(om, cnt, T, T_thr, lane);
            done = ct.hit;
            T = __shfl(ct.Tn, ct.stop - 1, 64);
        }
        const int64_t end = last > 0 ? min(Nr[i], (int64_t)last) : Nr[i];
        if (lane == 0) cnt_s[w * CS_RPW + i] = (!done && Nr[i] > first) ? (int32_t)(end - first) : 0;
    }
    __syncthreads();
    if (w == 0) {
        // ---- own rows: exclusive scan
        const int64_t r = r0 + lane;
        const int32_t c = r < r1 ? cnt_s[lane % CS_ROWS] : 0;
        const int32_t x = wave_incl_scan(c, lane);
        lofs[lane] = x - c;
        const int32_t A = __shfl(x, 63, 64);
        if (lane == 63) lofs[CS_ROWS] = x;
        src[lane] = r < r1 ? rays_a[3 * r + 1] + first : 0;
        // ---- look-back
        const int64_t P = lookback_prefix(lb, b, gen, A, lane);
        if (lane == 0) {
            sh_prefix = P;
            if (b == nb - 1) {
                *total = P + A;
                if (total_acc)
                    atomicAdd((unsigned long long*)total_acc,
                              (unsigned long long)(P + A + (total_acc_add ? *total_acc_add : 0)));
            }
        }
    }
    __syncthreads();
    const int64_t prefix = sh_prefix;
    if (t < r1 - r0) start_ws[r0 + t] = prefix + lofs[t];
    const int32_t nbe = lofs[CS_ROWS];
    for (int32_t q = t; q < nbe; q += CS_THREADS) {
        int lo = 0, hi = CS_ROWS;  // lofs[lo] <= q < lofs[hi]
#pragma unroll
        for (int k = 0; k < CS_LOG; ++k) {
            const int mid = (lo + hi) >> 1;
            if (lofs[mid] <= q) lo = mid; else hi = mid;
        }
        sample_idx[prefix + q] = (int32_t)(src[lo] + (q - lofs[lo]));
    }
    if (t == 0) lookback_finish(lb, gen, nb);
}

}  // namespace ngp

using namespace ngp;

// The rows of (dL/dsigma, dL/drgb) with a nonzero entry: the samples that
// carry gradient (the compositing backward, volumerendering.cu:86-150, leaves
// every sample past its ray's termination at exact zero, and a zero upstream
// gradient adds exactly nothing to the parameters' gradient) -> idx[0..*count).
// A block takes 1024 consecutive rows (a wave 256 of them), counts them per wave,
// reserves its range with ONE atomic (a per-wave atomic on the one counter
// serialised ~9 K reservations: 57 us per launch) and writes the rows in
// order; blocks land in reservation order.
__global__ void __launch_bounds__(256) grad_rows_kernel(const float* __restrict__ dsig, const float* __restrict__ drgb,
                                                        int64_t n, int32_t* __restrict__ idx,
                                                        unsigned long long* __restrict__ count) {
    __shared__ uint32_t wcnt[4];
    __shared__ unsigned long long base_s;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t b0 = (int64_t)blockIdx.x * 1024; b0 < n; b0 += (int64_t)gridDim.x * 1024) {
        uint64_t m[4];
        uint32_t c = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // wave w takes rows b0 + 256 w .. + 255, 64 per step
            const int64_t i = b0 + 256 * w + 64 * q + lane;
            bool nz = false;
            if (i < n) nz = dsig[i] != 0.f || drgb[3 * i] != 0.f || drgb[3 * i + 1] != 0.f || drgb[3 * i + 2] != 0.f;
            m[q] = __ballot(nz);
            c += (uint32_t)__popcll(m[q]);
        }
        if (lane == 0) wcnt[w] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            base_s = tot ? atomicAdd(count, (unsigned long long)tot) : 0ull;
        }
        __syncthreads();
        unsigned long long o = base_s;
        for (int v = 0; v < w; ++v) o += wcnt[v];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if ((m[q] >> lane) & 1ull)
                idx[o + __popcll(m[q] & ((1ull << lane) - 1ull))] = (int32_t)(b0 + 256 * w + 64 * q + lane);
            o += __popcll(m[q]);
        }
        __syncthreads();  // wcnt / base_s are rewritten next round
    }
}

extern "C" {

int ngp_chunk_counts(const int64_t* rays_a, int64_t n_rows, int first, const float* sigmas, const float* deltas,
                     float T_threshold, int32_t* counts, void* stream) {
    return ngp_chunk_counts_range(rays_a, n_rows, first, 0, sigmas, deltas, T_threshold, counts, stream);
}

int ngp_chunk_counts_range(const int64_t* rays_a, int64_t n_rows, int first, int last, const float* sigmas,
                           const float* deltas, float T_threshold, int32_t* counts, void* stream) {
    NGP_CHECK_ARG(n_rows >= 0 && first >= 1 && counts && rays_a && (last <= 0 || last > first));
    if (n_rows == 0) return NGP_OK;
    if (!sigmas) {
        NGP_TIMED(NGP_K_CHUNK, as_stream(stream), chunk_first_kernel<<<(unsigned)((n_rows + 255) / 256), 256, 0, as_stream(stream)>>>(rays_a, n_rows, first,
                                                                                           counts));
    } else {
        NGP_CHECK_ARG(deltas != nullptr);
        NGP_TIMED(NGP_K_CHUNK, as_stream(stream), chunk_rest_kernel<<<(unsigned)((n_rows + 3) / 4), 256, 0, as_stream(stream)>>>(sigmas, deltas, rays_a, n_rows,
                                                                                      first, last, T_threshold, counts));
    }
    return ngp_launch_status();
}

int ngp_rays_nonempty(const int64_t* rays_a, int64_t n_rays, int32_t* rows, int64_t* n_rows, int32_t* rest,
                      int64_t* zero, void* stream) {
    NGP_CHECK_ARG(n_rays >= 0 && n_rays <= 0x7fffffff && n_rows);
    NGP_CHECK_ARG(n_rays == 0 || (rays_a && rows));
    NGP_TIMED(NGP_K_SEGMENTS, as_stream(stream), rays_nonempty_kernel<<<1, 1024, 0, as_stream(stream)>>>(rays_a, n_rays, rows, n_rows, rest, zero));
    return ngp_launch_status();
}

size_t ngp_chunk_segments_workspace(int64_t n_rows) {
    const int64_t blocks = n_rows > 0 ? (n_rows + CS_ROWS - 1) / CS_ROWS : 1;
    return 16 + 8 * (size_t)blocks;
}

int ngp_chunk_segments(const float* sigmas, const float* deltas, const int64_t* rays_a, int64_t n_rows, int first,
                       int last, float T_threshold, void* lookback_ws, int64_t* start_ws, int64_t* total,
                       int64_t* total_acc, const int64_t* total_acc_add, int32_t* sample_idx, void* stream) {
    NGP_CHECK_ARG(n_rows >= 0 && first >= 1 && (last <= 0 || last > first) && total);
    NGP_CHECK_ARG(!total_acc_add || total_acc);
    hipStream_t s = as_stream(stream);
    if (n_rows == 0) {
        active_scan_kernel<<<1, 1024, 0, s>>>(nullptr, 0, start_ws, total, total_acc);  // total = 0
        return ngp_launch_status();
    }
    NGP_CHECK_ARG(sigmas && deltas && rays_a && lookback_ws && start_ws && sample_idx &&
                  ((uintptr_t)lookback_ws & 7) == 0);
    const int64_t blocks = (n_rows + CS_ROWS - 1) / CS_ROWS;
    NGP_CHECK_ARG(blocks <= (int64_t)0x7fffffff);
    NGP_TIMED(NGP_K_SEGMENTS, s, chunk_segments_kernel<<<(unsigned)blocks, CS_THREADS, 0, s>>>(
        sigmas, deltas, rays_a, n_rows, first, last, T_threshold, (LookbackWs*)lookback_ws, start_ws, total,
        total_acc, total_acc_add, sample_idx));
    return ngp_launch_status();
}

int ngp_ray_segments(const int32_t* counts, const int64_t* rays_a, int64_t n_rows, int first, int64_t* start_ws,
                     int64_t* total, int64_t* total_acc, int32_t* sample_idx, void* stream) {
    NGP_CHECK_ARG(n_rows >= 0 && total && first >= 0);
    hipStream_t s = as_stream(stream);
    if (n_rows > 0) NGP_CHECK_ARG(counts && rays_a && start_ws && sample_idx);
    if (n_rows > 0 && n_rows <= SEG_MAX_ROWS) {
        launch_segments(counts, rays_a, n_rows, 0, first, start_ws, total, total_acc, sample_idx, s);
        return ngp_launch_status();
    }
    active_scan_kernel<<<1, 1024, 0, s>>>(counts, n_rows, start_ws, total, total_acc);
    if (n_rows > 0)
        active_map_kernel<<<(unsigned)((n_rows + 3) / 4), 256, 0, s>>>(counts, rays_a, start_ws, n_rows, sample_idx,
                                                                      first);
    return ngp_launch_status();
}

int ngp_ray_segments_capped(const int64_t* rays_a, int64_t n_rows, int cap, int64_t* start_ws, int64_t* total,
                            int64_t* total_acc, int32_t* sample_idx, void* stream) {
    NGP_CHECK_ARG(n_rows >= 0 && total && cap >= 1);
    hipStream_t s = as_stream(stream);
    if (n_rows == 0) {
        active_scan_kernel<<<1, 1024, 0, s>>>(nullptr, 0, start_ws, total, total_acc);  // total = 0
        return ngp_launch_status();
    }
    NGP_CHECK_ARG(rays_a && start_ws && sample_idx);
    if (n_rows <= SEG_MAX_ROWS) {
        launch_segments(nullptr, rays_a, n_rows, cap, 0, start_ws, total, total_acc, sample_idx, s);
        return ngp_launch_status();
    }
    return NGP_ERANGE;
}

int ngp_gradient_rows(const float* dL_dsigmas, const float* dL_drgbs, int64_t n, int32_t* idx, int64_t* count,
                      void* stream) {
    NGP_CHECK_ARG(n >= 0 && n < (1ll << 31) && count && ((uintptr_t)count & 7) == 0);
    hipStream_t s = as_stream(stream);
    zero_words_kernel<<<1, 64, 0, s>>>(reinterpret_cast<unsigned long long*>(count), 1);
    if (n > 0) {
        NGP_CHECK_ARG(dL_dsigmas && dL_drgbs && idx);
        const int64_t b = (n + 1023) / 1024;
        grad_rows_kernel<<<(unsigned)(b < 4096 ? b : 4096), 256, 0, s>>>(
            dL_dsigmas, dL_drgbs, n, idx, reinterpret_cast<unsigned long long*>(count));
    }
    return ngp_launch_status();
}

int ngp_active_samples(const int32_t* n_active, const int64_t* rays_a, int64_t n_rows, int64_t* act_start_ws,
                       int64_t* n_active_total, int32_t* sample_idx, void* stream) {
    NGP_CHECK_ARG(n_rows >= 0 && n_active_total);
    hipStream_t s = as_stream(stream);
    if (n_rows > 0) NGP_CHECK_ARG(n_active && rays_a && act_start_ws && sample_idx);
    if (n_rows > 0 && n_rows <= SEG_MAX_ROWS) {
        NGP_CHECK_ARG(n_active && rays_a && act_start_ws && sample_idx);
        launch_segments(n_active, rays_a, n_rows, 0, 0, act_start_ws, n_active_total, nullptr, sample_idx, s);
        return ngp_launch_status();
    }
    active_scan_kernel<<<1, 1024, 0, s>>>(n_active, n_rows, act_start_ws, n_active_total);
    if (n_rows > 0)
        active_map_kernel<<<(unsigned)((n_rows + 3) / 4), 256, 0, s>>>(n_active, rays_a, act_start_ws, n_rows,
                                                                      sample_idx, 0);
    return ngp_launch_status();
}

}  // extern "C"
