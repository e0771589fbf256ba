// Wave (64 lanes) and workgroup reductions and scans: the one statement of
// the sums that the loss, the occupancy update and every list builder rest on.
//
// The ORDER of each is part of its contract -- floating-point callers are
// pinned bit for bit against it, so it must not be reassociated:
//  * wave_sum: xor butterfly at offsets 32, 16, 8, 4, 2, 1, each step
//    v = v + (lane ^ o's v).  Every lane ends with the same value.
//  * wave_incl_scan: Hillis-Steele at offsets 1, 2, 4, 8, 16, 32, each step
//    v = v + (lane - o's v) for lanes >= o.  (The reference's per-ray serial
//    sums, reassociated: fp32 sums over <= 64 lanes, carried chunk to chunk by
//    the caller.)
// Value types in use: float, double, int32_t, uint32_t, int64_t, unsigned
// long long.  Not routed through here, on purpose: the product scan of
// transmittance.h, the lane-group sum of inputgrad.hip ((g0+g1)+(g2+g3), two
// wave_xor_add steps in its own order), field_bwd.hip's DPP / permlane
// reductions, the stride-4 run logic of hash_bwd.hip and hashbin.hip, and
// composite.hip's serial readlane folds.
#pragma once
#include "common.h"

namespace ngp {

// one butterfly step
template <typename T>
__device__ __forceinline__ T wave_xor_add(T v, int m) {
    return v + __shfl_xor(v, m, 64);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = wave_xor_add(v, o);
    return v;
}

// wave_sum's butterfly over fmaxf
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// lane = threadIdx.x & 63
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    return v;
}

// Exclusive scan over a 1024-thread workgroup (16 waves), tile after tile:
// `local` is this thread's total for the tile, the result its exclusive
// offset, the carry of the tiles before included.  wave_sums[16] and *carry_s
// are LDS words of the kernel, which zeroes *carry_s (and barriers) first.
// A wave scan, then the 16 wave totals scanned by wave 0: two barriers.  The
// caller writes its items and calls block_scan_carry_1024 (the tile's other
// two barriers) before the next tile or before reading the total in *carry_s.
template <typename T>
__device__ __forceinline__ int64_t block_excl_scan_1024(T local, T* wave_sums, const int64_t* carry_s, int lane,
                                                        int wid) {
    const T incl = wave_incl_scan(local, lane);
    if (lane == 63) wave_sums[wid] = incl;
    __syncthreads();
    if (wid == 0) {
        T ws = lane < 16 ? wave_sums[lane] : 0;
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const T y = __shfl_up(ws, off, 64);
            if (lane >= off) ws += y;
        }
        if (lane < 16) wave_sums[lane] = ws;  // inclusive over waves
    }
    __syncthreads();
    return *carry_s + (wid > 0 ? wave_sums[wid - 1] : 0) + incl - local;
}

// Advances the carry by the tile's total, after every thread has used it.
template <typename T>
__device__ __forceinline__ void block_scan_carry_1024(const T* wave_sums, int64_t* carry_s) {
    __syncthreads();
    if (threadIdx.x == 0) *carry_s += wave_sums[15];
    __syncthreads();
}

}  // namespace ngp
