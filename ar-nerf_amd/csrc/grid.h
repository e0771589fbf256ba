// The hash grid's level table and the one statement of its per-level
// arithmetic (tcnn GridEncoding: pos_fract, the trilinear weights, grid_index),
// which every kernel that touches a level calls: the forward gathers (level.h,
// for field.hip), the coarse scatter (hash_bwd.hip), the binned backward
// (hashbin.hip) and the input gradients (normal.hip, inputgrad.hip).  What is
// bit-exact against the oracle
// (or_* in oracle/vren_oracle.c) is so because it is written here once.
#pragma once
#pragma clang fp contract(off)
#include "common.h"

namespace ngp {

constexpr int L = 16;  // levels (x2 features = the 32-wide MLP input)

struct GridArgs {
    ngp_hashgrid_t g;
    uint32_t dense_mask;  // bit l: level l indexes densely (res^3 <= size)
    uint32_t pow2_mask;   // bit l: size_l is a power of two
};

struct LevelLds {
    float scale[L];
    uint32_t res[L], off[L], size[L];
    uint32_t dense, pow2;
};

__device__ __forceinline__ void load_levels(const GridArgs& ga, LevelLds& lv) {
    const int t = threadIdx.x;
    if (t < L) {
        lv.scale[t] = ga.g.scales[t];
        lv.res[t] = ga.g.res[t];
        lv.off[t] = ga.g.offsets[t];
        lv.size[t] = ga.g.sizes[t];
    }
    if (t == 0) { lv.dense = ga.dense_mask; lv.pow2 = ga.pow2_mask; }
}

// The cell of x01 at a level of scale `scale` (tcnn pos_fract): its integer
// corner pg and the position pos in [0, 1) inside it.
__device__ __forceinline__ void level_cell(float scale, const float in[3], uint32_t pg[3], float pos[3]) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float p = fmaf(scale, in[d], 0.5f);
        const float fl = floorf(p);
        pg[d] = (uint32_t)(int)fl;
        pos[d] = p - fl;
    }
}

// Trilinear weight of corner c = cx | cy << 1 | cz << 2.  The product runs in
// tcnn's dimension order (wt = 1; wt *= d0; wt *= d1; wt *= d2) and that order
// is part of the contract: the weights round differently in any other.  A
// caller that needs only part of a product (one x side, the y/z factor) may
// form it itself where calling this would change the order.
__device__ __forceinline__ float corner_weight(const float pos[3], int c) {
    float wt = 1.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) wt *= (c & (1 << d)) ? pos[d] : 1 - pos[d];
    return wt;
}
__device__ __forceinline__ void corner_weights(const float pos[3], float w[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] = corner_weight(pos, c);
}

// One corner's step of the weights' position gradient: acc_d += dw_c/dpos_d * val
// (dw_c/dpos_d: +-1 for dimension d times the other two dimensions' factors,
// in dimension order).
__device__ __forceinline__ void corner_pos_grad(const float pos[3], int c, float val, float acc[3]) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float dw = (c >> d) & 1 ? 1.0f : -1.0f;
#pragma unroll
        for (int d2 = 0; d2 < 3; ++d2)
            if (d2 != d) dw *= (c >> d2) & 1 ? pos[d2] : 1 - pos[d2];
        acc[d] = fmaf(dw, val, acc[d]);
    }
}

// tcnn grid_index before the modulo: the dense (res2 = res * res) or the
// hashed index of corner (px, py, pz).
__device__ __forceinline__ uint32_t raw_index(uint32_t px, uint32_t py, uint32_t pz, uint32_t res, uint32_t res2,
                                              bool dense) {
    // (the y/z part in brackets: integer sums and xors associate exactly, and the two x sides
    // of a pair then share it)
    return dense ? px + (py * res + pz * res2) : (px * 1u) ^ ((py * 2654435761u) ^ (pz * 805459861u));
}

// idx % size: hashed levels have a power-of-two size (mask); a dense level's
// corner index is below 2 * size (coordinates <= res, size >= res^3), so one
// conditional subtract; a real division only for other tables.
__device__ __forceinline__ uint32_t reduce_index(uint32_t idx, uint32_t size, bool dense, bool pow2) {
    if (pow2) return idx & (size - 1u);
    // (dense: below 2 * size for coordinates in [0, res]; inputs outside the grid's box --
    // coordinates past it -- take the full modulo, as tcnn's grid_index does)
    if (dense) idx = idx >= size ? idx - size : idx;
    return __builtin_expect(idx >= size, 0) ? idx % size : idx;
}

// tcnn grid_index for one corner (see oracle or_* restatement).
__device__ __forceinline__ uint32_t corner_index(uint32_t px, uint32_t py, uint32_t pz, uint32_t res, uint32_t size,
                                                 bool dense, bool pow2) {
    return reduce_index(raw_index(px, py, pz, res, res * res, dense), size, dense, pow2);
}

__device__ __forceinline__ void load_x01(const float* __restrict__ xyzs, int64_t i, bool valid, const GridArgs& ga,
                                         float in[3]) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float x = valid ? xyzs[3 * i + d] : 0.0f;
        // models/networks.py:104
        in[d] = (x - ga.g.xyz_min[d]) / (ga.g.xyz_max[d] - ga.g.xyz_min[d]);
    }
}

static int grid_args(const ngp_hashgrid_t* grid, GridArgs& ga) {
    if (!grid || grid->n_levels != L) return NGP_ERANGE;
    ga.g = *grid;
    ga.dense_mask = 0;
    ga.pow2_mask = 0;
    for (int l = 0; l < L; ++l) {
        const uint64_t r = grid->res[l];
        if (r * r * r <= (uint64_t)grid->sizes[l]) ga.dense_mask |= 1u << l;
        if ((grid->sizes[l] & (grid->sizes[l] - 1u)) == 0) ga.pow2_mask |= 1u << l;
        if (grid->sizes[l] == 0) return NGP_EINVAL;
    }
    return NGP_OK;
}

static unsigned persistent_blocks(int64_t n, int samples_per_block, unsigned cap) {
    int64_t b = (n + samples_per_block - 1) / samples_per_block;
    if (b < 1) b = 1;
    return (unsigned)(b < cap ? b : cap);
}

}  // namespace ngp
