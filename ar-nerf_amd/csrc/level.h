// One level's hash encoding as the forward gathers it: the paired table fetches
// (fetch_pair), a level's parameters as scalar or per-lane values (LevelU), the
// cell's eight entries, the fp32 corner sum and its fp16x2 packing; the cell,
// the weights and the indices themselves are grid.h's.  Included by
// field.hip (and scripts/diag/encode_diag.hip); hash_bwd.hip's scatter takes
// one corner per lane and calls grid.h directly.
#pragma once
#pragma clang fp contract(off)
#include "common.h"
#include "field_net.h"
#include "grid.h"

namespace ngp {

struct __attribute__((aligned(4))) u2a4 {
    uint32_t x, y;
    __device__ operator uint2() const { return make_uint2(x, y); }
};

__device__ __forceinline__ uint32_t pick4(uint4 q, uint32_t k) {
    return k == 0 ? q.x : k == 1 ? q.y : k == 2 ? q.z : q.w;
}

// The two entries i0 (corner x) and i1 (corner x+1) of one y/z pair of a
// level's table tl.  Dense levels: always neighbours, one 8-byte load.
// Hashed levels (x term of the hash is px*1, size a power of two): i1 =
// i0 ^ (px ^ (px+1)), so both sit in one aligned 4-entry group unless px = 3
// mod 4 -- one 16-byte load for 3 of 4 pairs, plus a 4-byte load otherwise
// (the gather cost is per lane request, not per byte).
__device__ __forceinline__ void fetch_pair(const uint32_t* __restrict__ tl, uint32_t i0, uint32_t i1, bool dense,
                                           uint32_t& v0, uint32_t& v1) {
    const uint32_t lo = min(i0, i1), hi = max(i0, i1);
    uint32_t vlo, vhi;
    if (dense) {
        const bool adj = hi - lo == 1u;
        const uint2 pr = *reinterpret_cast<const u2a4*>(tl + (adj ? lo : (lo & ~1u)));
        vlo = adj ? pr.x : ((lo & 1u) ? pr.y : pr.x);
        vhi = pr.y;
        if (!adj) vhi = tl[hi];
    } else {
        const uint4 q = *reinterpret_cast<const uint4*>(tl + (lo & ~3u));
        const bool near = (hi ^ lo) < 4u;
        uint32_t vfar = 0u;
        if (!near) vfar = tl[hi];  // (the branch only issues the load: no wait inside it)
        vlo = pick4(q, lo & 3u);
        vhi = near ? pick4(q, hi & 3u) : vfar;
    }
    v0 = i0 < i1 ? vlo : vhi;
    v1 = i0 < i1 ? vhi : vlo;
}

// ------------------------------------------------------ one level's encoding
// One level's parameters as wave-uniform (scalar) values, so the per-level
// index variant is chosen by scalar branches, not computed for every lane.
struct LevelU {
    float sc;
    uint32_t res, res2, size, off;
    bool dense, pow2;
};
__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ LevelU level_u(const LevelLds& lv, int l) {
    LevelU u;
    u.sc = __uint_as_float(rfl(__float_as_uint(lv.scale[l])));
    u.res = rfl(lv.res[l]);
    u.res2 = u.res * u.res;
    u.size = rfl(lv.size[l]);
    u.off = rfl(lv.off[l]);
    u.dense = (rfl(lv.dense) >> l) & 1u;
    u.pow2 = (rfl(lv.pow2) >> l) & 1u;
    return u;
}
// the same level as per-lane values (l differs between the lanes of a wave)
__device__ __forceinline__ LevelU level_lane(const LevelLds& lv, int l) {
    return LevelU{lv.scale[l], lv.res[l], lv.res[l] * lv.res[l], lv.size[l], lv.off[l], (bool)((lv.dense >> l) & 1u),
                  (bool)((lv.pow2 >> l) & 1u)};
}

// grid.h's cell and corner index of a level held as LevelU
__device__ __forceinline__ void level_cell(const float in[3], const LevelU& u, uint32_t pg[3], float pos[3]) {
    level_cell(u.sc, in, pg, pos);
}
__device__ __forceinline__ uint32_t corner_index(uint32_t px, uint32_t py, uint32_t pz, const LevelU& u) {
    return reduce_index(raw_index(px, py, pz, u.res, u.res2, u.dense), u.size, u.dense, u.pow2);
}

// The indices i0 (corner x) and i1 (corner x + 1) of y/z pair yz of cell pg.
__device__ __forceinline__ void pair_index(const uint32_t pg[3], int yz, const LevelU& u, uint32_t& i0, uint32_t& i1) {
    const uint32_t qy = pg[1] + (yz & 1), qz = pg[2] + (yz >> 1);
    i0 = corner_index(pg[0], qy, qz, u);
    i1 = corner_index(pg[0] + 1u, qy, qz, u);
}

// The level's eight table entries of cell pg, as four x-adjacent pairs
// (v[2 yz], v[2 yz + 1]: corners (0, y, z) and (1, y, z)): every index first,
// then the four fetch_pair loads.
// (level sizes are multiples of 4 and offsets of 8 entries: the aligned
// groups stay inside the level)
__device__ __forceinline__ void gather_cell(const uint32_t pg[3], const LevelU& u, const uint32_t* __restrict__ table,
                                            uint32_t v[8]) {
    uint32_t i0[4], i1[4];
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) pair_index(pg, yz, u, i0[yz], i1[yz]);
    const uint32_t* tl = table + u.off;
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) fetch_pair(tl, i0[yz], i1[yz], u.dense || !u.pow2, v[2 * yz], v[2 * yz + 1]);
}

// One level's encoding in two halves, so a caller can issue the gathers of
// several levels before it consumes any: corner weights + the level's loads,
// then the fp32 corner sum (fmaf over the corners in tcnn's order; the caller
// rounds once to fp16)
__device__ __forceinline__ void gather_level_u(const float in[3], const LevelU& u, const uint32_t* __restrict__ table,
                                               float w[8], uint32_t v[8]) {
    float pos[3];
    uint32_t pg[3];
    level_cell(in, u, pg, pos);
    corner_weights(pos, w);
    gather_cell(pg, u, table, v);
}

__device__ __forceinline__ void sum_level(const float w[8], const uint32_t v[8], float& a0, float& a1) {
    a0 = 0.f;
    a1 = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const _Float16 f0 = __builtin_bit_cast(_Float16, (uint16_t)(v[c] & 0xffffu));
        const _Float16 f1 = __builtin_bit_cast(_Float16, (uint16_t)(v[c] >> 16));
        a0 = fmaf(w[c], (float)f0, a0);
        a1 = fmaf(w[c], (float)f1, a1);
    }
}

__device__ __forceinline__ uint32_t pack_h2(float a, float b) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)a) | ((uint32_t)__builtin_bit_cast(uint16_t, (_Float16)b) << 16);
}

// gather_level_u in two halves that keep fewer registers live across the
// loads' latency: the loads alone (indices from the cell corner), then -- once
// they have returned -- the corner weights recomputed from the position and
// the fp32 corner sum
__device__ __forceinline__ void gather_level_loads(const float in[3], const LevelU& u,
                                                   const uint32_t* __restrict__ table, uint32_t v[8]) {
    float pos[3];
    uint32_t pg[3];
    level_cell(in, u, pg, pos);
    gather_cell(pg, u, table, v);
}
__device__ __forceinline__ uint32_t level_sum_h2(const float in[3], const LevelU& u, const uint32_t v[8]) {
    float pos[3], w[8];
    uint32_t pg[3];
    level_cell(in, u, pg, pos);
    corner_weights(pos, w);
    float a0, a1;
    sum_level(w, v, a0, a1);
    return pack_h2(a0, a1);
}

// Hash-encode one level of one sample: the two features (fp32 accumulation,
// rounded once to fp16 by the caller).
__device__ __forceinline__ void encode_level(const float in[3], const LevelU& u, const uint32_t* __restrict__ table,
                                             float& a0, float& a1) {
    float pos[3], w[8];
    uint32_t pg[3], v[8];
    level_cell(in, u, pg, pos);
    corner_weights(pos, w);
    // (each pair's load right after its indices, not gather_cell's indices-first order.  The
    // order is part of no value; it is kept because the launch geometry follows from it: with
    // gather_cell's, field_fwd_kernel<false, false> takes 123 VGPRs + 4 AGPRs instead of 127 + 4
    // and <true, false> 129 + 4 instead of 133 + 4, the density kernel crosses an occupancy
    // step (4 waves per SIMD instead of 3) and its persistent grid resizes)
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) {
        uint32_t i0, i1;
        pair_index(pg, yz, u, i0, i1);
        fetch_pair(table + u.off, i0, i1, u.dense || !u.pow2, v[2 * yz], v[2 * yz + 1]);
    }
    sum_level(w, v, a0, a1);
}

// Hash-encode levels 4g..4g+3 of one sample -> 8 fp16 values (enc[8g..8g+7]).
__device__ __forceinline__ h8 encode4(const float in[3], int g, const LevelLds& lv, const uint32_t* __restrict__ table) {
    h8 e;
#pragma unroll
    for (int jl = 0; jl < 4; ++jl) {
        float a0, a1;
        encode_level(in, level_lane(lv, 4 * g + jl), table, a0, a1);
        e[2 * jl] = (_Float16)a0;
        e[2 * jl + 1] = (_Float16)a1;
    }
    return e;
}

}  // namespace ngp
