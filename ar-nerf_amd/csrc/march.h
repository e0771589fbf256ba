// The occupancy-grid walk of the training / test marchers (march.hip) and of
// the device-resident test render loop (render.hip), each part stated once:
// the probe of one point (probe_cell), the serial walk (march_step,
// march_walk_serial) and the wave-per-ray lattice walk (lat_build,
// lat_near_occupied, lat_walk).  The kernels keep what differs between them:
// the entry test, the sample limit and where an emitted sample is stored.
// raymarching.cu:11-60,166-234,335-404 of the reference.
#pragma once
#pragma clang fp contract(off)
#include "common.h"

namespace ngp {

// ------------------------------------------------------------- AABB
// (shared by the intersection / ray-generation kernels of march.hip and the
// probe-ray kernel of probe.hip)
__device__ __forceinline__ void aabb_t1t2(const float o[3], const float inv[3], const float* c,
                                          const float* h, float& t1, float& t2) {
    // intersection.cu:5-22
    float lo[3], hi[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float tmin = (c[i] - h[i] - o[i]) * inv[i];
        const float tmax = (c[i] + h[i] - o[i]) * inv[i];
        lo[i] = fminf(tmin, tmax);
        hi[i] = fmaxf(tmin, tmax);
    }
    t1 = fmaxf(fmaxf(lo[0], lo[1]), lo[2]);
    t2 = fminf(fminf(hi[0], hi[1]), hi[2]);
    if (t1 > t2) { t1 = -1.0f; t2 = -1.0f; }
}

// ------------------------------------------------------ ray generation
// (shared by the ray-generation kernels of march.hip, the insertion frame
// opening of insert.hip and the object shade of shade.hip)
// datasets/ray_utils.py:45-70: rays_d = dir_cam @ R^T of one (3,4) pose P.
__device__ __forceinline__ void ray_dir(const float* __restrict__ P, const float* __restrict__ dc,
                                        float* __restrict__ d) {
    const float d0 = dc[0], d1 = dc[1], d2 = dc[2];
    // einsum 'n1c,nba->n1a' of rearranged c2w: d_i = sum_c dc_c * R[i][c],
    // evaluated c-major like the batched matmul (fp32, no contraction).
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = d0 * P[4 * i + 0] + d1 * P[4 * i + 1] + d2 * P[4 * i + 2];
}

// ray_dir and rays_o = c2w[:,3] for the gathered training batch
// (train.py:85-87), then the single-box AABB test and the near clamp of
// models/rendering.py:29-31.
__device__ __forceinline__ void gen_ray(const float* __restrict__ P, const float* __restrict__ dc,
                                        const float* __restrict__ center, const float* __restrict__ half_size,
                                        float near, float* __restrict__ ro, float* __restrict__ rd,
                                        float* __restrict__ ht) {
    float d[3], o[3];
    ray_dir(P, dc, d);
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = P[4 * i + 3];
    const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
    float t1, t2;
    aabb_t1t2(o, inv, center, half_size, t1, t2);
    float h0 = -1.0f, h1 = -1.0f;
    if (t2 > 0) { h0 = fmaxf(t1, 0.0f); h1 = t2; }
    if (h0 >= 0 && h0 < near) h0 = near;
#pragma unroll
    for (int i = 0; i < 3; ++i) { ro[i] = o[i]; rd[i] = d[i]; }
    ht[0] = h0;
    ht[1] = h1;
}

// --------------------------------------------------------- marching
struct MarchParams {
    const uint8_t* bitfield;
    const uint32_t* summary;  // nullable: bit w = (64-bit bitfield word w != 0), see ngp_bitfield_summary
    int n_sum32;              // uint32 words of summary
    int cascades, grid_size, max_samples;
    float scale, esf, dt_scale;  // dt_scale: `scale` (train) or `cascades` (test quirk)
};

// One step of the reference's occupancy walk (raymarching.cu:205-233):
// returns true and advances t by dt if the sample at t is occupied,
// otherwise jumps t over the empty voxel with repeated calc_dt steps.
// SIMPLE = (cascades == 1 && esf == 0): then mip == 0, mip_bound ==
// min(0.5, scale) and dt == sqrt(3)/max_samples exactly (the general
// expressions fold to these constants), so the compiler drops frexp /
// scalbn / the division per step -- same values, bit for bit.
// `wcache` holds the 64-bit bitfield word (a Morton-aligned 4x4x4 block of
// cells) last loaded by this lane; consecutive samples along a ray mostly
// stay in the same block, so most occupancy tests need no memory access.
struct WordCache {
    uint32_t idx = 0xffffffffu;
    uint64_t word = 0;
    const uint32_t* sum = nullptr;  // LDS copy of the bitfield summary (nullable)
    const uint32_t* dil = nullptr;  // its one-block dilation (nullable; mip-0 blocks of cascade 0)
};

// Copy the bitfield summary into LDS (whole workgroup; call before any
// early return, followed by __syncthreads()).  Returns the LDS pointer or
// nullptr when the launch has no summary.
__device__ __forceinline__ const uint32_t* load_summary(const MarchParams& p, uint32_t* lds) {
    if (!p.summary) return nullptr;
    for (int i = threadIdx.x; i < 2 * p.n_sum32; i += blockDim.x) lds[i] = p.summary[i];
    return lds;
}

// The occupancy test of the point (x, y, z) = o + t d in one cascade, stated
// once: cell, bitfield word (through the lane's word cache), bit, and for an
// empty cell the voxel-exit target t_target (raymarching.cu:214-228) that the
// walk then steps past.  mip_base = mip * G^3 is the cascade's first cell.
__device__ __forceinline__ bool probe_cell(float t, float x, float y, float z, const float d[3], const float dinv[3],
                                           const uint8_t* bitfield, uint32_t mip_base, float mip_bound,
                                           float mip_bound_inv, float grid_f, float grid_size_inv, float gm1,
                                           WordCache& wc, float& t_target) {
    const int nx = (int)clampf(0.5f * (x * mip_bound_inv + 1) * grid_f, 0.0f, gm1);
    const int ny = (int)clampf(0.5f * (y * mip_bound_inv + 1) * grid_f, 0.0f, gm1);
    const int nz = (int)clampf(0.5f * (z * mip_bound_inv + 1) * grid_f, 0.0f, gm1);
    const uint32_t idx = mip_base + morton3((uint32_t)nx, (uint32_t)ny, (uint32_t)nz);
    const uint32_t wi = idx >> 6;
    if (wi != wc.idx) {  // bitfield is (C*G^3/8) bytes, G^3 a multiple of 64 for G >= 4
        // an all-empty word is known from the LDS summary: no global load, so
        // a wave crossing empty space never waits on memory
        const bool any = !wc.sum || ((wc.sum[wi >> 5] >> (wi & 31u)) & 1u);
        wc.word = any ? reinterpret_cast<const uint64_t*>(bitfield)[wi] : 0ull;
        wc.idx = wi;
    }
    const bool occ = (wc.word >> (idx & 63u)) & 1ull;
    if (occ) return true;
    const float tx = (((nx + 0.5f + 0.5f * copysignf(1.0f, d[0])) * grid_size_inv * 2 - 1) * mip_bound - x) * dinv[0];
    const float ty = (((ny + 0.5f + 0.5f * copysignf(1.0f, d[1])) * grid_size_inv * 2 - 1) * mip_bound - y) * dinv[1];
    const float tz = (((nz + 0.5f + 0.5f * copysignf(1.0f, d[2])) * grid_size_inv * 2 - 1) * mip_bound - z) * dinv[2];
    t_target = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
    return false;
}

// The occupancy test at t (raymarching.cu:205-221): position, dt, cascade,
// then probe_cell.  Returns the bit; for an empty cell also t_target.
template <bool SIMPLE>
__device__ __forceinline__ bool march_probe(float t, const float o[3], const float d[3], const float dinv[3],
                                            const MarchParams& p, float& x, float& y, float& z, float& dt,
                                            WordCache& wc, float& t_target) {
    const uint32_t G = (uint32_t)p.grid_size;
    x = o[0] + t * d[0]; y = o[1] + t * d[1]; z = o[2] + t * d[2];
    int mip;
    float mip_bound;
    if constexpr (SIMPLE) {
        dt = NGP_SQRT3 / p.max_samples;  // = clamp(t*0, sqrt3/max, 2 sqrt3 scale/G), t finite
        mip = 0;
        mip_bound = fminf(0.5f, p.scale);
    } else {
        dt = calc_dt(t, p.esf, p.max_samples, p.grid_size, p.dt_scale);
        mip = max(mip_from_pos(x, y, z, p.cascades), mip_from_dt(dt, p.grid_size, p.cascades));
        mip_bound = fminf(scalbnf(1.0f, mip - 1), p.scale);
    }
    return probe_cell(t, x, y, z, d, dinv, p.bitfield, (uint32_t)mip * (G * G * G), mip_bound, 1 / mip_bound,
                      (float)p.grid_size, 1.0f / p.grid_size, p.grid_size - 1.0f, wc, t_target);
}

// march_probe<true>'s per-launch constants, computed once (the wave march
// keeps them in scalar registers: uniform VALU results would otherwise sit in
// VGPRs for the whole kernel)
struct ProbeConsts {
    float mip_bound, mip_bound_inv, grid_f, grid_size_inv, gm1;
};
__device__ __forceinline__ float uniform_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ ProbeConsts probe_consts(const MarchParams& p) {
    ProbeConsts c;
    c.mip_bound = uniform_f(fminf(0.5f, p.scale));
    c.mip_bound_inv = uniform_f(1 / c.mip_bound);
    c.grid_f = uniform_f((float)p.grid_size);
    c.grid_size_inv = uniform_f(1.0f / p.grid_size);
    c.gm1 = uniform_f(p.grid_size - 1.0f);
    return c;
}
// march_probe<true> with the constants precomputed
__device__ __forceinline__ bool march_probe_simple(float t, const float o[3], const float d[3], const float dinv[3],
                                                   const MarchParams& p, const ProbeConsts& k, WordCache& wc,
                                                   float& t_target) {
    const float x = o[0] + t * d[0], y = o[1] + t * d[1], z = o[2] + t * d[2];
    return probe_cell(t, x, y, z, d, dinv, p.bitfield, 0u, k.mip_bound, k.mip_bound_inv, k.grid_f, k.grid_size_inv,
                      k.gm1, wc, t_target);
}

template <bool SIMPLE>
__device__ __forceinline__ bool march_step(float& t, const float o[3], const float d[3], const float dinv[3],
                                           const MarchParams& p, float& x, float& y, float& z, float& dt,
                                           WordCache& wc) {
    float t_target;
    if (march_probe<SIMPLE>(t, o, d, dinv, p, x, y, z, dt, wc, t_target)) {
        t += dt;
        return true;
    }
    // (t past 2^24 steps of dt: t + dt == t, the reference's loop would never end -- only a
    // degenerate ray (huge t2) gets there; it ends the ray instead and counts a guard hit.)
    // Every step advances t while dt exceeds half an ulp of each t the loop visits, i.e. when
    // dt > 2^-24 max(|t|, |t_target|) (the general dt only grows along the ray): then the plain
    // loop runs; a per-step check inside it cost the test-time march 20-26 % (r6m)
    const bool advances = dt * 16777216.0f > fmaxf(fabsf(t), fabsf(t_target));
    if constexpr (SIMPLE) {
        if (advances) {
            do { t += dt; } while (t < t_target);
        } else {
            do {
                const float tn = t + dt;
                if (!(tn > t)) { t = INFINITY; ngp_guard_hit(); break; }
                t = tn;
            } while (t < t_target);
        }
    } else {
        if (advances) {
            do { t += calc_dt(t, p.esf, p.max_samples, p.grid_size, p.dt_scale); } while (t < t_target);
        } else {
            do {
                const float tn = t + calc_dt(t, p.esf, p.max_samples, p.grid_size, p.dt_scale);
                if (!(tn > t)) { t = INFINITY; ngp_guard_hit(); break; }
                t = tn;
            } while (t < t_target);
        }
    }
    return false;
}

// The serial walk (raymarching.cu:200-234, 366-400), stated once: steps from
// t while t < t2 and fewer than `limit` samples are out, and calls
// emit(s, tc, x, y, z, dt, t_after) for sample s at t = tc (t_after: the walk's
// t behind it).  Returns the number of samples; t is left where the walk
// stopped.  The training marches' `0 <= t` is the caller's test at entry: t
// only grows or becomes +inf, so it holds for the whole loop or not at all.
template <bool SIMPLE, class Emit>
__device__ __forceinline__ int march_walk_serial(float& t, float t2, int limit, const float o[3], const float d[3],
                                                 const float dinv[3], const MarchParams& p, WordCache& wc, Emit emit) {
    int s = 0;
    float x, y, z, dt;
    while (t < t2 && s < limit) {
        const float tc = t;
        if (march_step<SIMPLE>(t, o, d, dinv, p, x, y, z, dt, wc)) {
            emit(s, tc, x, y, z, dt, t);
            s++;
        }
    }
    return s;
}

__device__ __forceinline__ void load_ray(const float* rays_o, const float* rays_d, int64_t r, float o[3],
                                         float d[3], float dinv[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = rays_o[3 * r + i];
        d[i] = rays_d[3 * r + i];
        dinv[i] = 1.0f / d[i];
    }
}

// custom_functions.py:83 noise + raymarching.cu:193-198 start perturbation
__device__ __forceinline__ float start_t(const float* hits_t, const float* noise, int64_t r, const MarchParams& p) {
    float t1 = hits_t[2 * r];
    if (t1 >= 0) {
        const float dt = calc_dt(t1, p.esf, p.max_samples, p.grid_size, p.scale);
        t1 += dt * noise[r];
    }
    return t1;
}

// ---------------------------------------------- wave-per-ray lattice march
// For SIMPLE launches (one cascade, esf = 0) every t the walk ever holds is a
// point of the lattice t_0, t_{k+1} = fl(t_k + dt) with a constant dt, and
// that lattice has a closed form: inside one binade [2^e, 2^(e+1)) adding dt
// moves a multiple of the binade's ulp u by the SAME multiple of u every time
// (dt/u has no exact .5 fraction; with one, the increment is constant from
// the second step on), so t_k = t_s + (k - s) * inc_s exactly (fmaf of an
// exact product).  This holds per binade only: a start at t_0 == 0 (any
// hits_t the C ABI is handed; the product's callers clamp to NEAR_DISTANCE)
// lies in none, and fl(k dt) from 0 parts from the serial sums within a dozen
// points, so lat_build gives 0 a single-point segment and the closed form
// starts at t_1 = dt.  The walk (march_step) from point k goes to k + 1 when the
// cell at t_k is occupied, else to the first j > k with t_j >= t_target(k).
// So one wave takes one ray (lat_walk): lane i evaluates lattice point c + i
// of a 64-point window (occupancy + jump target, in parallel), then the wave
// resolves the walk's chain through the window by pointer doubling and hands
// the visited occupied points, ranked, to the caller's emit.  Bit-identical
// to the serial walk; ~8192 waves per batch instead of 128 latency-bound ones.
// Used by march_slots_wave_kernel (training: (t, dt) into the ray's slots) and
// by the wave mode of render_march_kernel (sample-major test-render slots).
//
// Segment table (per ray, in LDS): segment q starts at lattice index K[q]
// with value T[q] and advances by I[q] per index until K[q + 1].
constexpr int LSEG = 32;
struct LatSeg {
    int K[LSEG + 1];
    float T[LSEG], I[LSEG];
};

// Conservative early out (exact), wave-wide: points every 0.45 of a 4^3 block
// along [t0, t2]; the walk's every probe lies within one block of one of
// them, so if no point's block has an occupied cell within one block (dil:
// the dilated summary), the walk emits nothing.  Most rays crossing the box
// miss the object and cost this instead of a full lattice walk.  Returns
// whether any point is near an occupied block (wave-uniform).
__device__ __forceinline__ bool lat_near_occupied(const float o[3], const float d[3], float t0, float t2,
                                                  const MarchParams& p, const uint32_t* dil) {
    const int lane = threadIdx.x & 63;
    const float mb = fminf(0.5f, p.scale);
    const float dn = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const float step = 0.45f * (4.0f * 2.0f * mb / p.grid_size) / dn;
    const int npts = (int)ceilf((t2 - t0) / step) + 1;
    const float gm1 = p.grid_size - 1.0f, mbi = 1 / mb;
    bool near = false;
    for (int j0 = 0; j0 < npts && !near; j0 += 64) {
        const int j = j0 + lane;
        bool b = false;
        if (j < npts) {
            const float t = fminf(t0 + (float)j * step, t2);
            const float x = o[0] + t * d[0], y = o[1] + t * d[1], z = o[2] + t * d[2];
            const int nx = (int)clampf(0.5f * (x * mbi + 1) * p.grid_size, 0.0f, gm1);
            const int ny = (int)clampf(0.5f * (y * mbi + 1) * p.grid_size, 0.0f, gm1);
            const int nz = (int)clampf(0.5f * (z * mbi + 1) * p.grid_size, 0.0f, gm1);
            const uint32_t wi = morton3((uint32_t)nx >> 2, (uint32_t)ny >> 2, (uint32_t)nz >> 2);
            b = (dil[wi >> 5] >> (wi & 31u)) & 1u;
        }
        near = __ballot(b) != 0ull;
    }
    return near;
}

// Builds the segments from t0 (>= 0) until the lattice passes t2 and returns
// k_end = first index with t >= t2 (the walk's stop), or -1 if the table
// overflows (caller falls back to the serial walk).  Wave-uniform.
__device__ __forceinline__ int lat_build(float t0, float t2, float dt, LatSeg& sg, int& nseg, bool write) {
    int k = 0, q = 0;
    float ts = t0;
    while (true) {
        if (!(ts < t2)) {  // this point already stops the walk
            if (write) sg.K[q] = k;
            nseg = q;
            return k;
        }
        if (q == LSEG) return -1;
        int e;
        frexpf(ts, &e);
        const float upper = ldexpf(1.0f, e);  // binade [upper/2, upper)
        const float a = ts + dt, b = a + dt;
        int n_max;  // last index offset of this segment
        float inc;
        if (!(a > ts)) return -1;  // dt below half an ulp: no progress, leave it to the serial walk
        if (!(ts > 0) || !(b < upper) || (b - a) != (a - ts)) {
            // single-point segment: binade end, a tie step, or ts == 0, which lies in no binade (frexpf gives
            // e = 0: [0, 1) would be walked as fl(k dt), while the serial walk rounds every sum); the next
            // point, fl(0 + dt), is in one
            n_max = 0;
            inc = a - ts;
        } else {
            inc = a - ts;
            n_max = (int)ceilf((upper - ts) / inc) - 1;
            while (fmaf((float)(n_max + 1), inc, ts) < upper) ++n_max;
            while (n_max > 0 && !(fmaf((float)n_max, inc, ts) < upper)) --n_max;
        }
        if (write) { sg.K[q] = k; sg.T[q] = ts; sg.I[q] = inc; }
        // the stop may fall inside this segment
        const float last = fmaf((float)n_max, inc, ts);
        if (!(last < t2)) {
            int n = (int)ceilf((t2 - ts) / inc);
            n = max(0, min(n, n_max));
            while (n > 0 && !(fmaf((float)(n - 1), inc, ts) < t2)) --n;
            while (fmaf((float)n, inc, ts) < t2) ++n;
            if (write) sg.K[q + 1] = k + n_max + 1;
            nseg = q + 1;
            return k + n;
        }
        ts = last + dt;  // the step that leaves the binade, as the walk rounds it
        k += n_max + 1;
        ++q;
    }
}

// first j > k with t_j >= T, for lane point k with value tk: inside the
// window's segment [Kq, Kn) (value Tq, increment Iq, its reciprocal invIq, in
// registers) from one estimate and exact fix-ups; a jump that would leave the
// segment steps on serially, t_{j+1} = fl(t_j + dt) -- the lattice's own
// definition (march_step's `do t += dt while (t < t_target)`), exact across
// any binade boundary.  The first index with t_j >= T is unique, so the
// estimate only sets the cost.
__device__ __forceinline__ int lat_jump_seg(int k, float tk, float T, float dt, int k_end, int Kq, int Kn, float Tq,
                                            float Iq, float invIq) {
    int j = k + 1;
    if (j < Kn) {
        if (fmaf((float)(j - Kq), Iq, Tq) >= T) return j;
        const float need = (T - fmaf((float)(j - Kq), Iq, Tq)) * invIq;
        int jj = min(j + (need < 4096.f ? max(1, (int)need) : 4096), Kn);
        while (jj > j + 1 && fmaf((float)(jj - 1 - Kq), Iq, Tq) >= T) --jj;
        if (jj < Kn) {
            while (jj < Kn && fmaf((float)(jj - Kq), Iq, Tq) < T) ++jj;
            if (jj < Kn) return jj;
        }
        // every point of the segment from j on lies below T: continue from its last one
        j = Kn;
        tk = fmaf((float)(Kn - 1 - Kq), Iq, Tq);
    }
    float t = tk;
    j -= 1;  // (t = t_j)
    do {
        t = t + dt;
        ++j;
    } while (t < T && j < k_end);
    return min(j, k_end);
}

// The lattice walk of one ray by one wave (all 64 lanes call it; the ray's
// o / d / dinv / dt and the table sg / nseg / k_end of lat_build are
// wave-uniform): windows of 64 lattice points until the walk reaches k_end or
// `limit` samples are out.  Calls emit(slot, tk, last) on the lane of every
// emitted point, slot = its index among the ray's samples, tk its t, last =
// it is the last one this window emits.  Returns the number of samples.  No
// block barrier inside: waves of a block may take different trip counts.
template <class Emit>
__device__ __forceinline__ int lat_walk(const float o[3], const float d[3], const float dinv[3], float dt, int k_end,
                                        int nseg, const LatSeg& sg, const MarchParams& p, const ProbeConsts& pc,
                                        WordCache& wc, int limit, Emit emit) {
    const int lane = threadIdx.x & 63;
    // the window's segment q0 = [Kq, Kn) in registers (re-read when the window passes Kn)
    int c = 0, N = 0, q0 = 0;
    int Kq = 0, Kn = -1;
    float Tq = 0.f, Iq = 0.f, invIq = 0.f;
    while (c < k_end && N < limit) {
        if (c >= Kn) {
            while (q0 + 1 < nseg && c >= sg.K[q0 + 1]) ++q0;
            Kq = sg.K[q0];
            Kn = q0 + 1 < nseg ? sg.K[q0 + 1] : k_end;
            Tq = uniform_f(sg.T[q0]);
            Iq = uniform_f(sg.I[q0]);
            invIq = uniform_f(1.0f / Iq);
        }
        const int k = c + lane;
        const bool live = k < k_end;
        bool occ = false;
        int nxt = k_end;
        float tk = 0.f;
        if (live) {
            if (k < Kn) {
                tk = fmaf((float)(k - Kq), Iq, Tq);
            } else {  // past the window's segment (the window straddles a binade): step on from its last point
                float t = fmaf((float)(Kn - 1 - Kq), Iq, Tq);
                for (int i = Kn; i <= k; ++i) t = t + dt;
                tk = t;
            }
            float T;
            occ = march_probe_simple(tk, o, d, dinv, p, pc, wc, T);
            nxt = occ ? k + 1 : lat_jump_seg(k, tk, T, dt, k_end, Kq, Kn, Tq, Iq, invIq);
        }
        const uint64_t occm = __ballot(occ);
        const uint64_t livem = __ballot(live);
        // The walk's chain through the window.  A window whose live points are all
        // occupied is visited whole (successor k + 1 throughout).  Otherwise, in
        // parallel: J_b(i) = the 2^b-th successor of window point i (64 = out of the
        // window), built by pointer doubling; every lane then climbs from point 0 with
        // binary lifting to the last chain point <= itself -- it is on the chain iff
        // that is itself (successors only move forward).  (A scalar hop per empty
        // chain point instead: ~14 hops per window in empty space, 30 SALU
        // instructions and 3 branches each, the kernel 1.6x slower with every wave
        // resident -- the CU's scalar unit is shared, profiles/r06/march_variants.txt.)
        uint64_t vis;
        int pnt;
        if (occm == livem) {
            vis = livem;
            pnt = (livem >> 63) ? c + 64 : k_end;
        } else {
            int J[6];
            J[0] = live ? min(nxt - c, 64) : 64;
#pragma unroll
            for (int b = 1; b < 6; ++b) {
                const int prev = J[b - 1];
                const int v = __builtin_amdgcn_ds_bpermute(min(prev, 63) << 2, prev);
                J[b] = prev >= 64 ? 64 : v;
            }
            int cu = 0;
#pragma unroll
            for (int b = 5; b >= 0; --b) {
                const int v = __builtin_amdgcn_ds_bpermute(min(cu, 63) << 2, J[b]);
                const int to = cu >= 64 ? 64 : v;
                if (to <= lane) cu = to;
            }
            vis = __ballot(cu == lane);
            const int last = 63 - __builtin_clzll(vis);  // the chain's last point in the window
            pnt = __builtin_amdgcn_readlane(nxt, last);  // k_end if it ends the walk
        }
        vis &= occm;
        // emit the chain's occupied points, at most up to the limit
        const int room = limit - N;
        const int ne = min(__builtin_popcountll(vis), room);
        if ((vis >> lane) & 1ull) {
            const int rank = __builtin_popcountll(vis & ((1ull << lane) - 1ull));
            if (rank < room) emit(N + rank, tk, rank == ne - 1);
        }
        N += ne;
        c = pnt;
    }
    return N;
}

}  // namespace ngp

using ngp::MarchParams;

// cascades == 1 and esf == 0 (the Lego configuration): see march_step.
// Also requires the bitfield to be 8-byte aligned for the word loads (torch
// allocations are).  dt_scale must be >= 0 so the constant-dt fold holds.
static inline bool march_simple(const MarchParams& p) { return p.cascades == 1 && p.esf == 0.0f && p.dt_scale >= 0.0f; }

static inline int march_params(const uint8_t* bf, int cascades, int grid_size, float scale, float esf, int max_samples,
                        MarchParams& p) {
    if (!bf || cascades < 1 || grid_size < 4 || grid_size > 1024 || max_samples < 1) return NGP_EINVAL;
    if (((uintptr_t)bf & 7u) != 0) return NGP_EINVAL;  // 64-bit word loads
    p.bitfield = bf; p.summary = nullptr; p.n_sum32 = 0; p.cascades = cascades; p.grid_size = grid_size; p.max_samples = max_samples;
    p.scale = scale; p.esf = esf; p.dt_scale = scale;
    return NGP_OK;
}


// Attach a bitfield summary (ngp_bitfield_summary output for this bitfield).
// Requires the LDS copy to fit the launch's dynamic LDS budget.
constexpr int MAX_SUM32 = 8192;  // 2 x 32 KB of LDS: cascades * G^3 <= 2^24 cells
static inline int march_attach_summary(MarchParams& p, const uint32_t* summary) {
    if (!summary) return NGP_OK;
    const int64_t cells = (int64_t)p.cascades * p.grid_size * p.grid_size * p.grid_size;
    if (cells % 2048 != 0) return NGP_EINVAL;  // whole summary words
    if (cells / 2048 > MAX_SUM32) return NGP_ERANGE;
    p.summary = summary;
    p.n_sum32 = (int)(cells / 2048);
    return NGP_OK;
}
// LDS for the summary and its dilation (both n_sum32 words)
static inline size_t march_summary_lds(const MarchParams& p) { return (size_t)2 * p.n_sum32 * sizeof(uint32_t); }

// ------------------------------------------- device-resident test render
namespace ngp {
// state (int64[NGP_RENDER_STATE_WORDS]) word indices (render.hip, insert.hip)
enum : int { RS_ALIVE0 = 0, RS_ALIVE1 = 1, RS_SAMPLES = 2, RS_NS = 3, RS_ACTIVE = 4, RS_VALID = 5, RS_TOTAL = 6,
             RS_ITERS = 7 };
// render_march_kernel over at most n_rays alive rays (render.hip)
void render_march_launch(const float* rays_o, const float* rays_d, float* hits_t, int64_t n_rays, const MarchParams& p,
                         int parity, int64_t* state, const int32_t* alive, float* xyzs, float* dirs, float* deltas,
                         float* ts, int32_t* n_eff, int32_t* sample_idx, hipStream_t s);
}  // namespace ngp
