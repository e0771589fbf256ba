// The field's forward (its MLP backward: field_bwd.hip; the hash-table backward:
// hash_bwd.hip).  Fused multires hash-grid encoding + tiny MLPs (density 32-64-16,
// colour 32-64-64-16) on gfx950 MFMA.  Replaces tiny-cuda-nn's
// NetworkWithInputEncoding / Encoding(SH4) / Network as the reference uses
// them (models/networks.py:37-78, 95-146).
//
// Work decomposition (one 64-lane wave = one 16-sample column block):
//   lane l -> sample s = l & 15 of the block, lane group g = l >> 4.
//   Lane (s, g) gathers hash levels 4g..4g+3 of sample s (32 independent
//   4-byte gathers of fp16x2 table entries), which lands the 8 encoding
//   values enc[s][8g..8g+7] directly in the B-operand layout of
//   v_mfma_f32_16x16x32_f16 (B[k = 8g + j][n = s]).  Every layer is computed
//   transposed, Y^T = W X^T (M = output units, N = samples), so each MFMA's
//   accumulator (rows 4g + r, column s) is re-packed in registers into the
//   next layer's B operand; the K order of that operand is permuted and the
//   weight columns are stored in LDS with the same permutation (field_net.h:
//   place_fwd8, P64inv / P32inv).
//   Weights (10240 fp16) live in LDS for the whole persistent wave loop.
// Numerics (tcnn storage points): fp16 params, fp32 interpolation weights
// and feature accumulation (fmaf over corners in tcnn order), fp16 encoding,
// fp32 MFMA accumulation, fp16 layer outputs, fp32 TruncExp / sigmoid.
#pragma clang fp contract(off)

#include "common.h"
#include "field_net.h"
#include "grid.h"
#include "level.h"
#include "transmittance.h"

namespace ngp {

// (types, weight-image layout, the nets, SH4 and the colour modes: field_net.h; one level's
// encoding: level.h)

// The colour half of one column block, the same at every forward site: sample
// i's direction (0, 0, 1 for a lane without a sample, ok false), SH4, the
// colour net on [SH, h] and the three colour outputs, stored by lane group 0.
__device__ __forceinline__ void color_column(const float* __restrict__ dirs, int64_t i, bool ok, h4 hh,
                                             const _Float16* sw, int s, int g, float* __restrict__ rgbs, int act) {
    const float dx = ok ? dirs[3 * i] : 0.f, dy = ok ? dirs[3 * i + 1] : 0.f, dz = ok ? dirs[3 * i + 2] : 1.f;
    float sh[4];
    sh4_select(dx, dy, dz, g, sh);
    const h8 cin = {(_Float16)sh[0], (_Float16)sh[1], (_Float16)sh[2], (_Float16)sh[3], hh[0], hh[1], hh[2], hh[3]};
    h4 h3[4], h4v[4];
    const h4 o = color_net(cin, sw, s, g, h3, h4v);
    if (ok && g == 0) {
        rgbs[3 * i] = rgb_out(o[0], act);
        rgbs[3 * i + 1] = rgb_out(o[1], act);
        rgbs[3 * i + 2] = rgb_out(o[2], act);
    }
}

// Sample i's levels [pre, 16) (E[l]: level l's two features, fp16x2) into the
// pair-major enc_pm of row stride n: pairs [pre / 2, 8).
__device__ __forceinline__ void store_enc_pm(_Float16* __restrict__ enc_pm, int64_t n, int64_t i, const uint32_t E[16],
                                             int pre) {
#pragma unroll
    for (int pr = 0; pr < 8; ++pr)
        if (2 * pr >= pre)
            *reinterpret_cast<uint2*>(enc_pm + ((int64_t)pr * n + i) * 4) = make_uint2(E[2 * pr], E[2 * pr + 1]);
}

// ENC_IN: the encoding comes from ngp_hash_encode (pair-major enc_in with
// row stride enc_stride) instead of being gathered here.
template <bool COLOR, bool ENC_IN = false>
__global__ void __launch_bounds__(256) field_fwd_kernel(const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                        int64_t n, const int64_t* __restrict__ n_dev, GridArgs ga,
                                                        const uint32_t* __restrict__ table,
                                                        const _Float16* __restrict__ mlp, float* __restrict__ sigmas,
                                                        float* __restrict__ rgbs, _Float16* __restrict__ enc_out,
                                                        _Float16* __restrict__ h_out,
                                                        const _Float16* __restrict__ enc_in = nullptr,
                                                        int64_t enc_stride = 0,
                                                        const int32_t* __restrict__ sidx = nullptr,
                                                        int act = NGP_RGB_SIGMOID) {
    __shared__ __attribute__((aligned(16))) _Float16 sw[SWF];
    __shared__ LevelLds lv;
    load_fwd_weights_direct(mlp, sw, COLOR);
    if constexpr (!ENC_IN) load_levels(ga, lv);
    __syncthreads();
    const int64_t N = ngp_capped_count(n_dev, n);  // (a device count never past the capacity: a guard hit)
    const int lane = threadIdx.x & 63, s = lane & 15, g = lane >> 4;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t base = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16; base < N; base += nw * 16) {
        const int64_t j = base + s;  // row of the launch; sample i (sidx: only the listed samples)
        const bool valid = j < N;
        const int64_t i = valid && sidx ? (int64_t)sidx[j] : j;
        h8 e;
        if constexpr (ENC_IN) {
            const h4 z4 = {0, 0, 0, 0};
            const h4 ea = valid ? *reinterpret_cast<const h4*>(enc_in + ((2 * g) * enc_stride + i) * 4) : z4;
            const h4 eb = valid ? *reinterpret_cast<const h4*>(enc_in + ((2 * g + 1) * enc_stride + i) * 4) : z4;
            e = pack(ea, eb);
        } else {
            float in[3];
            load_x01(xyzs, i, valid, ga, in);
            e = encode4(in, g, lv, table);
        }
        h4 h1[4];
        const h4 hh = density_net(e, sw, s, g, h1);
        if (valid) {
            if (enc_out) *reinterpret_cast<h8*>(enc_out + i * 32 + 8 * g) = e;
            if (h_out) *reinterpret_cast<h4*>(h_out + i * 16 + 4 * g) = hh;
            if (g == 0) sigmas[i] = expf((float)hh[0]);  // TruncExp forward (custom_functions.py:165-167)
        }
        if constexpr (COLOR) color_column(dirs, i, valid, hh, sw, s, g, rgbs, act);
    }
}

// ------------------------------------------------------ hash encode alone
// Multires hash encoding alone (the gathers of field_fwd_kernel, same
// arithmetic, bit-identical values), written pair-major:
//   enc_pm[p][i][0..3] = enc[i][4p .. 4p+3]  (levels 2p, 2p+1; p = 0..7).
// Each lane encodes every level of one sample, so a wave instruction gathers
// ONE level for 64 consecutive samples (a ray's neighbours: shared lines on
// the coarse levels) -- 1.55x the rate of one level pair per XCD and 1.8x
// field_fwd_kernel's lane (sample, level group) layout
// (scripts/diag/encode_split.py).  sidx (nullable): rows j < N encode sample
// sidx[j] (rows of enc_pm are samples).
__global__ void __launch_bounds__(256) hash_encode_kernel(const float* __restrict__ xyzs, int64_t n,
                                                          const int64_t* __restrict__ n_dev,
                                                          const int32_t* __restrict__ sidx, GridArgs ga,
                                                          const uint32_t* __restrict__ table,
                                                          _Float16* __restrict__ enc_pm) {
    __shared__ LevelLds lv;
    load_levels(ga, lv);
    __syncthreads();
    const int64_t N = ngp_capped_count(n_dev, n);  // (a device count never past the capacity: a guard hit)
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = sidx ? (int64_t)sidx[j] : j;
        float in[3];
        load_x01(xyzs, i, true, ga, in);
#pragma unroll 1
        for (int pr = 0; pr < 8; ++pr) {
            float w[2][8];
            uint32_t v[2][8];
            gather_level_u(in, level_u(lv, 2 * pr), table, w[0], v[0]);
            gather_level_u(in, level_u(lv, 2 * pr + 1), table, w[1], v[1]);
            float a0, a1, b0, b1;
            sum_level(w[0], v[0], a0, a1);
            sum_level(w[1], v[1], b0, b1);
            *reinterpret_cast<h4*>(enc_pm + ((int64_t)pr * n + i) * 4) =
                h4{(_Float16)a0, (_Float16)a1, (_Float16)b0, (_Float16)b1};
        }
    }
}

// ------------------------------ fused encode + MLP forward, register form
// field_fwd_kernel's arithmetic (bit-identical outputs) on 64-sample chunks,
// one lane per sample for the gathers and one column block at a time for the
// nets:
//  * the encoding never goes through LDS: a lane keeps its sample's 16 level
//    dwords (fp16x2 features) in registers, and a 4 x 4 transpose of 4-dword
//    groups across the wave's four 16-lane rows (two v_permlane32_swap and
//    two v_permlane16_swap stages) lands, for column block c, the operand
//    enc[16c + s][8g .. 8g+7] in lane (s, g) -- the B layout of
//    v_mfma_f32_16x16x32_f16; a block's LDS is the 24 KB weight image alone,
//    so occupancy is set by registers (parking the rows in LDS took 40 KB more);
//  * FEM_LPR levels are gathered per round (their loads issued together), so a
//    lane's chain of dependent gather rounds is 16 / FEM_LPR long;
//  * 64-sample chunks are dealt to waves interleaved over the whole grid
//    (chunk k -> wave k / G of block k % G): every resident block gets the
//    same number of chunks within one, so no CU holds two blocks' worth of
//    work while others hold one (a one-pass grid of ceil(N/512) blocks left
//    ~20 % of the CUs doubly loaded).

// 4 x 4 transpose of 4-dword groups across the wave's 16-lane rows: on entry
// register group r (E[4r..4r+3]) of lane row q holds group r of the row's
// sample; on exit group c of lane row g holds group g of row c's sample.
__device__ __forceinline__ void transpose_rows4(uint32_t E[16]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // stage 1: upper 32 lanes of groups 0 / 1 <-> lower 32 lanes of groups 2 / 3
        const auto a = __builtin_amdgcn_permlane32_swap(E[k], E[8 + k], false, false);
        E[k] = a[0];
        E[8 + k] = a[1];
        const auto b = __builtin_amdgcn_permlane32_swap(E[4 + k], E[12 + k], false, false);
        E[4 + k] = b[0];
        E[12 + k] = b[1];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // stage 2: odd rows of groups 0 / 2 <-> even rows of groups 1 / 3
        const auto a = __builtin_amdgcn_permlane16_swap(E[k], E[4 + k], false, false);
        E[k] = a[0];
        E[4 + k] = a[1];
        const auto b = __builtin_amdgcn_permlane16_swap(E[8 + k], E[12 + k], false, false);
        E[8 + k] = b[0];
        E[12 + k] = b[1];
    }
}

// 8 waves per block; 2 levels per gather round (4: the loads of 4 levels in flight need > 128
// VGPRs and spill, -3 %)
constexpr int FEM2_WAVES = 8, FEM_LPR = 2;
constexpr int PRE_LEVELS = 8;  // coarse levels round 1 may find pre-encoded (encode_coarse_first_kernel)
static_assert(PRE_LEVELS % FEM_LPR == 0 && PRE_LEVELS % 2 == 0, "pre-encoded levels: whole rounds and pairs");
static_assert(L % FEM_LPR == 0, "levels per round");
// The gather rounds [r0, L / FEM_LPR) of one sample's encoding, FEM_LPR levels each, not
// unrolled (an unrolled chain hoists every round's loads: 256 VGPRs); each round shifts its
// levels into the top of E (fp16x2 per level), so after the last round E[l] holds level l
// (levels below FEM_LPR * r0: whatever the caller put at the top of E).
__device__ __forceinline__ void encode_rounds(const float in[3], const LevelLds& lv, const uint32_t* __restrict__ table,
                                              int r0, uint32_t E[16]) {
#pragma unroll 1
    for (int r = r0; r < L / FEM_LPR; ++r) {
        uint32_t v[FEM_LPR][8];
#pragma unroll
        for (int q = 0; q < FEM_LPR; ++q) gather_level_loads(in, level_u(lv, FEM_LPR * r + q), table, v[q]);
#pragma unroll
        for (int q = 0; q < 16 - FEM_LPR; ++q) E[q] = E[q + FEM_LPR];
#pragma unroll
        for (int q = 0; q < FEM_LPR; ++q) E[16 - FEM_LPR + q] = level_sum_h2(in, level_u(lv, FEM_LPR * r + q), v[q]);
    }
}
template <bool COLOR>
__global__ void __launch_bounds__(64 * FEM2_WAVES, FEM2_WAVES / 2) field_encode_mlp_reg_kernel(
    const float* __restrict__ xyzs, const float* __restrict__ dirs, int64_t n, const int64_t* __restrict__ n_dev,
    const int32_t* __restrict__ sidx, GridArgs ga, const uint32_t* __restrict__ table,
    const _Float16* __restrict__ mlp, _Float16* __restrict__ enc_pm, float* __restrict__ sigmas,
    float* __restrict__ rgbs, _Float16* __restrict__ h_out, int act) {
    __shared__ __attribute__((aligned(16))) _Float16 sw[SWF];
    __shared__ LevelLds lv;
    NGP_PROBE_BEGIN(NGP_P_FIELD_ENCODE_MLP);
    const int64_t N = ngp_capped_count(n_dev, n);  // (a device count never past the capacity: a guard hit)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t G = gridDim.x;
    const int64_t chunks = (N + 63) >> 6;
    int64_t k = (int64_t)wv * G + blockIdx.x;  // first chunk of this wave (wave-uniform)
    // the first chunk's index and position (count -> index -> position: dependent round
    // trips) requested before the weight image is built, so the two overlap
    int64_t i_first = 0;
    float in_first[3];
    {
        const int64_t j = k * 64 + lane;
        const bool valid = k < chunks && j < N;
        i_first = valid ? (sidx ? (int64_t)sidx[j] : j) : 0;
        load_x01(xyzs, i_first, valid, ga, in_first);
    }
    load_fwd_weights_direct(mlp, sw, COLOR);
    load_levels(ga, lv);
    __syncthreads();
    bool first = true;
    for (; k < chunks; k += (int64_t)FEM2_WAVES * G) {
        int lane_l = lane;  // (opaque per iteration: lane-derived addresses are not held across the loop)
        asm volatile("" : "+v"(lane_l));
        const int s = lane_l & 15, g = lane_l >> 4;
        const int64_t j = k * 64 + lane_l;
        const bool valid = j < N;
        int64_t i = i_first;
        float in[3] = {in_first[0], in_first[1], in_first[2]};
        if (!first) {
            i = valid ? (sidx ? (int64_t)sidx[j] : j) : 0;
            load_x01(xyzs, i, valid, ga, in);
        }
        first = false;
        uint32_t E[16];  // level l's two features, fp16x2
        encode_rounds(in, lv, table, 0, E);
        if (valid && enc_pm) store_enc_pm(enc_pm, n, i, E, 0);
        transpose_rows4(E);
        const int32_t imine = valid ? (int32_t)i : -1;
        // column blocks in a loop (not unrolled: register pressure); block c's operand is
        // E[0..3] after c rotations by one group
#pragma unroll 1
        for (int c = 0; c < 4; ++c) {
            const int32_t ic = __shfl(imine, 16 * c + s, 64);
            const bool ok = ic >= 0;
            const h8 e = __builtin_bit_cast(h8, make_uint4(E[0], E[1], E[2], E[3]));
#pragma unroll
            for (int q = 0; q < 12; ++q) E[q] = E[q + 4];
            h4 h1[4];
            const h4 hh = density_net(e, sw, s, g, h1);
            if (ok) {
                if (h_out) *reinterpret_cast<h4*>(h_out + (int64_t)ic * 16 + 4 * g) = hh;
                if (g == 0) sigmas[ic] = expf((float)hh[0]);  // TruncExp forward (custom_functions.py:165-167)
            }
            if constexpr (COLOR) color_column(dirs, ic, ok, hh, sw, s, g, rgbs, act);
        }
    }
    NGP_PROBE_END();
}

// Encode + MLPs of the 64-sample chunk [i0, i0 + cnt) on one wave (lane =
// sample i0 + lane): field_encode_mlp_reg_kernel's body for a contiguous
// chunk; returns this lane's sigma (0 past cnt) for a transmittance epilogue.
// pre (0 or PRE_LEVELS): levels [0, pre) are already in enc_pm (written by
// encode_coarse_first_kernel with the same arithmetic) and only read back.
template <bool COLOR>
__device__ __forceinline__ float encode_mlp_chunk(const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                  int64_t i0, int cnt, int64_t n, const GridArgs& ga,
                                                  const LevelLds& lv, const uint32_t* __restrict__ table,
                                                  const _Float16* sw, _Float16* __restrict__ enc_pm,
                                                  float* __restrict__ sigmas, float* __restrict__ rgbs, int pre = 0,
                                                  int act = NGP_RGB_SIGMOID) {
    int lane_l = threadIdx.x & 63;  // (opaque: lane-derived addresses are rematerialised, not held)
    asm volatile("" : "+v"(lane_l));
    const int s = lane_l & 15, g = lane_l >> 4;
    const bool valid = lane_l < cnt;
    const int64_t i = i0 + lane_l;
    float in[3];
    load_x01(xyzs, i, valid, ga, in);
    uint32_t E[16];
    if (pre) {
        // after pre / FEM_LPR rounds the chain holds levels [0, pre) at the top of E
#pragma unroll
        for (int pr = 0; pr < PRE_LEVELS / 2; ++pr) {
            const uint2 q = valid ? *reinterpret_cast<const uint2*>(enc_pm + ((int64_t)pr * n + i) * 4) : make_uint2(0u, 0u);
            E[16 - PRE_LEVELS + 2 * pr] = q.x;
            E[16 - PRE_LEVELS + 2 * pr + 1] = q.y;
        }
    }
    encode_rounds(in, lv, table, pre / FEM_LPR, E);
    if (valid && enc_pm) store_enc_pm(enc_pm, n, i, E, pre);
    transpose_rows4(E);
    float sg = 0.f;
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        if (16 * c >= cnt) break;  // (wave-uniform: no sample in this or a later column block)
        const bool ok = 16 * c + s < cnt;
        const int64_t ic = i0 + 16 * c + s;
        const h8 e = __builtin_bit_cast(h8, make_uint4(E[0], E[1], E[2], E[3]));
#pragma unroll
        for (int q = 0; q < 12; ++q) E[q] = E[q + 4];
        h4 h1[4];
        const h4 hh = density_net(e, sw, s, g, h1);
        const float sig = expf((float)hh[0]);  // TruncExp forward (custom_functions.py:165-167)
        if (ok && g == 0) sigmas[ic] = sig;
        const float sgc = __shfl(sig, lane_l & 15, 64);  // sample 16 c + s's sigma to lane 16 c + s
        if ((lane_l >> 4) == c) sg = sgc;
        if constexpr (COLOR) color_column(dirs, ic, ok, hh, sw, s, g, rgbs, act);
    }
    return sg;
}

// Round 1 of the chunked training forward with the round-2 counts fused in:
// one wave per non-empty row (rows[], built beside the previous step by
// ngp_rays_nonempty, so no wave holds more than its one chunk while rows are
// fewer than resident waves), its first min(N, 64) samples encoded and run
// through the MLPs, then the row's transmittance over them
// (chunk_transmittance, the composite's product scan: the same function and
// expressions as chunk_segments_kernel) -> rc = N - 64 if the row is still
// transparent after its first chunk, else 0.  rest (nullable): rest[r] = rc
// (the counts ngp_chunk_counts_range gives).  list2 (nullable): the row's
// round-2 samples start + 64 .. start + N appended to list2 at a range
// reserved by one atomic on *total2 (zero at launch): the round-2 list
// without any scan -- rows land in reservation order, each row's samples
// contiguous (the forward's outputs are per sample, so the order changes no
// value); their count is added to *evaluated with the first chunks'.  A wave
// per row rather than 64 packed list entries (~8 % idle lanes on this step's
// rows); the sigmas never leave registers.
template <bool COLOR>
__global__ void __launch_bounds__(64 * FEM2_WAVES, FEM2_WAVES / 2) field_first_chunk_kernel(
    const float* __restrict__ xyzs, const float* __restrict__ dirs, const float* __restrict__ deltas,
    const int64_t* __restrict__ rays_a, const int32_t* __restrict__ rows, const int64_t* __restrict__ n_rows_dev,
    int64_t n_rows, int64_t n, float T_thr, GridArgs ga, const uint32_t* __restrict__ table,
    const _Float16* __restrict__ mlp, _Float16* __restrict__ enc_pm, float* __restrict__ sigmas,
    float* __restrict__ rgbs, int32_t* __restrict__ rest, int32_t* __restrict__ list2, int64_t* __restrict__ total2,
    int64_t* __restrict__ evaluated, int pre, int act) {
    __shared__ __attribute__((aligned(16))) _Float16 sw[SWF];
    __shared__ LevelLds lv;
    __shared__ unsigned long long blk_eval;
    NGP_PROBE_BEGIN(NGP_P_FIRST_CHUNK);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t NR = ngp_capped_count(n_rows_dev, n_rows);  // (a device count never past the capacity: a guard hit)
    const int64_t G = gridDim.x, stride = (int64_t)FEM2_WAVES * G;
    int64_t j = (int64_t)wv * G + blockIdx.x;  // the wave's first row (wave-uniform)
    // its row (list -> rays_a: dependent round trips) requested before the weight image is built
    int64_t r = 0, start = 0, N = 0;
    if (j < NR) {
        r = rows ? (int64_t)rows[j] : j;
        start = rays_a[3 * r + 1];
        N = rays_a[3 * r + 2];
    }
    if (threadIdx.x == 0) blk_eval = 0ull;
    load_fwd_weights_direct(mlp, sw, COLOR);
    load_levels(ga, lv);
    __syncthreads();
    int64_t ev = 0;
    for (; j < NR; j += stride) {
        const int cnt = (int)(N < 64 ? N : 64);
        int32_t rc = 0;
        if (cnt > 0) {
            const float dl = lane < cnt ? deltas[start + lane] : 0.f;
            const float sg = encode_mlp_chunk<COLOR>(xyzs, dirs, start, cnt, n, ga, lv, table, sw, enc_pm, sigmas, rgbs,
                                                     pre, act);
            const float om = 1.0f - (1.0f - __expf(-sg * dl));  // chunk_segments_kernel's expression
            const ChunkT ct = chunk_transmittance(om, cnt, 1.0f, T_thr, lane);
            rc = (!ct.hit && N > 64) ? (int32_t)(N - 64) : 0;
            ev += cnt;
        }
        if (rest && lane == 0) rest[r] = rc;
        if (list2 && rc > 0) {
            unsigned long long o = 0;
            if (lane == 0) o = atomicAdd((unsigned long long*)total2, (unsigned long long)rc);
            const int64_t o2 = (int64_t)__shfl(o, 0, 64);
            if (lane == 0 && o2 + rc > n) ngp_guard_hit();  // (past the list's capacity n: counted, then bounded)
            for (int t = lane; t < rc && o2 + t < n; t += 64) list2[o2 + t] = (int32_t)(start + 64 + t);
            ev += rc;
        }
        const int64_t jn = j + stride;
        if (jn < NR) {
            r = rows ? (int64_t)rows[jn] : jn;
            start = rays_a[3 * r + 1];
            N = rays_a[3 * r + 2];
        }
    }
    if (lane == 0 && ev) atomicAdd(&blk_eval, (unsigned long long)ev);
    __syncthreads();
    if (threadIdx.x == 0 && evaluated && blk_eval) atomicAdd((unsigned long long*)evaluated, blk_eval);
    NGP_PROBE_END();
}

// Levels [0, PRE_LEVELS) of round 1's encoding, ahead of time: for the rows
// rows[j], j < *n_rows_dev, of the NEXT batch (its march and row list are
// done beside the current step), the first min(N, 64) samples' coarse-level
// features, written to the pair-major enc_pm (pairs [0, PRE_LEVELS / 2)) with
// encode_mlp_chunk's arithmetic.  Those levels' parameters are final once the
// MLP + coarse levels' Adam of the current step has run, ~a bucket
// accumulation before the step ends, so this runs beside the binned levels'
// accumulation and round 1 of the next step (field_first_chunk_kernel with
// pre = PRE_LEVELS) gathers only the fine levels: half its dependent gather
// rounds leave the critical path.
__global__ void __launch_bounds__(256) encode_coarse_first_kernel(
    const float* __restrict__ xyzs, const int64_t* __restrict__ rays_a, const int32_t* __restrict__ rows,
    const int64_t* __restrict__ n_rows_dev, int64_t n_rows, int64_t n, GridArgs ga,
    const uint32_t* __restrict__ table, _Float16* __restrict__ enc_pm) {
    __shared__ LevelLds lv;
    NGP_PROBE_BEGIN(NGP_P_PRE_ENCODE);
    load_levels(ga, lv);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t NR = ngp_capped_count(n_rows_dev, n_rows);  // (a device count never past the capacity: a guard hit)
    // a wave item = (row, level pair): one gather round per item, the row's PRE_LEVELS / 2 pairs
    // on consecutive waves (one dependent round each instead of PRE_LEVELS / 2 per row: the rows
    // are ~2.7 K, a third of the waves the chip holds)
    constexpr int NP = PRE_LEVELS / 2;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t q = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); q < NR * NP; q += stride) {
        const int64_t j = q / NP;
        const int pr = (int)(q - j * NP);
        const int64_t r = rows ? (int64_t)rows[j] : j;
        const int64_t start = rays_a[3 * r + 1], N = rays_a[3 * r + 2];
        const bool valid = lane < N;
        const int64_t i = start + lane;
        float in[3];
        load_x01(xyzs, i, valid, ga, in);
        uint32_t v[2][8];
        gather_level_loads(in, level_u(lv, 2 * pr), table, v[0]);
        gather_level_loads(in, level_u(lv, 2 * pr + 1), table, v[1]);
        const uint32_t e0 = level_sum_h2(in, level_u(lv, 2 * pr), v[0]);
        const uint32_t e1 = level_sum_h2(in, level_u(lv, 2 * pr + 1), v[1]);
        if (valid) *reinterpret_cast<uint2*>(enc_pm + ((int64_t)pr * n + i) * 4) = make_uint2(e0, e1);
    }
    NGP_PROBE_END();
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_field_forward(const float* xyzs, const float* dirs, int64_t n, const int64_t* n_dev,
                      const ngp_hashgrid_t* grid, const void* table_f16, const void* mlp_f16, float* sigmas,
                      float* rgbs, void* enc_f16, void* h_f16, void* stream) {
    return ngp_field_forward_act(xyzs, dirs, n, n_dev, grid, table_f16, mlp_f16, sigmas, rgbs, enc_f16, h_f16,
                                 NGP_RGB_SIGMOID, stream);
}

int ngp_field_forward_act(const float* xyzs, const float* dirs, int64_t n, const int64_t* n_dev,
                          const ngp_hashgrid_t* grid, const void* table_f16, const void* mlp_f16, float* sigmas,
                          float* rgbs, void* enc_f16, void* h_f16, int rgb_act, void* stream) {
    NGP_CHECK_RGB_ACT(rgb_act);
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n >= 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(xyzs && dirs && table_f16 && mlp_f16 && sigmas && rgbs);
    NGP_CHECK_ARG(((uintptr_t)table_f16 & 15) == 0);  // 16-byte group gathers
    NGP_CHECK_ARG(((uintptr_t)mlp_f16 & 15) == 0);
    static const unsigned cap = resident_blocks(field_fwd_kernel<true>, 256, 0);
    field_fwd_kernel<true><<<persistent_blocks(n, 64, cap), 256, 0, as_stream(stream)>>>(
        xyzs, dirs, n, n_dev, ga, (const uint32_t*)table_f16, (const _Float16*)mlp_f16, sigmas, rgbs,
        (_Float16*)enc_f16, (_Float16*)h_f16, nullptr, 0, nullptr, rgb_act);
    return ngp_launch_status();
}

int ngp_field_forward_indexed(const float* xyzs, const float* dirs, int64_t n, const int64_t* n_dev,
                              const int32_t* sample_idx, const ngp_hashgrid_t* grid, const void* table_f16,
                              const void* mlp_f16, float* sigmas, float* rgbs, void* enc_f16, void* stream) {
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n >= 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(xyzs && dirs && sample_idx && table_f16 && mlp_f16 && sigmas && rgbs);
    NGP_CHECK_ARG(((uintptr_t)table_f16 & 15) == 0);  // 16-byte group gathers
    NGP_CHECK_ARG(((uintptr_t)mlp_f16 & 15) == 0);
    static const unsigned cap = resident_blocks(field_fwd_kernel<true>, 256, 0);
    field_fwd_kernel<true><<<persistent_blocks(n, 64, cap), 256, 0, as_stream(stream)>>>(
        xyzs, dirs, n, n_dev, ga, (const uint32_t*)table_f16, (const _Float16*)mlp_f16, sigmas, rgbs,
        (_Float16*)enc_f16, nullptr, nullptr, 0, sample_idx);
    return ngp_launch_status();
}

int ngp_density_forward(const float* xyzs, int64_t n, const int64_t* n_dev, const ngp_hashgrid_t* grid,
                        const void* table_f16, const void* mlp_f16, float* sigmas, void* h_f16, void* stream) {
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n >= 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(xyzs && table_f16 && mlp_f16 && sigmas);
    NGP_CHECK_ARG(((uintptr_t)table_f16 & 15) == 0);  // 16-byte group gathers
    NGP_CHECK_ARG(((uintptr_t)mlp_f16 & 15) == 0);
    static const unsigned cap = resident_blocks(field_fwd_kernel<false>, 256, 0);
    field_fwd_kernel<false><<<persistent_blocks(n, 64, cap), 256, 0, as_stream(stream)>>>(
        xyzs, nullptr, n, n_dev, ga, (const uint32_t*)table_f16, (const _Float16*)mlp_f16, sigmas, nullptr, nullptr,
        (_Float16*)h_f16);
    return ngp_launch_status();
}

int ngp_hash_encode(const float* xyzs, int64_t n, const int64_t* n_dev, const int32_t* sample_idx,
                    const ngp_hashgrid_t* grid, const void* table_f16, void* enc_pm, void* stream) {
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n >= 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(xyzs && table_f16 && enc_pm && ((uintptr_t)enc_pm & 7) == 0);
    NGP_CHECK_ARG(((uintptr_t)table_f16 & 15) == 0);  // 16-byte group gathers
    hipStream_t s = as_stream(stream);
    static const unsigned cap = resident_blocks(hash_encode_kernel, 256, 0);
    NGP_TIMED(NGP_K_HASH_ENCODE, s, hash_encode_kernel<<<persistent_blocks(n, 256, cap), 256, 0, s>>>(
        xyzs, n, n_dev, sample_idx, ga, (const uint32_t*)table_f16, (_Float16*)enc_pm));
    return ngp_launch_status();
}

int ngp_field_encode_mlp(const float* xyzs, const float* dirs, int64_t n, const int64_t* n_dev,
                         const int32_t* sample_idx, const ngp_hashgrid_t* grid, const void* table_f16,
                         const void* mlp_f16, void* enc_pm, float* sigmas, float* rgbs, void* h_f16, void* stream) {
    return ngp_field_encode_mlp_act(xyzs, dirs, n, n_dev, sample_idx, grid, table_f16, mlp_f16, enc_pm, sigmas, rgbs,
                                    h_f16, NGP_RGB_SIGMOID, stream);
}

int ngp_field_encode_mlp_act(const float* xyzs, const float* dirs, int64_t n, const int64_t* n_dev,
                             const int32_t* sample_idx, const ngp_hashgrid_t* grid, const void* table_f16,
                             const void* mlp_f16, void* enc_pm, float* sigmas, float* rgbs, void* h_f16, int rgb_act,
                             void* stream) {
    NGP_CHECK_RGB_ACT(rgb_act);
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n >= 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(xyzs && table_f16 && mlp_f16 && sigmas && (dirs != nullptr) == (rgbs != nullptr));
    NGP_CHECK_ARG(((uintptr_t)table_f16 & 15) == 0 && ((uintptr_t)mlp_f16 & 15) == 0 && ((uintptr_t)enc_pm & 7) == 0);
    hipStream_t s = as_stream(stream);
    // grid = every resident block (the chunks are dealt over the whole grid)
    if (!dirs) {
        static const unsigned capd = resident_blocks(field_encode_mlp_reg_kernel<false>, 64 * FEM2_WAVES, 0);
        NGP_TIMED(NGP_K_HASH_ENCODE, s, field_encode_mlp_reg_kernel<false><<<persistent_blocks(n, 64 * FEM2_WAVES, capd), 64 * FEM2_WAVES, 0, s>>>(
            xyzs, nullptr, n, n_dev, sample_idx, ga, (const uint32_t*)table_f16, (const _Float16*)mlp_f16,
            (_Float16*)enc_pm, sigmas, nullptr, (_Float16*)h_f16, NGP_RGB_SIGMOID));
        return ngp_launch_status();
    }
    static const unsigned capr = resident_blocks(field_encode_mlp_reg_kernel<true>, 64 * FEM2_WAVES, 0);
    NGP_TIMED(NGP_K_HASH_ENCODE, s, field_encode_mlp_reg_kernel<true><<<persistent_blocks(n, 64 * FEM2_WAVES, capr), 64 * FEM2_WAVES, 0, s>>>(
        xyzs, dirs, n, n_dev, sample_idx, ga, (const uint32_t*)table_f16, (const _Float16*)mlp_f16,
        (_Float16*)enc_pm, sigmas, rgbs, (_Float16*)h_f16, rgb_act));
    return ngp_launch_status();
}

int ngp_field_forward_first_pre(const float* xyzs, const float* dirs, const float* deltas, const int64_t* rays_a,
                                const int32_t* rows, const int64_t* n_rows_dev, int64_t n_rows, int64_t n,
                                float T_threshold, const ngp_hashgrid_t* grid, const void* table_f16,
                                const void* mlp_f16, void* enc_pm, float* sigmas, float* rgbs, int32_t* rest,
                                int32_t* list2, int64_t* total2, int64_t* evaluated, int pre_levels, void* stream) {
    return ngp_field_forward_first_pre_act(xyzs, dirs, deltas, rays_a, rows, n_rows_dev, n_rows, n, T_threshold, grid,
                                           table_f16, mlp_f16, enc_pm, sigmas, rgbs, rest, list2, total2, evaluated,
                                           pre_levels, NGP_RGB_SIGMOID, stream);
}

int ngp_field_forward_first_pre_act(const float* xyzs, const float* dirs, const float* deltas, const int64_t* rays_a,
                                    const int32_t* rows, const int64_t* n_rows_dev, int64_t n_rows, int64_t n,
                                    float T_threshold, const ngp_hashgrid_t* grid, const void* table_f16,
                                    const void* mlp_f16, void* enc_pm, float* sigmas, float* rgbs, int32_t* rest,
                                    int32_t* list2, int64_t* total2, int64_t* evaluated, int pre_levels, int rgb_act,
                                    void* stream) {
    NGP_CHECK_RGB_ACT(rgb_act);
    NGP_CHECK_ARG(pre_levels == 0 || (pre_levels == PRE_LEVELS && enc_pm));
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n_rows >= 0 && n >= 0);
    if (n_rows == 0) return NGP_OK;
    NGP_CHECK_ARG(xyzs && dirs && deltas && rays_a && table_f16 && mlp_f16 && sigmas && rgbs && (rest || list2));
    NGP_CHECK_ARG(!list2 || (total2 && ((uintptr_t)total2 & 7) == 0));
    NGP_CHECK_ARG(((uintptr_t)table_f16 & 15) == 0 && ((uintptr_t)mlp_f16 & 15) == 0 && ((uintptr_t)enc_pm & 7) == 0 &&
                  ((uintptr_t)evaluated & 7) == 0);
    hipStream_t s = as_stream(stream);
    // grid = every resident block: the rows are dealt over all resident waves
    static const unsigned cap = resident_blocks(field_first_chunk_kernel<true>, 64 * FEM2_WAVES, 0);
    const unsigned blocks = persistent_blocks(n_rows, FEM2_WAVES, cap);
    NGP_TIMED(NGP_K_HASH_ENCODE, s, field_first_chunk_kernel<true><<<blocks, 64 * FEM2_WAVES, 0, s>>>(
        xyzs, dirs, deltas, rays_a, rows, n_rows_dev, n_rows, n, T_threshold, ga, (const uint32_t*)table_f16,
        (const _Float16*)mlp_f16, (_Float16*)enc_pm, sigmas, rgbs, rest, list2, total2, evaluated, pre_levels,
        rgb_act));
    return ngp_launch_status();
}

int ngp_field_forward_first(const float* xyzs, const float* dirs, const float* deltas, const int64_t* rays_a,
                            const int32_t* rows, const int64_t* n_rows_dev, int64_t n_rows, int64_t n,
                            float T_threshold, const ngp_hashgrid_t* grid, const void* table_f16, const void* mlp_f16,
                            void* enc_pm, float* sigmas, float* rgbs, int32_t* rest, int32_t* list2,
                            int64_t* total2, int64_t* evaluated, void* stream) {
    return ngp_field_forward_first_pre(xyzs, dirs, deltas, rays_a, rows, n_rows_dev, n_rows, n, T_threshold, grid,
                                       table_f16, mlp_f16, enc_pm, sigmas, rgbs, rest, list2, total2, evaluated, 0,
                                       stream);
}

int ngp_field_encode_first_coarse(const float* xyzs, const int64_t* rays_a, const int32_t* rows,
                                  const int64_t* n_rows_dev, int64_t n_rows, int64_t n, const ngp_hashgrid_t* grid,
                                  const void* table_f16, void* enc_pm, void* stream) {
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    NGP_CHECK_ARG(n_rows >= 0 && n >= 0);
    if (n_rows == 0) return NGP_OK;
    NGP_CHECK_ARG(xyzs && rays_a && table_f16 && enc_pm && ((uintptr_t)table_f16 & 15) == 0 &&
                  ((uintptr_t)enc_pm & 7) == 0);
    hipStream_t s = as_stream(stream);
    static const unsigned cap = resident_blocks(encode_coarse_first_kernel, 256, 0);
    const unsigned blocks = persistent_blocks(n_rows * (PRE_LEVELS / 2), 4, cap);
    encode_coarse_first_kernel<<<blocks, 256, 0, s>>>(xyzs, rays_a, rows, n_rows_dev, n_rows, n, ga,
                                                      (const uint32_t*)table_f16, (_Float16*)enc_pm);
    return ngp_launch_status();
}

int ngp_field_mlp_forward(const void* enc_pm, const float* dirs, int64_t n, const int64_t* n_dev,
                          const int32_t* sample_idx, const void* mlp_f16, float* sigmas, float* rgbs, void* h_f16,
                          void* stream) {
    NGP_CHECK_ARG(n >= 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(enc_pm && mlp_f16 && sigmas && (dirs != nullptr) == (rgbs != nullptr));
    NGP_CHECK_ARG(((uintptr_t)mlp_f16 & 15) == 0 && ((uintptr_t)enc_pm & 7) == 0);
    GridArgs ga{};
    if (!dirs) {  // density net only (occupancy updates)
        static const unsigned capd = resident_blocks(field_fwd_kernel<false, true>, 256, 0);
        NGP_TIMED(NGP_K_FIELD_MLP, as_stream(stream),
                  field_fwd_kernel<false, true><<<persistent_blocks(n, 64, capd), 256, 0, as_stream(stream)>>>(
                      nullptr, nullptr, n, n_dev, ga, nullptr, (const _Float16*)mlp_f16, sigmas, nullptr, nullptr,
                      (_Float16*)h_f16, (const _Float16*)enc_pm, n, sample_idx));
        return ngp_launch_status();
    }
    static const unsigned cap = resident_blocks(field_fwd_kernel<true, true>, 256, 0);
    NGP_TIMED(NGP_K_FIELD_MLP, as_stream(stream),
              field_fwd_kernel<true, true><<<persistent_blocks(n, 64, cap), 256, 0, as_stream(stream)>>>(
                  nullptr, dirs, n, n_dev, ga, nullptr, (const _Float16*)mlp_f16, sigmas, rgbs, nullptr,
                  (_Float16*)h_f16, (const _Float16*)enc_pm, n, sample_idx));
    return ngp_launch_status();
}

}  // extern "C"
