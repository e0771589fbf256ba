// The field's MLP backward: the cooperative kernel (forward recomputed through field_net.h's nets), its entry
// points, and the composed ngp_field_backward*, which reach ngp_hash_backward (hash_bwd.hip) across the unit
// boundary through its C declaration.
#pragma clang fp contract(off)

#include "common.h"
#include "field_net.h"
#include "grid.h"
#include "wave.h"

namespace ngp {

// ------------------------------------------------------------------ backward
// MLP backward helpers: v_mfma_f32_16x16x16_f16, whose B operand layout
// B[k = 4g + j][n = s] IS the accumulator layout, so every gradient tile of
// the data chain re-enters the next MFMA from registers.
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f4 mfma16(h4 a, h4 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ h4 lds4(const _Float16* p) { return *reinterpret_cast<const h4*>(p); }

constexpr int RT16 = 20, RT64 = 68;  // transposed-weight rows: 16 / 64 halfs + pad
constexpr int BT5 = SWF, BT4 = BT5 + 64 * RT16, BT3 = BT4 + 64 * RT64, BT2 = BT3 + 16 * RT64, BT1 = BT2 + 64 * RT16,
              BTE = BT1 + 32 * RT64;
// operand tiles of the weight-gradient sums: [sample][unit] 16x16 images
// (32-byte rows: the packed 8-byte stores and the ds_read_b64_tr_b16 reads
// of a 32-lane half both cover 64 distinct banks), after the weight images
constexpr int TROW = 16, TTILE = 16 * TROW;
constexpr int SCR = (BTE + 7) & ~7;

// The backward's weight images straight from global memory in one pass: the
// forward image (field_net.h: place_fwd8) at sw, and behind it, at BT5..BT1, the
// matrices transposed with padded rows (pitch RT16 / RT64):
//   W5T[i][o] = W5[o][i] (64 x 16); W4T (64 x 64); W3hT[i][o] = W3[o][16+i] (16 x 64);
//   W2T[i][o] = W2[o][i] (64 x 16); W1T[i][o] = W1[o][i] (32 x 64)
// A thread item is two rows (o, o+1) x 8 columns of one matrix, two 16-byte
// loads; the forward image takes each half at its permuted position, the
// transposed matrices a 4-byte pair {W[o][i], W[o+1][i]} per column (no staging
// buffer in LDS and no barrier between two passes: 6.4 -> ~3 us per block,
// scripts/diag/mlpbwd_phases.py).
__device__ __forceinline__ void load_bwd_weights_direct(const _Float16* __restrict__ mlp, _Float16* sw) {
    // items: W1 32 row pairs x 4 column blocks, W2 8 x 8, W3 32 x 4, W4 32 x 8, W5 8 x 8
    constexpr int N1 = 128, N2 = 64, N3 = 128, N4 = 256, N5 = 64, NI = N1 + N2 + N3 + N4 + N5;
    for (int it = threadIdx.x; it < NI; it += blockDim.x) {
        int ow, lg_cb, li, bt, rt, skip;  // matrix offset, log2(column blocks), local item, bwd image, row, skipped cols
        if (it < N1) { ow = OW1; lg_cb = 2; li = it; bt = BT1; rt = RT64; skip = 0; }
        else if (it < N1 + N2) { ow = OW2; lg_cb = 3; li = it - N1; bt = BT2; rt = RT16; skip = 0; }
        else if (it < N1 + N2 + N3) { ow = OW3; lg_cb = 2; li = it - N1 - N2; bt = BT3; rt = RT64; skip = 16; }
        else if (it < NI - N5) { ow = OW4; lg_cb = 3; li = it - N1 - N2 - N3; bt = BT4; rt = RT64; skip = 0; }
        else { ow = OW5; lg_cb = 3; li = it - (NI - N5); bt = BT5; rt = RT16; skip = 0; }
        const int in_dim = 8 << lg_cb, o = 2 * (li >> lg_cb), i0 = 8 * (li & ((1 << lg_cb) - 1));
        const int f0 = ow + o * in_dim + i0;
        const h8 a = *reinterpret_cast<const h8*>(mlp + f0);
        const h8 b = *reinterpret_cast<const h8*>(mlp + f0 + in_dim);
        place_fwd8(f0, a, sw);
        place_fwd8(f0 + in_dim, b, sw);
        if (i0 >= skip) {  // (W3: only the h columns 16..31 are transposed)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj)
                *reinterpret_cast<h2v*>(sw + bt + (i0 - skip + jj) * rt + o) = h2v{a[jj], b[jj]};
        }
    }
}

__device__ __forceinline__ float max4(f4 v) { return fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))); }
// Per-sample power-of-two scales of the data chain: a gradient tile travels in
// fp16 as value x 2^E, E per sample (the same in its four lanes).  At the
// chain's two inputs (dL/drgb through the sigmoid, dL/dh with TruncExp's dL/dsigma)
// E comes from the sample's largest |value| so that it lands in [2^13, 2^14): a
// full 11-bit mantissa for everything within 2^27 of it.  A layer's MFMA output
// is in units of the previous E; after W^T the next E is the previous one minus
// the block's bound exponent of W^T (colsum_exp: the output stays below 2^14, no
// per-sample max), and one power-of-two factor 2^(E_new - E_prev) re-scales it
// (exact).  A sample whose chain input is all zero (a row past the count, a
// sample without gradient) takes E_MAX: its tiles are zeros at any scale, and it
// must not enter the block minimum of the weight-gradient re-scale below with an
// exponent of its own -- frexpf(0)'s exponent 0 gave it the absolute E = 14,
// which in every block with such a row replaced "the block's largest gradient
// at [2^13, 2^14)" and flushed the weight gradients of small upstream gradients.
constexpr int E_MIN = -100, E_MAX = 100;
// m = f 2^e, f in [0.5, 1), m >= 0: frexpf's exponent read from the biased field, so that 0 (and the
// subnormals, which E_MAX clamps either way) gives -126: next_exp(0) = E_MAX
__device__ __forceinline__ int fexp(float m) { return (int)(__float_as_uint(m) >> 23) - 126; }
__device__ __forceinline__ int next_exp(float m_scaled, int e_prev) {
    return min(max(e_prev + 14 - fexp(m_scaled), E_MIN), E_MAX);
}
__device__ __forceinline__ h4 cvt4(f4 v, float r) {
    return h4{(_Float16)(v[0] * r), (_Float16)(v[1] * r), (_Float16)(v[2] * r), (_Float16)(v[3] * r)};
}
// ReLU' of an fp16 gradient tile by its layer's activation tile (relu_h's
// output: sign clear): keep a half where act > 0, i.e. its bits are nonzero --
// (act + 0x7fff) has bit 15 set exactly then, an arithmetic shift spreads it.
__device__ __forceinline__ uint32_t mask_h2(uint32_t gv, uint32_t av) {
    const s16x2 t = __builtin_bit_cast(s16x2, __builtin_bit_cast(u16x2, av) + (u16x2){0x7fff, 0x7fff});
    return gv & __builtin_bit_cast(uint32_t, t >> (s16x2){15, 15});
}
__device__ __forceinline__ h4 relu_mask(h4 gr, h4 act) {
    const uint2 gv = __builtin_bit_cast(uint2, gr), av = __builtin_bit_cast(uint2, act);
    return __builtin_bit_cast(h4, make_uint2(mask_h2(gv.x, av.x), mask_h2(gv.y, av.y)));
}
// 2^k (k <= 0) as a pair of fp16 (subnormal down to 2^-24, 0 below)
__device__ __forceinline__ uint32_t f16_pow2_x2(int k) {
    const uint32_t b = k >= -14 ? (uint32_t)(k + 15) << 10 : k >= -24 ? 1u << (k + 24) : 0u;
    return b | (b << 16);
}
// an fp16 tile times a per-lane fp16 factor pair (v_pk_mul_f16; exact for powers of two)
typedef _Float16 hx2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h4 mul_h4(h4 v, uint32_t f2) {
    const uint2 u = __builtin_bit_cast(uint2, v);
    const hx2 f = __builtin_bit_cast(hx2, f2);
    return __builtin_bit_cast(h4, make_uint2(__builtin_bit_cast(uint32_t, __builtin_bit_cast(hx2, u.x) * f),
                                             __builtin_bit_cast(uint32_t, __builtin_bit_cast(hx2, u.y) * f)));
}
// v x 2^k (k <= 0) rounded once to fp16: one v_pk_mul_f16 by the fp16 factor
// while 2^k is representable (k >= -24, subnormal factors included); below,
// where the factor is not but the product may be (an fp16 subnormal or even
// normal value), through fp32 -- the same single rounding
__device__ __forceinline__ h4 scale_h4(h4 v, int k) {
    if (k >= -24) return mul_h4(v, f16_pow2_x2(k));
    const float f = ldexpf(1.0f, k);
    return h4{(_Float16)((float)v[0] * f), (_Float16)((float)v[1] * f), (_Float16)((float)v[2] * f),
              (_Float16)((float)v[3] * f)};
}
// min over the wave's 16 samples of a per-sample int (lanes 0-15 hold samples 0-15)
__device__ __forceinline__ int samples_min(int v) {
#define NGP_DPP_ROR_I(x, n) __builtin_amdgcn_update_dpp(0, (x), 0x120 + (n), 0xf, 0xf, false)
    v = min(v, NGP_DPP_ROR_I(v, 1));
    v = min(v, NGP_DPP_ROR_I(v, 2));
    v = min(v, NGP_DPP_ROR_I(v, 4));
    v = min(v, NGP_DPP_ROR_I(v, 8));
#undef NGP_DPP_ROR_I
    return __builtin_amdgcn_readfirstlane(v);
}
// Accumulator tile X[4g + r][s] (lane (s, g)) -> image row s, units 4g..4g+3.
// The four 8-byte chunks of row s sit XOR-swizzled, chunk c at c ^ ((s >> 2) & 3):
// a ds_write_b64 group (16 lanes, banks mod 32) then covers 32 distinct banks
// (unswizzled, rows 8 dwords apart hit 4 banks 4 ways), and get_tile's reads
// stay conflict-free.
__device__ __forceinline__ void put_tile(_Float16* T, h4 v, int s, int g) {
    *reinterpret_cast<h4*>(T + s * TROW + 4 * (g ^ ((s >> 2) & 3))) = v;
}
// units 8h..8h+7 of row s (chunks 2h, 2h+1; e0 = units 8h..8h+3) under the same swizzle
__device__ __forceinline__ void put_tile_pair(_Float16* T, h4 e0, h4 e1, int s, int h) {
    const int sw = (s >> 2) & 3;
    *reinterpret_cast<h8*>(T + s * TROW + 4 * ((2 * h) ^ (sw & 2))) = (sw & 1) ? pack(e1, e0) : pack(e0, e1);
}
// Transposed read: lane (u = s, g) receives X[u][4g + q], q = 0..3, i.e. the
// K = sample fragment of the 16x16x16 operand.  Lane 4q+p of each 16-lane
// group addresses image row 4g+q, units 4p..4p+3 (= T + 4*lane).
typedef __fp16 hp4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ h4 get_tile(const _Float16* T, int s, int g) {
    // row 4g + (s >> 2), chunk s & 3 -> stored at chunk (s & 3) ^ g (put_tile's swizzle)
    const _Float16* a = T + 64 * g + 4 * ((s & 12) | ((s & 3) ^ g));
    return __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                                      (__attribute__((address_space(3))) hp4*)(const_cast<_Float16*>(a))));
}
// accumulator tile k -> (matrix offset, in_dim, o0, i0)
__device__ __forceinline__ void acc_tile_info(int k, int& ow, int& in_dim, int& o0, int& i0) {
    if (k < 4) { ow = OW5; in_dim = 64; o0 = 0; i0 = 16 * k; return; }
    k -= 4;
    if (k < 16) { ow = OW4; in_dim = 64; o0 = 16 * (k >> 2); i0 = 16 * (k & 3); return; }
    k -= 16;
    if (k < 8) { ow = OW3; in_dim = 32; o0 = 16 * (k >> 1); i0 = 16 * (k & 1); return; }
    k -= 8;
    if (k < 4) { ow = OW2; in_dim = 64; o0 = 0; i0 = 16 * k; return; }
    k -= 4;
    ow = OW1; in_dim = 32; o0 = 16 * (k >> 1); i0 = 16 * (k & 1);
}

// Kernel A: the MLP backward, block-cooperative.  Eight waves per block (two
// per SIMD -- a per-wave kernel holding all 40 weight-gradient tiles in
// registers ran one wave per SIMD, latency-bound on its dependent MFMA / LDS
// chain: 105.8 vs 78.8 us, profiles/r02/mlp_split_coop.json).  Each wave
// back-propagates its own 16-sample column block (forward recomputed from the
// saved fp16 encoding); the weight gradients are then summed by
// the block: every wave puts its operand tiles into its LDS region and wave w
// accumulates output tiles {k} over all eight regions (K = 128 samples per
// block iteration), 5 of the 40 tiles per wave.  Operands go through LDS in
// two phases (layers 5-3: 19 tiles, then layers 2-1: 11 tiles) so eight
// regions fit beside the weight images.  Gradient operands of the data
// chain are fp16 scaled per SAMPLE (column of the B operand; the four lanes
// of a sample exchange their maxima with v_permlane16/32_swap) by a power of
// two, unscaled exactly in fp32 for dL/denc; the weight gradients take the
// same fp16 values re-scaled to one power of two per layer and block
// (tcnn's fp16 operands with the role of its loss scale, no global scale to
// tune).
// (diagnostics only: scripts/diag/mlpbwd_phases.hip defines these to stamp the
// phases of a block iteration and the kernel's edges; empty in the product build)
#ifndef NGP_BWD_PHASE
#define NGP_BWD_PHASE(k)
#define NGP_BWD_EDGE(k)
#endif
// CW waves per block (CW / 4 per SIMD; 12 fit the LDS at <= 168 VGPRs but measured -3 %, DESIGN.md
// section 9 round 4)
constexpr int CW = 8, NT1 = 19, NT2 = 11, CSCRW = NT1 * TTILE;
constexpr int COOP_LDS_HALFS = SCR + CW * CSCRW;
static_assert(CW % 4 == 0, "waves per block: a multiple of 4");
static_assert(NT2 <= NT1, "phase-2 tiles exceed the scratch");
static_assert(COOP_LDS_HALFS * 2 <= 160 * 1024, "cooperative MLP backward exceeds the LDS");
// output tiles per phase (phase 1: layers 5, 4, 3 = 4 + 16 + 8; phase 2: layers 2, 1 = 4 + 8), dealt
// to the CW waves in contiguous runs (tiles sharing a G operand stay together), at most KT1 / KT2 each
constexpr int NK1 = 28, NK2 = 12, KT1 = (NK1 + CW - 1) / CW, KT2 = (NK2 + CW - 1) / CW;
// phase-1 / phase-2 tile ids inside a wave's region
constexpr int P_DO = 0, P_DA4 = 1, P_DA3 = 5, P_H4 = 9, P_H3 = 13, P_C = 17;
constexpr int Q_DH = 0, Q_DA1 = 1, Q_H1 = 5, Q_E = 9;

// max over the four lanes of one sample (lanes s, s+16, s+32, s+48)
__device__ __forceinline__ float sample_max(float v) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    const auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(q[0]), __uint_as_float(q[1]));
}

// ceil(log2(max_i sum_o |W^T[i][o]|)) of a transposed weight image (rows of nout halfs,
// pitch rt, nin rows; one row per lane, max over the wave): |W^T x| < 2^k max|x| for
// every x, so a gradient tile scaled below 2^14 stays below 2^14 after W^T and a
// re-scale by 2^-k (the inner layers' exponents without per-sample maxima: only the
// chain's two inputs, dL/drgb and dL/dsigma, set a per-sample exponent).  Whole wave,
// uniform result.
__device__ __forceinline__ int colsum_exp(const _Float16* img, int nin, int nout, int rt, int lane) {
    float a = 0.f;
    if (lane < nin)
        for (int o = 0; o < nout; o += 4) {  // (8-byte row reads; the same sequential sum)
            const h4 v = *reinterpret_cast<const h4*>(img + lane * rt + o);
            a += fabsf((float)v[0]);
            a += fabsf((float)v[1]);
            a += fabsf((float)v[2]);
            a += fabsf((float)v[3]);
        }
    a = wave_max(a);
    int e = 0;
    const float m = frexpf(a, &e);
    e = a == 0.f ? -30 : (m == 0.5f ? e - 1 : e);  // ceil(log2(a)) (a = 2^(e-1) exactly: e - 1)
    return __builtin_amdgcn_readfirstlane(e);
}

// output tile k (acc_tile_info order) -> operand tile ids (G, H) in its phase's region
__device__ __forceinline__ void coop_tile_ops(int k, int& gid, int& hid) {
    if (k < 4) { gid = P_DO; hid = P_H4 + k; return; }
    if (k < 20) { gid = P_DA4 + ((k - 4) >> 2); hid = P_H3 + ((k - 4) & 3); return; }
    if (k < 28) { gid = P_DA3 + ((k - 20) >> 1); hid = P_C + ((k - 20) & 1); return; }
    if (k < 32) { gid = Q_DH; hid = Q_H1 + (k - 28); return; }
    gid = Q_DA1 + ((k - 32) >> 1);
    hid = Q_E + ((k - 32) & 1);
}

// wave w owns tiles [start, start + n) of a phase of NK tiles: the first NK % CW waves one more
template <int NK>
__device__ __forceinline__ int coop_start(int w) { return w * (NK / CW) + min(w, NK % CW); }
template <int NK>
__device__ __forceinline__ int coop_count(int w) { return NK / CW + (w < NK % CW ? 1 : 0); }
__device__ __forceinline__ int coop_k1(int w, int t) { return coop_start<NK1>(w) + t; }
__device__ __forceinline__ int coop_n1(int w) { return coop_count<NK1>(w); }
__device__ __forceinline__ int coop_k2(int w, int t) { return NK1 + coop_start<NK2>(w) + t; }
__device__ __forceinline__ int coop_n2(int w) { return coop_count<NK2>(w); }

// layer of output tile k: 0 = W5 (G = dL/dout), 1 = W4 (dL/da4), 2 = W3 (dL/da3),
// 3 = W2 (dL/dh), 4 = W1 (dL/da1)
__device__ __forceinline__ int tile_layer(int k) { return k < 4 ? 0 : k < 20 ? 1 : k < 28 ? 2 : k < 32 ? 3 : 4; }

// v_mfma_f32_16x16x32_f16 over two source regions at a time: the K order
// (lane group g, element j) <- sample 4g + (j & 3) of region src + (j >> 2) is
// the same for the A and the B operand, so the sum over K is the sum over the
// 32 samples.  The G tiles of one layer carry the block's common scale 2^B, so
// each tile's block sum is added to its accumulator times 2^-B (Bl[layer]).
template <int NTL>
__device__ __forceinline__ void coop_dw(const _Float16* scr, int w, int s, int g, int n, int (*kf)(int, int), f4* acc,
                                        const int* Bl) {
    int gid[NTL], hid[NTL];
    float sc[NTL];
    f4 part[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
        const int k = kf(w, t < n ? t : 0);
        coop_tile_ops(k, gid[t], hid[t]);
        const int l = tile_layer(k);  // (wave-uniform: the select stays scalar)
        sc[t] = ldexpf(1.0f, -(l == 0 ? Bl[0] : l == 1 ? Bl[1] : l == 2 ? Bl[2] : l == 3 ? Bl[3] : Bl[4]));
    }
#pragma unroll
    for (int src = 0; src < CW; src += 2) {
        const _Float16* R0 = scr + src * CSCRW;
        const _Float16* R1 = R0 + CSCRW;
        h4 G0 = get_tile(R0 + gid[0] * TTILE, s, g), G1 = get_tile(R1 + gid[0] * TTILE, s, g);
#pragma unroll
        for (int t = 0; t < NTL; ++t) {
            if (t >= n) break;
            if (t > 0 && gid[t] != gid[t - 1]) {
                G0 = get_tile(R0 + gid[t] * TTILE, s, g);
                G1 = get_tile(R1 + gid[t] * TTILE, s, g);
            }
            const h8 H = pack(get_tile(R0 + hid[t] * TTILE, s, g), get_tile(R1 + hid[t] * TTILE, s, g));
            part[t] = mfma32(pack(G0, G1), H, src == 0 ? f4{0.f, 0.f, 0.f, 0.f} : part[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < NTL; ++t)
        if (t < n) acc[t] = part[t] * sc[t] + acc[t];
}

__global__ void __launch_bounds__(64 * CW, CW / 4) field_bwd_mlp_coop_kernel(
    const float* __restrict__ dirs, int64_t n, const int64_t* __restrict__ n_dev, const int32_t* __restrict__ sidx,
    const _Float16* __restrict__ enc, const _Float16* __restrict__ mlp, const float* __restrict__ dL_dsig,
    const float* __restrict__ dL_drgb, float* __restrict__ denc, float* __restrict__ grad_mlp, int64_t enc_pm_stride,
    int act) {
    extern __shared__ __attribute__((aligned(16))) _Float16 smem[];
    // per-wave minima of the layers' per-sample exponents (double-buffered by iteration parity)
    __shared__ __attribute__((aligned(16))) int emin[2][5][CW];
    _Float16* sw = smem;
    _Float16* scr = smem + SCR;
    NGP_BWD_EDGE(0);
    NGP_PROBE_BEGIN(NGP_P_MLP_BWD);
    const int64_t N = ngp_capped_count(n_dev, n);  // (a device count never past the capacity: a guard hit)
    const int lane = threadIdx.x & 63, s = lane & 15, g = lane >> 4;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    _Float16* mine = scr + wid * CSCRW;
    const f4 z = {0.f, 0.f, 0.f, 0.f};
    f4 acc1[KT1], acc2[KT2];
#pragma unroll
    for (int t = 0; t < KT1; ++t) acc1[t] = z;
#pragma unroll
    for (int t = 0; t < KT2; ++t) acc2[t] = z;
    struct In {
        h8 e;
        float dx, dy, dz, dsig, gr[3];
    };
    // the sample of row jj (-1 past the end): listed rows' indices are loaded
    // two iterations ahead, so the dependent loads of the next iteration's
    // inputs never wait on an index load
    auto row_index = [&](int64_t jj) -> int32_t {
        return jj < N ? (sidx ? sidx[jj] : (int32_t)jj) : -1;
    };
    auto load_in = [&](int32_t ii, In& x) {
        x.e = h8{0, 0, 0, 0, 0, 0, 0, 0};
        x.dx = 0.f; x.dy = 0.f; x.dz = 1.f; x.dsig = 0.f; x.gr[0] = x.gr[1] = x.gr[2] = 0.f;
        if (ii >= 0) {
            if (enc_pm_stride > 0)  // pair-major (ngp_hash_encode): pairs 2g, 2g+1
                x.e = pack(*reinterpret_cast<const h4*>(enc + ((2 * g) * enc_pm_stride + ii) * 4),
                           *reinterpret_cast<const h4*>(enc + ((2 * g + 1) * enc_pm_stride + ii) * 4));
            else
                x.e = *reinterpret_cast<const h8*>(enc + (int64_t)ii * 32 + 8 * g);
            x.dx = dirs[3 * (int64_t)ii]; x.dy = dirs[3 * (int64_t)ii + 1]; x.dz = dirs[3 * (int64_t)ii + 2];
            x.dsig = dL_dsig[ii];
            x.gr[0] = dL_drgb[3 * (int64_t)ii]; x.gr[1] = dL_drgb[3 * (int64_t)ii + 1];
            x.gr[2] = dL_drgb[3 * (int64_t)ii + 2];
        }
    };
    const int64_t stride = (int64_t)gridDim.x * CW * 16;
    const int64_t j0 = (int64_t)blockIdx.x * CW * 16 + 16 * wid + s;
    // the first iteration's inputs (count -> index -> rows: three dependent
    // round trips) are requested before the weight images are staged, so the
    // two overlap
    In cur;
    load_in(row_index(j0), cur);
    int32_t i_next = row_index(j0 + stride);
    load_bwd_weights_direct(mlp, sw);
    __syncthreads();
    // per-block bounds of W5^T, W4^T, W2^T: the inner layers' exponents follow from their input's
    // (round 5; rounds 3-4 took a per-sample max after every layer: 12 % more VALU, 6 % longer);
    // one wave per matrix (round 6: every wave computed all three, ~1.3 M VALU per launch)
    __shared__ int kex[3];
    if (wid < 3) {
        const int e = wid == 0 ? colsum_exp(sw + BT5, 64, 16, RT16, lane)
                    : wid == 1 ? colsum_exp(sw + BT4, 64, 64, RT64, lane) : colsum_exp(sw + BT2, 64, 16, RT16, lane);
        if (lane == 0) kex[wid] = e;
    }
    __syncthreads();
    const int k5 = __builtin_amdgcn_readfirstlane(kex[0]), k4 = __builtin_amdgcn_readfirstlane(kex[1]);
    const int k2 = __builtin_amdgcn_readfirstlane(kex[2]);
    NGP_BWD_EDGE(1);
    int par = 0;
    // block-uniform trip count: every wave reaches every barrier
    for (int64_t bb = (int64_t)blockIdx.x * CW * 16; bb < N; bb += stride, par ^= 1) {
        const int64_t base = bb + 16 * wid;
        In nxt;
        load_in(i_next, nxt);
        i_next = row_index(base + s + 2 * stride);
        NGP_BWD_PHASE(0);
        // the lane's (sample, group) re-derived opaquely per iteration: the LDS / global
        // addresses built from them are recomputed here instead of held (or spilled) across the
        // loop as loop-invariant registers
        int lane_l = lane;
        asm volatile("" : "+v"(lane_l));
        const int s = lane_l & 15, g = lane_l >> 4;
        const int64_t j = base + s;
        const bool valid = j < N;
        const h8 e = cur.e;

        // ---- forward recompute
        h4 h1[4];
        const h4 hh = density_net(e, sw, s, g, h1);
        float sh[4];
        sh4_select(cur.dx, cur.dy, cur.dz, g, sh);
        const h4 shh = {(_Float16)sh[0], (_Float16)sh[1], (_Float16)sh[2], (_Float16)sh[3]};
        h4 h3[4], h4v[4];
        const h4 o = color_net(pack(shh, hh), sw, s, g, h3, h4v);
        NGP_BWD_PHASE(1);
        // ---- output layer: the colour activation's backward on rows 0..2
        f4 dout = z;
        if (g == 0) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                dout[r] = rgb_out_grad(o[r], cur.gr[r], act);
            }
        }
        const int Eo = next_exp(sample_max(max4(dout)), 0);
        const h4 do_h = cvt4(dout, ldexpf(1.0f, Eo));
        // ---- dL/da4 = ReLU'(W5^T do)   (MFMA output in units of 2^Eo; |.| < 2^(14 + k5))
        f4 c4[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) c4[t] = mfma16(lds4(sw + BT5 + (16 * t + s) * RT16 + 4 * g), do_h, z);
        const int E4 = max(Eo - k5, E_MIN);
        h4 da4h[4];
        {
            const float r = ldexpf(1.0f, E4 - Eo);
#pragma unroll
            for (int t = 0; t < 4; ++t) da4h[t] = relu_mask(cvt4(c4[t], r), h4v[t]);
        }
        // ---- dL/da3 = ReLU'(W4^T da4)
        f4 c3[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f4 c = z;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) c = mfma16(lds4(sw + BT4 + (16 * t + s) * RT64 + 16 * kt + 4 * g), da4h[kt], c);
            c3[t] = c;
        }
        const int E3 = max(E4 - k4, E_MIN);
        h4 da3h[4];
        {
            const float r = ldexpf(1.0f, E3 - E4);
#pragma unroll
            for (int t = 0; t < 4; ++t) da3h[t] = relu_mask(cvt4(c3[t], r), h3[t]);
        }
        // ---- dL/dh (colour-net input, h part) = W3h^T da3, + TruncExp backward (true units)
        f4 dh = z;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) dh = mfma16(lds4(sw + BT3 + s * RT64 + 16 * kt + 4 * g), da3h[kt], dh);
        dh = dh * ldexpf(1.0f, -E3);
        if (g == 0) dh[0] += cur.dsig * expf(fminf(fmaxf((float)hh[0], -15.f), 15.f));  // custom_functions.py:169-173
        const int Eh = next_exp(sample_max(max4(dh)), 0);
        const h4 dhh = cvt4(dh, ldexpf(1.0f, Eh));
        // ---- dL/da1 = ReLU'(W2^T dh)
        f4 c1[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) c1[t] = mfma16(lds4(sw + BT2 + (16 * t + s) * RT16 + 4 * g), dhh, z);
        const int E1 = max(Eh - k2, E_MIN);
        h4 da1h[4];
        {
            const float r = ldexpf(1.0f, E1 - Eh);
#pragma unroll
            for (int t = 0; t < 4; ++t) da1h[t] = relu_mask(cvt4(c1[t], r), h1[t]);
        }
        // ---- dL/denc = W1^T da1 (rows 16t + 4g + r of sample s), true units
        {
            const float r = ldexpf(1.0f, -E1);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f4 c = z;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) c = mfma16(lds4(sw + BT1 + (16 * t + s) * RT64 + 16 * kt + 4 * g), da1h[kt], c);
                c = c * r;
                if (valid) *reinterpret_cast<f4*>(denc + j * 32 + 16 * t + 4 * g) = c;
            }
        }
        NGP_BWD_PHASE(2);
        cur = nxt;
        // ---- weight gradients: fp16 operands (tcnn's precision), K = samples.  The G
        // (gradient) tiles of a layer are re-scaled from their per-sample exponent E_s
        // to the block's common one B = min_s E_s (the block's largest gradient at
        // [2^13, 2^14); factors <= 1, exact down to fp16 subnormals), the H tiles are
        // the fp16 activations / encoding as they are.  (All-zero samples sit at E_MAX
        // and below: never under a sample that carries gradient; a block of none adds zeros.)
        const int Es[5] = {Eo, E4, E3, Eh, E1};
        int wmin[5];
#pragma unroll
        for (int l = 0; l < 5; ++l) wmin[l] = samples_min(Es[l]);  // (uniform: the DPP reads every lane of the row)
        if (lane == 0) {
#pragma unroll
            for (int l = 0; l < 5; ++l) emin[par][l][wid] = wmin[l];
        }
        __syncthreads();  // every wave's phase-2 reads of the previous iteration are done; emin[par] complete
        NGP_BWD_PHASE(3);
        int fk[5];  // per-sample re-scale exponents B - E_s (<= 0)
        int Bl[5];
#pragma unroll
        for (int l = 0; l < 5; ++l) {
            int mn = 1 << 30;
#pragma unroll
            for (int q = 0; q < CW; q += 4) {
                const int4 a = *reinterpret_cast<const int4*>(&emin[par][l][q]);
                mn = min(mn, min(min(a.x, a.y), min(a.z, a.w)));
            }
            Bl[l] = __builtin_amdgcn_readfirstlane(mn);
            fk[l] = Bl[l] - Es[l];
        }
        // phase 1 (layers 5, 4, 3)
        put_tile(mine + P_DO * TTILE, scale_h4(do_h, fk[0]), s, g);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            put_tile(mine + (P_DA4 + t) * TTILE, scale_h4(da4h[t], fk[1]), s, g);
            put_tile(mine + (P_DA3 + t) * TTILE, scale_h4(da3h[t], fk[2]), s, g);
            put_tile(mine + (P_H4 + t) * TTILE, h4v[t], s, g);
            put_tile(mine + (P_H3 + t) * TTILE, h3[t], s, g);
        }
        put_tile(mine + P_C * TTILE, shh, s, g);
        put_tile(mine + (P_C + 1) * TTILE, hh, s, g);
        __syncthreads();
        NGP_BWD_PHASE(4);
        coop_dw<KT1>(scr, wid, s, g, coop_n1(wid), coop_k1, acc1, Bl);
        __syncthreads();  // phase-1 reads done: the regions take the phase-2 tiles
        NGP_BWD_PHASE(5);
        // ---- phase 2 (layers 2, 1)
        put_tile(mine + Q_DH * TTILE, scale_h4(dhh, fk[3]), s, g);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            put_tile(mine + (Q_DA1 + t) * TTILE, scale_h4(da1h[t], fk[4]), s, g);
            put_tile(mine + (Q_H1 + t) * TTILE, h1[t], s, g);
        }
        // enc fragment: lane holds enc[8g + j] of sample s -> tile g>>1, units 8(g&1)+j
        put_tile_pair(mine + (Q_E + (g >> 1)) * TTILE, h4{e[0], e[1], e[2], e[3]}, h4{e[4], e[5], e[6], e[7]}, s, g & 1);
        __syncthreads();
        NGP_BWD_PHASE(6);
        coop_dw<KT2>(scr, wid, s, g, coop_n2(wid), coop_k2, acc2, Bl);
        NGP_BWD_PHASE(7);
    }
    // each output tile lives in exactly one wave of the block: one global add
    // per weight.  Wave w of every block owns the same tiles, so the adds of a
    // lane start at a block-dependent rotation (same-address adds serialise at
    // the memory-side atomic unit: 12 -> 7 us per launch; per-block partial
    // rows + a reduction launch measured slower).
    NGP_BWD_EDGE(2);
    const int n1 = coop_n1(wid), n2 = coop_n2(wid), nadd = 4 * (n1 + n2);
    const int rot = (int)(blockIdx.x % (unsigned)nadd);
    // (q = 4 t + r over the wave's tiles in order, taken from q = rot on: two passes over a fully
    // unrolled tile loop, so each add's accumulator element and weight offset are static -- the
    // dynamically indexed version spent ~1000 VALU per wave selecting them)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int t = 0; t < KT1 + KT2; ++t) {
            const bool p1 = t < KT1;
            const int tt = p1 ? t : t - KT1;
            if (p1 ? tt >= n1 : tt >= n2) continue;
            const int tflat = p1 ? tt : n1 + tt;
            const f4 a = p1 ? acc1[p1 ? tt : 0] : acc2[p1 ? 0 : tt];
            const int k = p1 ? coop_k1(wid, tt) : coop_k2(wid, tt);
            int ow, in_dim, o0, i0;
            acc_tile_info(k, ow, in_dim, o0, i0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = 4 * tflat + r;
                if ((pass == 0) != (q >= rot)) continue;
                atomicAdd(&grad_mlp[ow + (o0 + 4 * g + r) * in_dim + i0 + s], a[r]);
            }
        }
    }
    NGP_BWD_EDGE(3);
    NGP_PROBE_END();
}

static int launch_bwd_mlp(const float* dirs, int64_t n, const int64_t* n_dev, const int32_t* sample_idx,
                          const void* enc_f16, int64_t enc_pm_stride, const void* mlp_f16, const float* dL_dsigmas,
                          const float* dL_drgbs, float* denc_ws, float* grad_mlp, int act, void* stream) {
    static bool attr_set = false;
    const size_t clds = (size_t)COOP_LDS_HALFS * sizeof(_Float16);
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)field_bwd_mlp_coop_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)clds) != hipSuccess)
            return NGP_ERANGE;
        attr_set = true;
    }
    hipStream_t s = as_stream(stream);
    static const unsigned ccap = resident_blocks(field_bwd_mlp_coop_kernel, 64 * CW, clds);
    const unsigned cb = persistent_blocks(n, CW * 16, ccap);
    NGP_TIMED(NGP_K_MLP_BWD, s, field_bwd_mlp_coop_kernel<<<cb, 64 * CW, clds, s>>>(
        dirs, n, n_dev, sample_idx, (const _Float16*)enc_f16, (const _Float16*)mlp_f16, dL_dsigmas, dL_drgbs, denc_ws,
        grad_mlp, enc_pm_stride, act));
    return ngp_launch_status();
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_field_backward_mlp(const float* dirs, int64_t n, const int64_t* n_dev, const int32_t* sample_idx,
                           const void* enc_f16, int64_t enc_pm_stride, const void* mlp_f16, const float* dL_dsigmas,
                           const float* dL_drgbs, float* denc_ws, float* grad_mlp, void* stream) {
    return ngp_field_backward_mlp_act(dirs, n, n_dev, sample_idx, enc_f16, enc_pm_stride, mlp_f16, dL_dsigmas,
                                      dL_drgbs, denc_ws, grad_mlp, NGP_RGB_SIGMOID, stream);
}

int ngp_field_backward_mlp_act(const float* dirs, int64_t n, const int64_t* n_dev, const int32_t* sample_idx,
                               const void* enc_f16, int64_t enc_pm_stride, const void* mlp_f16,
                               const float* dL_dsigmas, const float* dL_drgbs, float* denc_ws, float* grad_mlp,
                               int rgb_act, void* stream) {
    NGP_CHECK_RGB_ACT(rgb_act);
    NGP_CHECK_ARG(n >= 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(dirs && enc_f16 && mlp_f16 && dL_dsigmas && dL_drgbs && denc_ws && grad_mlp);
    NGP_CHECK_ARG(((uintptr_t)mlp_f16 & 15) == 0);
    return launch_bwd_mlp(dirs, n, n_dev, sample_idx, enc_f16, enc_pm_stride, mlp_f16, dL_dsigmas, dL_drgbs,
                          denc_ws, grad_mlp, rgb_act, stream);
}

int ngp_field_backward(const float* xyzs, const float* dirs, int64_t n, const int64_t* n_dev,
                       const ngp_hashgrid_t* grid, const void* enc_f16, const void* mlp_f16,
                       const float* dL_dsigmas, const float* dL_drgbs, float* denc_ws, float* grad_mlp,
                       float* grad_table, void* stream) {
    return ngp_field_backward_act(xyzs, dirs, n, n_dev, grid, enc_f16, mlp_f16, dL_dsigmas, dL_drgbs, denc_ws,
                                  grad_mlp, grad_table, NGP_RGB_SIGMOID, stream);
}

int ngp_field_backward_act(const float* xyzs, const float* dirs, int64_t n, const int64_t* n_dev,
                           const ngp_hashgrid_t* grid, const void* enc_f16, const void* mlp_f16,
                           const float* dL_dsigmas, const float* dL_drgbs, float* denc_ws, float* grad_mlp,
                           float* grad_table, int rgb_act, void* stream) {
    NGP_CHECK_RGB_ACT(rgb_act);
    GridArgs ga;
    int st = grid_args(grid, ga);
    if (st) return st;
    st = ngp_field_backward_mlp_act(dirs, n, n_dev, nullptr, enc_f16, 0, mlp_f16, dL_dsigmas, dL_drgbs, denc_ws,
                                    grad_mlp, rgb_act, stream);
    if (st) return st;
    return ngp_hash_backward(xyzs, n, n_dev, nullptr, grid, denc_ws, grad_table, stream);
}

}  // extern "C"
