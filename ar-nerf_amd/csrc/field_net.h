// The field networks as the forward kernels evaluate them (field.hip): the
// fp16 weight image in LDS, the MFMA density / colour nets on one 16-sample
// column block, SH4 and the colour-output modes.  Shared with the input
// gradient (inputgrad.hip), which recomputes the forward through these same
// functions so that its ReLU masks are the forward's own.
#pragma once
#include "common.h"

namespace ngp {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// fp16 MLP buffer offsets (halfs), matrices row-major [out][in]
constexpr int OW1 = 0, OW2 = 2048, OW3 = 3072, OW4 = 5120, OW5 = 9216;
// LDS image of the forward weights (halfs): rows padded to 40 / 72 halfs
constexpr int R32 = 40, R64 = 72;
constexpr int SW1 = 0, SW2 = SW1 + 64 * R32, SW3 = SW2 + 16 * R64, SW4 = SW3 + 64 * R32, SW5 = SW4 + 64 * R64,
              SWF = SW5 + 16 * R64;

__device__ __forceinline__ f4 mfma32(h8 a, h8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

// tcnn SphericalHarmonics degree 4 of (d/|d|+1)/2 (models/networks.py:144-145),
// returning the 4 values SH[4g..4g+3] this lane group needs.
__device__ __forceinline__ void sh4_select(float dx, float dy, float dz, int g, float out[4]) {
    const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float x = ((dx / nrm + 1) / 2) * 2.f - 1.f;
    const float y = ((dy / nrm + 1) / 2) * 2.f - 1.f;
    const float z = ((dz / nrm + 1) / 2) * 2.f - 1.f;
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    float o[16];
    o[0] = 0.28209479177387814f;
    o[1] = -0.48860251190291987f * y;
    o[2] = 0.48860251190291987f * z;
    o[3] = -0.48860251190291987f * x;
    o[4] = 1.0925484305920792f * xy;
    o[5] = -1.0925484305920792f * yz;
    o[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
    o[7] = -1.0925484305920792f * xz;
    o[8] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
    o[9] = 0.59004358992664352f * y * (-3.0f * x2 + y2);
    o[10] = 2.8906114426405538f * xy * z;
    o[11] = 0.45704579946446572f * y * (1.0f - 5.0f * z2);
    o[12] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
    o[13] = 0.45704579946446572f * x * (1.0f - 5.0f * z2);
    o[14] = 1.4453057213202769f * z * (x2 - y2);
    o[15] = 0.59004358992664352f * x * (-x2 + 3.0f * y2);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        out[r] = g == 0 ? o[r] : g == 1 ? o[4 + r] : g == 2 ? o[8 + r] : o[12 + r];
}

__device__ __forceinline__ h8 pack(h4 a, h4 b) { return h8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }
// ReLU of an fp32 accumulator tile, rounded to fp16: round first (v_cvt_pk),
// then clear every half whose sign is set (round(c) <= 0 exactly when c <= 0,
// so the result equals round(max(c, 0)) bit for bit, +0 included) -- two
// packed integer ops per pair instead of a canonicalize + max per element.
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t relu_bits(uint32_t x) {
    const uint32_t neg = __builtin_bit_cast(uint32_t, __builtin_bit_cast(s16x2, x) >> (s16x2){15, 15});
    return x & ~neg;
}
__device__ __forceinline__ h4 relu_h(f4 c) {
    const uint2 u = __builtin_bit_cast(uint2, h4{(_Float16)c[0], (_Float16)c[1], (_Float16)c[2], (_Float16)c[3]});
    uint32_t x = u.x, y = u.y;
    asm volatile("" : "+v"(x), "+v"(y));  // (opaque: one v_cvt_pk per pair, not re-derived per use)
    return __builtin_bit_cast(h4, make_uint2(relu_bits(x), relu_bits(y)));
}
__device__ __forceinline__ h4 to_h(f4 c) { return h4{(_Float16)c[0], (_Float16)c[1], (_Float16)c[2], (_Float16)c[3]}; }
__device__ __forceinline__ h8 lds8(const _Float16* p) { return *reinterpret_cast<const h8*>(p); }

// K permutations matching the register re-pack of accumulator tiles, as the
// position of weight column i in the permuted row.  P64: position 32q + 8g + j
// (step q, lane group g, element j) holds hidden unit 32q + (j<4 ? 4g+j :
// 16+4g+j-4); P32, the colour-net input [SH(16), h(16)]: position 8g + j holds
// j<4 ? SH[4g+j] : h[4g+j-4].
__device__ __forceinline__ int P64inv(int i) {
    const int q = i >> 5, r = i & 31;
    return 32 * q + (r < 16 ? 8 * (r >> 2) + (r & 3) : 8 * ((r - 16) >> 2) + 4 + (r & 3));
}
__device__ __forceinline__ int P32inv(int i) { return i < 16 ? 8 * (i >> 2) + (i & 3) : 8 * ((i - 16) >> 2) + 4 + (i & 3); }

// The forward weight image (permuted columns, padded rows) built straight from
// global memory: coalesced 16-byte loads of the row-major buffer, each half
// scattered to its permuted LDS position (8 consecutive halfs share one row);
// the image is all the LDS a forward block needs.
// the 8 halfs v of the row-major buffer at flat index i0 (a multiple of 8) into
// the forward image: their row, each column at its permuted position
__device__ __forceinline__ void place_fwd8(int i0, h8 v, _Float16* sw) {
    int row, col0;  // destination row start, and the first column
    bool p64 = false, p32 = false;
    if (i0 < OW2) { row = SW1 + (i0 >> 5) * R32; col0 = i0 & 31; }
    else if (i0 < OW3) { row = SW2 + ((i0 - OW2) >> 6) * R64; col0 = (i0 - OW2) & 63; p64 = true; }
    else if (i0 < OW4) { row = SW3 + ((i0 - OW3) >> 5) * R32; col0 = (i0 - OW3) & 31; p32 = true; }
    else if (i0 < OW5) { row = SW4 + ((i0 - OW4) >> 6) * R64; col0 = (i0 - OW4) & 63; p64 = true; }
    else { row = SW5 + ((i0 - OW5) >> 6) * R64; col0 = (i0 - OW5) & 63; p64 = true; }
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const int col = col0 + jj;
        sw[row + (p64 ? P64inv(col) : p32 ? P32inv(col) : col)] = v[jj];
    }
}

__device__ __forceinline__ void load_fwd_weights_direct(const _Float16* __restrict__ mlp, _Float16* sw, bool color) {
    const h8* src = reinterpret_cast<const h8*>(mlp);
    const int nv = (color ? NGP_MLP_PARAMS : OW3) / 8;
    for (int c = threadIdx.x; c < nv; c += blockDim.x) place_fwd8(8 * c, src[c], sw);
}

// Density net on one column block: returns h (rows 4g+r of sample s) and
// the four relu'd hidden tiles.
__device__ __forceinline__ h4 density_net(h8 e, const _Float16* sw, int s, int g, h4 h1[4]) {
    const f4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) h1[t] = relu_h(mfma32(lds8(sw + SW1 + (16 * t + s) * R32 + 8 * g), e, z));
    f4 c = z;
#pragma unroll
    for (int q = 0; q < 2; ++q) c = mfma32(lds8(sw + SW2 + s * R64 + 32 * q + 8 * g), pack(h1[2 * q], h1[2 * q + 1]), c);
    return to_h(c);
}

__device__ __forceinline__ h4 color_net(h8 cin, const _Float16* sw, int s, int g, h4 h3[4], h4 h4v[4]) {
    const f4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) h3[t] = relu_h(mfma32(lds8(sw + SW3 + (16 * t + s) * R32 + 8 * g), cin, z));
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        f4 c = z;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            c = mfma32(lds8(sw + SW4 + (16 * t + s) * R64 + 32 * q + 8 * g), pack(h3[2 * q], h3[2 * q + 1]), c);
        h4v[t] = relu_h(c);
    }
    f4 c = z;
#pragma unroll
    for (int q = 0; q < 2; ++q) c = mfma32(lds8(sw + SW5 + s * R64 + 32 * q + 8 * g), pack(h4v[2 * q], h4v[2 * q + 1]), c);
    return to_h(c);
}

__device__ __forceinline__ float sigmoid_h(_Float16 o) {
    return (float)(_Float16)(1.0f / (1.0f + expf(-(float)o)));
}

// Colour output of the rgb_net row o (networks.py:68-78, 152-157) in mode act
// (NGP_RGB_*, wave-uniform: a scalar branch): the sigmoid, the raw value
// (rgb_act='None'), F.leaky_relu on the fp16 row as torch evaluates it (fp32
// opmath, slope 0.01f, rounded to half; o == 0 takes the slope branch) for
// raw-HDR training, and relu for output_radiance.
__device__ __forceinline__ float rgb_out(_Float16 o, int act) {
    if (act == NGP_RGB_SIGMOID) return sigmoid_h(o);
    const float f = (float)o;
    if (act == NGP_RGB_NONE || f > 0.f) return f;
    return act == NGP_RGB_LEAKY_RELU ? (float)(_Float16)(f * 0.01f) : 0.f;
}

// dL/do of rgb_out from the upstream g (fp32)
__device__ __forceinline__ float rgb_out_grad(_Float16 o, float g, int act) {
    if (act == NGP_RGB_SIGMOID) {
        const float y = 1.0f / (1.0f + expf(-(float)o));
        return g * (y * (1.0f - y));
    }
    if (act == NGP_RGB_NONE || (float)o > 0.f) return g;
    return act == NGP_RGB_LEAKY_RELU ? g * 0.01f : 0.f;
}

}  // namespace ngp
