// SSDF soft shadows for insertion frames on gfx950: the two calls every SG-lit
// frame of the reference app makes into insert/sg_shadow.py -- the self-shadow
// decay of each light's amplitude per object pixel
// (SGShadow.calc_self_shadow_light_dacay, main.py:558-567) and the cast-shadow
// factor over the surface points of the whole screen
// (SGShadow.calc_shadow_factor, main.py:492-519) with its 3 x 3 blur and
// multiply -- without the (points, C) PCA tensor and the (points, L)
// temporaries of the torch formulation.
//
//   ssdf_lights_kernel   per light: the C components and the mean sampled at the
//                        light's direction, the table row coordinate, fh_n, the
//                        amplitude; and inte_L.  One block.
//   ssdf_block           the hot path, one block per SS_PTS = 64 points: a wave
//                        gathers a point's 8 corners x C coefficients (a corner's
//                        C values are contiguous: one coalesced read per 64) and
//                        leaves the trilinear PCA vector in LDS; per tile of
//                        NGP_SSDF_LIGHT_TILE lights the sampled components are
//                        staged beside it and each thread forms a 4 x 2 block of
//                        the (points x C) x (C x lights) product, c ascending;
//                        the table lookup, the decay and, through LDS, the
//                        light sum of the factor (lights ascending, one owner
//                        thread per point) follow from registers.
//   ssdf_points_kernel / ssdf_frame_decay_kernel   front ends of ssdf_block over
//                        a point list / the covered pixels of a frame.
//   shadow_apply_kernel  out = frame_rgb * blur3x3(factor), reflect padding.
//
// Every value is a function of its own point and the lights alone: no atomics,
// fixed summation orders, nothing depends on the launch shape.
#pragma clang fp contract(off)
#include "bilinear.h"
#include "insert.h"
#include "march.h"

namespace ngp {

constexpr int SS_PTS = 64;                      // points per block
constexpr int SS_TILE = NGP_SSDF_LIGHT_TILE;    // lights per tile
constexpr int SS_MAXC = NGP_SSDF_MAX_COMPONENTS;
constexpr int SS_LW = NGP_SSDF_LIGHT_WORDS;     // workspace floats per light
constexpr int LW_MEAN = SS_MAXC, LW_ROW = SS_MAXC + 1, LW_FHN = SS_MAXC + 2, LW_AMP = SS_MAXC + 3, LW_POS = SS_MAXC + 6;
static_assert(SS_MAXC == 128 && LW_POS + 2 == SS_LW, "the pre-pass maps a thread to a component with a mask");
// LDS: the PCA vectors c-major (a thread's 4 points are one 16-byte read; 68 keeps that read aligned and spreads
// the gather's per-c writes over banks), the staged components c-major (a thread's 2 lights are one 8-byte read,
// the 16 light pairs of a wave a contiguous 128 bytes).  The point records (before the first tile) and the fh
// values (after a tile's product) live in the components' space.
constexpr int SS_A_STRIDE = SS_PTS + 4, SS_B_STRIDE = SS_TILE + 4, SS_FH_STRIDE = SS_TILE + 1;
constexpr int SS_A_FLOATS = SS_MAXC * SS_A_STRIDE, SS_B_FLOATS = SS_MAXC * SS_B_STRIDE;
static_assert(SS_PTS * SS_FH_STRIDE <= SS_B_FLOATS && SS_PTS * 5 <= SS_B_FLOATS, "aliases fit the components' space");
static_assert(SS_TILE == 32 && SS_PTS == 64, "the 4 x 2 thread blocks below cover 64 points x 32 lights");

constexpr float SS_PI = 3.14159265358979323846f;
constexpr float SS_HALF_PI = 1.57079632679489661923f;

// light_axis_to_cood, the table row of calc_inte_L_V, fh_n and calc_inte_L (sg_shadow.py:34-73, 143-144)
__global__ void __launch_bounds__(256) ssdf_lights_kernel(const float* __restrict__ lSGs, int L,
                                                          const float* __restrict__ rot,
                                                          const float* __restrict__ components,
                                                          const float* __restrict__ mean, int C, int envH, int envW,
                                                          float* __restrict__ ws) {
    // once per light: its sample position (kept in the light's two spare words), row coordinate, fh_n, amplitude
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        const float* s = lSGs + 7 * (int64_t)l;
        float* o = ws + (int64_t)l * SS_LW;
        float a[3] = {s[0], s[1], s[2]};
        if (rot) {
            const float b0 = a[0], b1 = a[1], b2 = a[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) a[i] = rot[3 * i] * b0 + rot[3 * i + 1] * b1 + rot[3 * i + 2] * b2;
        }
        const float phi = acosf(a[1]), theta = atan2f(a[2], a[0]);
        o[LW_POS] = theta / SS_PI;
        o[LW_POS + 1] = phi / SS_PI * 2.f - 1.f;  // (reaches 3: the border clamp holds it)
        const float lam = s[3];
        o[LW_ROW] = (log10f(fabsf(lam + 1e-6f)) - 1.5f) / 2.5f;
        o[LW_FHN] = 2.f * SS_PI / lam * (1.f - expf(-1.f * lam));
        o[LW_AMP] = s[4]; o[LW_AMP + 1] = s[5]; o[LW_AMP + 2] = s[6];
    }
    __syncthreads();  // (one block: its own global writes are visible to it after the barrier)
    // thread = component (128 = the mean), two lights a pass: no division
    const int c = threadIdx.x & (SS_MAXC - 1);
    for (int l = threadIdx.x >> 7; l < L; l += blockDim.x >> 7) {
        float* o = ws + (int64_t)l * SS_LW;
        const float x = o[LW_POS], y = o[LW_POS + 1];
        o[c] = c < C ? bilinear_border(components + (int64_t)c * envH * envW, envH, envW, x, y) : 0.f;
        if (c == 0) o[LW_MEAN] = bilinear_border(mean, envH, envW, x, y);
    }
    if (threadIdx.x < 3) {  // calc_inte_L: lights ascending, in the reference's order of operations
        float acc = 0.f;
        for (int l = 0; l < L; ++l) {
            const float* s = lSGs + 7 * (int64_t)l;
            acc += 2.f * SS_PI * (s[4 + threadIdx.x] / s[3]) * (1.f - expf(-1.f * s[3]));
        }
        ws[(int64_t)L * SS_LW + threadIdx.x] = acc;
    }
    if (threadIdx.x == 3) ws[(int64_t)L * SS_LW + 3] = 0.f;
}

// what the kernels below share beyond their points
struct Ssdf {
    const float* coeff;
    int G, C;
    const float* ws;
    int L;
    const float* fh_tab;
    int n_lambda, n_theta;
    float shadow_pow, self_pow;
    float* factor;
    float* decay;
};

// Record point i of the block (threads 0..63, one each): m = the point minus the model's position.  fetch_ssdf's
// normalisation (sg_shadow.py:80-87) after the optional rotation; row < 0: no such point.
__device__ __forceinline__ void ssdf_stage_point(float* __restrict__ rec, int i, int32_t row, const float m_in[3],
                                                 const float* __restrict__ rot, float scale, float vol_range,
                                                 float angle_decay_fac) {
    float m[3] = {m_in[0], m_in[1], m_in[2]};
    if (rot) {
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] = rot[3 * k] * m_in[0] + rot[3 * k + 1] * m_in[1] + rot[3 * k + 2] * m_in[2];
    }
    float q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = m[k] / scale / vol_range;
    const float dis = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), 1.f);
#pragma unroll
    for (int k = 0; k < 3; ++k) rec[4 * i + k] = q[k] / dis;
    rec[4 * i + 3] = (asinf(1.f / vol_range) - asinf(1.f / (dis * vol_range))) * angle_decay_fac;
    reinterpret_cast<int32_t*>(rec + 4 * SS_PTS)[i] = row;
}

// one axis of the volume sample: align_corners=True, border padding
__device__ __forceinline__ void volume_axis(float q, int G, int& i0, int& i1, float& w0, float& w1) {
    float g = (q + 1.f) / 2.f * (float)(G - 1);
    g = fminf(fmaxf(g, 0.f), (float)(G - 1));
    const float f = floorf(g);
    i0 = (int)f;
    i1 = min(i0 + 1, G - 1);  // (past the face the weight is 0)
    w1 = g - f;
    w0 = (f + 1.f) - g;
}

// The block's 64 recorded points (smem's component space holds their records) against all lights.
// Called by all 256 threads; decay rows and factor entries of points with row < 0 are not written.
__device__ __forceinline__ void ssdf_block(float* __restrict__ smem, const Ssdf& S) {
    float* const A = smem;                 // [C][SS_A_STRIDE]
    float* const B = smem + SS_A_FLOATS;   // [C][SS_B_STRIDE]; before: the records; after a product: fh [64][33]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = S.C, G = S.G;

    // ---- the gather: wave w takes points 16 w .. 16 w + 15, lane = component (and component + 64)
    const int32_t* rows = reinterpret_cast<const int32_t*>(B + 4 * SS_PTS);
    for (int k = 0; k < SS_PTS / 4; ++k) {
        const int i = wave * (SS_PTS / 4) + k;
        float v0 = 0.f, v1 = 0.f;
        if (rows[i] >= 0) {
            int x0, x1, y0, y1, z0, z1;
            float wx0, wx1, wy0, wy1, wz0, wz1;
            volume_axis(B[4 * i + 0], G, x0, x1, wx0, wx1);
            volume_axis(B[4 * i + 1], G, y0, y1, wy0, wy1);
            volume_axis(B[4 * i + 2], G, z0, z1, wz0, wz1);
            // x indexes the first stored axis (the reference's permute(3,2,1,0)); corners in grid_sample's order
            const int xs[2] = {x0, x1}, ys[2] = {y0, y1}, zs[2] = {z0, z1};
            const float wxs[2] = {wx0, wx1}, wys[2] = {wy0, wy1}, wzs[2] = {wz0, wz1};
#pragma unroll
            for (int corner = 0; corner < 8; ++corner) {
                const int dx = corner & 1, dy = (corner >> 1) & 1, dz = corner >> 2;
                const float w = wxs[dx] * wys[dy] * wzs[dz];
                const float* cell = S.coeff + (((int64_t)xs[dx] * G + ys[dy]) * G + zs[dz]) * C;
                if (lane < C) v0 = fmaf(cell[lane], w, v0);
                if (lane + 64 < C) v1 = fmaf(cell[lane + 64], w, v1);
            }
        }
        if (lane < C) A[lane * SS_A_STRIDE + i] = v0;
        if (lane + 64 < C) A[(lane + 64) * SS_A_STRIDE + i] = v1;
    }
    // this thread's block of the product: points 4 tp .. 4 tp + 3, lights 2 tl, 2 tl + 1 of the tile
    const int tp = tid >> 4, tl = tid & 15;
    float delta[4];
    int32_t row[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        delta[a] = B[4 * (4 * tp + a) + 3];
        row[a] = rows[4 * tp + a];
    }
    const int32_t own_row = tid < SS_PTS ? rows[tid] : -1;
    // the factor's light sums of point `tid` (threads 0..63): compensated (Kahan), so that 32 or 64 terms of mixed
    // size cost one rounding, not a random walk of them
    float sum[3] = {0.f, 0.f, 0.f}, comp[3] = {0.f, 0.f, 0.f};

    for (int j0 = 0; j0 < S.L; j0 += SS_TILE) {
        const int nt = min(SS_TILE, S.L - j0);
        __syncthreads();  // the records / the previous tile's fh are read
        if ((tid & (SS_MAXC - 1)) < C) {  // thread = component, two lights a pass: coalesced reads, no division
            const int c = tid & (SS_MAXC - 1);
            for (int l = tid >> 7; l < SS_TILE; l += 2)
                B[c * SS_B_STRIDE + l] = l < nt ? S.ws[(int64_t)(j0 + l) * SS_LW + c] : 0.f;
        }
        __syncthreads();
        float acc[4][2] = {};
        for (int c = 0; c < C; ++c) {
            const float4 av = *reinterpret_cast<const float4*>(A + c * SS_A_STRIDE + 4 * tp);
            const float2 bv = *reinterpret_cast<const float2*>(B + c * SS_B_STRIDE + 2 * tl);
            const float as[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                acc[a][0] = fmaf(as[a], bv.x, acc[a][0]);
                acc[a][1] = fmaf(as[a], bv.y, acc[a][1]);
            }
        }
        float fh[4][2] = {};
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int l = 2 * tl + b;
            if (l >= nt) continue;
            const float* lw = S.ws + (int64_t)(j0 + l) * SS_LW;
            const float mean = lw[LW_MEAN], rowc = lw[LW_ROW], fhn = lw[LW_FHN];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (row[a] < 0) continue;
                float ssdf = acc[a][b] + mean + delta[a];
                ssdf = fminf(fmaxf(ssdf, -SS_HALF_PI), SS_HALF_PI);
                fh[a][b] = bilinear_border(S.fh_tab, S.n_lambda, S.n_theta, ssdf / SS_HALF_PI, rowc);
                if (S.decay) {
                    const float d = fminf(fmaxf(fabsf(fh[a][b] / fhn), 0.f), 1.f);
                    S.decay[(int64_t)row[a] * S.L + j0 + l] = powf(d, S.self_pow);
                }
            }
        }
        if (!S.factor) continue;  // (uniform over the block)
        __syncthreads();          // the product has read the components
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            B[(4 * tp + a) * SS_FH_STRIDE + 2 * tl] = fh[a][0];
            B[(4 * tp + a) * SS_FH_STRIDE + 2 * tl + 1] = fh[a][1];
        }
        __syncthreads();
        if (own_row >= 0) {  // fhs @ lcols: lights ascending in this one thread
            for (int l = 0; l < nt; ++l) {
                const float f = B[tid * SS_FH_STRIDE + l];
                const float* amp = S.ws + (int64_t)(j0 + l) * SS_LW + LW_AMP;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float y = f * amp[c] - comp[c];
                    const float t = sum[c] + y;
                    comp[c] = (t - sum[c]) - y;
                    sum[c] = t;
                }
            }
        }
    }
    if (S.factor && own_row >= 0) {
        const float* inte = S.ws + (int64_t)S.L * SS_LW;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = fminf(fmaxf(fabsf(sum[c] / inte[c]), 0.f), 1.f);
        const float luma = 0.2989f * v[0] + 0.5870f * v[1] + 0.1140f * v[2];
        S.factor[own_row] = powf(luma, S.shadow_pow);
    }
}

__global__ void __launch_bounds__(256) ssdf_points_kernel(const float* __restrict__ pts, int64_t P,
                                                          const float* __restrict__ model_pos,
                                                          const float* __restrict__ rot, float scale, float vol_range,
                                                          float angle_decay_fac, Ssdf S) {
    __shared__ __attribute__((aligned(16))) float smem[SS_A_FLOATS + SS_B_FLOATS];
    if (threadIdx.x < SS_PTS) {
        const int64_t p = (int64_t)blockIdx.x * SS_PTS + threadIdx.x;
        float m[3] = {0.f, 0.f, 0.f};
        if (p < P) {
#pragma unroll
            for (int k = 0; k < 3; ++k) m[k] = pts[3 * p + k] - model_pos[k];
        }
        ssdf_stage_point(smem + SS_A_FLOATS, threadIdx.x, p < P ? (int32_t)p : -1, m, rot, scale, vol_range,
                         angle_decay_fac);
    }
    __syncthreads();
    ssdf_block(smem, S);
}

// pts = rays_o + depth * normalize(rays_d) on the covered pixels of the model's box (main.py:526, 551-561)
__global__ void __launch_bounds__(256) ssdf_frame_decay_kernel(
    const int32_t* __restrict__ bbox, int64_t H, int64_t W, const float* __restrict__ directions,
    const float* __restrict__ pose, const float* __restrict__ obj_depth, const float* __restrict__ model_pos,
    const float* __restrict__ rot, float scale, float vol_range, float angle_decay_fac, Ssdf S) {
    __shared__ __attribute__((aligned(16))) float smem[SS_A_FLOATS + SS_B_FLOATS];
    const Rect r = clamp_rect(bbox[0], bbox[1], bbox[2], bbox[3], H, W);
    bool covered = false;
    if (threadIdx.x < SS_PTS) {
        const int64_t p = (int64_t)blockIdx.x * SS_PTS + threadIdx.x;
        float m[3] = {0.f, 0.f, 0.f};
        if (p < H * W && r.n > 0) {
            const int64_t y = p / W, x = p % W;
            covered = y >= r.hs && y < r.hl && x >= r.ws && x < r.wl && obj_depth[p] > 1e-6f;
        }
        if (covered) {
            float d[3];
            ray_dir(pose, directions + 3 * p, d);
            const float dl = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);  // insert_utils.normalize: no epsilon
            const float dep = obj_depth[p];
#pragma unroll
            for (int k = 0; k < 3; ++k) m[k] = (pose[4 * k + 3] + dep * (d[k] / dl)) - model_pos[k];
        }
        ssdf_stage_point(smem + SS_A_FLOATS, threadIdx.x, covered ? (int32_t)p : -1, m, rot, scale, vol_range,
                         angle_decay_fac);
    }
    if (!__syncthreads_or(covered)) return;  // (uniform: no pixel of this block is covered)
    ssdf_block(smem, S);
}

// torchvision's gaussian_blur(kernel (3,3)): sigma 0.8, weights exp(-0.5 (x/0.8)^2) / sum over x = -1, 0, 1
constexpr float BLUR_W0 = 0.52201146875f, BLUR_W1 = 0.23899426562f;

__device__ __forceinline__ int64_t reflect(int64_t i, int64_t n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__global__ void __launch_bounds__(256) shadow_apply_kernel(const float* __restrict__ frame_rgb,
                                                           const float* __restrict__ factor, int64_t H, int64_t W,
                                                           float* __restrict__ out_rgb) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= H * W) return;
    const int64_t y = p / W, x = p % W;
    const int64_t xl = reflect(x - 1, W), xr = reflect(x + 1, W);
    float h[3];  // the row pass at rows y - 1, y, y + 1 (the 2-D kernel is the outer product of the 1-D weights)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* row = factor + reflect(y - 1 + k, H) * W;
        h[k] = BLUR_W1 * (row[xl] + row[xr]) + BLUR_W0 * row[x];
    }
    const float blur = BLUR_W1 * (h[0] + h[2]) + BLUR_W0 * h[1];
#pragma unroll
    for (int c = 0; c < 3; ++c) out_rgb[3 * p + c] = frame_rgb[3 * p + c] * blur;
}

static bool ssdf_args_ok(const float* coeff, int G, int C, const float* ws, int L, const float* fh_tab, int n_lambda,
                         int n_theta) {
    return coeff && ws && fh_tab && G >= 2 && G <= 1024 && C >= 1 && C <= SS_MAXC && L >= 1 &&
           (int64_t)G * G * G * C < INT32_MAX && n_lambda >= 1 && n_theta >= 1 &&
           (int64_t)n_lambda * n_theta < INT32_MAX;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_sg_shadow_lights(const float* lSGs, int n_lights, const float* rot_inv, const float* components,
                         const float* mean, int n_components, int env_h, int env_w, float* light_ws, void* stream) {
    NGP_CHECK_ARG(lSGs && components && mean && light_ws);
    NGP_CHECK_ARG(n_lights >= 1 && n_lights <= (1 << 20));
    NGP_CHECK_ARG(n_components >= 1 && n_components <= SS_MAXC);
    NGP_CHECK_ARG(env_h >= 1 && env_w >= 1 && (int64_t)env_h * env_w * n_components < INT32_MAX);
    ssdf_lights_kernel<<<1, 256, 0, as_stream(stream)>>>(lSGs, n_lights, rot_inv, components, mean, n_components,
                                                         env_h, env_w, light_ws);
    return ngp_launch_status();
}

int ngp_sg_shadow_points(const float* pts, int64_t n_points, const float* model_pos, const float* rot_inv,
                         float scale, const float* coeff, int grid_size, int n_components, float vol_range,
                         float angle_decay_fac, const float* light_ws, int n_lights, const float* fh_tab,
                         int n_lambda, int n_theta, float shadow_pow, float self_shadow_pow, float* factor,
                         float* decay, void* stream) {
    NGP_CHECK_ARG(n_points >= 0 && n_points < INT32_MAX);
    NGP_CHECK_ARG(ssdf_args_ok(coeff, grid_size, n_components, light_ws, n_lights, fh_tab, n_lambda, n_theta));
    NGP_CHECK_ARG(model_pos && (factor || decay));
    NGP_CHECK_ARG(scale > 0.f && vol_range > 0.f);
    if (n_points == 0) return NGP_OK;
    NGP_CHECK_ARG(pts);
    const Ssdf S = {coeff, grid_size, n_components, light_ws, n_lights, fh_tab, n_lambda, n_theta,
                    shadow_pow, self_shadow_pow, factor, decay};
    const unsigned blocks = (unsigned)((n_points + SS_PTS - 1) / SS_PTS);
    ssdf_points_kernel<<<blocks, 256, 0, as_stream(stream)>>>(pts, n_points, model_pos, rot_inv, scale, vol_range,
                                                              angle_decay_fac, S);
    return ngp_launch_status();
}

int ngp_sg_shadow_frame_decay(const int32_t* bbox, int64_t H, int64_t W, const float* directions, const float* pose,
                              const float* obj_depth, const float* model_pos, const float* rot_inv, float scale,
                              const float* coeff, int grid_size, int n_components, float vol_range,
                              float angle_decay_fac, const float* light_ws, int n_lights, const float* fh_tab,
                              int n_lambda, int n_theta, float self_shadow_pow, float* decay, void* stream) {
    NGP_CHECK_ARG(H >= 1 && W >= 1 && H < INT32_MAX && W < INT32_MAX && H * W < INT32_MAX);
    NGP_CHECK_ARG(bbox && directions && pose && obj_depth && model_pos && decay);
    NGP_CHECK_ARG(ssdf_args_ok(coeff, grid_size, n_components, light_ws, n_lights, fh_tab, n_lambda, n_theta));
    NGP_CHECK_ARG(scale > 0.f && vol_range > 0.f);
    const Ssdf S = {coeff, grid_size, n_components, light_ws, n_lights, fh_tab, n_lambda, n_theta,
                    1.f, self_shadow_pow, nullptr, decay};
    const unsigned blocks = (unsigned)((H * W + SS_PTS - 1) / SS_PTS);
    ssdf_frame_decay_kernel<<<blocks, 256, 0, as_stream(stream)>>>(bbox, H, W, directions, pose, obj_depth, model_pos,
                                                                   rot_inv, scale, vol_range, angle_decay_fac, S);
    return ngp_launch_status();
}

int ngp_shadow_apply(const float* frame_rgb, const float* factor, int64_t H, int64_t W, float* out_rgb, void* stream) {
    NGP_CHECK_ARG(H >= 2 && W >= 2 && H < INT32_MAX && W < INT32_MAX && H * W < INT32_MAX);
    NGP_CHECK_ARG(frame_rgb && factor && out_rgb);
    const unsigned blocks = (unsigned)((H * W + 255) / 256);
    shadow_apply_kernel<<<blocks, 256, 0, as_stream(stream)>>>(frame_rgb, factor, H, W, out_rgb);
    return ngp_launch_status();
}

}  // extern "C"
