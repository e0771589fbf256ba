// SG light probes on gfx950: what the insertion app's generate_probe(pt,
// SH_probe=False) (insert/main.py:306-352) does with the cube map it has
// rendered -- cubemap2env_map (insert/render_utils.py:117-189) and the Adam
// fit of L spherical Gaussians to the env map (EnvOptim.eval,
// insert/envfit.py:275-297) -- without the (pixels, L, 3) tensors of the torch
// formulation.
//
//   cubemap_sample_kernel  one lane per direction: face choice, bilinear lookup.
//   sg_envmap_kernel       one lane per pixel, the parsed lights in LDS.
//   sg_fit_grad_kernel     one block per SF_PIX = 64 pixels.  Wave 0, a lane per
//                          pixel: the env value (lights ascending), the residual,
//                          g = 2 r / (3 P), into LDS; the block's sum of r^2
//                          (wave_sum).  Then every thread takes (light, group of
//                          8 pixels) items, lanes over lights, and sums its seven
//                          quantities over the group serially in fp64; one owner
//                          per (light, quantity) adds the 8 groups ascending and
//                          writes the block's row of the workspace.
//   sg_fit_step_kernel     one block: one owner per sum adds the rows in ascending
//                          block order; chain rule, loss, torch's Adam step with a
//                          device step count.
//
// Per-pair arithmetic is fp32 (v . a - 1 from the squared difference, one
// expf); the lights are parsed and the sums kept in fp64, in fixed orders: no
// atomics, nothing depends on timing.
#pragma clang fp contract(off)
#include "bilinear.h"
#include "wave.h"

namespace ngp {

constexpr int SF_PIX = NGP_SG_FIT_BLOCK_PIXELS;  // pixels per block: one wave forms their residuals
constexpr int SF_GROUPS = 8;                     // pixel groups of a block's serial sums
constexpr int SF_GPIX = SF_PIX / SF_GROUPS;
constexpr int SF_MAXL = NGP_SG_FIT_MAX_LIGHTS;
constexpr int SF_THREADS = 256;
constexpr float SF_TINY = 1e-8f;
static_assert(SF_PIX == 64, "wave 0 holds one pixel per lane");

// Words per light in LDS, S[SF_WORDS][L]: the axis (0..2), |sharpness| (3), |amplitude| (4..6), the axis's low
// part (7..9) and (|a|^2 - 1) / 2 (10).  parse_raw_sg per light in fp64: a = lobe / (|lobe| + 1e-8) is kept as a
// float pair (hi, lo), so that what a pair sees of it does not carry the rounding of a to fp32 -- an error shared
// by every pixel of the light, which a sharp light's exponent multiplies by its sharpness.
constexpr int SF_WORDS = 11;

__device__ __forceinline__ void sg_stage_lights(const float* __restrict__ raw, int L, float* __restrict__ S) {
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        const float* r = raw + 7 * l;
        const double x0 = r[0], x1 = r[1], x2 = r[2];
        const double n = sqrt(x0 * x0 + x1 * x1 + x2 * x2) + (double)SF_TINY;
        const double a[3] = {x0 / n, x1 / n, x2 / n};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float hi = (float)a[k];
            S[k * L + l] = hi;
            S[(7 + k) * L + l] = (float)(a[k] - (double)hi);
        }
#pragma unroll
        for (int k = 3; k < 7; ++k) S[k * L + l] = fabsf(r[k]);
        S[10 * L + l] = (float)(((a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) - 1.0) * 0.5);
    }
}

// (|v|^2 - 1) / 2 of a direction, once per pixel
__device__ __forceinline__ float sg_half_excess(const float v[3]) {
    return (float)((((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]) - 1.0) * 0.5);
}

// v . a - 1 of one pair as (|v|^2 - 1)/2 + (|a|^2 - 1)/2 - |v - a|^2 / 2: where the pair matters (v near a) the
// difference is small and nearly exact, so the result carries a few roundings of ITS OWN size, not of the size of
// the products v_k a_k (6e-8 absolute, which a sharpness of 100 turns into 6e-6 of the exponential).
__device__ __forceinline__ float sg_dot_minus_one(const float* __restrict__ S, int L, int l, float v0, float v1,
                                                  float v2, float cv) {
    const float d0 = (v0 - S[l]) - S[7 * L + l];
    const float d1 = (v1 - S[L + l]) - S[8 * L + l];
    const float d2 = (v2 - S[2 * L + l]) - S[9 * L + l];
    const float dd = fmaf(d2, d2, fmaf(d1, d1, d0 * d0));
    return fmaf(-0.5f, dd, cv + S[10 * L + l]);
}

// sum_l mu_l exp(lam_l (v . a_l - 1)), lights ascending
__device__ __forceinline__ void sg_env_pixel(const float* __restrict__ S, int L, const float v[3], float cv,
                                             float rgb[3]) {
    rgb[0] = rgb[1] = rgb[2] = 0.f;
    for (int l = 0; l < L; ++l) {
        const float e = expf(S[3 * L + l] * sg_dot_minus_one(S, L, l, v[0], v[1], v[2], cv));
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] += S[(4 + c) * L + l] * e;
    }
}

__global__ void __launch_bounds__(256) cubemap_sample_kernel(const float* __restrict__ cubemap, int res,
                                                             const float* __restrict__ dirs, int64_t n,
                                                             float* __restrict__ rgb) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float d[3] = {dirs[3 * p], dirs[3 * p + 1], dirs[3 * p + 2]};
    int axis = 0;
    float m = fabsf(d[0]);
    if (fabsf(d[1]) > m) { axis = 1; m = fabsf(d[1]); }
    if (fabsf(d[2]) > m) { axis = 2; m = fabsf(d[2]); }
    const float q[3] = {d[0] / m, d[1] / m, d[2] / m};
    const float s = axis == 0 ? q[0] : (axis == 1 ? q[1] : q[2]);
    float out[3] = {1.f, 1.f, 1.f};
    if (s > 0.f || s < 0.f) {  // (0 / 0 and inf / inf are NaN: neither)
        const float u = axis == 0 ? q[1] : q[0], v = axis == 2 ? q[1] : q[2];
        const int face = (axis == 0 ? 2 : (axis == 1 ? 4 : 0)) + (s < 0.f ? 1 : 0);
        const float* img = cubemap + (int64_t)face * res * res * 3;
        // tex2D(..., reverseHW=True): grid x = v walks the face's second index, grid y = u its first
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = bilinear_border<3>(img + c, res, res, v, u);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[3 * p + c] = out[c];
}

__global__ void __launch_bounds__(256) sg_envmap_kernel(const float* __restrict__ raw, int L,
                                                        const float* __restrict__ dirs, int64_t P,
                                                        float* __restrict__ rgb) {
    __shared__ float S[SF_WORDS * SF_MAXL];
    sg_stage_lights(raw, L, S);
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const float v[3] = {dirs[3 * p], dirs[3 * p + 1], dirs[3 * p + 2]};
    float c[3];
    sg_env_pixel(S, L, v, sg_half_excess(v), c);
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[3 * p + k] = c[k];
}

// dynamic LDS: double part[7][SF_GROUPS][L]
__global__ void __launch_bounds__(SF_THREADS) sg_fit_grad_kernel(const float* __restrict__ raw, int L,
                                                                 const float* __restrict__ dirs,
                                                                 const float* __restrict__ target, int P,
                                                                 float gscale, double* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) double part[];
    __shared__ float S[SF_WORDS * SF_MAXL];
    __shared__ float V[4][SF_PIX], Gd[3][SF_PIX];  // V[3]: (|v|^2 - 1) / 2
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * SF_PIX;
    const int np = min(SF_PIX, P - p0);
    double* const row = ws + (int64_t)blockIdx.x * L * 8;
    sg_stage_lights(raw, L, S);
    __syncthreads();
    if (tid < SF_PIX) {  // wave 0
        double sq = 0.0;
        float v[3] = {0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f}, cv = 0.f;
        if (tid < np) {
            const int p = p0 + tid;
            float env[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = dirs[3 * p + k];
            cv = sg_half_excess(v);
            sg_env_pixel(S, L, v, cv, env);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float r = env[c] - target[3 * p + c];
                g[c] = r * gscale;
                sq += (double)r * (double)r;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            V[k][tid] = v[k];
            Gd[k][tid] = g[k];
        }
        V[3][tid] = cv;
        sq = wave_sum(sq);
        if (tid == 0) row[7] = sq;
    }
    __syncthreads();
    // items (group, light), lanes over lights: the lights' words are read conflict-free, a pixel's as a broadcast
    for (int item = tid; item < SF_GROUPS * L; item += SF_THREADS) {
        const int l = item % L, grp = item / L;
        const float lam = S[3 * L + l];
        const float mu0 = S[4 * L + l], mu1 = S[5 * L + l], mu2 = S[6 * L + l];
        double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const int jend = min(np, (grp + 1) * SF_GPIX);
        for (int j = grp * SF_GPIX; j < jend; ++j) {
            const float v0 = V[0][j], v1 = V[1][j], v2 = V[2][j];
            const float g0 = Gd[0][j], g1 = Gd[1][j], g2 = Gd[2][j];
            const float dm = sg_dot_minus_one(S, L, l, v0, v1, v2, V[3][j]);
            const float e = expf(lam * dm);
            acc[0] += (double)(e * g0);
            acc[1] += (double)(e * g1);
            acc[2] += (double)(e * g2);
            const float se = (mu0 * g0 + mu1 * g1 + mu2 * g2) * e;
            acc[3] += (double)(se * dm);
            const float sel = se * lam;
            acc[4] += (double)(sel * v0);
            acc[5] += (double)(sel * v1);
            acc[6] += (double)(sel * v2);
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) part[(k * SF_GROUPS + grp) * L + l] = acc[k];
    }
    __syncthreads();
    for (int o = tid; o < 7 * L; o += SF_THREADS) {
        const int l = o % L, k = o / L;
        double sum = 0.0;
#pragma unroll
        for (int grp = 0; grp < SF_GROUPS; ++grp) sum += part[(k * SF_GROUPS + grp) * L + l];
        row[l * 8 + k] = sum;
    }
}

// dynamic LDS: double sums[L][8]
__global__ void __launch_bounds__(SF_THREADS) sg_fit_step_kernel(float* __restrict__ raw, int L,
                                                                 const double* __restrict__ ws, int blocks, int P,
                                                                 float* __restrict__ exp_avg,
                                                                 float* __restrict__ exp_avg_sq,
                                                                 int64_t* __restrict__ step, float lr,
                                                                 float* __restrict__ grad, float* __restrict__ loss) {
    extern __shared__ __attribute__((aligned(16))) double sums[];
    __shared__ float R[7 * SF_MAXL];
    const int tid = threadIdx.x;
    const int64_t t = *step + 1;
    for (int i = tid; i < 7 * L; i += SF_THREADS) R[i] = raw[i];
    for (int j = tid; j < 8 * L; j += SF_THREADS) {
        if ((j & 7) == 7 && j != 7) continue;  // (slot 7 is the loss, kept in light 0's row)
        double acc = 0.0;
        for (int b = 0; b < blocks; ++b) acc += ws[(int64_t)b * L * 8 + j];
        sums[j] = acc;
    }
    __syncthreads();  // (every thread has read *step and raw)
    if (tid == 0) {
        *step = t;
        *loss = (float)(sums[7] / (3.0 * (double)P));
    }
    const double b1 = 0.9, b2 = 0.999;
    const double bc1 = 1.0 - pow(b1, (double)t), bc2_sqrt = sqrt(1.0 - pow(b2, (double)t));
    const float step_size = (float)((double)lr / bc1), bc2s = (float)bc2_sqrt;
    const float w1 = (float)(1.0 - b1), fb2 = (float)b2, w2 = (float)(1.0 - b2);
    for (int i = tid; i < 7 * L; i += SF_THREADS) {
        const int l = i / 7, k = i % 7;
        const double* s = sums + 8 * l;
        const float* x = R + 7 * l;
        double g;
        if (k < 3) {
            const double x0 = x[0], x1 = x[1], x2 = x[2];
            const double n = sqrt(x0 * x0 + x1 * x1 + x2 * x2), ne = n + (double)SF_TINY;
            const double dax = s[4] * x0 + s[5] * x1 + s[6] * x2;
            // (the norm's own derivative is 0 at a zero vector, as torch's is; da / eps remains)
            g = s[4 + k] / ne - (n > 0.0 ? (double)x[k] * dax / (n * ne * ne) : 0.0);
        } else {
            const float sign = x[k] > 0.f ? 1.f : (x[k] < 0.f ? -1.f : 0.f);
            g = (double)sign * (k == 3 ? s[3] : s[k - 4]);
        }
        const float gf = (float)g;
        grad[i] = gf;
        float m = exp_avg[i], v = exp_avg_sq[i];
        m = m + w1 * (gf - m);
        v = v * fb2 + w2 * (gf * gf);
        exp_avg[i] = m;
        exp_avg_sq[i] = v;
        const float denom = sqrtf(v) / bc2s + 1e-8f;
        raw[i] = x[k] - step_size * (m / denom);
    }
}

static bool sg_fit_shape_ok(int64_t n_pixels, int n_lights) {
    return n_lights >= 1 && n_lights <= SF_MAXL && n_pixels >= 1 && n_pixels <= (1 << 24);
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_cubemap_sample(const float* cubemap, int res, const float* dirs, int64_t n_dirs, float* rgb, void* stream) {
    NGP_CHECK_ARG(cubemap && res >= 1 && res <= 8192);
    NGP_CHECK_ARG(n_dirs >= 0 && n_dirs < INT32_MAX);
    if (n_dirs == 0) return NGP_OK;
    NGP_CHECK_ARG(dirs && rgb);
    const unsigned blocks = (unsigned)((n_dirs + 255) / 256);
    cubemap_sample_kernel<<<blocks, 256, 0, as_stream(stream)>>>(cubemap, res, dirs, n_dirs, rgb);
    return ngp_launch_status();
}

int ngp_sg_envmap(const float* lgtSGs, int n_lights, const float* dirs, int64_t n_pixels, float* rgb, void* stream) {
    NGP_CHECK_ARG(lgtSGs && dirs && rgb);
    NGP_CHECK_ARG(n_lights >= 1 && n_lights <= SF_MAXL);
    NGP_CHECK_ARG(n_pixels >= 1 && n_pixels < INT32_MAX);
    const unsigned blocks = (unsigned)((n_pixels + 255) / 256);
    sg_envmap_kernel<<<blocks, 256, 0, as_stream(stream)>>>(lgtSGs, n_lights, dirs, n_pixels, rgb);
    return ngp_launch_status();
}

int64_t ngp_sg_fit_workspace_bytes(int64_t n_pixels, int n_lights) {
    if (!sg_fit_shape_ok(n_pixels, n_lights)) return 0;
    return (n_pixels + SF_PIX - 1) / SF_PIX * n_lights * 8 * (int64_t)sizeof(double);
}

int ngp_sg_fit(float* lgtSGs, int n_lights, const float* dirs, const float* target, int64_t n_pixels, int n_iter,
               float lr, float* exp_avg, float* exp_avg_sq, int64_t* step, void* workspace, float* grad,
               float* losses, void* stream) {
    NGP_CHECK_ARG(lgtSGs && dirs && target && exp_avg && exp_avg_sq && step && workspace && grad && losses);
    NGP_CHECK_ARG(sg_fit_shape_ok(n_pixels, n_lights));
    NGP_CHECK_ARG(n_iter >= 0);
    NGP_CHECK_ARG(((uintptr_t)workspace & 7) == 0);
    if (n_iter == 0) return NGP_OK;
    const int L = n_lights, P = (int)n_pixels;
    const int blocks = (P + SF_PIX - 1) / SF_PIX;
    const float gscale = (float)(2.0 / (3.0 * (double)P));
    const size_t grad_lds = (size_t)7 * SF_GROUPS * L * sizeof(double), step_lds = (size_t)8 * L * sizeof(double);
    double* ws = static_cast<double*>(workspace);
    for (int it = 0; it < n_iter; ++it) {
        sg_fit_grad_kernel<<<(unsigned)blocks, SF_THREADS, grad_lds, as_stream(stream)>>>(lgtSGs, L, dirs, target, P,
                                                                                          gscale, ws);
        sg_fit_step_kernel<<<1, SF_THREADS, step_lds, as_stream(stream)>>>(lgtSGs, L, ws, blocks, P, exp_avg,
                                                                           exp_avg_sq, step, lr, grad, losses + it);
    }
    return ngp_launch_status();
}

}  // extern "C"
