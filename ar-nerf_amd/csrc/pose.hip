// Camera pose refinement of the fused training step (--optimize_ext,
// train.py:92-95, 132-137): every training image carries an axis-angle
// correction dR and a translation dT, one flat parameter
// ext = [dR (N,3) | dT (N,3) | pad] (pose_refine.PoseRefiner).
//
// pose_compose_kernel   poses_out[i] = [Rod(dR_i) R_i | t_i + dT_i], one lane per
//                       image.  Rod as the reference defines it (datasets/
//                       ray_utils.py:39-53): theta = |v| + 1e-7, R = I + A K +
//                       B K^2, A = sin(theta)/theta, B = (1 - cos(theta))/theta^2
//                       evaluated as 2 (sin(theta/2)/theta)^2 (no 1 - cos
//                       cancellation), K^2 written out as v v^T - |v|^2 I with the
//                       diagonal -(v_b^2 + v_c^2) (no cancellation either).  At
//                       v = 0, K = K^2 = 0 and Rod = I exactly.
// pose_grad_kernel      the chain rule from the per-ray gradients (dL/drays_o,
//                       dL/drays_d of ngp_ray_segment_sum) to ext's gradient, one
//                       block of four waves per image: threads stride the batch's
//                       img_idx, each holding 12 partial sums (dL/dT: sum go;
//                       G[a][c] = sum gd[a] dir[c], the transpose of get_rays),
//                       added in ray order within a thread, across a wave's lanes
//                       by a fixed xor butterfly and across the four waves in wave
//                       order -- no sort, no atomics, bit-identical from run to
//                       run.  (One wave per image, the first form, walked 8192
//                       indices in 128 dependent steps: 137 us for 10 images, all
//                       load latency.)  Then, per image (wave 0 holds the sums;
//                       lanes 0-2 write): M = G R_i^T = dL/dRod and
//                         dL/dv_k = A w_k + B ((M v)_k + (M^T v)_k - 2 v_k tr M)
//                                 + (A' <w, v> + B' (v^T M v - |v|^2 tr M)) v_k/|v|
//                       with w = (M21 - M12, M02 - M20, M10 - M01) (the
//                       contraction of M with the skew generators; K^2 = v v^T -
//                       |v|^2 I differentiated in closed form) and the last term 0
//                       at |v| = 0 (torch.norm's gradient there).  A' = (theta cos
//                       theta - sin theta)/theta^2 and B' = (theta sin theta - 2
//                       (1 - cos theta))/theta^3 cancel catastrophically in fp32
//                       for small theta, where refinement lives: below a
//                       threshold each is its Taylor series (rod_dA, rod_dB).
//                       Images with no ray get zeros (their sums are empty), and
//                       image 0's block zeroes the padding: the caller zeroes
//                       nothing.
#pragma clang fp contract(off)
#include "common.h"
#include "wave.h"

namespace ngp {

struct RodCoef {
    float A, B, dA, dB;
};

// A'(theta) = (theta cos theta - sin theta) / theta^2 = -theta/3 + theta^3/30 - theta^5/840 + ...
// (coefficient of theta^(2n-1): (-1)^n 2n/(2n+1)!).  Series below 1.5 (next term theta^13/9.3e10: under
// 1e-8 of the value); from 1.5 on theta cos theta and -sin theta no longer cancel (cos <= 0.07).
__device__ __forceinline__ float rod_dA(float th, float s, float c) {
    if (th < 1.5f) {
        const float x = th * th;
        float p = 1.0f / 518918400.0f;
        p = 1.0f / 3991680.0f - x * p;
        p = 1.0f / 45360.0f - x * p;
        p = 1.0f / 840.0f - x * p;
        p = 1.0f / 30.0f - x * p;
        p = 1.0f / 3.0f - x * p;
        return -(th * p);
    }
    return (th * c - s) / (th * th);
}

// B'(theta) = (theta sin theta - 2 (1 - cos theta)) / theta^3 = -theta/12 + theta^3/180 - theta^5/6720 + ...
// (coefficient of theta^(2n-1): (-1)^n 2n/(2n+2)!).  Series below 2.5 (next term 18/20! theta^17: under 1e-9
// of the value); from 2.5 on the two terms differ by more than a factor 2 (2 (1 - cos) as 4 sin^2(theta/2)).
__device__ __forceinline__ float rod_dB(float th, float s, float sh) {
    if (th < 2.5f) {
        const float x = th * th;
        float p = 16.0f / 6402373705728000.0f;
        p = 14.0f / 20922789888000.0f - x * p;
        p = 1.0f / 7264857600.0f - x * p;
        p = 1.0f / 47900160.0f - x * p;
        p = 1.0f / 453600.0f - x * p;
        p = 1.0f / 6720.0f - x * p;
        p = 1.0f / 180.0f - x * p;
        p = 1.0f / 12.0f - x * p;
        return -(th * p);
    }
    return (th * s - 4.0f * (sh * sh)) / (th * th * th);
}

// theta = |v| + 1e-7 and the coefficients at it; nv = |v| (without the guard)
__device__ __forceinline__ RodCoef rod_coef(const float v[3], bool grad, float& nv) {
    nv = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const float th = nv + 1e-7f;
    const float s = sinf(th), sh = sinf(0.5f * th);
    const float q = sh / th;
    RodCoef r;
    r.A = s / th;
    r.B = 2.0f * (q * q);
    r.dA = r.dB = 0.f;
    if (grad) {
        r.dA = rod_dA(th, s, cosf(th));
        r.dB = rod_dB(th, s, sh);
    }
    return r;
}

__global__ void __launch_bounds__(64) pose_compose_kernel(const float* __restrict__ poses,
                                                          const float* __restrict__ ext, int64_t n_img,
                                                          float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n_img) return;
    const float v[3] = {ext[3 * i], ext[3 * i + 1], ext[3 * i + 2]};
    float nv;
    const RodCoef k = rod_coef(v, false, nv);
    // Rod = (I + A K) + B K^2
    float rod[3][3];
    rod[0][0] = 1.0f + k.B * -(v[1] * v[1] + v[2] * v[2]);
    rod[1][1] = 1.0f + k.B * -(v[0] * v[0] + v[2] * v[2]);
    rod[2][2] = 1.0f + k.B * -(v[0] * v[0] + v[1] * v[1]);
    rod[0][1] = k.A * -v[2] + k.B * (v[0] * v[1]);
    rod[1][0] = k.A * v[2] + k.B * (v[0] * v[1]);
    rod[0][2] = k.A * v[1] + k.B * (v[0] * v[2]);
    rod[2][0] = k.A * -v[1] + k.B * (v[0] * v[2]);
    rod[1][2] = k.A * -v[0] + k.B * (v[1] * v[2]);
    rod[2][1] = k.A * v[0] + k.B * (v[1] * v[2]);
    const float* P = poses + 12 * i;
    float* O = out + 12 * i;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b)
            O[4 * a + b] = (rod[a][0] * P[b] + rod[a][1] * P[4 + b]) + rod[a][2] * P[8 + b];
        O[4 * a + 3] = P[4 * a + 3] + ext[3 * n_img + 3 * i + a];
    }
}

// A, B, A', B' at theta = theta[j] (no guard added): the coefficient functions on their own, for the tests
__global__ void __launch_bounds__(256) rod_coefficients_kernel(const float* __restrict__ theta, int64_t n,
                                                               float* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const float th = theta[j];
    const float s = sinf(th), sh = sinf(0.5f * th);
    const float q = sh / th;
    out[4 * j] = s / th;
    out[4 * j + 1] = 2.0f * (q * q);
    out[4 * j + 2] = rod_dA(th, s, cosf(th));
    out[4 * j + 3] = rod_dB(th, s, sh);
}

constexpr int POSE_THREADS = 256, POSE_WAVES = POSE_THREADS / 64;

__global__ void __launch_bounds__(POSE_THREADS) pose_grad_kernel(
    const float* __restrict__ go, const float* __restrict__ gd, const int64_t* __restrict__ img_idx,
    const int64_t* __restrict__ pix_idx, int64_t n_rays, const float* __restrict__ directions,
    const float* __restrict__ poses, const float* __restrict__ ext, int64_t n_img, float* __restrict__ grad_ext) {
    __shared__ float part[POSE_WAVES][12];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t i = blockIdx.x;  // one block per image
    float st[3] = {0.f, 0.f, 0.f}, G[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    // thread t takes rays t, t + 256, ...: four index loads in flight at a time (the walk is bound by their
    // latency), matches accumulated in ascending ray order
    for (int64_t base = threadIdx.x; base < n_rays; base += 4 * POSE_THREADS) {
        int64_t im[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t r = base + (int64_t)u * POSE_THREADS;
            im[u] = r < n_rays ? img_idx[r] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (im[u] != i) continue;
            const int64_t r = base + (int64_t)u * POSE_THREADS;
            const int64_t p = pix_idx[r];
            const float c[3] = {directions[3 * p], directions[3 * p + 1], directions[3 * p + 2]};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                st[a] += go[3 * r + a];
                const float g = gd[3 * r + a];
#pragma unroll
                for (int b = 0; b < 3; ++b) G[a][b] = fmaf(g, c[b], G[a][b]);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        st[a] = wave_sum(st[a]);
#pragma unroll
        for (int b = 0; b < 3; ++b) G[a][b] = wave_sum(G[a][b]);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            part[wid][a] = st[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) part[wid][3 + 3 * a + b] = G[a][b];
        }
    }
    __syncthreads();
    if (wid != 0) return;
    // the four waves' partial sums in wave order: ((w0 + w1) + w2) + w3
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        st[a] = ((part[0][a] + part[1][a]) + part[2][a]) + part[3][a];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int k = 3 + 3 * a + b;
            G[a][b] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
        }
    }
    // every lane of wave 0 holds the image's sums; the 3x3 algebra once, lanes 0-2 write
    const float* P = poses + 12 * i;
    float M[3][3];  // M = G R_i^T
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) M[a][b] = (G[a][0] * P[4 * b] + G[a][1] * P[4 * b + 1]) + G[a][2] * P[4 * b + 2];
    const float v[3] = {ext[3 * i], ext[3 * i + 1], ext[3 * i + 2]};
    float nv;
    const RodCoef k = rod_coef(v, true, nv);
    const float w[3] = {M[2][1] - M[1][2], M[0][2] - M[2][0], M[1][0] - M[0][1]};
    const float tr = (M[0][0] + M[1][1]) + M[2][2];
    float Mv[3], Mtv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        Mv[a] = (M[a][0] * v[0] + M[a][1] * v[1]) + M[a][2] * v[2];
        Mtv[a] = (M[0][a] * v[0] + M[1][a] * v[1]) + M[2][a] * v[2];
    }
    const float wv = (w[0] * v[0] + w[1] * v[1]) + w[2] * v[2];
    const float vMv = (v[0] * Mv[0] + v[1] * Mv[1]) + v[2] * Mv[2];
    const float n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const float radial = k.dA * wv + k.dB * (vMv - n2 * tr);
    float dv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float rho = nv > 0.f ? v[a] / nv : 0.f;
        dv[a] = (k.A * w[a] + k.B * ((Mv[a] + Mtv[a]) - 2.0f * (v[a] * tr))) + radial * rho;
    }
    if (lane < 3) {
        grad_ext[3 * i + lane] = lane == 0 ? dv[0] : lane == 1 ? dv[1] : dv[2];
        grad_ext[3 * n_img + 3 * i + lane] = lane == 0 ? st[0] : lane == 1 ? st[1] : st[2];
    }
    if (i == 0) {  // the padding of ext's length to a multiple of 4 (at most 3 floats)
        const int64_t n = 6 * n_img, n_pad = (n + 3) / 4 * 4;
        if (n + lane < n_pad) grad_ext[n + lane] = 0.f;
    }
}

}  // namespace ngp

using namespace ngp;

extern "C" int ngp_pose_compose(const float* poses, const float* ext, int64_t n_img, float* poses_out,
                                void* stream) {
    NGP_CHECK_ARG(n_img >= 0);
    NGP_CHECK_ARG(poses && ext && poses_out);
    if (n_img == 0) return NGP_OK;
    NGP_CHECK_ARG((n_img + 63) / 64 <= 0x7fffffffLL);
    hipStream_t s = as_stream(stream);
    NGP_TIMED(NGP_K_POSE_COMPOSE, s, pose_compose_kernel<<<(unsigned)((n_img + 63) / 64), 64, 0, s>>>(
        poses, ext, n_img, poses_out));
    return ngp_launch_status();
}

extern "C" int ngp_pose_rod_coefficients(const float* theta, int64_t n, float* out, void* stream) {
    NGP_CHECK_ARG(n >= 0);
    NGP_CHECK_ARG(theta && out);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG((n + 255) / 256 <= 0x7fffffffLL);
    rod_coefficients_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(theta, n, out);
    return ngp_launch_status();
}

extern "C" int ngp_pose_grad(const float* dL_drays_o, const float* dL_drays_d, const int64_t* img_idx,
                             const int64_t* pix_idx, int64_t n_rays, const float* directions, const float* poses,
                             const float* ext, int64_t n_img, float* grad_ext, void* stream) {
    NGP_CHECK_ARG(n_rays >= 0 && n_img >= 0);
    NGP_CHECK_ARG(poses && ext && grad_ext);
    NGP_CHECK_ARG(n_rays == 0 || (dL_drays_o && dL_drays_d && img_idx && pix_idx && directions));
    if (n_img == 0) return NGP_OK;
    NGP_CHECK_ARG(n_img <= 0x7fffffffLL);
    hipStream_t s = as_stream(stream);
    NGP_TIMED(NGP_K_POSE_GRAD, s, pose_grad_kernel<<<(unsigned)n_img, POSE_THREADS, 0, s>>>(
        dL_drays_o, dL_drays_d, img_idx, pix_idx, n_rays, directions, poses, ext, n_img, grad_ext));
    return ngp_launch_status();
}
