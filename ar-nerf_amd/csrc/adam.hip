// Fused Adam with the fp16 shadow write and gradient zeroing, and the
// per-step device counters.  Replaces (apex FusedAdam at train.py:146-152).
#pragma clang fp contract(off)

#include "common.h"

namespace ngp {

// ------------------------------------------------------------------ Adam
// apex FusedAdam, adam_w_mode with weight_decay 0 == Adam (train.py:146):
//   m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2
//   p -= lr * (m / bc1) / (sqrt(v / bc2) + eps)
// g = grad * grad_scale (1/world_size after an all-reduce SUM).  Writes the
// fp16 shadow the kernels read and zeroes the gradient for the next step.
// 4 params per lane, 16-B loads/stores.
// lr_dev / step_dev (nullable): learning rate and the 0-based count of steps
// already taken read from device memory (graph replays), bias corrections
// for step *step_dev + 1 computed here (same fp32 powf as the host path).
__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, float* __restrict__ grad, float* __restrict__ m,
                                                   float* __restrict__ v, _Float16* __restrict__ p16, int64_t n4,
                                                   float lr, float b1, float b2, float eps, float bc1, float bc2,
                                                   float grad_scale, int zero_grad, const float* __restrict__ lr_dev,
                                                   const int64_t* __restrict__ step_dev, float* __restrict__ rep = nullptr,
                                                   int64_t rep_lo4 = 0, int64_t rep4 = 0, int nrep = 0,
                                                   float* __restrict__ zero = nullptr, int64_t zero4 = 0) {
    NGP_PROBE_BEGIN(NGP_P_ADAM);
    adam_bias(lr_dev, step_dev, b1, b2, lr, bc1, bc2);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 P = reinterpret_cast<float4*>(p)[i], Gd = reinterpret_cast<float4*>(grad)[i];
        float4 M = reinterpret_cast<float4*>(m)[i], V = reinterpret_cast<float4*>(v)[i];
        const int64_t j = i - rep_lo4;
        if (rep && j >= 0 && j < rep4) {  // gradient replicas (ngp_hash_backward_levels_rep), folded in order
            // One replica in flight per lane (round 5): the kernel's 60 VGPRs let one Adam wave per SIMD
            // run beside the accumulation's 1024-thread blocks (105 VGPRs), where with all 8 replicas'
            // loads issued first (round 3) it waited for those blocks to retire: +2.0 % end to end with
            // the accumulation's prefetch at one group (profiles/r05/ab/round5_ab.txt r5bb / r5cc).
            float4* r4 = reinterpret_cast<float4*>(rep);
            for (int r = 0; r < nrep; ++r) {
                const float4 c = r4[r * rep4 + j];
                Gd.x += c.x; Gd.y += c.y; Gd.z += c.z; Gd.w += c.w;
                r4[r * rep4 + j] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        float* pp = &P.x; float* gp = &Gd.x; float* mp = &M.x; float* vp = &V.x;
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        h4 out;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            adam_elem(pp[k], mp[k], vp[k], gp[k] * grad_scale, lr, b1, b2, eps, bc1, bc2);
            out[k] = (_Float16)pp[k];
        }
        reinterpret_cast<float4*>(p)[i] = P;
        reinterpret_cast<float4*>(m)[i] = M;
        reinterpret_cast<float4*>(v)[i] = V;
        reinterpret_cast<h4*>(p16)[i] = out;
        if (zero_grad) reinterpret_cast<float4*>(grad)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // (ngp_adam_step_dev_zero) a second range cleared by the same launch
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < zero4; i += stride)
        reinterpret_cast<float4*>(zero)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    NGP_PROBE_END();
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* params_f16, int64_t n,
                  float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale, int zero_grad,
                  void* stream) {
    NGP_CHECK_ARG(n >= 0 && step >= 1);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && params_f16);
    if (n % 4 != 0) return NGP_ERANGE;
    const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    NGP_TIMED(NGP_K_ADAM, as_stream(stream), adam_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(params, grads, exp_avg, exp_avg_sq,
                                                                 (_Float16*)params_f16, n4, lr, beta1, beta2, eps, bc1,
                                                                 bc2, grad_scale, zero_grad, nullptr, nullptr));
    return ngp_launch_status();
}

int ngp_adam_step_dev(float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* params_f16, int64_t n,
                      const float* lr_dev, float beta1, float beta2, float eps, const int64_t* step_dev,
                      float grad_scale, int zero_grad, void* stream) {
    NGP_CHECK_ARG(n >= 0);
    if (n == 0) return NGP_OK;
    NGP_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && params_f16 && lr_dev && step_dev);
    if (n % 4 != 0) return NGP_ERANGE;
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    NGP_TIMED(NGP_K_ADAM, as_stream(stream), adam_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(params, grads, exp_avg, exp_avg_sq,
                                                                 (_Float16*)params_f16, n4, 0.f, beta1, beta2, eps, 1.f,
                                                                 1.f, grad_scale, zero_grad, lr_dev, step_dev, nullptr, 0,
                                                                 0, 0));
    return ngp_launch_status();
}

int ngp_adam_step_dev_zero(float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* params_f16, int64_t n,
                           const float* lr_dev, float beta1, float beta2, float eps, const int64_t* step_dev,
                           float grad_scale, int zero_grad, float* zero, int64_t zero_n, void* stream) {
    NGP_CHECK_ARG(n >= 0 && zero_n >= 0 && zero_n % 4 == 0 && (zero_n == 0 || (zero && ((uintptr_t)zero & 15) == 0)));
    if (n == 0 && zero_n == 0) return NGP_OK;
    NGP_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && params_f16 && lr_dev && step_dev);
    if (n % 4 != 0) return NGP_ERANGE;
    const int64_t n4 = n / 4, z4 = zero_n / 4;
    int64_t blocks = (std::max(n4, z4) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    NGP_TIMED(NGP_K_ADAM, as_stream(stream), adam_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(params, grads, exp_avg, exp_avg_sq,
                                                                 (_Float16*)params_f16, n4, 0.f, beta1, beta2, eps, 1.f,
                                                                 1.f, grad_scale, zero_grad, lr_dev, step_dev, nullptr, 0,
                                                                 0, 0, zero, z4));
    return ngp_launch_status();
}

int ngp_adam_step_dev_rep(float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* params_f16, int64_t n,
                          const float* lr_dev, float beta1, float beta2, float eps, const int64_t* step_dev,
                          float grad_scale, int zero_grad, float* rep, int64_t rep_offset, int64_t rep_n, int n_rep,
                          void* stream) {
    if (!rep || rep_n == 0)
        return ngp_adam_step_dev(params, grads, exp_avg, exp_avg_sq, params_f16, n, lr_dev, beta1, beta2, eps,
                                 step_dev, grad_scale, zero_grad, stream);
    NGP_CHECK_ARG(n >= 0 && rep_offset >= 0 && rep_n > 0 && rep_offset % 4 == 0 && rep_n % 4 == 0 &&
                  rep_offset + rep_n <= n && n_rep >= 1 && n_rep <= 64 && ((uintptr_t)rep & 15) == 0);
    NGP_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && params_f16 && lr_dev && step_dev);
    if (n % 4 != 0) return NGP_ERANGE;
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    NGP_TIMED(NGP_K_ADAM, as_stream(stream), adam_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(params, grads, exp_avg, exp_avg_sq,
                                                                 (_Float16*)params_f16, n4, 0.f, beta1, beta2, eps, 1.f,
                                                                 1.f, grad_scale, zero_grad, lr_dev, step_dev, rep,
                                                                 rep_offset / 4, rep_n / 4, n_rep));
    return ngp_launch_status();
}

// counters[i] += 1 for i < n (the per-step device counters a replayed graph
// advances at its end: Adam's step count, the batch RNG counter)
__global__ void counters_inc_kernel(int64_t* __restrict__ c, int n) {
    NGP_PROBE_BEGIN(NGP_P_COUNTERS);  // (the row of the step the increment closes: read before it)
    if ((int)threadIdx.x < n) c[threadIdx.x] += 1;
    NGP_PROBE_END();
}

int ngp_counters_inc(int64_t* counters, int n, void* stream) {
    NGP_CHECK_ARG(counters && n >= 1 && n <= 64);
    counters_inc_kernel<<<1, 64, 0, as_stream(stream)>>>(counters, n);
    return ngp_launch_status();
}

}  // extern "C"
