// Object shading for insertion frames on gfx950: the SG branch of the
// reference app's Insertor.render_object (insert/main.py:521-594) and its
// SG_render_core (insert/render_utils.py:265-375) in one launch over the
// H x W frame, one lane per pixel.  The result is the whole-frame obj_rgb
// that insert_frame_finish_kernel (insert.hip) blends in behind the field.
//
// A pixel is covered when it lies in the model's box (a device rectangle,
// clamped like insert.hip's) and obj_depth > 1e-6 (main.py:526, an fp32
// compare); every other pixel of the frame is written 0 (main.py:585-589).
// A covered pixel is shaded under L spherical-Gaussian lights
// (axis, sharpness, rgb amplitude): the normal distribution becomes an SG
// about the reflected view direction, its product with each light and the
// light itself are integrated against the clamped cosine (SGIrradiance: a
// product with the cosine lobe and two hemisphere integrals), the sums over
// the lights are rectified AFTER the sum, and the Fresnel / geometry terms
// close the BRDF.  All of it is fp32 in the reference's order of operations,
// every clip and relu where the reference has it.
//
// Lights are wave-uniform: a tile of SG_TILE lights is staged in LDS together
// with the part of each light's own hemisphere integral that depends on its
// sharpness alone (the same device function every lane uses for the product
// lobes, so staging changes no bit), and all lanes read a light at the same
// address (a broadcast).  The light sum runs lights ascending in one lane: a
// pixel's value does not depend on the launch shape.  No atomics.
//
// Out of contract: a covered pixel with a zero normal (0/0 in the reference).
#pragma clang fp contract(off)
#include "insert.h"
#include "march.h"

namespace ngp {

constexpr int SG_TILE = NGP_SG_LIGHT_TILE;
constexpr float SG_EPS = 1e-6f;

// what SGHemisphereIntegral (render_utils.py:280-300) derives from the sharpness alone
struct Hemi {
    float t, inv_a, one_m_inv_a, Ab, Au;
};

__device__ __forceinline__ Hemi hemi_consts(float lambda) {
    Hemi h;
    const float lv = fmaxf(lambda, SG_EPS);
    const float il = 1.f / lv;
    h.t = sqrtf(lv) * (1.6988f + 10.8438f * il) / (1.f + 6.2201f * il + 10.2415f * il * il);
    h.inv_a = expf(-h.t);
    h.one_m_inv_a = 1.f - h.inv_a;
    const float k = 6.2831853071795864769f / lv;
    const float e1 = expf(-lv);
    h.Ab = k * (e1 - expf(-2.f * lv));
    h.Au = k * (1.f - e1);
    return h;
}

// the integral of a unit-amplitude SG over the hemisphere about the normal, cos_beta = axis . normal
__device__ __forceinline__ float hemi_integral(const Hemi& h, float cos_beta) {
    // cos_beta >= 0: inv_b = exp(-t cos_beta), s1; else b = exp(t cos_beta), s2 -- one exp serves both
    const float e = expf(-(h.t * fabsf(cos_beta)));
    const bool up = cos_beta >= 0.f;
    const float ie = h.inv_a * e;
    const float num = up ? 1.f - ie : e - h.inv_a;
    const float den = up ? h.one_m_inv_a + e - ie : h.one_m_inv_a * (e + 1.f);
    const float s = num / den;
    return h.Ab * (1.f - s) + h.Au * s;
}

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// SGProduct (render_utils.py:266-276) of two lobes' axes and sharpnesses: the product's axis and sharpness, and
// the factor exp(lm (|um| - 1)) its amplitude takes
__device__ __forceinline__ void sg_product(const float ax1[3], float l1, const float ax2[3], float l2, float ax[3],
                                           float& lambda, float& gain) {
    const float lm = l1 + l2;
    float um[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) um[c] = (l1 * ax1[c] + l2 * ax2[c]) / lm;
    const float len = sqrtf(dot3(um, um));
    const float inv = 1.f / len;
#pragma unroll
    for (int c = 0; c < 3; ++c) ax[c] = um[c] * inv;
    lambda = lm * len;
    gain = expf(lm * (len - 1.f));
}

// SGIrradiance (render_utils.py:304-317) of one lobe before the sum: unit-amplitude value w (the caller multiplies
// the lobe's rgb amplitude in, in the reference's order) as the pair (w_cos, w_own):
//   irradiance_c = (amp_c * 32.7080 * gain) * w_cos - 31.7003 * (w_own * amp_c)
struct Irr {
    float gain, w_cos, w_own;
};
__device__ __forceinline__ Irr sg_irradiance(const float ax[3], float lambda, const Hemi& own, const float n[3]) {
    Irr r;
    float axc[3], lc;
    sg_product(ax, lambda, n, 0.0315f, axc, lc, r.gain);
    r.w_cos = hemi_integral(hemi_consts(lc), dot3(axc, n));
    r.w_own = hemi_integral(own, dot3(ax, n));
    return r;
}
__device__ __forceinline__ float irr_channel(const Irr& r, float amp) {
    return r.w_cos * (amp * 32.7080f * r.gain) - 31.7003f * (r.w_own * amp);
}

// one staged light: axis, sharpness, amplitude and its own hemisphere constants
struct Light {
    float ax[3], lambda, amp[3];
    Hemi h;
};

__global__ void __launch_bounds__(256) sg_shade_kernel(
    const int32_t* __restrict__ bbox, int64_t H, int64_t W, const float* __restrict__ directions,
    const float* __restrict__ pose, const float* __restrict__ normals, const float* __restrict__ obj_depth,
    const float* __restrict__ lSGs, int L, const float* __restrict__ decay, const float* __restrict__ albedo,
    int albedo_rows, const float* __restrict__ metal_map, float metal_s, const float* __restrict__ rough_map,
    float rough_s, int clamp01, float* __restrict__ obj_rgb) {
    __shared__ Light lights[SG_TILE];
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Rect r = clamp_rect(bbox[0], bbox[1], bbox[2], bbox[3], H, W);
    const bool inframe = p < H * W;
    bool covered = false;
    if (inframe && r.n > 0) {
        const int64_t y = p / W, x = p % W;
        covered = y >= r.hs && y < r.hl && x >= r.ws && x < r.wl && obj_depth[p] > 1e-6f;  // main.py:526
    }

    float n[3] = {0.f, 0.f, 1.f}, v[3] = {0.f, 0.f, 1.f}, dax[3] = {0.f, 0.f, 1.f};
    float ndv = 1.f, rough = 1.f, metal = 0.f, alb[3] = {1.f, 1.f, 1.f}, dlam = 1.f, damp = 1.f;
    if (covered) {
        float d[3];
        ray_dir(pose, directions + 3 * p, d);
        const float dl = sqrtf(dot3(d, d));  // insert_utils.normalize: no epsilon
        const float nx = normals[3 * p], ny = normals[3 * p + 1], nz = normals[3 * p + 2];
        const float nl = sqrtf(nx * nx + ny * ny + nz * nz);
        n[0] = nx / nl; n[1] = ny / nl; n[2] = nz / nl;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = -(d[c] / dl);  // render_utils.py:322: the direction TO the camera
        ndv = dot3(n, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) dax[c] = ndv * n[c] * 2.f - v[c];  // reflect_dir
        rough = rough_map ? fminf(fmaxf(rough_map[p], 0.2f), 1.0f) : rough_s;  // main.py:539-542: only the map is clipped
        metal = metal_map ? metal_map[p] : metal_s;
        if (albedo) {
            const float* a = albedo + (albedo_rows == 1 ? 0 : 3 * p);
            alb[0] = a[0]; alb[1] = a[1]; alb[2] = a[2];
        }
        const float m2 = rough * rough;
        dlam = 2.f / m2 / (4.f * fmaxf(ndv, SG_EPS));  // pos_dot_eps
        damp = 1.f / (3.14159265358979323846f * m2);
    }

    float spec[3] = {0.f, 0.f, 0.f}, diff[3] = {0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < L; j0 += SG_TILE) {
        const int nt = min(SG_TILE, L - j0);
        __syncthreads();  // the previous tile is read
        if ((int)threadIdx.x < nt) {
            const float* s = lSGs + 7 * (int64_t)(j0 + threadIdx.x);
            Light& lt = lights[threadIdx.x];
            lt.ax[0] = s[0]; lt.ax[1] = s[1]; lt.ax[2] = s[2];
            lt.lambda = s[3];
            lt.amp[0] = s[4]; lt.amp[1] = s[5]; lt.amp[2] = s[6];
            lt.h = hemi_consts(s[3]);
        }
        __syncthreads();
        if (!covered) continue;
        for (int j = 0; j < nt; ++j) {
            const Light& lt = lights[j];
            float amp[3] = {lt.amp[0], lt.amp[1], lt.amp[2]};
            if (decay) {  // sg_shadow.py:143-152: the self-shadow decay scales the amplitude
                const float dc = decay[p * L + j0 + j];
#pragma unroll
                for (int c = 0; c < 3; ++c) amp[c] = amp[c] * dc;
            }
            // specular: the distribution lobe times the light
            float pax[3], plam, pgain;
            sg_product(dax, dlam, lt.ax, lt.lambda, pax, plam, pgain);
            const Irr si = sg_irradiance(pax, plam, hemi_consts(plam), n);
            // diffuse: the light alone
            const Irr di = sg_irradiance(lt.ax, lt.lambda, lt.h, n);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                spec[c] += irr_channel(si, damp * amp[c] * pgain);
                diff[c] += irr_channel(di, amp[c]);
            }
        }
    }
    if (!inframe) return;
    float out[3] = {0.f, 0.f, 0.f};
    if (covered) {
        const float ndv_pos = fmaxf(ndv, 0.f);  // pos_dot: NdotL = NdotV (render_utils.py:350-351)
        const float om = 1.f - ndv_pos;
        const float om2 = om * om;
        const float om5 = om2 * om2 * om;
        // GeometryBlender: NdotV = 0 gives +inf here, G = 0 and Moi = 0 (finite, as the reference's)
        const float tan2 = rough * rough * fmaxf(1.f / (ndv_pos * ndv_pos) - 1.f, 0.f);
        const float G = 1.f / (0.5f * (sqrtf(1.f + tan2) - 1.f) * 2.f + 1.f);
        const float denom = 4.f * ndv_pos * ndv_pos + SG_EPS;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float F0 = 0.04f * (1.f - metal) + alb[c] * metal;  // get_F0
            const float F = F0 + (1.f - F0) * om5;                      // fresnelSchlick
            const float Moi = F * G / denom;
            const float s = Moi * fmaxf(spec[c], 0.f);                 // relu after the light sum
            const float df = alb[c] / 3.14159265358979323846f * fmaxf(diff[c], 0.f);
            const float kS = F0 + (fmaxf(1.f - rough, F0) - F0) * om5;  // fresnelSchlickRoughness
            const float kD = (1.f - kS) * (1.f - metal);
            const float rad = kD * df + s;
            out[c] = clamp01 ? fminf(fmaxf(rad, 0.f), 1.f) : fmaxf(rad, 0.f);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) obj_rgb[3 * p + c] = out[c];
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_sg_shade(const int32_t* bbox, int64_t H, int64_t W, const float* directions, const float* pose,
                 const float* normals, const float* obj_depth, const float* lSGs, int n_lights, const float* decay,
                 const float* albedo, int albedo_rows, const float* metal_map, float metal, const float* rough_map,
                 float rough, int clamp01, float* obj_rgb, void* stream) {
    NGP_CHECK_ARG(H >= 1 && W >= 1 && H < INT32_MAX && W < INT32_MAX && H * W < INT32_MAX);
    NGP_CHECK_ARG(bbox && directions && pose && normals && obj_depth && lSGs && obj_rgb);
    NGP_CHECK_ARG(n_lights >= 1);
    NGP_CHECK_ARG(albedo ? (albedo_rows == 1 || albedo_rows == H * W) : albedo_rows == 0);
    const unsigned blocks = (unsigned)((H * W + 255) / 256);
    sg_shade_kernel<<<blocks, 256, 0, as_stream(stream)>>>(bbox, H, W, directions, pose, normals, obj_depth, lSGs,
                                                           n_lights, decay, albedo, albedo_rows, metal_map, metal,
                                                           rough_map, rough, clamp01, obj_rgb);
    return ngp_launch_status();
}

}  // extern "C"
