// Insertion frames for gfx950: the per-frame call of the reference's insertion
// app (insert/main.py:620-684, Insertor.render_insert_object) on the device
// render loop of render.hip.  The app renders the screen rectangle the
// virtual object covers (getUpdateRange, main.py:608-617), with every ray
// ended at the object's surface (mesh_depth_map, models/rendering.py:38-44)
// and the shaded object blended in behind what is left (IM_bkg,
// rendering.py:245-250), and writes the result into persistent canvases
// (main.py:652-654).
//
// The rectangle changes size on almost every frame, so here the ray count is
// a DEVICE value: the frame opening derives it from the rectangle and leaves
// it in a small header, the loop's iteration rule reads it from there, and
// every launch is sized for the whole frame (grids are upper bounds: all loop
// kernels stride over the alive count in `state`).  One set of captured
// graphs then renders any rectangle, bit for bit as a renderer built for it.
//
//   insert_frame_begin_kernel   rectangle -> n, rays of its pixels (gen_ray),
//                               mesh clip, loop state, alive list, zeroed outputs
//   render_iter_n_kernel        render_iter_kernel with N_rays = header[0]
//   insert_frame_finish_kernel  IM_bkg blend + scatter into the canvases + pts
#pragma clang fp contract(off)
#include "insert.h"
#include "march.h"

namespace ngp {

// header (int64[NGP_INSERT_HEADER_WORDS]) word indices
enum : int { IH_N = 0, IH_HS = 1, IH_WS = 2, IH_HL = 3, IH_WL = 4, IH_H = 5, IH_W = 6 };

__global__ void __launch_bounds__(256) insert_frame_begin_kernel(
    const int32_t* __restrict__ rect, int64_t H, int64_t W, const float* __restrict__ directions,
    const float* __restrict__ pose, const float* __restrict__ center, const float* __restrict__ half_size, float near,
    const float* __restrict__ obj_depth, float* __restrict__ rays_o, float* __restrict__ rays_d,
    float* __restrict__ hits_t, int64_t* __restrict__ state, int32_t* __restrict__ alive0,
    float* __restrict__ opacity, float* __restrict__ depth, float* __restrict__ rgb, int64_t* __restrict__ header) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Rect r = clamp_rect(rect[0], rect[1], rect[2], rect[3], H, W);
    if (i < NGP_RENDER_STATE_WORDS) {  // render_begin_kernel's state for n rays
        int64_t v = 0;
        if (i == RS_ALIVE0) v = r.n;
        if (i == RS_ACTIVE) v = 1;
        state[i] = v;
    }
    if (i < NGP_INSERT_HEADER_WORDS) {
        int64_t v = 0;
        if (i == IH_N) v = r.n;
        if (i == IH_HS) v = r.hs;
        if (i == IH_WS) v = r.ws;
        if (i == IH_HL) v = r.hl;
        if (i == IH_WL) v = r.wl;
        if (i == IH_H) v = H;
        if (i == IH_W) v = W;
        header[i] = v;
    }
    if (i >= r.n) return;
    const int64_t w = r.wl - r.ws;
    const int64_t p = (r.hs + i / w) * W + r.ws + i % w;  // directions[hs:hl, ws:wl] flattened (main.py:639)
    float o[3], d[3], ht[2];
    gen_ray(pose, directions + 3 * p, center, half_size, near, o, d, ht);
    // rendering.py:38-44: rays end at the object's surface (a ray that misses the box keeps -1)
    const float od = obj_depth[p];
    if (od >= 1e-6f) ht[1] = fmaxf(fminf(ht[1], od), ht[0]);
#pragma unroll
    for (int c = 0; c < 3; ++c) { rays_o[3 * i + c] = o[c]; rays_d[3 * i + c] = d[c]; }
    hits_t[2 * i] = ht[0];
    hits_t[2 * i + 1] = ht[1];
    alive0[i] = (int32_t)i;  // torch.arange(N_rays) (rendering.py:183)
    opacity[i] = 0.f;
    depth[i] = 0.f;
    rgb[3 * i] = 0.f; rgb[3 * i + 1] = 0.f; rgb[3 * i + 2] = 0.f;
}

// render_iter_kernel (render.hip) with the frame's ray count read from device
// memory (capped to what the buffers were sized for)
__global__ void render_iter_n_kernel(int64_t* __restrict__ state, int parity, const int64_t* __restrict__ n_rays_dev,
                                     int64_t n_rays_cap, int min_samples, int64_t sample_budget) {
    if (threadIdx.x != 0 || !state[RS_ACTIVE]) return;
    const int64_t n_rays = ngp_capped_count(n_rays_dev, n_rays_cap);
    const int64_t n_alive = state[parity];
    if (n_alive == 0 || state[RS_SAMPLES] >= sample_budget) {  // rendering.py:187-190
        state[RS_ACTIVE] = 0;
        state[RS_VALID] = 0;
        return;
    }
    int64_t ns = n_rays / n_alive;
    ns = ns < 64 ? ns : 64;
    ns = ns > min_samples ? ns : min_samples;
    state[RS_SAMPLES] += ns;
    state[RS_NS] = ns;
    state[RS_VALID] = 0;
    state[parity ^ 1] = 0;
    state[RS_ITERS] += 1;
}

// rendering.py:245-250 (rgb += IM_bkg * (1 - opacity)) and main.py:652-654
// (the scatter into last_rgb / last_depth), one thread per ray of the rectangle;
// pts = rays_o + rays_d * depth_sur (main.py:429).  Every pixel has one writer.
__global__ void __launch_bounds__(256) insert_frame_finish_kernel(
    const int64_t* __restrict__ header, int64_t H, int64_t W, const float* __restrict__ opacity,
    const float* __restrict__ depth, const float* __restrict__ rgb, const float* __restrict__ rays_o,
    const float* __restrict__ rays_d, const float* __restrict__ obj_rgb, float* __restrict__ frame_rgb,
    float* __restrict__ frame_depth, float* __restrict__ frame_pts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // (clamped again: a header written for another frame size cannot reach past this one)
    const Rect r = clamp_rect(header[IH_HS], header[IH_WS], header[IH_HL], header[IH_WL], H, W);
    const int64_t n = header[IH_N] < r.n ? header[IH_N] : r.n;
    if (i >= n) return;
    const int64_t w = r.wl - r.ws;
    const int64_t p = (r.hs + i / w) * W + r.ws + i % w;
    const float m = 1 - opacity[i], dp = depth[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) frame_rgb[3 * p + c] = rgb[3 * i + c] + obj_rgb[3 * p + c] * m;
    frame_depth[p] = dp;
    if (frame_pts) {
#pragma unroll
        for (int c = 0; c < 3; ++c) frame_pts[3 * p + c] = rays_o[3 * i + c] + rays_d[3 * i + c] * dp;
    }
}

}  // namespace ngp

using namespace ngp;

static inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

extern "C" {

int ngp_insert_frame_begin(const int32_t* rect, int64_t H, int64_t W, const float* directions, const float* pose,
                           const float* center, const float* half_size, float near_distance, const float* obj_depth,
                           float* rays_o, float* rays_d, float* hits_t, int64_t* state, int32_t* alive0, float* opacity,
                           float* depth, float* rgb, int64_t* header, void* stream) {
    NGP_CHECK_ARG(H >= 1 && W >= 1 && H < INT32_MAX && W < INT32_MAX && H * W < INT32_MAX);
    NGP_CHECK_ARG(rect && directions && pose && center && half_size && obj_depth && rays_o && rays_d && hits_t &&
                  state && alive0 && opacity && depth && rgb && header);
    static_assert(NGP_INSERT_HEADER_WORDS <= 256 && NGP_RENDER_STATE_WORDS <= 256, "written by the first block");
    insert_frame_begin_kernel<<<nblk(H * W, 256), 256, 0, as_stream(stream)>>>(
        rect, H, W, directions, pose, center, half_size, near_distance, obj_depth, rays_o, rays_d, hits_t, state,
        alive0, opacity, depth, rgb, header);
    return ngp_launch_status();
}

int ngp_render_test_march_n(const float* rays_o, const float* rays_d, float* hits_t, const int64_t* n_rays_dev,
                            int64_t n_rays_cap, const uint8_t* bitfield, int cascades, int grid_size, float scale,
                            float exp_step_factor, int max_samples, int min_samples, int64_t sample_budget, int parity,
                            int64_t* state, const int32_t* alive, const uint32_t* occ_summary, float* xyzs,
                            float* dirs, float* deltas, float* ts, int32_t* n_eff, int32_t* sample_idx, void* stream) {
    MarchParams p;
    int st = march_params(bitfield, cascades, grid_size, scale, exp_step_factor, max_samples, p);
    if (st) return st;
    st = march_attach_summary(p, occ_summary);
    if (st) return st;
    p.dt_scale = (float)cascades;  // raymarching.cu:370,399 quirk (test time)
    NGP_CHECK_ARG(n_rays_dev && n_rays_cap >= 0 && n_rays_cap < INT32_MAX && min_samples >= 1 &&
                  (parity == 0 || parity == 1) && state);
    NGP_CHECK_ARG(ngp_render_test_capacity(n_rays_cap, min_samples) < INT32_MAX);
    NGP_CHECK_ARG(n_rays_cap == 0 ||
                  (rays_o && rays_d && hits_t && alive && xyzs && dirs && deltas && ts && n_eff && sample_idx));
    hipStream_t s = as_stream(stream);
    render_iter_n_kernel<<<1, 64, 0, s>>>(state, parity, n_rays_dev, n_rays_cap, min_samples, sample_budget);
    if (n_rays_cap == 0) return ngp_launch_status();
    render_march_launch(rays_o, rays_d, hits_t, n_rays_cap, p, parity, state, alive, xyzs, dirs, deltas, ts, n_eff,
                        sample_idx, s);
    return ngp_launch_status();
}

int ngp_insert_frame_finish(const int64_t* header, int64_t H, int64_t W, const float* opacity, const float* depth,
                            const float* rgb, const float* rays_o, const float* rays_d, const float* obj_rgb,
                            float* frame_rgb, float* frame_depth, float* frame_pts, void* stream) {
    NGP_CHECK_ARG(H >= 1 && W >= 1 && H < INT32_MAX && W < INT32_MAX && H * W < INT32_MAX);
    NGP_CHECK_ARG(header && opacity && depth && rgb && rays_o && rays_d && obj_rgb && frame_rgb && frame_depth);
    insert_frame_finish_kernel<<<nblk(H * W, 256), 256, 0, as_stream(stream)>>>(
        header, H, W, opacity, depth, rgb, rays_o, rays_d, obj_rgb, frame_rgb, frame_depth, frame_pts);
    return ngp_launch_status();
}

}  // extern "C"
