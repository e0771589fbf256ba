// Test-set metrics (train.py:68-70, 208-249 of the reference: torchmetrics'
// PeakSignalNoiseRatio and StructuralSimilarityIndexMeasure, data_range 1):
// the frame's mean squared error and its SSIM (Wang et al. 2004; 11x11
// Gaussian window, sigma 1.5, whole windows only) in one pass.
//
//  * image_metrics_tile_kernel: one workgroup per IM_TW x IM_TH tile of
//    windows.  The tile's halo of both images goes to LDS (all three channels,
//    coordinates clamped to the frame: nothing outside it is read); per channel
//    a horizontal pass leaves the five moment rows E[x], E[y], E[x^2], E[y^2],
//    E[xy] in an fp64 LDS image and a vertical pass finishes the windows.  The
//    tile's index sum and the squared error of the input pixels it owns go to
//    its slot of the workspace through a fixed-order reduction.
//  * image_metrics_finish_kernel: one wave adds the slots in index order.
//
// Everything between the fp32 loads and the fp32 stores is fp64: the index
// divides E[x^2] - mx^2 by C2 = 9e-4, and on flat bright regions (a white
// background) fp32 loses that difference to cancellation.
// No atomics: two calls give the same bits.
#pragma clang fp contract(off)

#include "common.h"
#include "wave.h"

namespace ngp {

constexpr int IM_K = 11;                    // window taps per axis
constexpr int IM_TW = 32, IM_TH = 16;       // windows per tile
constexpr int IM_HW = IM_TW + IM_K - 1;     // halo pixels per tile row
constexpr int IM_HH = IM_TH + IM_K - 1;
constexpr int IM_THREADS = 256;
constexpr int IM_WAVES = IM_THREADS / 64;
constexpr double IM_C1 = 1e-4, IM_C2 = 9e-4;  // (0.01 L)^2, (0.03 L)^2 at data_range L = 1

struct ImWindow {
    double g[IM_K];
};

__global__ void __launch_bounds__(IM_THREADS) image_metrics_tile_kernel(const float* __restrict__ pred,
                                                                       const float* __restrict__ gt, int h, int w,
                                                                       int clamp01, ImWindow win, int nbx, int nby,
                                                                       double* __restrict__ slots,
                                                                       float* __restrict__ ssim_map) {
    __shared__ float sx[IM_HH][IM_HW * 3], sy[IM_HH][IM_HW * 3];
    __shared__ double sm[5][IM_HH][IM_TW];
    __shared__ double part[2][IM_WAVES];
    const int tid = threadIdx.x;
    const int bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
    const int x0 = bx * IM_TW, y0 = by * IM_TH;
    const int oh = h - (IM_K - 1), ow = w - (IM_K - 1);
    // Input pixels this tile owns for the squared error: its own IM_TH x IM_TW
    // block, the last tile of a row / column also the frame's remaining
    // (<= 10 + a partial tile) columns / rows -- all inside the halo.
    const int own_h = by == nby - 1 ? h - y0 : IM_TH, own_w = bx == nbx - 1 ? w - x0 : IM_TW;
    double se = 0.0, ss = 0.0;
    for (int i = tid; i < IM_HH * IM_HW * 3; i += IM_THREADS) {
        const int r = i / (IM_HW * 3), j = i - r * (IM_HW * 3), col = j / 3;
        const int yy = min(y0 + r, h - 1), xx = min(x0 + col, w - 1);
        const int idx = (yy * w + xx) * 3 + (j - col * 3);  // < 3 h w < 2^31
        float p = pred[idx];
        const float g = gt[idx];
        if (clamp01) p = p < 0.0f ? 0.0f : (p > 1.0f ? 1.0f : p);  // (keeps a NaN, as torch.clamp does)
        sx[r][j] = p;
        sy[r][j] = g;
        if (r < own_h && col < own_w) {
            const double d = (double)p - (double)g;
            se += d * d;
        }
    }
    __syncthreads();
    for (int c = 0; c < 3; ++c) {
        for (int i = tid; i < IM_HH * IM_TW; i += IM_THREADS) {
            const int r = i / IM_TW, ox = i % IM_TW;
            double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < IM_K; ++k) {
                const double x = sx[r][(ox + k) * 3 + c], y = sy[r][(ox + k) * 3 + c], g = win.g[k];
                a[0] = fma(g, x, a[0]);
                a[1] = fma(g, y, a[1]);
                a[2] = fma(g, x * x, a[2]);  // (fp32 values square exactly in fp64)
                a[3] = fma(g, y * y, a[3]);
                a[4] = fma(g, x * y, a[4]);
            }
#pragma unroll
            for (int m = 0; m < 5; ++m) sm[m][r][ox] = a[m];
        }
        __syncthreads();
        for (int i = tid; i < IM_TH * IM_TW; i += IM_THREADS) {
            const int oy = i / IM_TW, ox = i % IM_TW;
            double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < IM_K; ++k)
#pragma unroll
                for (int m = 0; m < 5; ++m) a[m] = fma(win.g[k], sm[m][oy + k][ox], a[m]);
            if (y0 + oy < oh && x0 + ox < ow) {
                const double mx = a[0], my = a[1];
                const double vx = a[2] - mx * mx, vy = a[3] - my * my, cxy = a[4] - mx * my;
                const double num = (2.0 * (mx * my) + IM_C1) * (2.0 * cxy + IM_C2);
                const double den = ((mx * mx + my * my) + IM_C1) * ((vx + vy) + IM_C2);
                const double v = num / den;
                ss += v;
                if (ssim_map) ssim_map[(c * oh + (y0 + oy)) * ow + (x0 + ox)] = (float)v;
            }
        }
        __syncthreads();
    }
    se = wave_sum(se);
    ss = wave_sum(ss);
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = se;
        part[1][tid >> 6] = ss;
    }
    __syncthreads();
    if (tid < 2) {
        double s = part[tid][0];
#pragma unroll
        for (int v = 1; v < IM_WAVES; ++v) s += part[tid][v];
        slots[2 * (int64_t)blockIdx.x + tid] = s;
    }
}

// out[0] = sum of the squared-error slots / (3 h w), out[1] = sum of the index
// slots / (3 (h-10) (w-10)), each added in slot order by one lane (lane 0 the
// error, lane 1 the index): the wave stages IM_FIN slots at a time in LDS, so
// the chain of dependent adds waits on no global load.
constexpr int IM_FIN = 1024;
__global__ void __launch_bounds__(64) image_metrics_finish_kernel(const double* __restrict__ slots, int n_slots,
                                                                 double n_elems, double n_windows,
                                                                 float* __restrict__ out) {
    __shared__ double buf[2][IM_FIN];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int base = 0; base < n_slots; base += IM_FIN) {
        const int m = min(IM_FIN, n_slots - base);
        for (int i = tid; i < m; i += 64) {
            buf[0][i] = slots[2 * (int64_t)(base + i)];
            buf[1][i] = slots[2 * (int64_t)(base + i) + 1];
        }
        __syncthreads();
        if (tid < 2) {
#pragma unroll 8
            for (int i = 0; i < m; ++i) acc += buf[tid][i];
        }
        __syncthreads();
    }
    if (tid < 2) out[tid] = (float)(acc / (tid == 0 ? n_elems : n_windows));
}

}  // namespace ngp

using namespace ngp;

// tiles of windows per axis / in all; 0 for a frame ngp_image_metrics refuses
static int64_t im_tiles(int h, int w, int* nbx, int* nby) {
    if (h < IM_K || w < IM_K || (int64_t)3 * h * w > (int64_t)INT32_MAX) return 0;
    *nbx = (w - (IM_K - 1) + IM_TW - 1) / IM_TW;
    *nby = (h - (IM_K - 1) + IM_TH - 1) / IM_TH;
    return (int64_t)*nbx * *nby;
}

extern "C" {

size_t ngp_image_metrics_ws_bytes(int h, int w) {
    int nbx, nby;
    return (size_t)im_tiles(h, w, &nbx, &nby) * 2 * sizeof(double);
}

int ngp_image_metrics(const float* pred, const float* gt, int h, int w, int clamp01, void* ws, float* out,
                      float* ssim_map, void* stream) {
    NGP_CHECK_ARG(pred && gt && ws && out && ((uintptr_t)ws & 7) == 0);
    NGP_CHECK_ARG(h >= IM_K && w >= IM_K);
    int nbx, nby;
    const int64_t n_tiles = im_tiles(h, w, &nbx, &nby);
    if (n_tiles == 0) return NGP_ERANGE;
    // the window of torchmetrics' _gaussian (functional/image/utils.py): exp(-(d / sigma)^2 / 2), d = -5..5, sum 1
    ImWindow win;
    double sum = 0.0;
    for (int k = 0; k < IM_K; ++k) {
        const double d = (double)(k - IM_K / 2) / 1.5;
        sum += win.g[k] = exp(-0.5 * d * d);
    }
    for (int k = 0; k < IM_K; ++k) win.g[k] /= sum;
    double* slots = static_cast<double*>(ws);
    image_metrics_tile_kernel<<<(unsigned)n_tiles, IM_THREADS, 0, as_stream(stream)>>>(pred, gt, h, w, clamp01, win, nbx,
                                                                                       nby, slots, ssim_map);
    const int rc = ngp_launch_status();
    if (rc != NGP_OK) return rc;
    image_metrics_finish_kernel<<<1, 64, 0, as_stream(stream)>>>(slots, (int)n_tiles, 3.0 * (double)h * (double)w,
                                                                 3.0 * (double)(h - (IM_K - 1)) *
                                                                     (double)(w - (IM_K - 1)),
                                                                 out);
    return ngp_launch_status();
}

}  // extern "C"
