// The one statement of F.grid_sample's 2-D bilinear lookup with border padding
// and pixel centres (align_corners=False), shared by the SSDF shadows
// (shadow.hip: the component images and the hemisphere-integral table) and the
// cube-map lookup of the SG light probes (sgfit.hip: one face, three
// interleaved channels).  The order of operations is part of its contract:
// shadow.hip's results are pinned bit for bit against it.
#pragma once
#include "common.h"

namespace ngp {

// F.grid_sample(img (h,w), (x,y), bilinear, padding_mode="border", align_corners=False) of one image whose
// pixels lie STRIDE floats apart (1: a plain image; 3: one channel of an (h,w,3) image)
template <int STRIDE = 1>
__device__ __forceinline__ float bilinear_border(const float* __restrict__ img, int h, int w, float x, float y) {
    float ix = ((x + 1.f) * (float)w - 1.f) / 2.f;
    float iy = ((y + 1.f) * (float)h - 1.f) / 2.f;
    ix = fminf(fmaxf(ix, 0.f), (float)(w - 1));  // (a NaN coordinate lands on 0: no index leaves the image)
    iy = fminf(fmaxf(iy, 0.f), (float)(h - 1));
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);  // (past the edge the weight is 0)
    const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix, wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
    const float* r0 = img + (int64_t)y0 * w * STRIDE;
    const float* r1 = img + (int64_t)y1 * w * STRIDE;
    float v = r0[x0 * STRIDE] * (wx0 * wy0);
    v += r0[x1 * STRIDE] * (wx1 * wy0);
    v += r1[x0 * STRIDE] * (wx0 * wy1);
    v += r1[x1 * STRIDE] * (wx1 * wy1);
    return v;
}

}  // namespace ngp
