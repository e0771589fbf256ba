// The screen rectangle of an insertion frame, shared by the frame kernels of
// insert.hip and the object shade of shade.hip: both clamp a device
// (hs, ws, hl, wl) to the frame by this one rule.
#pragma once
#include "common.h"

namespace ngp {

struct Rect {
    int64_t hs, ws, hl, wl, n;
};

// (hs, ws, hl, wl) clamped to [0,H] x [0,W]; inverted or empty: n = 0
__device__ __forceinline__ Rect clamp_rect(int64_t hs, int64_t ws, int64_t hl, int64_t wl, int64_t H, int64_t W) {
    Rect r;
    r.hs = hs < 0 ? 0 : (hs > H ? H : hs);
    r.hl = hl < 0 ? 0 : (hl > H ? H : hl);
    r.ws = ws < 0 ? 0 : (ws > W ? W : ws);
    r.wl = wl < 0 ? 0 : (wl > W ? W : wl);
    const int64_t h = r.hl - r.hs, w = r.wl - r.ws;
    r.n = (h > 0 && w > 0) ? h * w : 0;
    return r;
}

}  // namespace ngp
