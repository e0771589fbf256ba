// Real spherical harmonics up to band 2 (9 coefficients) in the order and
// with the constants of the insertion app (insert/insert_utils.py:102-127),
// shared by the light-probe kernels of probe.hip.
#pragma once
#pragma clang fp contract(off)
#include "common.h"

namespace ngp {

// Y[0..8] at the direction d = (x, y, z).  The two functions with a zero
// crossing that a plain evaluation reaches by cancellation keep a relative
// error of a few ulp everywhere: 3z^2 - 1 is rounded once (the rounding error
// of z*z is recovered with an fma and added back), x^2 - y^2 is (x-y)(x+y).
// So a single ray near such a crossing (a one-ray probe) is as accurate as a
// sum over many.
__device__ __forceinline__ void sh9_basis(float x, float y, float z, float Y[9]) {
    const float zz = z * z;
    const float zz_err = fmaf(z, z, -zz);  // z*z - zz, exact
    Y[0] = 0.2820947918f;
    Y[1] = 0.4886025119f * y;
    Y[2] = 0.4886025119f * z;
    Y[3] = 0.4886025119f * x;
    Y[4] = 1.0925484306f * x * y;
    Y[5] = 1.0925484306f * y * z;
    Y[6] = 0.3153915653f * (fmaf(3.0f, zz, -1.0f) + 3.0f * zz_err);
    Y[7] = 1.0925484306f * x * z;
    Y[8] = 0.5462742153f * ((x - y) * (x + y));
}

}  // namespace ngp
