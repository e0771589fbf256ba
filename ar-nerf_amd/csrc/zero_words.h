// Zeroes n 64-bit words in stream order.  Used instead of hipMemsetAsync for
// the small counters zeroed inside captured graphs: in the exact-mode step
// graph a captured 8-byte memset was not reliably ordered before the kernel
// that reads the counter (ngp_guard_hits counted the fallout), a kernel node
// is.  Static: each translation unit that launches it carries its own copy.
#pragma once
#include "common.h"

namespace ngp {
static __global__ void zero_words_kernel(unsigned long long* __restrict__ p, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0ull;
}
}  // namespace ngp
