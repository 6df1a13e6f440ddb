// k_roi.hip -- region-of-interest quantisation: the compose launch.  One thread per four macroblocks: the map's values t (pinned host
// memory or device memory: the picture's own copy, which nothing writes while it is in flight) and, with adaptive quantisation, the offsets aq_kernel wrote in
// front of this launch on the same stream, into the picture's offsets off[m] = clamp(aq[m] + t[m], -12, 12) (roi_host.h), in place over aq.  Words where four
// macroblocks are there, bytes in the tail; plain vector loads and stores.
#include "kernels_common.hpp"
#include "roi_host.h"

__global__ __launch_bounds__(256) void roi_compose_kernel(const int8_t *__restrict__ t, int8_t *__restrict__ off, int nmb, int have_aq) {
    const int m = 4 * (int)(blockIdx.x * 256 + threadIdx.x);
    if (m >= nmb) return;
    if (m + 4 <= nmb) { // (both buffers are at least 4-byte aligned: hipMalloc / hipHostMalloc)
        const unsigned tw = ldg32(t + m), aw = have_aq ? ldg32(off + m) : 0u;
        unsigned o = 0;
        for (int k = 0; k < 4; k++) o |= ((unsigned)roi_compose((int)(int8_t)(aw >> (8 * k)), (int)(int8_t)(tw >> (8 * k))) & 255u) << (8 * k);
        stg32(off + m, o);
    } else
        for (int i = m; i < nmb; i++) stg8(off + i, (unsigned)roi_compose(have_aq ? (int)(int8_t)ldg8(off + i) : 0, (int)(int8_t)ldg8(t + i)) & 255u);
}
void k_launch_roi_compose(const int8_t *t, int8_t *d_off, int nmb, int have_aq, hipStream_t s) {
    hipLaunchKernelGGL(roi_compose_kernel, dim3((nmb + 1023) / 1024), dim3(256), 0, s, t, d_off, nmb, have_aq);
}
