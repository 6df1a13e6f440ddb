/* roi_host.h -- the rule of region-of-interest quantisation in plain C, all integers: what the host entry points of the ABI
 * (mi355enc_roi_*), the handle (enc_roi.cpp) and the kernel (k_roi.hip) share.  No device needed. */
#ifndef MI355_ROI_HOST_H
#define MI355_ROI_HOST_H
#include <stdint.h>

#define ROI_RECTS_MAX 8
#define ROI_DELTA_MAX 12   /* |delta|, |a value of the caller's map|, |a composed offset|: two macroblocks then differ by at most 24, inside mb_qp_delta's -26 .. +25 */
#define ROI_FEATHER_MAX 8
#define ROI_BALANCE_MAX 12
#define ROI_COORD_MAX 65536 /* |x|, |y| <= this, 1 <= w, h <= this: every sum of two stays far inside an int */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ROI_FN static __host__ __device__ inline
#else
#define ROI_FN static inline
#endif

ROI_FN int roi_clip(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
/* what a macroblock's quantiser is moved by: the adaptive-quantisation offset (0 without aq_mode) and the map's value, clamped */
ROI_FN int roi_compose(int aq, int t) { return roi_clip(aq + t, -ROI_DELTA_MAX, ROI_DELTA_MAX); }

#endif
