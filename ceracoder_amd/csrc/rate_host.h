/* rate_host.h -- the rule of the frame-rate conversion, host only.  The entry points are the ABI's
 * (include/mi355enc.h: mi355enc_rate_check, mi355enc_rate_plan_init, mi355enc_rate_plan_step); this is what the shim shares with them. */
#ifndef MI355_RATE_HOST_H
#define MI355_RATE_HOST_H
#include "../../include/mi355enc.h"
#ifdef __cplusplus
extern "C" {
#endif
/* pts of tick k of an anchored plan: t0 + floor(k D / N), D = pps * fps_den, N = fps_num, in 128-bit arithmetic */
__attribute__((visibility("hidden"))) int64_t rate_tick_pts(const mi355enc_rate_plan_t *plan, int64_t k);
#ifdef __cplusplus
}
#endif
#endif
