/* denoise_host.h -- the rule of the temporal noise filter, host only.  The entry points are the ABI's (include/mi355enc.h:
 * mi355enc_denoise_default, _check, _tables, _motion_key); this is what the shim shares with them. */
#ifndef MI355_DENOISE_HOST_H
#define MI355_DENOISE_HOST_H
#include "../../include/mi355enc.h"
#ifdef __cplusplus
extern "C" {
#endif
/* which planes of a checked parameter set are filtered; 0: off */
enum { DENOISE_LUMA = 1, DENOISE_CHROMA = 2 };
__attribute__((visibility("hidden"))) int denoise_parts(const mi355enc_denoise_t *d);
/* the motion search's penalty per sample of vector length for the strength s that builds B (section 25) */
__attribute__((visibility("hidden"))) int denoise_motion_lambda(int s);
#ifdef __cplusplus
}
#endif
#endif
