/* adjust_host.h -- the rule of the picture controls, host only.  The entry points are the ABI's (include/mi355enc.h:
 * mi355enc_adjust_default, _check, _tables); this is what the shim shares with them. */
#ifndef MI355_ADJUST_HOST_H
#define MI355_ADJUST_HOST_H
#include "../../include/mi355enc.h"
#ifdef __cplusplus
extern "C" {
#endif
/* which parts of a checked parameter set are not neutral: the luma table is not the identity / the chroma rotation is not {4096, 0} / the stencil runs */
enum { ADJUST_LUMA = 1, ADJUST_CHROMA = 2, ADJUST_SHARPEN = 4 };
__attribute__((visibility("hidden"))) int adjust_parts(const mi355enc_adjust_t *a);
#ifdef __cplusplus
}
#endif
#endif
