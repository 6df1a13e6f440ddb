/* hdr_host.h -- the parameter block of the HDR tone map, host only.  The entry point is the ABI's
 * (include/mi355enc.h: mi355enc_hdr_tables); this is what the shim and the kernel's launch share with it. */
#ifndef MI355_HDR_HOST_H
#define MI355_HDR_HOST_H
#include "../../include/mi355enc.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the block's layout in int32 words: header, then the four tables */
enum { HDR_HEAD = 40, HDR_LIN_N = 4097, HDR_GAIN_N = 1282, HDR_OE_N = 1025,
       HDR_LIN_AT = HDR_HEAD, HDR_GA_AT = HDR_LIN_AT + HDR_LIN_N, HDR_GB_AT = HDR_GA_AT + HDR_GAIN_N, HDR_OE_AT = HDR_GB_AT + HDR_GAIN_N,
       HDR_WORDS = HDR_OE_AT + HDR_OE_N };
/* MI355ENC_OK, or MI355ENC_ERR_ARG for arguments outside mi355enc_hdr_tables's; peak / target 0 are resolved to 1000 / 203 */
__attribute__((visibility("hidden"))) int hdr_check(int transfer, int full_range, int peak_nits, int target_nits);
/* fills out[HDR_WORDS]; arguments checked by the caller (hdr_check; out_matrix 1, 5 or 6) */
__attribute__((visibility("hidden"))) void hdr_build(int transfer, int full_range, int peak_nits, int target_nits, int out_matrix, int out_full, int32_t *out);
#ifdef __cplusplus
}
#endif
#endif
