/* jpeg_host.h -- the host half of MJPEG input: marker parser, Huffman table builder and the serial
 * entropy decode of a baseline JPEG picture into dense int16 coefficient blocks.  Plain C, no device needed; the public entry
 * points mi355enc_jpeg_info / mi355enc_jpeg_entropy_decode (include/mi355enc.h) live in jpeg_host.c as well. */
#ifndef MI355_JPEG_HOST_H
#define MI355_JPEG_HOST_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/mi355enc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per component c < info->components: blocks per row and block rows of its MCU-padded plane, and where its first block lies in the
 * coefficient buffer (in blocks of 64 int16); returns the number of blocks of the whole picture */
size_t jpeg_host_layout(const mi355enc_jpeg_info_t *info, int bw[3], int bh[3], size_t first[3]);

#ifdef __cplusplus
}
#endif
#endif
