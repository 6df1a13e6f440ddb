/* snapshot_host.h -- the host half of the JPEG stills: the quality scale, the reciprocals the device quantises with, and the
 * baseline JFIF writer over the quantised levels the device leaves.  Plain C, no device needed; the public entry points mi355enc_snapshot_tables /
 * _reciprocal / _max_bytes / _write (include/mi355enc.h) live in snapshot_host.c as well. */
#ifndef MI355_SNAPSHOT_HOST_H
#define MI355_SNAPSHOT_HOST_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/mi355enc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the kernel reads per still: per component class (0 luminance, 1 chrominance) and natural position, {m, 4 q}: q the table entry,
 * m = ceil(2^32 / (8 q)), so that (n * m) >> 32 = n / (8 q) for every numerator the transform can produce (mi355enc_snapshot_reciprocal). */
typedef struct { uint32_t m, q4; } snapshot_qent_t;
typedef struct { snapshot_qent_t e[2][64]; } snapshot_tab_t;
void snapshot_host_tab(const uint16_t qt[2][64], snapshot_tab_t *t);

/* The writer with a hint per block (may be NULL): hint[b] = the zigzag index of block b's last non-zero level (0: none but perhaps DC), so
 * that no block is scanned beyond it.  Otherwise mi355enc_snapshot_write. */
int snapshot_host_write(const int16_t *levels, const uint8_t *hint, const uint16_t qt[2][64], int ow, int oh, uint8_t *out, size_t cap, size_t *len);
/* blocks of a still of ow x oh (4:2:0), and where each component's first block lies (jpeg_host_layout's) */
size_t snapshot_host_blocks(int ow, int oh, int bw[3], int bh[3], size_t first[3]);

#ifdef __cplusplus
}
#endif
#endif
