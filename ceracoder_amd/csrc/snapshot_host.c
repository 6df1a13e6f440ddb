/* snapshot_host.c -- the host half of the JPEG stills.
 *
 * The device (k_snapshot.hip) leaves a still as quantised levels: per component the blocks of its MCU-padded plane in raster order, 64 int16 each
 * in natural order -- the layout mi355enc_jpeg_entropy_decode returns.  Here: the quality scale (libjpeg's), the reciprocals the device divides
 * with, and the writer: a baseline JFIF file (SOF0, 8 bit, Y 2x2 + Cb + Cr, one interleaved scan, the typical Huffman tables of T.81 Annex K.3,
 * no restart markers).  The writer never writes outside `cap` bytes and keeps counting beyond them, so that a buffer that is too small learns
 * the size it needs. */
#include "snapshot_host.h"

#include <string.h>

#include "jpeg_host.h"
#include "jpeg_tables.h"

/* ---------------------------------------------------------------- tables */
int mi355enc_snapshot_tables(int quality, uint16_t qt[2][64]) {
    if (!qt || quality < 1 || quality > 100) return MI355ENC_ERR_ARG;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 2; c++)
        for (int k = 0; k < 64; k++) {
            int q = (k_std_quant[c][k] * scale + 50) / 100;
            qt[c][k] = (uint16_t)(q < 1 ? 1 : q > 255 ? 255 : q);
        }
    return MI355ENC_OK;
}

/* ceil(2^32 / (8 q)): with it (n * m) >> 32 == n / (8 q) as long as n * (m * 8 q - 2^32) < 2^32, and m * 8 q - 2^32 < 8 q <= 2040: every n below 2^21 */
uint32_t mi355enc_snapshot_reciprocal(int q) {
    if (q < 1 || q > 255) return 0;
    return 0xFFFFFFFFu / (uint32_t)(8 * q) + 1u;
}

void snapshot_host_tab(const uint16_t qt[2][64], snapshot_tab_t *t) {
    for (int c = 0; c < 2; c++)
        for (int k = 0; k < 64; k++) {
            const int q = qt[c][k] < 1 ? 1 : qt[c][k] > 255 ? 255 : qt[c][k];
            t->e[c][k].m = mi355enc_snapshot_reciprocal(q);
            t->e[c][k].q4 = (uint32_t)(4 * q);
        }
}

size_t snapshot_host_blocks(int ow, int oh, int bw[3], int bh[3], size_t first[3]) {
    const mi355enc_jpeg_info_t info = {ow, oh, 3, 2, 2, 0, 0};
    return jpeg_host_layout(&info, bw, bh, first);
}

/* Headers: SOI 2, APP0 18, two DQT 2 * 69, SOF0 19, four DHT 33 + 183 + 33 + 183, SOS 14 = 623 bytes, and EOI 2.  A block: its DC code (at most 11
 * bits) and 11 more, and at most 63 AC codes of at most 16 bits with 10 more each -- a ZRL or the EOB only ever stands in place of coefficients
 * that would have cost more -- 22 + 63 * 26 = 1660 bits, under 208 bytes, and byte stuffing at most doubles them. */
#define SNAP_HEADER_BYTES 623
size_t mi355enc_snapshot_max_bytes(int ow, int oh) {
    if (ow < 1 || oh < 1 || ow > 65535 || oh > 65535) return 0;
    int bw[3], bh[3];
    size_t first[3];
    return SNAP_HEADER_BYTES + 2 + 1 + snapshot_host_blocks(ow, oh, bw, bh, first) * 416;
}

/* ---------------------------------------------------------------- output: bounded, counting */
typedef struct { uint8_t *out; size_t cap, n; uint64_t acc; int bits; } bw_t;

static inline void put_byte(bw_t *b, unsigned v) { if (b->n < b->cap) b->out[b->n] = (uint8_t)v; b->n++; }
static void put_bytes(bw_t *b, const uint8_t *p, size_t n) { for (size_t i = 0; i < n; i++) put_byte(b, p[i]); }
static void put_be16(bw_t *b, unsigned v) { put_byte(b, v >> 8); put_byte(b, v & 255u); }
static inline void put_bits(bw_t *b, unsigned v, int n) { /* n <= 27 */
    b->acc = (b->acc << n) | (v & ((1u << n) - 1u));
    b->bits += n;
    while (b->bits >= 8) {
        const unsigned byte = (unsigned)(b->acc >> (b->bits - 8)) & 255u;
        put_byte(b, byte);
        if (byte == 0xFF) put_byte(b, 0);
        b->bits -= 8;
    }
}

typedef struct { uint16_t code[256]; uint8_t len[256]; } henc_t;
static void henc_build(henc_t *t, const uint8_t bits[16], const uint8_t *vals) {
    memset(t, 0, sizeof *t);
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {
        for (int i = 0; i < bits[l - 1]; i++, k++, code++) { t->code[vals[k]] = (uint16_t)code; t->len[vals[k]] = (uint8_t)l; }
        code <<= 1;
    }
}
static inline int bit_size(int v) { /* of |v| */
    unsigned a = (unsigned)(v < 0 ? -v : v);
    int s = 0;
    while (a) { s++; a >>= 1; }
    return s;
}
/* T.81 F.1.2.1: a value of size s is sent as its low s bits, a negative one after subtracting one */
static inline void put_value(bw_t *b, int v, int s) { put_bits(b, (unsigned)(v < 0 ? v - 1 : v), s); }

static int put_block(bw_t *b, const henc_t *dc, const henc_t *ac, int *pred, const int16_t *blk, int last) {
    const int d = blk[0] - *pred;
    *pred = blk[0];
    int s = bit_size(d);
    if (s > 11) return MI355ENC_ERR_ARG;
    put_bits(b, dc->code[s], dc->len[s]);
    if (s) put_value(b, d, s);
    while (last > 0 && !blk[k_natural[last]]) last--; /* (a hint is an upper bound; without one: 63) */
    int run = 0;
    for (int k = 1; k <= last; k++) {
        const int v = blk[k_natural[k]];
        if (!v) { run++; continue; }
        while (run > 15) { put_bits(b, ac->code[0xF0], ac->len[0xF0]); run -= 16; }
        s = bit_size(v);
        if (s > 10) return MI355ENC_ERR_ARG;
        put_bits(b, ac->code[(run << 4) | s], ac->len[(run << 4) | s]);
        put_value(b, v, s);
        run = 0;
    }
    if (last < 63) put_bits(b, ac->code[0], ac->len[0]);
    return MI355ENC_OK;
}

int snapshot_host_write(const int16_t *levels, const uint8_t *hint, const uint16_t qt[2][64], int ow, int oh, uint8_t *out, size_t cap, size_t *len) {
    if (!levels || !qt || !len || (!out && cap) || ow < 1 || oh < 1 || ow > 65535 || oh > 65535) return MI355ENC_ERR_ARG;
    for (int c = 0; c < 2; c++)
        for (int k = 0; k < 64; k++) if (qt[c][k] < 1 || qt[c][k] > 255) return MI355ENC_ERR_ARG;
    bw_t b = {out, cap, 0, 0, 0};
    static const uint8_t app0[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    put_byte(&b, 0xFF); put_byte(&b, 0xD8);
    put_bytes(&b, app0, sizeof app0);
    for (int c = 0; c < 2; c++) {
        put_byte(&b, 0xFF); put_byte(&b, 0xDB); put_be16(&b, 67); put_byte(&b, (unsigned)c);
        for (int k = 0; k < 64; k++) put_byte(&b, qt[c][k_natural[k]]);
    }
    put_byte(&b, 0xFF); put_byte(&b, 0xC0); put_be16(&b, 17); put_byte(&b, 8); put_be16(&b, (unsigned)oh); put_be16(&b, (unsigned)ow); put_byte(&b, 3);
    put_byte(&b, 1); put_byte(&b, 0x22); put_byte(&b, 0);
    put_byte(&b, 2); put_byte(&b, 0x11); put_byte(&b, 1);
    put_byte(&b, 3); put_byte(&b, 0x11); put_byte(&b, 1);
    henc_t he[2][2]; /* [class][index] */
    for (int i = 0; i < 2; i++)
        for (int cl = 0; cl < 2; cl++) {
            const uint8_t *vals = cl ? k_std_ac_vals[i] : k_std_dc_vals;
            unsigned cnt = 0;
            for (int l = 0; l < 16; l++) cnt += k_std_bits[cl][i][l];
            put_byte(&b, 0xFF); put_byte(&b, 0xC4); put_be16(&b, 19 + cnt); put_byte(&b, (unsigned)((cl << 4) | i));
            put_bytes(&b, k_std_bits[cl][i], 16);
            put_bytes(&b, vals, cnt);
            henc_build(&he[cl][i], k_std_bits[cl][i], vals);
        }
    static const uint8_t sos[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    put_bytes(&b, sos, sizeof sos);
    int bw[3], bh[3];
    size_t first[3];
    snapshot_host_blocks(ow, oh, bw, bh, first);
    const int mcux = bw[1], mcuy = bh[1];
    int pred[3] = {0, 0, 0};
    for (int my = 0; my < mcuy; my++)
        for (int mx = 0; mx < mcux; mx++)
            for (int c = 0; c < 3; c++) {
                const int n = c ? 1 : 2;
                for (int j = 0; j < n; j++)
                    for (int i = 0; i < n; i++) {
                        const size_t blk = first[c] + (size_t)(my * n + j) * (size_t)bw[c] + (size_t)(mx * n + i);
                        const int r = put_block(&b, &he[0][c ? 1 : 0], &he[1][c ? 1 : 0], &pred[c], levels + blk * 64, hint ? (hint[blk] & 63) : 63);
                        if (r) return r;
                    }
            }
    if (b.bits) put_bits(&b, (1u << (8 - b.bits)) - 1u, 8 - b.bits); /* 1-padding of the last byte */
    put_byte(&b, 0xFF); put_byte(&b, 0xD9);
    *len = b.n;
    return b.n > cap ? MI355ENC_ERR_OVERFLOW : MI355ENC_OK;
}

int mi355enc_snapshot_write(const int16_t *levels, const uint16_t qt[2][64], int ow, int oh, uint8_t *out, size_t cap, size_t *len) {
    return snapshot_host_write(levels, NULL, qt, ow, oh, out, cap, len);
}
