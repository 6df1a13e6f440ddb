/* jpeg_host.c -- the host half of MJPEG input.
 *
 * A baseline JPEG picture (SOF0 / SOF1, 8 bit, Huffman coded, one interleaved scan; grey, 4:2:0, 4:2:2 or 4:4:4) is parsed and its
 * entropy-coded segment decoded into dense blocks of 64 int16 in natural (row-major) order, per component the blocks of the MCU-padded
 * plane in raster order.  The quantisation tables are handed over beside them, not applied: dequantisation, the inverse DCT and the way to
 * NV12 are the device's (k_jpeg.hip).  Everything else is refused (MI355ENC_ERR_ARG), as is every picture whose entropy-coded data does
 * not decode: the decoder never reads past `len` and never writes outside the coefficient buffer.
 *
 * The Huffman decoder is table driven: nine bits of lookahead resolve every code of up to nine bits in one step, longer codes walk the
 * maxcode ladder of ITU-T T.81 F.2.2.3.  A picture without a DHT segment (AVI1-style MJPEG from UVC cameras) uses the typical tables of
 * T.81 Annex K.3. */
#include "jpeg_host.h"

#include <string.h>

#include "jpeg_tables.h"

/* ---------------------------------------------------------------- marker parser */
typedef struct {
    mi355enc_jpeg_info_t info;
    int tq[3], td[3], ta[3];           /* per component: quantisation / DC / AC table index */
    uint8_t qt[4][64];                 /* as sent: zigzag order */
    uint8_t have_qt[4], have_h[2][4];
    uint8_t hbits[2][4][16];
    uint8_t hvals[2][4][256];
    size_t scan;                       /* first byte of the entropy-coded segment */
} jhdr_t;

static int be16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

static int jpeg_parse(const uint8_t *d, size_t len, jhdr_t *h) {
    memset(h, 0, sizeof *h);
    if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) return MI355ENC_ERR_ARG;
    size_t pos = 2;
    int have_sof = 0, id[3] = {0, 0, 0};
    for (;;) {
        if (pos >= len || d[pos] != 0xFF) return MI355ENC_ERR_ARG;
        while (pos < len && d[pos] == 0xFF) pos++; /* fill bytes */
        if (pos >= len) return MI355ENC_ERR_ARG;
        const int m = d[pos++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return MI355ENC_ERR_ARG; /* nothing without a length belongs in front of the scan */
        if (pos + 2 > len) return MI355ENC_ERR_ARG;
        const size_t L = (size_t)be16(d + pos);
        if (L < 2 || pos + L > len) return MI355ENC_ERR_ARG;
        const uint8_t *seg = d + pos + 2;
        size_t n = L - 2;
        pos += L;
        if (m == 0xC0 || m == 0xC1) {
            if (have_sof || n < 6 || seg[0] != 8) return MI355ENC_ERR_ARG; /* (12-bit: refused) */
            const int nf = seg[5];
            if ((nf != 1 && nf != 3) || n != (size_t)(6 + 3 * nf)) return MI355ENC_ERR_ARG;
            h->info.height = be16(seg + 1); h->info.width = be16(seg + 3); h->info.components = nf;
            if (h->info.width < 1 || h->info.height < 1) return MI355ENC_ERR_ARG;
            int hv[3] = {0x11, 0x11, 0x11};
            for (int c = 0; c < nf; c++) { id[c] = seg[6 + 3 * c]; hv[c] = seg[7 + 3 * c]; h->tq[c] = seg[8 + 3 * c]; if (h->tq[c] > 3) return MI355ENC_ERR_ARG; }
            h->info.hs = h->info.vs = 1; /* (a single component: its sampling factors mean nothing, the MCU is one block) */
            if (nf == 3) {
                if (hv[1] != 0x11 || hv[2] != 0x11 || (hv[0] != 0x22 && hv[0] != 0x21 && hv[0] != 0x11)) return MI355ENC_ERR_ARG;
                h->info.hs = hv[0] >> 4; h->info.vs = hv[0] & 15;
            }
            have_sof = 1;
        } else if ((m >= 0xC2 && m <= 0xCF) && m != 0xC4) return MI355ENC_ERR_ARG; /* progressive, lossless, arithmetic, differential, DAC */
        else if (m == 0xC4) {
            while (n) {
                if (n < 17) return MI355ENC_ERR_ARG;
                const int tc = seg[0] >> 4, th = seg[0] & 15;
                if (tc > 1 || th > 3) return MI355ENC_ERR_ARG;
                size_t cnt = 0;
                for (int i = 0; i < 16; i++) cnt += seg[1 + i];
                if (cnt > 256 || n < 17 + cnt) return MI355ENC_ERR_ARG;
                memcpy(h->hbits[tc][th], seg + 1, 16);
                memcpy(h->hvals[tc][th], seg + 17, cnt);
                h->have_h[tc][th] = 1; h->info.has_dht = 1;
                seg += 17 + cnt; n -= 17 + cnt;
            }
        } else if (m == 0xDB) {
            while (n) {
                if (n < 65 || (seg[0] >> 4) != 0 || (seg[0] & 15) > 3) return MI355ENC_ERR_ARG; /* (16-bit tables: refused) */
                memcpy(h->qt[seg[0] & 15], seg + 1, 64);
                h->have_qt[seg[0] & 15] = 1;
                seg += 65; n -= 65;
            }
        } else if (m == 0xDD) {
            if (n != 2) return MI355ENC_ERR_ARG;
            h->info.restart_interval = be16(seg);
        } else if (m == 0xDA) {
            if (!have_sof || n < 1) return MI355ENC_ERR_ARG;
            const int ns = seg[0];
            if (ns != h->info.components || n != (size_t)(1 + 2 * ns + 3)) return MI355ENC_ERR_ARG; /* (a scan of fewer components: not interleaved) */
            for (int c = 0; c < ns; c++) {
                if (seg[1 + 2 * c] != id[c]) return MI355ENC_ERR_ARG;
                h->td[c] = seg[2 + 2 * c] >> 4; h->ta[c] = seg[2 + 2 * c] & 15;
                if (h->td[c] > 3 || h->ta[c] > 3) return MI355ENC_ERR_ARG;
            }
            const uint8_t *t = seg + 1 + 2 * ns;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return MI355ENC_ERR_ARG;
            h->scan = pos;
            break;
        }
        /* APPn, COM and anything else with a length: skipped */
    }
    for (int c = 0; c < h->info.components; c++) {
        if (!h->have_qt[h->tq[c]]) return MI355ENC_ERR_ARG;
        if (h->info.has_dht) { if (!h->have_h[0][h->td[c]] || !h->have_h[1][h->ta[c]]) return MI355ENC_ERR_ARG; }
        else if (h->td[c] > 1 || h->ta[c] > 1) return MI355ENC_ERR_ARG; /* the typical tables: 0 luminance, 1 chrominance */
    }
    return MI355ENC_OK;
}

size_t jpeg_host_layout(const mi355enc_jpeg_info_t *info, int bw[3], int bh[3], size_t first[3]) {
    const int mcux = (info->width + 8 * info->hs - 1) / (8 * info->hs), mcuy = (info->height + 8 * info->vs - 1) / (8 * info->vs);
    size_t n = 0;
    for (int c = 0; c < 3; c++) {
        bw[c] = bh[c] = 0; first[c] = n;
        if (c >= info->components) continue;
        bw[c] = mcux * (c ? 1 : info->hs); bh[c] = mcuy * (c ? 1 : info->vs);
        n += (size_t)bw[c] * (size_t)bh[c];
    }
    return n;
}

/* ---------------------------------------------------------------- Huffman tables */
#define LOOK_BITS 9
typedef struct {
    uint16_t look[1 << LOOK_BITS]; /* length << 8 | symbol for codes of up to LOOK_BITS bits; 0: longer */
    int maxcode[17], mincode[17], valptr[17], nvals;
    uint8_t vals[256];
} htab_t;

static int htab_build(htab_t *t, const uint8_t bits[16], const uint8_t *vals) {
    memset(t->look, 0, sizeof t->look);
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {
        const int cnt = bits[l - 1];
        t->valptr[l] = k; t->mincode[l] = (int)code; t->maxcode[l] = cnt ? (int)code + cnt - 1 : -1;
        if (code + (unsigned)cnt > (1u << l)) return MI355ENC_ERR_ARG; /* more codes than the length has */
        for (int i = 0; i < cnt; i++, k++, code++) {
            if (k >= 256) return MI355ENC_ERR_ARG;
            t->vals[k] = vals[k];
            if (l <= LOOK_BITS) {
                const unsigned first = code << (LOOK_BITS - l);
                for (unsigned j = 0; j < (1u << (LOOK_BITS - l)); j++) t->look[first + j] = (uint16_t)((l << 8) | vals[k]);
            }
        }
        code <<= 1;
    }
    t->nvals = k;
    return MI355ENC_OK;
}

/* ---------------------------------------------------------------- bit reader: stops in front of a marker and at `end`; what it hands out beyond that are zero
 * bits that it counts, and a decoder that consumes one of them has run out of data (bad) */
typedef struct { const uint8_t *p, *end; uint64_t acc; int n, fake, stopped, bad; } br_t;

static void br_fill(br_t *b) {
    while (b->n <= 56) {
        unsigned byte = 0;
        if (!b->stopped) {
            if (b->p < b->end && *b->p != 0xFF) byte = *b->p++;
            else if (b->end - b->p > 1 && b->p[1] == 0x00) { byte = 0xFF; b->p += 2; } /* a stuffed 0xFF */
            else b->stopped = 1;
        }
        if (b->stopped && b->fake < 128) b->fake += 8;
        b->acc = (b->acc << 8) | byte;
        b->n += 8;
    }
}
static inline void br_skip(br_t *b, int k) { b->n -= k; if (b->n < b->fake) b->bad = 1; }
static inline int br_get(br_t *b, int k) { /* 1 <= k <= 16 */
    if (b->n < k) br_fill(b);
    const int v = (int)((b->acc >> (b->n - k)) & ((1u << k) - 1u));
    br_skip(b, k);
    return v;
}
static inline int br_extend(br_t *b, int s) { /* T.81 F.2.2.1: s more bits as a signed value */
    const int v = br_get(b, s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}
static inline int huff_decode(br_t *b, const htab_t *t) {
    if (b->n < 16) br_fill(b);
    const unsigned v = (unsigned)((b->acc >> (b->n - 16)) & 0xFFFFu);
    const unsigned e = t->look[v >> (16 - LOOK_BITS)];
    if (e) { br_skip(b, (int)(e >> 8)); return (int)(e & 255u); }
    for (int l = LOOK_BITS + 1; l <= 16; l++) {
        const int code = (int)(v >> (16 - l));
        if (code <= t->maxcode[l]) {
            const int i = t->valptr[l] + code - t->mincode[l];
            if (i < 0 || i >= t->nvals) return -1;
            br_skip(b, l);
            return t->vals[i];
        }
    }
    return -1; /* no such code */
}

static int decode_block(br_t *b, const htab_t *dc, const htab_t *ac, int *pred, int16_t *blk) {
    int s = huff_decode(b, dc);
    if (s < 0 || s > 11) return MI355ENC_ERR_ARG;
    const int v = *pred + (s ? br_extend(b, s) : 0);
    if (v < -32768 || v > 32767) return MI355ENC_ERR_ARG;
    *pred = v;
    blk[0] = (int16_t)v;
    for (int k = 1; k < 64;) {
        const int rs = huff_decode(b, ac);
        if (rs < 0) return MI355ENC_ERR_ARG;
        const int r = rs >> 4;
        s = rs & 15;
        if (!s) {
            if (r != 15) break; /* end of block */
            k += 16;
            if (k > 64) return MI355ENC_ERR_ARG;
            continue;
        }
        if (s > 10) return MI355ENC_ERR_ARG;
        k += r;
        if (k > 63) return MI355ENC_ERR_ARG; /* a run past coefficient 63 */
        blk[k_natural[k]] = (int16_t)br_extend(b, s);
        k++;
    }
    return b->bad ? MI355ENC_ERR_ARG : MI355ENC_OK;
}

static int jpeg_decode(const uint8_t *d, size_t len, const jhdr_t *h, int16_t *coef) {
    htab_t tab[2][4];
    uint8_t built[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    const int nc = h->info.components;
    for (int c = 0; c < nc; c++)
        for (int cl = 0; cl < 2; cl++) {
            const int i = cl ? h->ta[c] : h->td[c];
            if (built[cl][i]) continue;
            const int r = h->info.has_dht ? htab_build(&tab[cl][i], h->hbits[cl][i], h->hvals[cl][i])
                                          : htab_build(&tab[cl][i], k_std_bits[cl][i], cl ? k_std_ac_vals[i] : k_std_dc_vals);
            if (r) return r;
            built[cl][i] = 1;
        }
    int bw[3], bh[3];
    size_t first[3];
    const size_t nblk = jpeg_host_layout(&h->info, bw, bh, first);
    memset(coef, 0, nblk * 64 * sizeof(int16_t));
    const int mcux = bw[0] / h->info.hs, mcuy = bh[0] / h->info.vs, ri = h->info.restart_interval;
    br_t b = {d + h->scan, d + len, 0, 0, 0, 0, 0};
    int pred[3] = {0, 0, 0}, left = ri, rst = 0;
    for (int my = 0; my < mcuy; my++)
        for (int mx = 0; mx < mcux; mx++) {
            if (ri && left == 0) { /* the interval is over: to the byte boundary, then RSTn in sequence */
                const uint8_t *p = b.p;
                if (p >= b.end || *p != 0xFF) return MI355ENC_ERR_ARG;
                while (p < b.end && *p == 0xFF) p++;
                if (p >= b.end || *p != 0xD0 + (rst & 7)) return MI355ENC_ERR_ARG;
                rst++;
                b.p = p + 1; b.acc = 0; b.n = 0; b.fake = 0; b.stopped = 0;
                pred[0] = pred[1] = pred[2] = 0;
                left = ri;
            }
            left--;
            for (int c = 0; c < nc; c++) {
                const int hc = c ? 1 : h->info.hs, vc = c ? 1 : h->info.vs;
                for (int j = 0; j < vc; j++)
                    for (int i = 0; i < hc; i++) {
                        int16_t *blk = coef + (first[c] + (size_t)(my * vc + j) * (size_t)bw[c] + (size_t)(mx * hc + i)) * 64;
                        const int r = decode_block(&b, &tab[0][h->td[c]], &tab[1][h->ta[c]], &pred[c], blk);
                        if (r) return r;
                    }
            }
        }
    return MI355ENC_OK;
}

/* ---------------------------------------------------------------- public entry points (host only) */
int mi355enc_jpeg_info(const uint8_t *data, size_t len, mi355enc_jpeg_info_t *info) {
    if (!data || !info) return MI355ENC_ERR_ARG;
    jhdr_t h;
    const int r = jpeg_parse(data, len, &h);
    if (r) return r;
    *info = h.info;
    return MI355ENC_OK;
}

int mi355enc_jpeg_entropy_decode(const uint8_t *data, size_t len, int16_t *coef, size_t coef_cap, uint16_t qt[3][64], mi355enc_jpeg_info_t *info) {
    if (!data || !coef || !qt) return MI355ENC_ERR_ARG;
    jhdr_t h;
    int r = jpeg_parse(data, len, &h);
    if (r) return r;
    int bw[3], bh[3];
    size_t first[3];
    const size_t nblk = jpeg_host_layout(&h.info, bw, bh, first);
    if (nblk > coef_cap / 64) return MI355ENC_ERR_OVERFLOW;
    r = jpeg_decode(data, len, &h, coef);
    if (r) return r;
    memset(qt, 0, 3 * 64 * sizeof(uint16_t));
    for (int c = 0; c < h.info.components; c++)
        for (int k = 0; k < 64; k++) qt[c][k_natural[k]] = h.qt[h.tq[c]][k];
    if (info) *info = h.info;
    return MI355ENC_OK;
}
