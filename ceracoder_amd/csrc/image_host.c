/* image_host.c -- host-only part of the image layers: the Netpbm PAM (P7) reader behind the element's image-location
 * property.  Plain C with no dependency on the device code: csrc/san_image_driver.c runs it under ASan + UBSan on truncated and damaged files. */
#include "../../include/mi355enc.h"

#include <string.h>

/* one header line [p, e): its first word against `key`; on a match *val points behind the blanks that follow the word */
static int pam_key(const uint8_t *p, const uint8_t *e, const char *key, const uint8_t **val) {
    const size_t n = strlen(key);
    if ((size_t)(e - p) < n || memcmp(p, key, n) != 0) return 0;
    p += n;
    if (p < e && *p != ' ' && *p != '\t') return 0;
    while (p < e && (*p == ' ' || *p == '\t')) p++;
    *val = p;
    return 1;
}
/* a decimal number that fills [p, e) but for trailing blanks; -1: none, or above 99999 */
static long pam_number(const uint8_t *p, const uint8_t *e) {
    long v = 0;
    int digits = 0;
    while (p < e && *p >= '0' && *p <= '9' && digits < 6) { v = v * 10 + (*p - '0'); p++; digits++; }
    while (p < e && (*p == ' ' || *p == '\t' || *p == '\r')) p++;
    return digits && digits < 6 && p == e ? v : -1;
}

int mi355enc_image_load_pam(const uint8_t *data, size_t len, int *w, int *h, uint8_t *rgba, size_t cap) {
    if (!data || !w || !h || len < 3 || memcmp(data, "P7\n", 3) != 0) return MI355ENC_ERR_ARG;
    long width = -1, height = -1, depth = -1, maxval = -1;
    int tuple = 0; /* 3 RGB, 4 RGB_ALPHA */
    size_t o = 3;
    int ended = 0;
    while (!ended) {
        const uint8_t *p = data + o, *nl = (const uint8_t *)memchr(p, '\n', len - o), *val;
        if (!nl) return MI355ENC_ERR_ARG; /* (no ENDHDR line) */
        const uint8_t *e = nl;
        o = (size_t)(nl - data) + 1;
        while (p < e && (*p == ' ' || *p == '\t')) p++;
        if (p == e || *p == '#') continue;
        if (pam_key(p, e, "ENDHDR", &val)) ended = 1;
        else if (pam_key(p, e, "WIDTH", &val)) { if (width >= 0 || (width = pam_number(val, e)) < 0) return MI355ENC_ERR_ARG; }
        else if (pam_key(p, e, "HEIGHT", &val)) { if (height >= 0 || (height = pam_number(val, e)) < 0) return MI355ENC_ERR_ARG; }
        else if (pam_key(p, e, "DEPTH", &val)) { if (depth >= 0 || (depth = pam_number(val, e)) < 0) return MI355ENC_ERR_ARG; }
        else if (pam_key(p, e, "MAXVAL", &val)) { if (maxval >= 0 || (maxval = pam_number(val, e)) < 0) return MI355ENC_ERR_ARG; }
        else if (pam_key(p, e, "TUPLTYPE", &val)) {
            const uint8_t *t = e;
            while (t > val && (t[-1] == ' ' || t[-1] == '\t' || t[-1] == '\r')) t--;
            if (tuple) return MI355ENC_ERR_ARG;
            if (t - val == 9 && memcmp(val, "RGB_ALPHA", 9) == 0) tuple = 4;
            else if (t - val == 3 && memcmp(val, "RGB", 3) == 0) tuple = 3;
            else return MI355ENC_ERR_ARG;
        } else return MI355ENC_ERR_ARG;
    }
    if (width < 1 || width > MI355ENC_IMAGE_MAX_DIM || height < 1 || height > MI355ENC_IMAGE_MAX_DIM || maxval != 255 || !tuple || depth != tuple) return MI355ENC_ERR_ARG;
    const size_t npix = (size_t)width * (size_t)height;
    if (len - o < npix * (size_t)tuple) return MI355ENC_ERR_ARG; /* truncated */
    *w = (int)width; *h = (int)height;
    if (!rgba) return MI355ENC_OK;
    if (cap < npix * 4) return MI355ENC_ERR_OVERFLOW;
    const uint8_t *s = data + o;
    if (tuple == 4) memcpy(rgba, s, npix * 4);
    else for (size_t i = 0; i < npix; i++) { rgba[4 * i] = s[3 * i]; rgba[4 * i + 1] = s[3 * i + 1]; rgba[4 * i + 2] = s[3 * i + 2]; rgba[4 * i + 3] = 255; }
    return MI355ENC_OK;
}
