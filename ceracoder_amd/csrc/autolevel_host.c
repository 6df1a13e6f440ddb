/* autolevel_host.c -- the rule of automatic levels and white balance on the host: setting and decision as the ABI exposes them
 * (mi355enc_autolevel_*).  The kernels of k_autolevel.hip compute the same numbers; tests/autolevelref.py restates them in numpy. */
#include "autolevel_host.h"

#include <stddef.h>

#include "../../include/mi355enc.h"

void mi355enc_autolevel_default(mi355enc_autolevel_t *a) {
    if (!a) return;
    a->levels = 0; a->balance = 0; a->speed = 16; a->clip_low = 50; a->clip_high = 50; a->max_gain = 2000; a->reach = 48;
}

int mi355enc_autolevel_check(const mi355enc_autolevel_t *a) {
    if (!a || a->levels < 0 || a->levels > 1000 || a->balance < 0 || a->balance > 1000 || a->speed < 1 || a->speed > 256) return MI355ENC_ERR_ARG;
    if (a->clip_low < 0 || a->clip_low > 2000 || a->clip_high < 0 || a->clip_high > 2000 || a->max_gain < 1000 || a->max_gain > 8000 || a->reach < 0 || a->reach > 127) return MI355ENC_ERR_ARG;
    return MI355ENC_OK;
}

int mi355enc_autolevel_decide(const mi355enc_autolevel_meas_t *m, const mi355enc_autolevel_t *a, int full_range, int prime, int32_t state[4],
                              mi355enc_autolevel_info_t *info, uint8_t table[256]) {
    if (!m || !state || !info || !table || mi355enc_autolevel_check(a)) return MI355ENC_ERR_ARG;
    if (m->chroma > (1u << 24) || m->voters > m->chroma || m->su > 255ull * m->voters || m->sv > 255ull * m->voters) return MI355ENC_ERR_ARG;
    if (!prime && (state[0] < 0 || state[0] > 65280 || state[1] < 0 || state[1] > 65280 || state[2] < -32768 || state[2] > 32767 || state[3] < -32768 || state[3] > 32767)) return MI355ENC_ERR_ARG;
    uint64_t N = 0;
    for (int v = 0; v < 256; v++) N += m->hist[v];
    if (N > (1ull << 26)) return MI355ENC_ERR_ARG;
    const int B = al_black(full_range), S = al_scale(full_range);
    int lo = 255, hi = 0;
    uint64_t cum = 0;
    for (int v = 0; v < 256; v++) {
        if (al_is_hi(cum, N, a->clip_high)) hi = v; /* (cum is cum(v - 1) here) */
        cum += m->hist[v];
        if (lo == 255 && al_is_lo(cum, N, a->clip_low)) lo = v;
    }
    const int set[7] = {a->levels, a->balance, a->speed, a->clip_low, a->clip_high, a->max_gain, a->reach};
    int st[4] = {state[0], state[1], state[2], state[3]}, rec[AL_REC_WORDS];
    const al_interval_t iv = al_decide(lo, hi, m->voters, m->su, m->sv, m->chroma, set, B, S, prime ? 1 : 0, st, rec);
    for (int i = 0; i < 4; i++) state[i] = st[i];
    info->lo = rec[0]; info->hi = rec[1]; info->voters = rec[2]; info->du = rec[3]; info->dv = rec[4];
    info->s_lo = rec[5]; info->s_hi = rec[6]; info->s_du = rec[7]; info->s_dv = rec[8];
    info->off_u = rec[9]; info->off_v = rec[10]; info->valid = rec[11];
    for (int v = 0; v < 256; v++) table[v] = (uint8_t)al_table(v, iv, B, S);
    return MI355ENC_OK;
}
