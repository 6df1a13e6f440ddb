// enc_mask.cpp -- the privacy masks of a handle (mi355enc_set_mask): the configuration the control thread sets, its latch per output
// picture, the handle's result surface and ping-pong planes, the launches on the slot's coded surfaces, the probe and the timed stages.  The rule itself is
// mask_host.h's and mask_host.c's, which need no device.
#include "enc_internal.hpp"

void mask_free(mi355enc_t *h) { // (mi355enc_close: nothing sets any more)
    if (h->d_mask) (void)hipFree(h->d_mask);
    h->d_mask = nullptr; h->mask_bytes = 0;
}

// the result surface and the two ping-pong planes, a coded picture each, in one allocation (a picture is a multiple of 16 bytes): by the first masked picture
static size_t mask_plane(const mi355enc_t *h) { return (size_t)h->W * h->H * 3 / 2; }
static int mask_alloc(mi355enc_t *h) {
    if (h->d_mask) return MI355ENC_OK;
    HIPCHK(hipMalloc((void **)&h->d_mask, 3 * mask_plane(h)));
    h->mask_bytes = 3 * mask_plane(h);
    return MI355ENC_OK;
}

// rule 4's matrix: the one RGB input and the image layers are converted with (a matrix code RGB cannot be converted with counts as unspecified: by the picture's size)
static void mask_coef(const mi355enc_t *h, int32_t coef[10]) {
    if (h->csc_ok) { for (int i = 0; i < 10; i++) coef[i] = h->csc_coef[i]; return; }
    (void)mi355enc_csc_coefficients((h->cfg.width > 1024 || h->cfg.height > 576) ? 1 : 6, h->col_full, coef);
}

static bool mask_any(const mi355enc_t *h, const mi355enc_mask_t *cfg) { // some region reaches the visible picture
    mask_tab_t t;
    int32_t coef[10];
    mask_coef(h, coef);
    if (mask_resolve(cfg, coef, h->cfg.width, h->cfg.height, &t)) return false;
    for (int k = 0; k < t.n; k++) if (!mask_empty(&t.r[k])) return true;
    return false;
}

// The value set last becomes the slot's: every picture that is drawn latches its own (with frame-rate conversion every output picture).  A configuration none
// of whose regions reaches the picture is carried and reported, and launches nothing.
int mask_latch(mi355enc_t *h, slot_t *s, bool) {
    s->mask_on = false; s->mask_gen = 0; s->mask.n = 0;
    if (!h->mask_set) return MI355ENC_OK; // (only ever set to true, under the lock: a handle that never called the setter takes no lock per picture)
    {
        std::lock_guard<std::mutex> g(h->mask_mu);
        if (!h->mask_on) return MI355ENC_OK;
        s->mask = h->mask_cur; s->mask_gen = h->mask_gen;
    }
    s->mask_on = mask_any(h, &s->mask);
    return s->mask_on ? mask_alloc(h) : MI355ENC_OK;
}

// the launches on surfaces of the coded size
static int mask_run(mi355enc_t *h, slot_t *s, const mi355enc_mask_t *cfg, int parts, hipStream_t st) {
    mask_tab_t t;
    int32_t coef[10];
    mask_coef(h, coef);
    if (mask_resolve(cfg, coef, h->cfg.width, h->cfg.height, &t)) return MI355ENC_ERR_ARG;
    const size_t pl = mask_plane(h);
    if (k_launch_mask(s->d_src_y, s->d_src_uv, h->W, h->H, h->cfg.width, h->cfg.height, &t, h->d_mask, h->d_mask + pl, h->d_mask + 2 * pl, pl, parts, nullptr, st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}

int mask_draw(mi355enc_t *h, slot_t *s, hipStream_t st) { // (every launch that uses the handle's three surfaces is enqueued on this one stream, picture after picture)
    return s->mask_on ? mask_run(h, s, &s->mask, 7, st) : MI355ENC_OK;
}

void mask_collected(mi355enc_t *h, slot_t *s) {
    h->mask_last_have = true;
    h->mask_last = s->mask; h->mask_last_gen = s->mask_gen;
}

// mi355enc_time_stage 38 (the pixelate launch and the commit launch, which is also the fill) and 39 (the blur launches): the value set last holds such a region
static bool mask_has(const mi355enc_mask_t &c, int stage) {
    for (int k = 0; k < c.n; k++) if (stage == 39 ? c.region[k].mode == MASK_MODE_BLUR : c.region[k].mode != MASK_MODE_BLUR) return true;
    return false;
}
bool mask_time_ready(mi355enc_t *h, int stage) { std::lock_guard<std::mutex> g(h->mask_mu); return h->mask_on && mask_has(h->mask_cur, stage); }
int mask_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *x) {
    { std::lock_guard<std::mutex> g(h->mask_mu); if (!h->mask_on || !mask_has(h->mask_cur, x->stage)) return MI355ENC_ERR_STATE; s->mask = h->mask_cur; }
    return mask_alloc(h);
}
int mask_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x) { return mask_run(h, s, &s->mask, x->stage == 39 ? 2 : 5, h->stream); }

extern "C" {

int mi355enc_set_mask(mi355enc_t *h, const mi355enc_mask_t *cfg) {
    if (!h) return MI355ENC_ERR_ARG;
    if (cfg && mi355enc_mask_check(cfg)) return MI355ENC_ERR_ARG; // (checked in the caller's thread, outside the lock)
    std::lock_guard<std::mutex> g(h->mask_mu);
    if (!cfg || cfg->n == 0) { h->mask_on = false; h->mask_cur.n = 0; }
    else { h->mask_cur = *cfg; h->mask_on = true; h->mask_gen++; }
    h->mask_set = true;
    return MI355ENC_OK;
}

int mi355enc_get_mask(const mi355enc_t *h, int *on, mi355enc_mask_t *cfg) {
    if (!h) return MI355ENC_ERR_ARG;
    mi355enc_t *m = const_cast<mi355enc_t *>(h);
    std::lock_guard<std::mutex> g(m->mask_mu);
    if (on) *on = h->mask_on ? 1 : 0;
    if (cfg) *cfg = h->mask_cur;
    return MI355ENC_OK;
}

int mi355enc_last_mask(mi355enc_t *h, mi355enc_mask_t *cfg, unsigned *generation) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!h->mask_last_have) return MI355ENC_ERR_STATE;
    if (cfg) *cfg = h->mask_last;
    if (generation) *generation = h->mask_last_gen;
    return MI355ENC_OK;
}

size_t mi355enc_debug_mask_bytes(const mi355enc_t *h) { return h ? h->mask_bytes : 0; }

int mi355enc_mask_probe(mi355enc_t *h, const mi355enc_mask_t *cfg, uint8_t *y, uint8_t *uv) {
    if (!h || !y || !uv || mi355enc_mask_check(cfg)) return MI355ENC_ERR_ARG;
    slot_t *s = &h->slot[0];
    { int r = stage_enter(h); if (r) return r; }
    { int r = mask_alloc(h); if (r) return r; }
    int r = stage_in(h, s, y, uv);
    if (!r) r = mask_run(h, s, cfg, 7, h->stream);
    return r ? r : stage_out(h, s, y, uv);
}

} // extern "C"
