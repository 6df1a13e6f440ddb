// enc_denoise.cpp -- temporal noise reduction of a handle (mi355enc_set_denoise): the value the control thread sets, its latch per input
// picture, the launch on the slot's coded surfaces and the handle's history, and the stage entry point.  The rule itself (ranges, tables) is denoise_host.c's,
// which needs no device.
#include "enc_internal.hpp"

// a checked parameter set with its tables; off: parts 0
static void denoise_make(const mi355enc_denoise_t *d, denoise_set_t *out) {
    out->d = *d;
    out->parts = denoise_parts(d);
    (void)mi355enc_denoise_tables(d, out->tabs, out->tabs + 256, out->tabs + 512);
}

void denoise_latch(mi355enc_t *h, slot_t *s, bool tables) {
    std::lock_guard<std::mutex> g(h->dn_mu);
    s->dn.d = h->dn_cur.d; s->dn.parts = h->dn_cur.parts;
    if (tables && h->dn_cur.parts) memcpy(s->dn.tabs, h->dn_cur.tabs, sizeof s->dn.tabs);
}

// the launch of the set `n` on NV12 surfaces and their histories, the previous picture through the step having had the strengths `prev`: a plane whose strength
// was 0 there has no valid history and primes (the luma's history follows the luma while only the chroma is filtered: the block measure reads it)
static int denoise_run(mi355enc_t *h, uint8_t *y, uint8_t *uv, uint16_t *hy, uint16_t *huv, const denoise_set_t *n, const mi355enc_denoise_t *prev, hipStream_t st) {
    const int lmode = n->d.luma > 0 && prev->luma > 0, cmode = n->d.chroma == 0 ? 0 : prev->chroma > 0 ? 2 : 1;
    if (k_launch_denoise(y, uv, hy, huv, h->W, h->H, h->cfg.width, h->cfg.height, lmode, cmode, n->tabs, st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}

// the history a set needs, allocated by the first picture that needs it
static int denoise_alloc(mi355enc_t *h, const denoise_set_t *n) {
    if (!h->d_dn_y) { HIPCHK(hipMalloc((void **)&h->d_dn_y, 2 * h->ysz)); h->dn_bytes += 2 * h->ysz; }
    if (n->d.chroma > 0 && !h->d_dn_uv) { HIPCHK(hipMalloc((void **)&h->d_dn_uv, 2 * h->csz)); h->dn_bytes += 2 * h->csz; }
    return MI355ENC_OK;
}

// a picture goes through the step with the set `n`: off, it only ends the history's validity
static int denoise_step(mi355enc_t *h, slot_t *s, const denoise_set_t *n, bool prime, hipStream_t st) {
    if (!n->parts) { h->dn_prev.luma = h->dn_prev.chroma = 0; return MI355ENC_OK; }
    { int r = denoise_alloc(h, n); if (r) return r; }
    const mi355enc_denoise_t none = {0, 0};
    int r = denoise_run(h, s->d_src_y, s->d_src_uv, h->d_dn_y, h->d_dn_uv, n, prime ? &none : &h->dn_prev, st);
    if (!r) h->dn_prev = n->d;
    return r;
}

int denoise_draw(mi355enc_t *h, slot_t *s, hipStream_t st) { return denoise_step(h, s, &s->dn, false, st); }

void denoise_collected(mi355enc_t *h, slot_t *s) {
    h->dn_last_have = true;
    h->dn_last.d = s->dn.d; h->dn_last.parts = s->dn.parts;
}

bool denoise_time_ready(mi355enc_t *h) {
    std::lock_guard<std::mutex> g(h->dn_mu);
    return h->dn_cur.parts != 0;
}
int denoise_time_launch(mi355enc_t *h, slot_t *s, bool prime) {
    denoise_set_t set;
    { std::lock_guard<std::mutex> g(h->dn_mu); set = h->dn_cur; }
    return denoise_step(h, s, &set, prime, h->stream);
}

void denoise_time_done(mi355enc_t *h) { h->dn_prev.luma = h->dn_prev.chroma = 0; }

void denoise_free(mi355enc_t *h) {
    if (h->d_dn_y) (void)hipFree(h->d_dn_y);
    if (h->d_dn_uv) (void)hipFree(h->d_dn_uv);
    h->d_dn_y = h->d_dn_uv = nullptr; h->dn_bytes = 0;
}

extern "C" {

int mi355enc_set_denoise(mi355enc_t *h, const mi355enc_denoise_t *d) {
    if (!h) return MI355ENC_ERR_ARG;
    mi355enc_denoise_t n;
    mi355enc_denoise_default(&n);
    if (!d) d = &n;
    if (mi355enc_denoise_check(d)) return MI355ENC_ERR_ARG;
    denoise_set_t set;
    denoise_make(d, &set); // (in the caller's thread, outside the lock)
    std::lock_guard<std::mutex> g(h->dn_mu);
    h->dn_cur = set;
    return MI355ENC_OK;
}

int mi355enc_get_denoise(const mi355enc_t *h, mi355enc_denoise_t *d) {
    if (!h || !d) return MI355ENC_ERR_ARG;
    mi355enc_t *m = const_cast<mi355enc_t *>(h);
    std::lock_guard<std::mutex> g(m->dn_mu);
    *d = h->dn_cur.d;
    return MI355ENC_OK;
}

int mi355enc_last_denoise(mi355enc_t *h, mi355enc_denoise_t *d) {
    if (!h || !d) return MI355ENC_ERR_ARG;
    if (!h->dn_last_have) return MI355ENC_ERR_STATE;
    *d = h->dn_last.d;
    return MI355ENC_OK;
}

int mi355enc_stage_denoise(mi355enc_t *h, const mi355enc_denoise_t *d, const uint16_t *hist_y, const uint16_t *hist_uv, uint8_t *y, uint8_t *uv,
                           uint16_t *hist_y_out, uint16_t *hist_uv_out) {
    if (!h || !y || !uv || mi355enc_denoise_check(d) || (hist_uv && !hist_y)) return MI355ENC_ERR_ARG; // (a chroma history is filtered by a measure, which reads the luma's)
    if (h->pending) return MI355ENC_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    { int r = sync_compute(h); if (r) return r; }
    denoise_set_t set;
    denoise_make(d, &set);
    slot_t *s = &h->slot[0];
    HIPCHK(hipMemcpyAsync(s->d_src_y, y, h->ysz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(s->d_src_uv, uv, h->csz, hipMemcpyHostToDevice, h->stream));
    if (!set.parts) return stage_out(h, s, y, uv);
    // histories of the call's own: the handle's are its stream's
    uint16_t *hy = nullptr, *huv = nullptr;
    int r = MI355ENC_OK;
    if (hipMalloc((void **)&hy, 2 * h->ysz) != hipSuccess || (d->chroma > 0 && hipMalloc((void **)&huv, 2 * h->csz) != hipSuccess)) r = MI355ENC_ERR_HIP;
    if (!r && hist_y && hipMemcpyAsync(hy, hist_y, 2 * h->ysz, hipMemcpyHostToDevice, h->stream) != hipSuccess) r = MI355ENC_ERR_HIP;
    if (!r && hist_uv && huv && hipMemcpyAsync(huv, hist_uv, 2 * h->csz, hipMemcpyHostToDevice, h->stream) != hipSuccess) r = MI355ENC_ERR_HIP;
    // what the previous picture must have had for these histories to be valid: the luma's was filtered (d->luma > 0) or followed (the chroma's was filtered)
    const mi355enc_denoise_t prev = {hist_y && d->luma > 0 ? d->luma : 0, hist_uv ? d->chroma : 0};
    if (!r) r = denoise_run(h, s->d_src_y, s->d_src_uv, hy, huv, &set, &prev, h->stream);
    if (!r) r = stage_out(h, s, y, uv); // (waits for the main stream)
    if (!r && hist_y_out && hipMemcpy(hist_y_out, hy, 2 * h->ysz, hipMemcpyDeviceToHost) != hipSuccess) r = MI355ENC_ERR_HIP;
    if (!r && hist_uv_out && huv && hipMemcpy(hist_uv_out, huv, 2 * h->csz, hipMemcpyDeviceToHost) != hipSuccess) r = MI355ENC_ERR_HIP;
    if (r) (void)hipStreamSynchronize(h->stream);
    if (hy) (void)hipFree(hy);
    if (huv) (void)hipFree(huv);
    return r;
}

size_t mi355enc_debug_denoise_bytes(const mi355enc_t *h) { return h ? h->dn_bytes : 0; }

} // extern "C"
