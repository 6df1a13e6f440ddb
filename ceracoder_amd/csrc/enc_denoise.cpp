// enc_denoise.cpp -- temporal noise reduction of a handle (mi355enc_set_denoise): the value the control thread sets, its latch per input
// picture, the launch on the slot's coded surfaces and the handle's history, the motion-compensated form (section 25) with its second histories, and the stage entry points.  The rule itself (ranges, tables, the search's key) is denoise_host.c's,
// which needs no device.
#include "enc_internal.hpp"

#include <utility>

// a checked parameter set with its tables; off: parts 0
static void denoise_make(const mi355enc_denoise_t *d, denoise_set_t *out) {
    out->d = *d;
    out->parts = denoise_parts(d);
    (void)mi355enc_denoise_tables(d, out->tabs, out->tabs + 256, out->tabs + 512);
}

int denoise_latch(mi355enc_t *h, slot_t *s, bool own) {
    std::lock_guard<std::mutex> g(h->dn_mu);
    s->dn.d = h->dn_cur.d; s->dn.parts = h->dn_cur.parts; s->dn.range = h->dn_cur.range;
    if (own && h->dn_cur.parts) memcpy(s->dn.tabs, h->dn_cur.tabs, sizeof s->dn.tabs); // (the tables: only the slot the step runs on needs them)
    return MI355ENC_OK;
}

// what a picture with the set `n` launches, the previous picture through the step having had the strengths `prev`: a plane whose strength was 0 there has no
// valid history and primes (the luma's history follows the luma while only the chroma is filtered: the block measure reads it).  mc: the compensated form --
// a range above 0 and something filtered (the search runs whenever the block measure would)
struct denoise_form_t { int lmode, cmode; bool mc; };
static denoise_form_t denoise_form(const denoise_set_t *n, const mi355enc_denoise_t *prev) {
    denoise_form_t f;
    f.lmode = n->d.luma > 0 && prev->luma > 0; f.cmode = n->d.chroma == 0 ? 0 : prev->chroma > 0 ? 2 : 1;
    f.mc = n->range > 0 && (f.lmode == 1 || f.cmode == 2);
    return f;
}

// the in-place launch on NV12 surfaces and their histories
static int denoise_run(mi355enc_t *h, uint8_t *y, uint8_t *uv, uint16_t *hy, uint16_t *huv, const denoise_set_t *n, const denoise_form_t &f, hipStream_t st) {
    if (k_launch_denoise(y, uv, hy, huv, h->W, h->H, h->cfg.width, h->cfg.height, f.lmode, f.cmode, n->tabs, st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}

// the search of the set `n` alone: the luma against its history, into vec
static int denoise_run_search(mi355enc_t *h, const uint8_t *y, const uint16_t *hy, unsigned *vec, const denoise_set_t *n, hipStream_t st) {
    const int s = n->d.luma ? n->d.luma : n->d.chroma;
    if (k_launch_denoise_search(y, hy, vec, h->W, h->H, h->cfg.width, h->cfg.height, n->range, denoise_motion_lambda(s), st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}

// the compensated launches: the search, then the filter from the histories (hy, huv) into the other ones (ny, nuv)
static int denoise_run_mc(mi355enc_t *h, uint8_t *y, uint8_t *uv, const uint16_t *hy, const uint16_t *huv, uint16_t *ny, uint16_t *nuv, unsigned *vec, const denoise_set_t *n,
                          const denoise_form_t &f, hipStream_t st) {
    { int r = denoise_run_search(h, y, hy, vec, n, st); if (r) return r; }
    if (k_launch_denoise_mc(y, uv, hy, huv, ny, nuv, vec, h->W, h->H, h->cfg.width, h->cfg.height, f.lmode, f.cmode, n->tabs, st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}

static size_t denoise_vec_bytes(const mi355enc_t *h) { return (size_t)(h->W >> 3) * (size_t)(h->H >> 3) * sizeof(unsigned); }

template <typename T> static int denoise_need(mi355enc_t *h, T **p, size_t bytes) {
    if (*p) return MI355ENC_OK;
    HIPCHK(hipMalloc((void **)p, bytes));
    h->dn_bytes += bytes;
    return MI355ENC_OK;
}

// the buffers a launch needs, allocated by the first picture that needs them: the current histories, and for the compensated form the other ones and the vectors
static int denoise_alloc(mi355enc_t *h, const denoise_set_t *n, bool mc) {
    int r = denoise_need(h, &h->d_dn_y, 2 * h->ysz);
    if (!r && n->d.chroma > 0) r = denoise_need(h, &h->d_dn_uv, 2 * h->csz);
    if (!r && mc) r = denoise_need(h, &h->d_dn_y_alt, 2 * h->ysz);
    if (!r && mc && n->d.chroma > 0) r = denoise_need(h, &h->d_dn_uv_alt, 2 * h->csz);
    if (!r && mc) r = denoise_need(h, &h->d_dn_vec, denoise_vec_bytes(h));
    return r;
}

// a picture goes through the step with the set `n`: off, it only ends the history's validity.  The compensated form writes the other histories, which then are
// the current ones (the chroma's only when the launch wrote them); every other form runs in place on the current ones
static int denoise_step(mi355enc_t *h, slot_t *s, const denoise_set_t *n, bool prime, hipStream_t st) {
    if (!n->parts) { h->dn_prev.luma = h->dn_prev.chroma = 0; return MI355ENC_OK; }
    const mi355enc_denoise_t none = {0, 0};
    const denoise_form_t f = denoise_form(n, prime ? &none : &h->dn_prev);
    { int r = denoise_alloc(h, n, f.mc); if (r) return r; }
    int r;
    if (f.mc) {
        r = denoise_run_mc(h, s->d_src_y, s->d_src_uv, h->d_dn_y, h->d_dn_uv, h->d_dn_y_alt, h->d_dn_uv_alt, h->d_dn_vec, n, f, st);
        if (!r) { std::swap(h->d_dn_y, h->d_dn_y_alt); if (f.cmode) std::swap(h->d_dn_uv, h->d_dn_uv_alt); }
    } else r = denoise_run(h, s->d_src_y, s->d_src_uv, h->d_dn_y, h->d_dn_uv, n, f, st);
    if (!r) h->dn_prev = n->d;
    return r;
}

int denoise_draw(mi355enc_t *h, slot_t *s, hipStream_t st) { return denoise_step(h, s, &s->dn, false, st); }

void denoise_collected(mi355enc_t *h, slot_t *s) {
    h->dn_last_have = true;
    h->dn_last.d = s->dn.d; h->dn_last.parts = s->dn.parts; h->dn_last.range = s->dn.range;
}

bool denoise_time_ready(mi355enc_t *h, int stage) {
    std::lock_guard<std::mutex> g(h->dn_mu);
    return h->dn_cur.parts != 0 && (stage < 27 || h->dn_cur.range > 0);
}
int denoise_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x) {
    const int stage = x->stage;
    denoise_set_t set;
    { std::lock_guard<std::mutex> g(h->dn_mu); set = h->dn_cur; }
    if (stage < 27) set.range = 0; // (the in-place forms)
    if (stage != 27 || (h->dn_prev.luma == 0 && h->dn_prev.chroma == 0)) return denoise_step(h, s, &set, stage == 26, h->stream); // (27 without a valid history: this launch primes)
    { int r = denoise_alloc(h, &set, true); if (r) return r; }
    return denoise_run_search(h, s->d_src_y, h->d_dn_y, h->d_dn_vec, &set, h->stream);
}

void denoise_time_done(mi355enc_t *h) { h->dn_prev.luma = h->dn_prev.chroma = 0; }

void denoise_free(mi355enc_t *h) {
    if (h->d_dn_y) (void)hipFree(h->d_dn_y);
    if (h->d_dn_uv) (void)hipFree(h->d_dn_uv);
    if (h->d_dn_y_alt) (void)hipFree(h->d_dn_y_alt);
    if (h->d_dn_uv_alt) (void)hipFree(h->d_dn_uv_alt);
    if (h->d_dn_vec) (void)hipFree(h->d_dn_vec);
    h->d_dn_y = h->d_dn_uv = h->d_dn_y_alt = h->d_dn_uv_alt = nullptr; h->d_dn_vec = nullptr; h->dn_bytes = 0;
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
    set.range = h->dn_cur.range; // (the range is set on its own)
    h->dn_cur = set;
    return MI355ENC_OK;
}

int mi355enc_set_denoise_motion(mi355enc_t *h, int range) {
    if (!h || range < 0 || range > MI355ENC_DENOISE_MOTION_MAX) return MI355ENC_ERR_ARG;
    std::lock_guard<std::mutex> g(h->dn_mu);
    h->dn_cur.range = range;
    return MI355ENC_OK;
}

int mi355enc_get_denoise_motion(const mi355enc_t *h, int *range) {
    if (!h || !range) return MI355ENC_ERR_ARG;
    mi355enc_t *m = const_cast<mi355enc_t *>(h);
    std::lock_guard<std::mutex> g(m->dn_mu);
    *range = h->dn_cur.range;
    return MI355ENC_OK;
}

int mi355enc_last_denoise_motion(mi355enc_t *h, int *range) {
    if (!h || !range) return MI355ENC_ERR_ARG;
    if (!h->dn_last_have) return MI355ENC_ERR_STATE;
    *range = h->dn_last.range;
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

int mi355enc_stage_denoise_mc(mi355enc_t *h, const mi355enc_denoise_t *d, int range, const uint16_t *hist_y, const uint16_t *hist_uv, uint8_t *y, uint8_t *uv,
                              uint16_t *hist_y_out, uint16_t *hist_uv_out, uint32_t *vec_out) {
    if (!h || !y || !uv || mi355enc_denoise_check(d) || (hist_uv && !hist_y)) return MI355ENC_ERR_ARG; // (a chroma history is filtered by a measure, which reads the luma's)
    if (range < 0 || range > MI355ENC_DENOISE_MOTION_MAX) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; }
    denoise_set_t set;
    denoise_make(d, &set);
    set.range = range;
    slot_t *s = &h->slot[0];
    const size_t vb = denoise_vec_bytes(h);
    if (vec_out) memset(vec_out, 0, vb);
    { int r = stage_in(h, s, y, uv); if (r) return r; }
    if (!set.parts) return stage_out(h, s, y, uv);
    // what the previous picture must have had for these histories to be valid: the luma's was filtered (d->luma > 0) or followed (the chroma's was filtered)
    const mi355enc_denoise_t prev = {hist_y && d->luma > 0 ? d->luma : 0, hist_uv ? d->chroma : 0};
    const denoise_form_t f = denoise_form(&set, &prev);
    // histories of the call's own: the handle's are its stream's.  The compensated form writes second ones
    stage_tmp_t thy(h->stream), thuv(h->stream), tny(h->stream), tnuv(h->stream), tvec(h->stream);
    if (thy.alloc(2 * h->ysz) || (d->chroma > 0 && thuv.alloc(2 * h->csz))) return MI355ENC_ERR_HIP;
    if (f.mc && (tny.alloc(2 * h->ysz) || tvec.alloc(vb) || (d->chroma > 0 && tnuv.alloc(2 * h->csz)))) return MI355ENC_ERR_HIP;
    uint16_t *hy = thy.as<uint16_t>(), *huv = thuv.as<uint16_t>(), *ny = tny.as<uint16_t>(), *nuv = tnuv.as<uint16_t>();
    unsigned *vec = tvec.as<unsigned>();
    if (hist_y) HIPCHK(hipMemcpyAsync(hy, hist_y, 2 * h->ysz, hipMemcpyHostToDevice, h->stream));
    if (hist_uv && huv) HIPCHK(hipMemcpyAsync(huv, hist_uv, 2 * h->csz, hipMemcpyHostToDevice, h->stream));
    int r = f.mc ? denoise_run_mc(h, s->d_src_y, s->d_src_uv, hy, huv, ny, nuv, vec, &set, f, h->stream) : denoise_run(h, s->d_src_y, s->d_src_uv, hy, huv, &set, f, h->stream);
    if (!r) r = stage_out(h, s, y, uv); // (waits for the main stream)
    if (r) return r;
    const uint16_t *oy = f.mc ? ny : hy, *ouv = f.mc ? nuv : huv;
    if (hist_y_out) HIPCHK(hipMemcpy(hist_y_out, oy, 2 * h->ysz, hipMemcpyDeviceToHost));
    if (hist_uv_out && ouv) HIPCHK(hipMemcpy(hist_uv_out, ouv, 2 * h->csz, hipMemcpyDeviceToHost));
    if (vec_out && vec) HIPCHK(hipMemcpy(vec_out, vec, vb, hipMemcpyDeviceToHost));
    return MI355ENC_OK;
}

int mi355enc_stage_denoise(mi355enc_t *h, const mi355enc_denoise_t *d, const uint16_t *hist_y, const uint16_t *hist_uv, uint8_t *y, uint8_t *uv,
                           uint16_t *hist_y_out, uint16_t *hist_uv_out) {
    return mi355enc_stage_denoise_mc(h, d, 0, hist_y, hist_uv, y, uv, hist_y_out, hist_uv_out, nullptr);
}

int mi355enc_stage_denoise_search(mi355enc_t *h, const mi355enc_denoise_t *d, int range, const uint8_t *y, const uint16_t *hist_y, uint32_t *vec_out) {
    if (!h || !y || !hist_y || !vec_out || mi355enc_denoise_check(d) || !denoise_parts(d) || range < 1 || range > MI355ENC_DENOISE_MOTION_MAX) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; }
    denoise_set_t set;
    denoise_make(d, &set);
    set.range = range;
    slot_t *s = &h->slot[0];
    HIPCHK(hipMemcpyAsync(s->d_src_y, y, h->ysz, hipMemcpyHostToDevice, h->stream));
    const size_t vb = denoise_vec_bytes(h);
    stage_tmp_t thy(h->stream), tvec(h->stream);
    if (thy.alloc(2 * h->ysz) || tvec.alloc(vb)) return MI355ENC_ERR_HIP;
    HIPCHK(hipMemcpyAsync(thy.p, hist_y, 2 * h->ysz, hipMemcpyHostToDevice, h->stream));
    int r = denoise_run_search(h, s->d_src_y, thy.as<uint16_t>(), tvec.as<unsigned>(), &set, h->stream);
    if (r) return r;
    HIPCHK(hipMemcpyAsync(vec_out, tvec.p, vb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}

size_t mi355enc_debug_denoise_bytes(const mi355enc_t *h) { return h ? h->dn_bytes : 0; }

} // extern "C"
