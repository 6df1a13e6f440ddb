// enc_lut3d.cpp -- the 3D colour LUT of a handle (mi355enc_set_lut3d): the setting and the table the control thread sets, their latch per
// input picture, the table's way to the device, the launch on the slot's coded surfaces, the probe and the timed stage.  The rule itself is lut3d_host.h's and
// lut3d_host.c's, which need no device.
#include "enc_internal.hpp"

// room for the largest table, in words (a multiple of four: the staged form copies 16 bytes at a time, and never beyond the table's own last whole group)
#define LUT3D_WORDS_MAX ((LUT3D_N_MAX * LUT3D_N_MAX * LUT3D_N_MAX + 3) & ~3)
static size_t lut3d_words(int N) { return (size_t)N * N * N; }

void lut3d_free(mi355enc_t *h) {
    if (h->d_lut) (void)hipFree(h->d_lut);
    if (h->h_lut) (void)hipHostFree(h->h_lut);
    h->d_lut = h->h_lut = nullptr; h->lut_bytes = 0; h->lut_sent = 0;
}
void lut3d_close(mi355enc_t *h) { // (mi355enc_close: nothing sets any more)
    lut3d_free(h);
    free(h->lut_nodes);
    h->lut_nodes = nullptr;
}

// the table on the device and one pinned copy of a table per slot, for 65^3 nodes whatever the size set: allocated by the first graded picture
static int lut3d_alloc(mi355enc_t *h) {
    if (h->d_lut) return MI355ENC_OK;
    const size_t bytes = (size_t)LUT3D_WORDS_MAX * sizeof(uint32_t);
    if (hipMalloc((void **)&h->d_lut, bytes) != hipSuccess || hipHostMalloc((void **)&h->h_lut, bytes * NSLOT, hipHostMallocDefault) != hipSuccess) {
        lut3d_free(h);
        return MI355ENC_ERR_HIP;
    }
    h->lut_bytes = bytes;
    return MI355ENC_OK;
}

// the output's matrix and range as the colour step resolves them (unspecified: by the picture's size); a matrix RGB cannot be converted with counts as that too
static void lut3d_coef(const mi355enc_t *h, int32_t coef[LUT3D_COEF_WORDS]) {
    const int by_size = (h->cfg.width > 1024 || h->cfg.height > 576) ? 1 : 6;
    if (mi355enc_lut3d_coefficients(h->col_mat != 2 ? h->col_mat : by_size, h->col_full, coef)) (void)mi355enc_lut3d_coefficients(by_size, h->col_full, coef);
}

// The value set last becomes the slot's.  own (the slot the input goes into): where its generation is not the one the device table holds -- or will hold, by the
// order of the upload stream -- the table is copied, under the lock, into the slot's pinned copy, which nothing touches again before the picture is collected.
int lut3d_latch(mi355enc_t *h, slot_t *s, bool own) {
    s->lut_send = false;
    bool on;
    { std::lock_guard<std::mutex> g(h->lut_mu); on = h->lut_on && h->lut_cur.strength > 0; }
    if (own && on) { int r = lut3d_alloc(h); if (r) return r; }
    std::lock_guard<std::mutex> g(h->lut_mu);
    s->lut_on = h->lut_on && h->lut_cur.strength > 0 && (!own || h->d_lut); // (set on between the two locks: this picture is not graded yet)
    s->lut = h->lut_cur;
    s->lut_gen = s->lut_on ? h->lut_gen : 0;
    if (!own || !s->lut_on) return MI355ENC_OK; // (a rate-conversion tick only reports: the input is graded once, in its own slot)
    lut3d_coef(h, s->lut_coef);
    if (s->lut_gen != h->lut_sent) {
        memcpy(h->h_lut + (size_t)LUT3D_WORDS_MAX * (s - h->slot), h->lut_nodes, lut3d_words(s->lut.size) * sizeof(uint32_t));
        s->lut_send = true;
    }
    return MI355ENC_OK;
}

// the launch on surfaces of the coded size, inside the picture rectangle, in place
static int lut3d_run(mi355enc_t *h, slot_t *s, const mi355enc_lut3d_t *set, const int32_t *coef, const uint32_t *d_nodes, int form, hipStream_t st) {
    int rect[4]; // the picture part; the launch grades its visible samples and, where it reaches the visible edge, writes the coded padding as their replica: a quad's
    yuv_rect(h, rect); // chroma comes from its own four samples, so padding graded as samples would be no replica of the graded picture
    if (k_launch_lut3d(s->d_src_y, s->d_src_uv, h->W, h->H, h->cfg.width, h->cfg.height, rect, d_nodes, set->size, set->strength, coef, form < 0 ? mi355enc_lut3d_plan(set->size) : form, st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}

int lut3d_draw(mi355enc_t *h, slot_t *s, hipStream_t st) {
    if (!s->lut_on) return MI355ENC_OK;
    if (s->lut_send) { // (every LUT launch of the stream and every transfer of a table is enqueued on this one stream: pictures in flight keep the table they latched)
        HIPCHK(hipMemcpyAsync(h->d_lut, h->h_lut + (size_t)LUT3D_WORDS_MAX * (s - h->slot), lut3d_words(s->lut.size) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        h->lut_sent = s->lut_gen; s->lut_send = false;
    }
    return lut3d_run(h, s, &s->lut, s->lut_coef, h->d_lut, h->lut_form, st);
}

void lut3d_collected(mi355enc_t *h, slot_t *s) {
    h->lut_last_have = true;
    h->lut_last_gen = s->lut_on ? s->lut_gen : 0;
    if (s->lut_on) h->lut_last = s->lut; else h->lut_last = {0, 0};
}

bool lut3d_time_ready(mi355enc_t *h, int) { std::lock_guard<std::mutex> g(h->lut_mu); return h->lut_on && h->lut_cur.strength > 0; }
int lut3d_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *) { // the table set last, through slot 0's pinned copy, on the main stream
    { int r = lut3d_alloc(h); if (r) return r; }
    {
        std::lock_guard<std::mutex> g(h->lut_mu);
        if (!h->lut_on || h->lut_cur.strength <= 0) return MI355ENC_ERR_STATE;
        s->lut = h->lut_cur;
        memcpy(h->h_lut, h->lut_nodes, lut3d_words(s->lut.size) * sizeof(uint32_t));
    }
    lut3d_coef(h, s->lut_coef);
    HIPCHK(hipMemcpyAsync(h->d_lut, h->h_lut, lut3d_words(s->lut.size) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    return MI355ENC_OK;
}
int lut3d_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *) { return lut3d_run(h, s, &s->lut, s->lut_coef, h->d_lut, h->lut_form, h->stream); }
void lut3d_time_done(mi355enc_t *h) { h->lut_sent = 0; } // (the next graded picture sends its table again, on its own stream)

extern "C" {

int mi355enc_set_lut3d(mi355enc_t *h, const mi355enc_lut3d_t *set, const uint32_t *nodes) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!set) { std::lock_guard<std::mutex> g(h->lut_mu); h->lut_on = false; return MI355ENC_OK; }
    if (set->strength < 0 || set->strength > 256 || mi355enc_lut3d_check(nodes, set->size)) return MI355ENC_ERR_ARG;
    uint32_t *copy = (uint32_t *)malloc(lut3d_words(set->size) * sizeof(uint32_t)); // (copied in the caller's thread, outside the lock)
    if (!copy) return MI355ENC_ERR_NOMEM;
    memcpy(copy, nodes, lut3d_words(set->size) * sizeof(uint32_t));
    std::lock_guard<std::mutex> g(h->lut_mu);
    free(h->lut_nodes);
    h->lut_nodes = copy; h->lut_cur = *set; h->lut_on = true; h->lut_gen++;
    return MI355ENC_OK;
}

int mi355enc_get_lut3d(const mi355enc_t *h, int *on, mi355enc_lut3d_t *set) {
    if (!h) return MI355ENC_ERR_ARG;
    mi355enc_t *m = const_cast<mi355enc_t *>(h);
    std::lock_guard<std::mutex> g(m->lut_mu);
    if (on) *on = h->lut_on ? 1 : 0;
    if (set && h->lut_on) *set = h->lut_cur;
    return MI355ENC_OK;
}

int mi355enc_last_lut3d(mi355enc_t *h, mi355enc_lut3d_t *set, unsigned *generation) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!h->lut_last_have) return MI355ENC_ERR_STATE;
    if (set) *set = h->lut_last;
    if (generation) *generation = h->lut_last_gen;
    return MI355ENC_OK;
}

size_t mi355enc_debug_lut3d_bytes(const mi355enc_t *h) { return h ? h->lut_bytes : 0; }

int mi355enc_debug_lut3d_form(mi355enc_t *h, int form) {
    if (!h || form < -1 || form > 1) return MI355ENC_ERR_ARG;
    h->lut_form = form;
    return MI355ENC_OK;
}

int mi355enc_lut3d_probe(mi355enc_t *h, const mi355enc_lut3d_t *set, const uint32_t *nodes, uint8_t *y, uint8_t *uv, int form) {
    if (!h || !set || !y || !uv || set->strength < 1 || set->strength > 256 || form < -1 || form > 1 || mi355enc_lut3d_check(nodes, set->size)) return MI355ENC_ERR_ARG;
    if (form == 1 && set->size > LUT3D_STAGED_FIT) return MI355ENC_ERR_ARG; // (in front of any HIP call: nothing is launched)
    slot_t *s = &h->slot[0];
    int32_t coef[LUT3D_COEF_WORDS];
    lut3d_coef(h, coef);
    { int r = stage_enter(h); if (r) return r; }
    stage_tmp_t t(h->stream);
    if (t.alloc((size_t)LUT3D_WORDS_MAX * sizeof(uint32_t))) return MI355ENC_ERR_HIP;
    HIPCHK(hipMemcpyAsync(t.p, nodes, lut3d_words(set->size) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    int r = stage_in(h, s, y, uv);
    if (!r) r = lut3d_run(h, s, set, coef, t.as<uint32_t>(), form, h->stream);
    return r ? r : stage_out(h, s, y, uv);
}

} // extern "C"
