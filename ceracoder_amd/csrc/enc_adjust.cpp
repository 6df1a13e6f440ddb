// enc_adjust.cpp -- picture controls of a handle (mi355enc_set_adjust): the value the control thread sets, its latch per input picture,
// the two launch forms on the slot's coded surfaces with the scratch luma plane of the stencil form, and the stage entry point.  The rule itself (ranges, luma
// table, chroma rotation) is adjust_host.c's, which needs no device.
#include "enc_internal.hpp"

// a checked parameter set with its tables for the handle's output range; neutral: parts 0
static void adjust_make(const mi355enc_t *h, const mi355enc_adjust_t *a, adjust_set_t *out) {
    out->a = *a;
    out->parts = adjust_parts(a);
    (void)mi355enc_adjust_tables(a, h->col_full, out->luma, out->chroma);
}

int adjust_latch(mi355enc_t *h, slot_t *s, bool) {
    std::lock_guard<std::mutex> g(h->adj_mu);
    if (h->adj_cur.parts) s->adj = h->adj_cur;
    else { s->adj.parts = 0; mi355enc_adjust_default(&s->adj.a); }
    return MI355ENC_OK;
}

void adjust_retable(mi355enc_t *h) {
    std::lock_guard<std::mutex> g(h->adj_mu);
    if (h->adj_cur.parts) adjust_make(h, &h->adj_cur.a, &h->adj_cur);
}

// the set `a` on the slot's coded surfaces: the picture part (yuv_rect) in place, the border keeps its bytes
static int adjust_run(mi355enc_t *h, slot_t *s, const adjust_set_t *a, hipStream_t st) {
    if (!a->parts) return MI355ENC_OK;
    int rect[4];
    yuv_rect(h, rect);
    const uint8_t *luma = (a->parts & ADJUST_LUMA) ? a->luma : nullptr;
    const int *chroma = (a->parts & ADJUST_CHROMA) ? a->chroma : nullptr;
    if (!(a->parts & ADJUST_SHARPEN)) { // pointwise: one launch, only the planes that change
        if (k_launch_adjust(s->d_src_y, s->d_src_uv, h->W, h->H, rect, luma, chroma, st)) return MI355ENC_ERR_ARG;
        HIPCHK(hipGetLastError());
        return MI355ENC_OK;
    }
    // stencil: chroma through the pointwise form; luma (table on the way in, none where it is neutral) into the scratch plane.  Where the rectangle is the whole
    // surface the launch has written every byte of it, and the slot and the handle exchange planes (ping-pong: the plane the slot gives up was last read by
    // this launch, and the next launch that writes it follows on the same stream); under a geometry the border has to keep its bytes, and the rectangle is
    // copied back instead.  (The scratch plane is a luma surface like a slot's, SURF_PAD included.)
    if (!h->d_adj) { HIPCHK(hipMalloc((void **)&h->d_adj, h->ysz + SURF_PAD)); h->adj_bytes = h->ysz; }
    if (chroma && k_launch_adjust(s->d_src_y, s->d_src_uv, h->W, h->H, rect, nullptr, chroma, st)) return MI355ENC_ERR_ARG;
    if (k_launch_adjust_sharpen(s->d_src_y, h->d_adj, h->W, h->H, h->cfg.width, h->cfg.height, rect, luma, a->a.sharpen, a->a.sharpen_threshold, st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    const size_t at = (size_t)rect[2] * h->W + rect[0];
    if (rect[0] == 0 && rect[1] == h->W && rect[2] == 0 && rect[3] == h->H) { uint8_t *t = s->d_src_y; s->d_src_y = h->d_adj; h->d_adj = t; }
    else HIPCHK(hipMemcpy2DAsync(s->d_src_y + at, h->W, h->d_adj + at, h->W, (size_t)(rect[1] - rect[0]), (size_t)(rect[3] - rect[2]), hipMemcpyDeviceToDevice, st));
    return MI355ENC_OK;
}

int adjust_draw(mi355enc_t *h, slot_t *s, hipStream_t st) { return adjust_run(h, s, &s->adj, st); }

void adjust_collected(mi355enc_t *h, slot_t *s) {
    h->adj_last_have = true;
    h->adj_last.a = s->adj.a; h->adj_last.parts = s->adj.parts;
}

bool adjust_time_ready(mi355enc_t *h, int stage) {
    std::lock_guard<std::mutex> g(h->adj_mu);
    return h->adj_cur.parts && !(h->adj_cur.parts & ADJUST_SHARPEN) == (stage != 24);
}
int adjust_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *) {
    adjust_set_t set;
    { std::lock_guard<std::mutex> g(h->adj_mu); set = h->adj_cur; }
    return adjust_run(h, s, &set, h->stream);
}

void adjust_free(mi355enc_t *h) {
    if (h->d_adj) (void)hipFree(h->d_adj);
    h->d_adj = nullptr; h->adj_bytes = 0;
}

extern "C" {

int mi355enc_set_adjust(mi355enc_t *h, const mi355enc_adjust_t *a) {
    if (!h) return MI355ENC_ERR_ARG;
    mi355enc_adjust_t n;
    mi355enc_adjust_default(&n);
    if (!a) a = &n;
    if (mi355enc_adjust_check(a)) return MI355ENC_ERR_ARG;
    adjust_set_t set;
    adjust_make(h, a, &set); // (in the caller's thread, outside the lock)
    std::lock_guard<std::mutex> g(h->adj_mu);
    h->adj_cur = set;
    return MI355ENC_OK;
}

int mi355enc_get_adjust(const mi355enc_t *h, mi355enc_adjust_t *a) {
    if (!h || !a) return MI355ENC_ERR_ARG;
    mi355enc_t *m = const_cast<mi355enc_t *>(h);
    std::lock_guard<std::mutex> g(m->adj_mu);
    if (h->adj_cur.parts) *a = h->adj_cur.a; else mi355enc_adjust_default(a);
    return MI355ENC_OK;
}

int mi355enc_last_adjust(mi355enc_t *h, mi355enc_adjust_t *a) {
    if (!h || !a) return MI355ENC_ERR_ARG;
    if (!h->adj_last_have) return MI355ENC_ERR_STATE;
    *a = h->adj_last.a;
    return MI355ENC_OK;
}

int mi355enc_stage_adjust(mi355enc_t *h, const mi355enc_adjust_t *a, uint8_t *y, uint8_t *uv) {
    if (!h || !y || !uv || mi355enc_adjust_check(a)) return MI355ENC_ERR_ARG;
    adjust_set_t set;
    adjust_make(h, a, &set);
    slot_t *s = &h->slot[0];
    int r = stage_enter(h);
    if (!r) r = stage_in(h, s, y, uv);
    if (!r) r = adjust_run(h, s, &set, h->stream);
    return r ? r : stage_out(h, s, y, uv);
}

size_t mi355enc_debug_adjust_bytes(const mi355enc_t *h) { return h ? h->adj_bytes : 0; }

} // extern "C"
