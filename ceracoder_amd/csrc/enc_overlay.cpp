// enc_overlay.cpp -- the text overlay of a handle: the text and style the control thread sets, their latch per submitted
// picture, the layout (resolved on the host, handed to the kernel by value) and the entry points that expose font and kernel to tests.
#include "enc_internal.hpp"

#include "overlay_font.h"

static const uint8_t k_font[95 * 16] = {OVERLAY_FONT_ROWS};

static bool style_ok(const mi355enc_overlay_style_t *st) {
    return st && st->halign >= 0 && st->halign <= 2 && st->valign >= 0 && st->valign <= 2 && st->xpad >= 0 && st->xpad <= 8192 && st->ypad >= 0 &&
           st->ypad <= 8192 && st->scale >= 0 && st->scale <= 8 && (st->shaded_background == 0 || st->shaded_background == 1);
}

// The layout of `len` bytes of text in a vw x vh picture inside a W x H surface.  false: nothing of the box is visible (no launch).
static bool overlay_layout(const char *text, int len, const mi355enc_overlay_style_t &st, int vw, int vh, int W, int H, overlay_args_t *a) {
    memset(a, 0, sizeof *a);
    int nl = 0, start = 0, maxlen = 0;
    for (int i = 0; i <= len; i++)
        if (i == len || text[i] == '\n') {
            a->line_end[nl++] = (uint8_t)i;
            if (i - start > maxlen) maxlen = i - start;
            start = i + 1;
        }
    memcpy(a->text, text, (size_t)len);
    const int s = st.scale ? st.scale : vh / 540 < 1 ? 1 : vh / 540 > 8 ? 8 : vh / 540;
    const int bw = 8 * s * maxlen + 2 * s, bh = 16 * s * nl + 2 * s;
    int bx = st.halign == 0 ? st.xpad : st.halign == 1 ? (vw - bw) / 2 : vw - st.xpad - bw;
    int by = st.valign == 0 ? st.ypad : st.valign == 1 ? (vh - bh) / 2 : vh - st.ypad - bh;
    bx = bx < 0 ? 0 : bx & ~1; by = by < 0 ? 0 : by & ~1;
    if (bx >= vw || by >= vh) return false;
    a->vw = vw; a->vh = vh; a->bx = bx; a->by = by; a->bw = bw; a->bh = bh;
    a->gx0 = bx; a->gy0 = by;
    a->gx1 = bx + bw >= vw ? vw : bx + bw; // (where the box reaches the last visible column / row, the margin up to W / H repeats what is drawn there)
    a->gy1 = by + bh >= vh ? vh : by + bh;
    a->W = W; a->H = H;
    a->scale = s; a->halign = st.halign; a->shaded = st.shaded_background; a->nlines = nl; a->maxlen = maxlen;
    return true;
}

int overlay_latch(mi355enc_t *h, slot_t *s, bool) {
    std::lock_guard<std::mutex> g(h->ov_mu);
    s->ov_len = h->ov_len;
    if (h->ov_len) { memcpy(s->ov_text, h->ov_text, (size_t)h->ov_len); s->ov_style = h->ov_style; }
    return MI355ENC_OK;
}

// layout and launch: `len` bytes of text into the slot's source surfaces; nothing with no text, or with none of its box visible
static int overlay_run(mi355enc_t *h, slot_t *s, const char *text, int len, const mi355enc_overlay_style_t &sty, hipStream_t st) {
    overlay_args_t a;
    if (!len || !overlay_layout(text, len, sty, h->cfg.width, h->cfg.height, h->W, h->H, &a)) return MI355ENC_OK;
    a.y = s->d_src_y; a.uv = s->d_src_uv; a.stride = h->W;
    k_launch_overlay(&a, st);
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}
int overlay_draw(mi355enc_t *h, slot_t *s, hipStream_t st) { return overlay_run(h, s, s->ov_text, s->ov_len, s->ov_style, st); }
void overlay_collected(mi355enc_t *h, slot_t *s) { h->ov_last_have = 1; h->ov_last_len = s->ov_len; if (s->ov_len) memcpy(h->ov_last, s->ov_text, (size_t)s->ov_len); }

extern "C" {

void mi355enc_overlay_default_style(mi355enc_overlay_style_t *st) {
    if (!st) return;
    st->halign = 2; st->valign = 0; st->xpad = 16; st->ypad = 16; st->scale = 0; st->shaded_background = 0;
}

int mi355enc_set_overlay_style(mi355enc_t *h, const mi355enc_overlay_style_t *st) {
    if (!h || !style_ok(st)) return MI355ENC_ERR_ARG;
    std::lock_guard<std::mutex> g(h->ov_mu);
    h->ov_style = *st;
    return MI355ENC_OK;
}

int mi355enc_set_overlay_text(mi355enc_t *h, const char *text) {
    if (!h) return MI355ENC_ERR_ARG;
    const size_t n = text ? strnlen(text, MI355ENC_OVERLAY_MAX_TEXT) : 0;
    std::lock_guard<std::mutex> g(h->ov_mu);
    if (n) memcpy(h->ov_text, text, n);
    h->ov_len = (int)n;
    return MI355ENC_OK;
}

int mi355enc_last_overlay(mi355enc_t *h, char *buf, size_t cap) {
    if (!h || (!buf && cap)) return MI355ENC_ERR_ARG;
    if (!h->ov_last_have) return MI355ENC_ERR_STATE;
    if (cap) {
        const size_t n = (size_t)h->ov_last_len < cap - 1 ? (size_t)h->ov_last_len : cap - 1;
        memcpy(buf, h->ov_last, n);
        buf[n] = 0;
    }
    return h->ov_last_len;
}

int mi355enc_overlay_glyph(int ch, uint8_t rows[16]) {
    if (ch < 0x20 || ch > 0x7E || !rows) return MI355ENC_ERR_ARG;
    memcpy(rows, k_font + (size_t)(ch - 0x20) * 16, 16);
    return MI355ENC_OK;
}

int mi355enc_stage_overlay(mi355enc_t *h, const char *text, const mi355enc_overlay_style_t *st, uint8_t *y, uint8_t *uv) {
    if (!h || !y || !uv) return MI355ENC_ERR_ARG;
    mi355enc_overlay_style_t sty;
    mi355enc_overlay_default_style(&sty);
    if (st) { if (!style_ok(st)) return MI355ENC_ERR_ARG; sty = *st; }
    slot_t *s = &h->slot[0];
    int r = stage_enter(h);
    if (!r) r = stage_in(h, s, y, uv);
    if (!r) r = overlay_run(h, s, text, text ? (int)strnlen(text, MI355ENC_OVERLAY_MAX_TEXT) : 0, sty, h->stream);
    return r ? r : stage_out(h, s, y, uv);
}

} // extern "C"
