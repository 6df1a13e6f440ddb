// enc_rate.cpp -- frame-rate conversion of a handle: the setter, the plan's step for a submit and its commit, the keep buffer, the mix /
// keep / repeat launches that ingest_end (enc_input.cpp) strings together, statistics, and the entry point that exposes the kernel to tests.  The rule itself is
// host C (rate_host.c).
#include "enc_internal.hpp"
#include "rate_host.h"

static uint8_t *keep_y(const mi355enc_t *h) { return h->d_keep; }
static uint8_t *keep_uv(const mi355enc_t *h) { return h->d_keep + h->ysz; } // (ysz is a multiple of 256: aligned like the surfaces)

void rate_free(mi355enc_t *h) {
    if (h->d_keep) (void)hipFree(h->d_keep);
    h->d_keep = nullptr;
}

int rate_begin(mi355enc_t *h, int64_t pts, int force_idr, int *ahead) {
    mi355enc_rate_plan_t next = h->rate_plan;
    int n = 0, resync = 0;
    if (mi355enc_rate_plan_step(&next, pts, &n, h->rate_pts, h->rate_w, &resync)) return MI355ENC_ERR_ARG;
    const int need = n > 0 ? n : h->rate.mode == 2 ? 1 : 0; // (blend: an input that yields no picture still passes through a slot on its way to the keep buffer)
    if (h->pending + need > h->cfg.pipeline_depth + 1) return MI355ENC_ERR_STATE;
    h->rate_next = next; h->rate_n = n; h->rate_resync = resync;
    if (!need) { rate_commit(h, force_idr); return INGEST_DROP; }
    *ahead = n > 0 ? n - 1 : 0;
    return MI355ENC_OK;
}

void rate_commit(mi355enc_t *h, int force_idr) {
    mi355enc_rate_stats_t *st = &h->rate_st;
    const int n = h->rate_n;
    h->rate_plan = h->rate_next;
    st->in++; st->out += (uint64_t)n; st->resyncs += (uint64_t)h->rate_resync;
    if (!n) { st->dropped++; h->rate_idr_owed |= force_idr != 0; }
    else {
        h->rate_idr_owed = 0;
        if (h->rate.mode == 1) st->repeated += (uint64_t)(n - 1);
        else for (int i = 0; i < n; i++) st->blended += h->rate_w[i] > 0 && h->rate_w[i] < 256;
    }
    h->last_count = n;
}

int rate_keep(mi355enc_t *h, slot_t *s, hipStream_t st) {
    if (!h->d_keep) return MI355ENC_OK;
    HIPCHK(hipMemcpyAsync(keep_y(h), s->d_src_y, h->ysz, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(keep_uv(h), s->d_src_uv, h->csz, hipMemcpyDeviceToDevice, st));
    return MI355ENC_OK;
}
int rate_repeat(mi355enc_t *h, slot_t *t, hipStream_t st) {
    if (!h->d_keep) return MI355ENC_ERR_STATE;
    HIPCHK(hipMemcpyAsync(t->d_src_y, keep_y(h), h->ysz, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(t->d_src_uv, keep_uv(h), h->csz, hipMemcpyDeviceToDevice, st));
    return MI355ENC_OK;
}
int rate_mix(mi355enc_t *h, slot_t *b, slot_t *out, int w256, bool keep, hipStream_t st) {
    if (!h->d_keep || (keep && out != b)) return MI355ENC_ERR_STATE;
    if (k_launch_rate_mix(keep_y(h), keep_uv(h), b->d_src_y, b->d_src_uv, out->d_src_y, out->d_src_uv, keep ? keep_y(h) : nullptr, keep ? keep_uv(h) : nullptr,
                          h->W, h->H, w256, st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}

extern "C" {

int mi355enc_set_rate_conversion(mi355enc_t *h, const mi355enc_rate_t *r) {
    if (!h || mi355enc_rate_check(r)) return MI355ENC_ERR_ARG;
    if (h->n_submitted || h->rate_st.in) return MI355ENC_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    rate_free(h);
    h->rate = *r;
    if (h->rate.max_fill > h->cfg.pipeline_depth) h->rate.max_fill = h->cfg.pipeline_depth; // a submit that yields n pictures takes n slots
    h->rate_idr_owed = 0; h->rate_n = 0;
    memset(&h->rate_st, 0, sizeof h->rate_st);
    mi355enc_rate_plan_init(&h->rate_plan, h->rate.mode, h->rate.pts_per_second, h->cfg.fps_num, h->cfg.fps_den, h->rate.max_fill, 0, -1);
    if (h->rate.mode == 2 || (h->rate.mode == 1 && h->rate.max_fill > 0)) {
        HIPCHK(hipMalloc((void **)&h->d_keep, h->ysz + h->csz));
        HIPCHK(hipMemset(h->d_keep, 0, h->ysz + h->csz)); // (the first picture's mix has w = 256: whatever a holds does not show, but it is read)
        HIPCHK(hipStreamSynchronize(nullptr));            // the fill runs on the null stream, which the handle's streams do not wait for: through before the first launch that touches the buffer is enqueued
    }
    return MI355ENC_OK;
}

int mi355enc_rate_peek(const mi355enc_t *h, int64_t pts) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!h->rate.mode) return 1;
    mi355enc_rate_plan_t p = h->rate_plan;
    int n = 0, resync = 0, w[MI355ENC_RATE_MAX_OUT];
    int64_t t[MI355ENC_RATE_MAX_OUT];
    const int r = mi355enc_rate_plan_step(&p, pts, &n, t, w, &resync);
    return r ? r : n;
}

int mi355enc_last_submit_count(const mi355enc_t *h) { return h ? h->last_count : 0; }

int mi355enc_rate_stats(mi355enc_t *h, mi355enc_rate_stats_t *st) {
    if (!h || !st) return MI355ENC_ERR_ARG;
    if (!h->rate.mode) return MI355ENC_ERR_STATE;
    *st = h->rate_st;
    return MI355ENC_OK;
}

size_t mi355enc_debug_rate_bytes(const mi355enc_t *h) { return h && h->d_keep ? h->ysz + h->csz : 0; }

// The launch as the encoder enqueues it for a submit's last tick: a in slot 0's surfaces (standing in for the keep buffer), b in slot 1's, the mix in place into
// slot 1 while b goes where a was.
int mi355enc_stage_rate(mi355enc_t *h, int w256, const uint8_t *a_y, const uint8_t *a_uv, const uint8_t *b_y, const uint8_t *b_uv, uint8_t *out_y, uint8_t *out_uv) {
    if (!h || !a_y || !a_uv || !b_y || !b_uv || !out_y || !out_uv || w256 < 0 || w256 > 256) return MI355ENC_ERR_ARG;
    slot_t *sa = &h->slot[0], *sb = &h->slot[1];
    int r = stage_enter(h);
    if (!r) r = stage_in(h, sa, a_y, a_uv);
    if (!r) r = stage_in(h, sb, b_y, b_uv);
    if (r) return r;
    if (k_launch_rate_mix(sa->d_src_y, sa->d_src_uv, sb->d_src_y, sb->d_src_uv, sb->d_src_y, sb->d_src_uv, sa->d_src_y, sa->d_src_uv, h->W, h->H, w256, h->stream))
        return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return stage_out(h, sb, out_y, out_uv);
}

} // extern "C"
