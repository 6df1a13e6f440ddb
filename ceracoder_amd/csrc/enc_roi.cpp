// enc_roi.cpp -- region-of-interest quantisation of a handle (mi355enc_set_roi): the configuration and the map the control thread sets,
// their latch per picture, the map's way to the device, the compose launch, the stage hook and the offsets probe.  The rule itself is roi_host.h's and
// roi_host.c's, which need no device.  What the picture's schedule makes of a map is enc_schedule.cpp's: a picture with an active one is an aq_mode 1 picture
// to the plan, one without is planned and coded as if this file were not there.
#include "enc_internal.hpp"

void roi_free(mi355enc_t *h) { // (mi355enc_close: nothing sets any more; the offset sets themselves are freed with the handle's other sets)
    for (int i = 0; i < NSLOT; i++) { if (h->slot[i].h_roi) (void)hipHostFree(h->slot[i].h_roi); h->slot[i].h_roi = nullptr; }
    free(h->roi_map); free(h->roi_stage);
    h->roi_map = h->roi_stage = nullptr;
}

// The offset sets, nmb + 16 bytes each as open() makes them for aq_mode: without it they are made here, by the first picture or stage call that needs them
// (hipMalloc alone: nothing in flight reads or writes them yet)
static int roi_alloc_sets(mi355enc_t *h) {
    for (int k = 0; k < NSET; k++)
        if (!h->d_qp_off[k]) { HIPCHK(hipMalloc((void **)&h->d_qp_off[k], (size_t)h->nmb + 16)); h->roi_bytes += (size_t)h->nmb + 16; }
    return MI355ENC_OK;
}

// The map set last becomes the slot's: copied under the lock into the slot's own pinned buffer, which the compose launch reads in stream order and nothing
// touches again before the picture is collected -- a later mi355enc_set_roi writes the handle's heap copy, never this one.
int roi_latch(mi355enc_t *h, slot_t *s) {
    s->roi_on = false; s->roi_bg = 0; s->roi_sum = 0;
    if (!h->roi_set) return MI355ENC_OK; // (only ever set to true, under the lock: a handle that never called the setter takes no lock per picture)
    bool on;
    { std::lock_guard<std::mutex> g(h->roi_mu); on = h->roi_active; }
    if (!on) return MI355ENC_OK;
    { int r = roi_alloc_sets(h); if (r) return r; }
    if (!s->h_roi) HIPCHK(hipHostMalloc((void **)&s->h_roi, (size_t)h->nmb + 16, hipHostMallocDefault));
    std::lock_guard<std::mutex> g(h->roi_mu);
    if (!h->roi_active) return MI355ENC_OK; // (set off between the two locks)
    memcpy(s->h_roi, h->roi_map, (size_t)h->nmb);
    s->roi_on = true; s->roi_bg = h->roi_bg; s->roi_sum = h->roi_sum;
    return MI355ENC_OK;
}

void roi_compose(mi355enc_t *h, const slot_t *s, int set, hipStream_t st) { k_launch_roi_compose(s->h_roi, h->d_qp_off[set], h->nmb, h->cfg.aq_mode != 0, st); }

int roi_stage_ctx(mi355enc_t *h, frame_ctx_t *c) {
    c->qp_off = nullptr; // (single stages: one QP per picture ...)
    if (!h->roi_stage) return MI355ENC_OK;
    { int r = roi_alloc_sets(h); if (r) return r; } // (... or the probe's map)
    HIPCHK(hipMemcpyAsync(h->d_qp_off[0], h->roi_stage, (size_t)h->nmb, hipMemcpyHostToDevice, h->stream));
    c->qp_off = h->d_qp_off[0];
    return MI355ENC_OK;
}

void roi_collected(mi355enc_t *h, slot_t *s) {
    h->roi_last_have = true;
    h->roi_last_active = s->roi_on ? 1 : 0; h->roi_last_bg = s->roi_on ? s->roi_bg : 0; h->roi_last_sum = s->roi_on ? s->roi_sum : 0;
}

extern "C" {

int mi355enc_set_roi(mi355enc_t *h, const mi355enc_roi_t *cfg, const int8_t *user_map) {
    if (!h) return MI355ENC_ERR_ARG;
    int8_t *t = nullptr;
    int active = 0, bg = 0;
    long sum = 0;
    if (cfg || user_map) { // (computed in the caller's thread, outside the lock)
        t = (int8_t *)malloc((size_t)h->nmb);
        if (!t) return MI355ENC_ERR_NOMEM;
        const int r = mi355enc_roi_map(cfg, user_map, h->mbw, h->mbh, t, &active, &bg);
        if (r) { free(t); return r; }
        for (int m = 0; m < h->nmb; m++) sum += t[m];
    }
    int8_t *old;
    {
        std::lock_guard<std::mutex> g(h->roi_mu);
        old = h->roi_map;
        h->roi_map = t; h->roi_active = active != 0; h->roi_bg = bg; h->roi_sum = (int)sum;
        if (cfg) h->roi_cur = *cfg; else mi355enc_roi_default(&h->roi_cur);
        h->roi_set = true;
    }
    free(old);
    return MI355ENC_OK;
}

int mi355enc_get_roi(const mi355enc_t *h, int *on, mi355enc_roi_t *cfg) {
    if (!h) return MI355ENC_ERR_ARG;
    mi355enc_t *m = const_cast<mi355enc_t *>(h);
    std::lock_guard<std::mutex> g(m->roi_mu);
    if (on) *on = h->roi_map ? 1 : 0;
    if (cfg) *cfg = h->roi_cur;
    return MI355ENC_OK;
}

int mi355enc_last_roi(mi355enc_t *h, int *active, int *background, int *sum) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!h->roi_last_have) return MI355ENC_ERR_STATE;
    if (active) *active = h->roi_last_active;
    if (background) *background = h->roi_last_bg;
    if (sum) *sum = h->roi_last_sum;
    return MI355ENC_OK;
}

size_t mi355enc_debug_roi_bytes(const mi355enc_t *h) { return h ? h->roi_bytes : 0; }

int mi355enc_roi_probe_set_map(mi355enc_t *h, const int8_t *map) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!map) { free(h->roi_stage); h->roi_stage = nullptr; return MI355ENC_OK; }
    for (int m = 0; m < h->nmb; m++) if (map[m] < -ROI_DELTA_MAX || map[m] > ROI_DELTA_MAX) return MI355ENC_ERR_ARG;
    if (!h->roi_stage && !(h->roi_stage = (int8_t *)malloc((size_t)h->nmb))) return MI355ENC_ERR_NOMEM;
    memcpy(h->roi_stage, map, (size_t)h->nmb);
    return MI355ENC_OK;
}

int mi355enc_roi_probe_offsets(mi355enc_t *h, const uint8_t *src_y, int8_t *off_out) {
    if (!h || !src_y || !off_out) return MI355ENC_ERR_ARG;
    slot_t *s = &h->slot[0];
    { int r = stage_enter(h); if (r) return r; }
    { int r = roi_alloc_sets(h); if (r) return r; }
    stage_tmp_t t(h->stream);
    if (t.alloc((size_t)h->nmb + 16)) return MI355ENC_ERR_HIP;
    {   // the map set last (none, or an inactive one: zeros), through a buffer of the call's own
        std::lock_guard<std::mutex> g(h->roi_mu);
        if (h->roi_map && h->roi_active) HIPCHK(hipMemcpy(t.p, h->roi_map, (size_t)h->nmb, hipMemcpyHostToDevice));
        else HIPCHK(hipMemset(t.p, 0, (size_t)h->nmb));
    }
    HIPCHK(hipMemcpyAsync(s->d_src_y, src_y, h->ysz, hipMemcpyHostToDevice, h->stream));
    frame_ctx_t c; // (a context of the call's own: what aq_kernel reads of it, as a picture of the stream sets it)
    memset(&c, 0, sizeof c);
    c.src_y = s->d_src_y; c.src_stride = h->W; c.vis_h = h->cfg.height; c.mbw = h->mbw; c.mbh = h->mbh;
    if (h->cfg.aq_mode) k_launch_aq(&c, h->d_qp_off[0], h->stream);
    k_launch_roi_compose(t.as<int8_t>(), h->d_qp_off[0], h->nmb, h->cfg.aq_mode != 0, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(off_out, h->d_qp_off[0], (size_t)h->nmb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}

} // extern "C"
