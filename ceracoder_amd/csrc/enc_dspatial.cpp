// enc_dspatial.cpp -- the spatial noise filter of a handle and its noise estimate (mi355enc_set_denoise_spatial): the value the control
// thread sets, its latch per input picture, the launches on the slot's coded surfaces with the handle's device block and scratch planes, the device probes, the
// stage entry point and the timed stages.  The rule itself is dspatial_host.h's and dspatial_host.c's, which need no device.
#include "enc_internal.hpp"

#include <vector>

// the handle's block: the state X (and seven words of room), NSLOT + 1 records (the last one: the stage calls'), the slabs, the 33 tables R_s
#define DS_STATE_WORDS 8
#define DS_TAB_WORDS (64 * (DS_MAX + 1))
static int *ds_slot(mi355enc_t *h, int i) { return h->d_ds + DS_STATE_WORDS + DS_REC_WORDS * i; }
static unsigned *ds_slabs(mi355enc_t *h) { return (unsigned *)(h->d_ds + DS_STATE_WORDS + DS_REC_WORDS * (NSLOT + 1)); }
static uint8_t *ds_tabs(mi355enc_t *h) { return (uint8_t *)(ds_slabs(h) + (size_t)DS_SLAB_WORDS * DS_SLABS_MAX); }
static bool ds_auto(const mi355enc_denoise_spatial_t *a) { return a->auto_gain > 0; }
static bool ds_filters(const mi355enc_denoise_spatial_t *a) { return a->luma > 0 || a->chroma > 0; }
static bool ds_active(const mi355enc_denoise_spatial_t *a) { return ds_auto(a) || ds_filters(a); }

void dspatial_free(mi355enc_t *h) {
    if (h->d_ds) (void)hipFree(h->d_ds);
    if (h->h_ds) (void)hipHostFree(h->h_ds);
    if (h->d_ds_y) (void)hipFree(h->d_ds_y);
    if (h->d_ds_uv) (void)hipFree(h->d_ds_uv);
    h->d_ds = h->h_ds = nullptr; h->d_ds_y = h->d_ds_uv = nullptr; h->ds_bytes = 0; h->ds_primed = false;
}

// what a picture with setting `a` needs: the block for an estimate (allocated by the first measured picture, the tables uploaded once), a scratch plane per
// filtered plane (allocated by the first picture that plane is filtered of)
static int ds_alloc(mi355enc_t *h, const mi355enc_denoise_spatial_t *a) {
    if (ds_auto(a) && !h->d_ds) {
        const size_t bytes = ((size_t)DS_STATE_WORDS + DS_REC_WORDS * (NSLOT + 1) + (size_t)DS_SLAB_WORDS * DS_SLABS_MAX + DS_TAB_WORDS) * sizeof(int);
        HIPCHK(hipMalloc((void **)&h->d_ds, bytes));
        h->ds_bytes += bytes; h->ds_primed = false;
        HIPCHK(hipHostMalloc((void **)&h->h_ds, (size_t)DS_REC_WORDS * (NSLOT + 1) * sizeof(int), hipHostMallocDefault));
        memset(h->h_ds, 0, (size_t)DS_REC_WORDS * (NSLOT + 1) * sizeof(int));
        std::vector<uint8_t> tabs((size_t)DS_TAB_WORDS * 4);
        for (int s = 0; s <= DS_MAX; s++) (void)mi355enc_denoise_spatial_tables(s, tabs.data() + 256 * s, nullptr);
        HIPCHK(hipMemset(h->d_ds, 0, (DS_STATE_WORDS + DS_REC_WORDS * (NSLOT + 1)) * sizeof(int)));
        HIPCHK(hipMemcpy(ds_tabs(h), tabs.data(), tabs.size(), hipMemcpyHostToDevice)); // (once; done when the call returns)
    }
    if (a->luma > 0 && !h->d_ds_y) { HIPCHK(hipMalloc((void **)&h->d_ds_y, h->ysz + SURF_PAD)); h->ds_bytes += h->ysz; }
    if (a->chroma > 0 && !h->d_ds_uv) { HIPCHK(hipMalloc((void **)&h->d_ds_uv, h->csz + SURF_PAD)); h->ds_bytes += h->csz; }
    return MI355ENC_OK;
}

int dspatial_latch(mi355enc_t *h, slot_t *s, bool own) {
    { std::lock_guard<std::mutex> g(h->ds_mu); s->ds = h->ds_cur; }
    s->ds_on = own && ds_active(&s->ds);
    s->ds_done = false;
    s->ds_full = h->col_full;
    if (own && !(s->ds_on && ds_auto(&s->ds))) h->ds_primed = false; // (off or manual: the next measured picture primes)
    return MI355ENC_OK;
}

static void ds_fields(const mi355enc_denoise_spatial_t *a, int set[5]) {
    set[0] = a->luma; set[1] = a->chroma; set[2] = a->auto_gain; set[3] = a->percentile; set[4] = a->speed;
}

// one plane through the filter launch into the handle's scratch plane, which then is the slot's: where the rectangle is the whole surface the launch has written
// every byte of it and the two change places (ping-pong: the plane the slot gives up was last read by this launch, and the next launch that writes it follows on
// the same stream); under a geometry the border has to keep its bytes, and the rectangle is copied back instead
static int ds_filter_plane(mi355enc_t *h, uint8_t **plane, uint8_t **scratch, const int rect[4], int chroma, const uint8_t *weight, const int *rec, hipStream_t st) {
    if (k_launch_dspatial_filter(*plane, *scratch, h->W, h->H, h->cfg.width, h->cfg.height, rect, chroma, weight, rec, weight ? nullptr : ds_tabs(h), st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    if (rect[0] == 0 && rect[1] == h->W && rect[2] == 0 && rect[3] == h->H) { uint8_t *t = *plane; *plane = *scratch; *scratch = t; }
    else {
        const size_t at = (size_t)(rect[2] >> chroma) * h->W + rect[0];
        HIPCHK(hipMemcpy2DAsync(*plane + at, h->W, *scratch + at, h->W, (size_t)(rect[1] - rect[0]), (size_t)((rect[3] - rect[2]) >> chroma), hipMemcpyDeviceToDevice, st));
    }
    return MI355ENC_OK;
}

// the launches on the slot's surfaces with record i: which & 1 measure and decide, & 2 the filter launches
static int ds_run(mi355enc_t *h, slot_t *s, const mi355enc_denoise_spatial_t *a, int full, bool prime, int i, int which, hipStream_t st) {
    int rect[4], set[5];
    yuv_rect(h, rect);
    ds_fields(a, set);
    if ((which & 1) && ds_auto(a)) { // on the luma as it enters the step
        const int g = k_launch_dspatial_measure(s->d_src_y, h->W, h->H, rect, h->cfg.width, h->cfg.height, full, ds_slabs(h), st);
        if (g < 1) return MI355ENC_ERR_ARG;
        int bx0, bcols, by0, brows;
        ds_blocks(rect, h->cfg.width, h->cfg.height, &bx0, &bcols, &by0, &brows);
        if (k_launch_dspatial_decide(ds_slabs(h), g, (unsigned)bcols * (unsigned)brows, set, prime ? 1 : 0, h->d_ds, ds_slot(h, i), st)) return MI355ENC_ERR_ARG;
        HIPCHK(hipGetLastError());
    }
    if (!(which & 2)) return MI355ENC_OK;
    uint8_t weight[256];
    if (a->luma > 0) {
        if (!ds_auto(a)) (void)mi355enc_denoise_spatial_tables(a->luma, weight, nullptr);
        int r = ds_filter_plane(h, &s->d_src_y, &h->d_ds_y, rect, 0, ds_auto(a) ? nullptr : weight, ds_auto(a) ? ds_slot(h, i) + 5 : nullptr, st);
        if (r) return r;
    }
    if (a->chroma > 0) {
        if (!ds_auto(a)) (void)mi355enc_denoise_spatial_tables(a->chroma, weight, nullptr);
        int r = ds_filter_plane(h, &s->d_src_uv, &h->d_ds_uv, rect, 1, ds_auto(a) ? nullptr : weight, ds_auto(a) ? ds_slot(h, i) + 6 : nullptr, st);
        if (r) return r;
    }
    return MI355ENC_OK;
}

int dspatial_draw(mi355enc_t *h, slot_t *s, hipStream_t st) {
    if (!s->ds_on) return MI355ENC_OK;
    const int i = (int)(s - h->slot);
    { int r = ds_alloc(h, &s->ds); if (r) return r; }
    { int r = ds_run(h, s, &s->ds, s->ds_full, !h->ds_primed, i, 3, st); if (r) return r; }
    if (ds_auto(&s->ds)) {
        HIPCHK(hipMemcpyAsync(h->h_ds + DS_REC_WORDS * i, ds_slot(h, i), DS_REC_WORDS * sizeof(int), hipMemcpyDeviceToHost, st));
        h->ds_primed = true; s->ds_done = true;
    }
    return MI355ENC_OK;
}

void dspatial_collected(mi355enc_t *h, slot_t *s) {
    h->ds_last_have = true;
    h->ds_last = s->ds;
    memset(&h->ds_last_info, 0, sizeof h->ds_last_info);
    if (!s->ds_on) return;
    if (!ds_auto(&s->ds)) { h->ds_last_info.s_luma = s->ds.luma; h->ds_last_info.s_chroma = s->ds.chroma; }
    else if (s->ds_done && h->h_ds) memcpy(&h->ds_last_info, h->h_ds + DS_REC_WORDS * (int)(s - h->slot), sizeof h->ds_last_info); // (the copy was enqueued in front of everything the collect has waited for)
}

bool dspatial_time_ready(mi355enc_t *h, int stage) {
    std::lock_guard<std::mutex> g(h->ds_mu);
    return ds_active(&h->ds_cur) && ds_auto(&h->ds_cur) == (stage == 37);
}
int dspatial_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *) {
    mi355enc_denoise_spatial_t set;
    { std::lock_guard<std::mutex> g(h->ds_mu); set = h->ds_cur; }
    { int r = ds_alloc(h, &set); if (r) return r; }
    const bool prime = !h->ds_primed;
    h->ds_primed = true;
    return ds_run(h, s, &set, h->col_full, prime, NSLOT, 3, h->stream);
}
void dspatial_time_done(mi355enc_t *h) { h->ds_primed = false; }

static_assert(sizeof(mi355enc_denoise_spatial_info_t) == DS_REC_WORDS * sizeof(int), "the record is the info struct");
static_assert(MI355ENC_DENOISE_SPATIAL_MAX == DS_MAX, "one largest strength");

extern "C" {

int mi355enc_set_denoise_spatial(mi355enc_t *h, const mi355enc_denoise_spatial_t *a) {
    if (!h) return MI355ENC_ERR_ARG;
    mi355enc_denoise_spatial_t off;
    mi355enc_denoise_spatial_default(&off);
    if (!a) a = &off;
    if (mi355enc_denoise_spatial_check(a)) return MI355ENC_ERR_ARG;
    std::lock_guard<std::mutex> g(h->ds_mu);
    h->ds_cur = ds_active(a) ? *a : off;
    return MI355ENC_OK;
}

int mi355enc_get_denoise_spatial(const mi355enc_t *h, mi355enc_denoise_spatial_t *a) {
    if (!h || !a) return MI355ENC_ERR_ARG;
    mi355enc_t *m = const_cast<mi355enc_t *>(h);
    std::lock_guard<std::mutex> g(m->ds_mu);
    *a = h->ds_cur;
    return MI355ENC_OK;
}

int mi355enc_last_denoise_spatial(mi355enc_t *h, mi355enc_denoise_spatial_t *a, mi355enc_denoise_spatial_info_t *info) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!h->ds_last_have) return MI355ENC_ERR_STATE;
    if (a) *a = h->ds_last;
    if (info) *info = h->ds_last_info;
    return MI355ENC_OK;
}

size_t mi355enc_debug_denoise_spatial_bytes(const mi355enc_t *h) { return h ? h->ds_bytes : 0; }

int mi355enc_denoise_spatial_probe_stage(mi355enc_t *h, const mi355enc_denoise_spatial_t *a, uint8_t *y, uint8_t *uv, mi355enc_denoise_spatial_info_t *info) {
    if (!h || !y || !uv || mi355enc_denoise_spatial_check(a) || !ds_active(a)) return MI355ENC_ERR_ARG;
    slot_t *s = &h->slot[0];
    int r = stage_enter(h);
    if (!r) r = ds_alloc(h, a);
    if (!r) r = stage_in(h, s, y, uv);
    if (!r) r = ds_run(h, s, a, h->col_full, true, NSLOT, 3, h->stream);
    if (r) return r;
    h->ds_primed = false; // (the state is this picture's: a stream that follows primes)
    mi355enc_denoise_spatial_info_t rec;
    memset(&rec, 0, sizeof rec);
    if (ds_auto(a)) HIPCHK(hipMemcpyAsync(h->h_ds + DS_REC_WORDS * NSLOT, ds_slot(h, NSLOT), DS_REC_WORDS * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    r = stage_out(h, s, y, uv);
    if (r) return r;
    if (ds_auto(a)) memcpy(&rec, h->h_ds + DS_REC_WORDS * NSLOT, sizeof rec);
    else { rec.s_luma = a->luma; rec.s_chroma = a->chroma; }
    if (info) *info = rec;
    return MI355ENC_OK;
}

int mi355enc_denoise_spatial_probe_measure(mi355enc_t *h, const uint8_t *y, int W, int H, const int rect[4], int vw, int vh, int full_range, mi355enc_denoise_spatial_meas_t *m) {
    if (!h || !y || !rect || !m || W < 16 || H < 2 || W > 8192 || H > 8192 || (W & 15) || (H & 1)) return MI355ENC_ERR_ARG;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > W || rect[3] > H || rect[0] >= rect[1] || rect[2] >= rect[3]) return MI355ENC_ERR_ARG;
    if (vw < 1 || vh < 1 || vw > W || vh > H || rect[0] >= vw || rect[2] >= vh) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; }
    const size_t ysz = (size_t)W * H, slab_bytes = (size_t)DS_SLAB_WORDS * DS_SLABS_MAX * sizeof(unsigned);
    stage_tmp_t pic(h->stream), out(h->stream);
    if (pic.alloc(ysz) || out.alloc(slab_bytes)) return MI355ENC_ERR_HIP;
    HIPCHK(hipMemcpyAsync(pic.p, y, ysz, hipMemcpyHostToDevice, h->stream));
    const int g = k_launch_dspatial_measure(pic.as<uint8_t>(), W, H, rect, vw, vh, full_range, out.as<unsigned>(), h->stream);
    if (g < 1) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    std::vector<unsigned> slabs((size_t)g * DS_SLAB_WORDS);
    HIPCHK(hipMemcpyAsync(slabs.data(), out.p, slabs.size() * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memset(m, 0, sizeof *m);
    for (int k = 0; k < g; k++)
        for (int v = 0; v < 256; v++) { m->hist[v] += slabs[(size_t)k * DS_SLAB_WORDS + v]; m->voters += slabs[(size_t)k * DS_SLAB_WORDS + v]; }
    int bx0, bcols, by0, brows;
    ds_blocks(rect, vw, vh, &bx0, &bcols, &by0, &brows);
    m->candidates = (uint32_t)bcols * (uint32_t)brows;
    return MI355ENC_OK;
}

int mi355enc_denoise_spatial_probe_decide(mi355enc_t *h, const mi355enc_denoise_spatial_meas_t *m, const mi355enc_denoise_spatial_t *a, int prime, int32_t *x, mi355enc_denoise_spatial_info_t *info) {
    if (!h) return MI355ENC_ERR_ARG;
    { // the host function's own checks, on a copy
        int32_t x2 = x && !prime ? *x : 0;
        mi355enc_denoise_spatial_info_t i2;
        if (!x || !info || mi355enc_denoise_spatial_decide(m, a, prime, &x2, &i2)) return MI355ENC_ERR_ARG;
    }
    { int r = stage_enter(h); if (r) return r; }
    stage_tmp_t buf(h->stream);
    if (buf.alloc((DS_SLAB_WORDS + DS_STATE_WORDS + DS_REC_WORDS) * sizeof(int))) return MI355ENC_ERR_HIP;
    int *d_state = buf.as<int>(), *d_rec = d_state + DS_STATE_WORDS;
    unsigned *d_slab = (unsigned *)(d_rec + DS_REC_WORDS);
    int set[5], state = *x;
    ds_fields(a, set);
    HIPCHK(hipMemcpyAsync(d_slab, m->hist, DS_SLAB_WORDS * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_state, &state, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream)); // (state lives on this call's stack)
    if (k_launch_dspatial_decide(d_slab, 1, m->candidates, set, prime ? 1 : 0, d_state, d_rec, h->stream)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(info, d_rec, sizeof *info, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&state, d_state, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *x = state;
    return MI355ENC_OK;
}

} // extern "C"
