// enc_autolevel.cpp -- automatic levels and white balance of a handle (mi355enc_set_autolevel): the value the control thread sets, its
// latch per input picture, the three launches on the slot's coded surfaces with the handle's device block, the device probes, the stage entry point and the
// timed stages.  The rule itself is autolevel_host.h's and autolevel_host.c's, which need no device.
#include "enc_internal.hpp"

// the handle's block: {Lo, Hi, Du, Dv} (and four words of room), NSLOT + 1 slot blocks (the last one: the stage calls'), the slabs
#define AL_STATE_WORDS 8
static int *al_slot(mi355enc_t *h, int i) { return h->d_al + AL_STATE_WORDS + AL_SLOT_WORDS * i; }
static unsigned *al_slabs(mi355enc_t *h) { return (unsigned *)(h->d_al + AL_STATE_WORDS + AL_SLOT_WORDS * (NSLOT + 1)); }
static bool al_active(const mi355enc_autolevel_t *a) { return a->levels > 0 || a->balance > 0; }

void autolevel_free(mi355enc_t *h) {
    if (h->d_al) (void)hipFree(h->d_al);
    if (h->h_al) (void)hipHostFree(h->h_al);
    h->d_al = h->h_al = nullptr; h->al_bytes = 0; h->al_primed = false;
}

// the block, allocated by the first autolevelled picture (or stage call)
static int al_alloc(mi355enc_t *h) {
    if (h->d_al) return MI355ENC_OK;
    const size_t bytes = ((size_t)AL_STATE_WORDS + AL_SLOT_WORDS * (NSLOT + 1) + (size_t)AL_SLAB_WORDS * AL_SLABS_MAX) * sizeof(int);
    HIPCHK(hipMalloc((void **)&h->d_al, bytes));
    if (hipHostMalloc((void **)&h->h_al, (size_t)AL_SLOT_WORDS * (NSLOT + 1) * sizeof(int), hipHostMallocDefault) != hipSuccess) { autolevel_free(h); return MI355ENC_ERR_HIP; }
    memset(h->h_al, 0, (size_t)AL_SLOT_WORDS * (NSLOT + 1) * sizeof(int));
    h->al_bytes = bytes; h->al_primed = false;
    return MI355ENC_OK;
}

int autolevel_latch(mi355enc_t *h, slot_t *s, bool own) {
    { std::lock_guard<std::mutex> g(h->al_mu); s->al = h->al_cur; }
    s->al_on = own && al_active(&s->al);
    s->al_done = false;
    s->al_full = h->col_full;
    if (own && !s->al_on) h->al_primed = false; // (off: the next picture it is on for primes)
    return MI355ENC_OK;
}

static void al_fields(const mi355enc_autolevel_t *a, int set[7]) {
    set[0] = a->levels; set[1] = a->balance; set[2] = a->speed; set[3] = a->clip_low; set[4] = a->clip_high; set[5] = a->max_gain; set[6] = a->reach;
}

// the launches on surfaces y / uv of the coded size into slot block i: which & 1 measure, & 2 decide, & 4 apply.  nslabs: what a measure launch left (in / out)
static int al_run(mi355enc_t *h, uint8_t *y, uint8_t *uv, const mi355enc_autolevel_t *a, int full, bool prime, int i, int which, int *nslabs, hipStream_t st) {
    int rect[4], set[7];
    yuv_rect(h, rect);
    al_fields(a, set);
    if (which & 1) {
        const int g = k_launch_autolevel_measure(y, uv, h->W, h->H, rect, h->cfg.width, h->cfg.height, full, a->reach, al_slabs(h), st);
        if (g < 1) return MI355ENC_ERR_ARG;
        *nslabs = g;
    }
    if ((which & 2) && k_launch_autolevel_decide(al_slabs(h), *nslabs, al_chroma_count(rect, h->cfg.width, h->cfg.height), set, full, prime ? 1 : 0, h->d_al, al_slot(h, i), st)) return MI355ENC_ERR_ARG;
    if ((which & 4) && k_launch_autolevel_apply(y, uv, h->W, h->H, rect, a->levels > 0, a->balance > 0, al_slot(h, i), st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}

int autolevel_draw(mi355enc_t *h, slot_t *s, hipStream_t st) {
    if (!s->al_on) return MI355ENC_OK;
    const int i = (int)(s - h->slot);
    int n = 0;
    { int r = al_alloc(h); if (r) return r; }
    { int r = al_run(h, s->d_src_y, s->d_src_uv, &s->al, s->al_full, !h->al_primed, i, 7, &n, st); if (r) return r; }
    HIPCHK(hipMemcpyAsync(h->h_al + AL_SLOT_WORDS * i, al_slot(h, i), AL_SLOT_WORDS * sizeof(int), hipMemcpyDeviceToHost, st));
    h->al_primed = true; s->al_done = true;
    return MI355ENC_OK;
}

static void al_info_of(const int *rec, mi355enc_autolevel_info_t *info, uint8_t *table) {
    if (info) memcpy(info, rec, sizeof *info);
    if (table) memcpy(table, rec + AL_TAB_AT, 256);
}

void autolevel_collected(mi355enc_t *h, slot_t *s) {
    h->al_last_have = true;
    h->al_last = s->al;
    memset(&h->al_last_info, 0, sizeof h->al_last_info);
    memset(h->al_last_tab, 0, sizeof h->al_last_tab);
    if (s->al_done && h->h_al) al_info_of(h->h_al + AL_SLOT_WORDS * (int)(s - h->slot), &h->al_last_info, h->al_last_tab); // (the copy was enqueued in front of everything the collect has waited for)
}

bool autolevel_time_ready(mi355enc_t *h, int) {
    std::lock_guard<std::mutex> g(h->al_mu);
    return al_active(&h->al_cur);
}

int autolevel_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *) {
    mi355enc_autolevel_t set;
    { std::lock_guard<std::mutex> g(h->al_mu); set = h->al_cur; }
    { int r = al_alloc(h); if (r) return r; }
    return al_run(h, s->d_src_y, s->d_src_uv, &set, h->col_full, true, NSLOT, 3, &h->al_time_n, h->stream);
}
int autolevel_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x) {
    mi355enc_autolevel_t set;
    { std::lock_guard<std::mutex> g(h->al_mu); set = h->al_cur; }
    return al_run(h, s->d_src_y, s->d_src_uv, &set, h->col_full, false, NSLOT, 1 << (x->stage - 32), &h->al_time_n, h->stream);
}
void autolevel_time_done(mi355enc_t *h) { h->al_primed = false; }

static_assert(sizeof(mi355enc_autolevel_info_t) == AL_REC_WORDS * sizeof(int), "the record is the info struct");
static_assert(AL_REC_WORDS <= AL_TAB_AT && AL_TAB_AT + 64 == AL_SLOT_WORDS, "a slot block: record, room, table");

extern "C" {

int mi355enc_set_autolevel(mi355enc_t *h, const mi355enc_autolevel_t *a) {
    if (!h) return MI355ENC_ERR_ARG;
    mi355enc_autolevel_t off;
    mi355enc_autolevel_default(&off);
    if (!a) a = &off;
    if (mi355enc_autolevel_check(a)) return MI355ENC_ERR_ARG;
    std::lock_guard<std::mutex> g(h->al_mu);
    h->al_cur = *a;
    return MI355ENC_OK;
}

int mi355enc_get_autolevel(const mi355enc_t *h, mi355enc_autolevel_t *a) {
    if (!h || !a) return MI355ENC_ERR_ARG;
    mi355enc_t *m = const_cast<mi355enc_t *>(h);
    std::lock_guard<std::mutex> g(m->al_mu);
    if (al_active(&h->al_cur)) *a = h->al_cur; else mi355enc_autolevel_default(a);
    return MI355ENC_OK;
}

int mi355enc_last_autolevel(mi355enc_t *h, mi355enc_autolevel_t *a, mi355enc_autolevel_info_t *info, uint8_t table[256]) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!h->al_last_have) return MI355ENC_ERR_STATE;
    if (a) *a = h->al_last;
    if (info) *info = h->al_last_info;
    if (table) memcpy(table, h->al_last_tab, 256);
    return MI355ENC_OK;
}

size_t mi355enc_debug_autolevel_bytes(const mi355enc_t *h) { return h ? h->al_bytes : 0; }

int mi355enc_autolevel_probe_stage(mi355enc_t *h, const mi355enc_autolevel_t *a, uint8_t *y, uint8_t *uv, mi355enc_autolevel_info_t *info, uint8_t table[256]) {
    if (!h || !y || !uv || mi355enc_autolevel_check(a) || !al_active(a)) return MI355ENC_ERR_ARG;
    slot_t *s = &h->slot[0];
    int n = 0;
    int r = stage_enter(h);
    if (!r) r = al_alloc(h);
    if (!r) r = stage_in(h, s, y, uv);
    if (!r) r = al_run(h, s->d_src_y, s->d_src_uv, a, h->col_full, true, NSLOT, 7, &n, h->stream);
    if (r) return r;
    h->al_primed = false; // (the state is this picture's: a stream that follows primes)
    int *rec = h->h_al + AL_SLOT_WORDS * NSLOT;
    HIPCHK(hipMemcpyAsync(rec, al_slot(h, NSLOT), AL_SLOT_WORDS * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    r = stage_out(h, s, y, uv);
    if (!r) al_info_of(rec, info, table);
    return r;
}

int mi355enc_autolevel_probe_measure(mi355enc_t *h, const uint8_t *y, const uint8_t *uv, int W, int H, const int rect[4], int vw, int vh, int full_range, int reach,
                                     mi355enc_autolevel_meas_t *m) {
    if (!h || !y || !uv || !rect || !m || W < 16 || H < 2 || W > 8192 || H > 8192 || (W & 15) || (H & 1) || reach < 0 || reach > 127) return MI355ENC_ERR_ARG;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > W || rect[3] > H || rect[0] >= rect[1] || rect[2] >= rect[3]) return MI355ENC_ERR_ARG;
    if (vw < 1 || vh < 1 || vw > W || vh > H || rect[0] >= vw || rect[2] >= vh) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; }
    const size_t ysz = (size_t)W * H, csz = ysz / 2, slab_bytes = (size_t)AL_SLAB_WORDS * AL_SLABS_MAX * sizeof(unsigned);
    stage_tmp_t pic(h->stream), out(h->stream);
    if (pic.alloc(ysz + csz) || out.alloc(slab_bytes)) return MI355ENC_ERR_HIP;
    HIPCHK(hipMemcpyAsync(pic.p, y, ysz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(pic.as<uint8_t>() + ysz, uv, csz, hipMemcpyHostToDevice, h->stream));
    const int g = k_launch_autolevel_measure(pic.as<uint8_t>(), pic.as<uint8_t>() + ysz, W, H, rect, vw, vh, full_range, reach, out.as<unsigned>(), h->stream);
    if (g < 1) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    unsigned *slabs = (unsigned *)malloc((size_t)g * AL_SLAB_WORDS * sizeof(unsigned));
    if (!slabs) return MI355ENC_ERR_NOMEM;
    const hipError_t e = hipMemcpyAsync(slabs, out.p, (size_t)g * AL_SLAB_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream);
    if (e != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) { free(slabs); return MI355ENC_ERR_HIP; }
    memset(m, 0, sizeof *m);
    for (int k = 0; k < g; k++) {
        const unsigned *t = slabs + (size_t)k * AL_SLAB_WORDS;
        for (int v = 0; v < 256; v++) m->hist[v] += t[v];
        m->voters += t[256]; m->su += t[257]; m->sv += t[258];
    }
    m->chroma = al_chroma_count(rect, vw, vh);
    free(slabs);
    return MI355ENC_OK;
}

int mi355enc_autolevel_probe_decide(mi355enc_t *h, const mi355enc_autolevel_meas_t *m, const mi355enc_autolevel_t *a, int full_range, int prime, int32_t state[4],
                                    mi355enc_autolevel_info_t *info, uint8_t table[256]) {
    if (!h) return MI355ENC_ERR_ARG;
    { // the host function's own checks, on copies
        int32_t st[4] = {0, 0, 0, 0};
        mi355enc_autolevel_info_t i2;
        uint8_t t2[256];
        if (state && !prime) memcpy(st, state, sizeof st);
        if (!state || !info || !table || mi355enc_autolevel_decide(m, a, full_range, prime, st, &i2, t2)) return MI355ENC_ERR_ARG;
    }
    { int r = stage_enter(h); if (r) return r; }
    stage_tmp_t buf(h->stream);
    if (buf.alloc((AL_SLAB_WORDS + AL_STATE_WORDS + AL_SLOT_WORDS) * sizeof(int))) return MI355ENC_ERR_HIP;
    unsigned slab[AL_SLAB_WORDS];
    memcpy(slab, m->hist, 256 * sizeof(unsigned));
    slab[256] = m->voters; slab[257] = (unsigned)m->su; slab[258] = (unsigned)m->sv; slab[259] = 0; // (su, sv <= 255 * 2^24: a word each)
    int *d_state = buf.as<int>(), *d_rec = d_state + AL_STATE_WORDS;
    unsigned *d_slab = (unsigned *)(d_rec + AL_SLOT_WORDS);
    int set[7], rec[AL_SLOT_WORDS];
    al_fields(a, set);
    HIPCHK(hipMemcpyAsync(d_slab, slab, sizeof slab, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_state, state, 4 * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream)); // (slab lives on this call's stack)
    if (k_launch_autolevel_decide(d_slab, 1, m->chroma, set, full_range, prime ? 1 : 0, d_state, d_rec, h->stream)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rec, d_rec, sizeof rec, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(state, d_state, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    al_info_of(rec, info, table);
    return MI355ENC_OK;
}

} // extern "C"
