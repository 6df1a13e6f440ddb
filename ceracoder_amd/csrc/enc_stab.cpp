// enc_stab.cpp -- electronic image stabilisation of a handle (mi355enc_set_stabilize): the value the control thread sets, its latch per
// input picture, the one place a picture's scale / geometry launch is enqueued (input_scale: with the slot stabilised the estimate runs in front of it, on the
// same stream, and the launch takes the crop's displacement from the word the match launch wrote), the device probes and the timed stages.  The rule itself is
// stab_host.h's and stab_host.c's, which need no device.
#include "enc_internal.hpp"

// the handle's block: {Sx, Sy} (and six words of room), NSLOT + 1 records (the last one: the stage calls'), two halves of sums
#define STAB_STATE_WORDS 8
static size_t stab_sum_words(int w, int ht) { return (size_t)STAB_BANDS * ((size_t)w + (size_t)ht); }
static int *stab_rec(mi355enc_t *h, int i) { return h->d_stab + STAB_STATE_WORDS + STAB_REC_WORDS * i; }
static unsigned *stab_sums(mi355enc_t *h, int half) { return (unsigned *)(h->d_stab + STAB_STATE_WORDS + STAB_REC_WORDS * (NSLOT + 1)) + stab_sum_words(h->stab_w, h->stab_h) * half; }

void stab_free(mi355enc_t *h) {
    if (h->d_stab) (void)hipFree(h->d_stab);
    if (h->h_stab) (void)hipHostFree(h->h_stab);
    h->d_stab = h->h_stab = nullptr; h->stab_bytes = 0; h->stab_primed = false; h->stab_w = h->stab_h = 0;
}

// the buffers, allocated by the first stabilised picture (or probe of the timed stages) for the handle's input size
static int stab_alloc(mi355enc_t *h) {
    if (h->d_stab && h->stab_w == h->in_w && h->stab_h == h->in_h) return MI355ENC_OK;
    stab_free(h);
    const size_t bytes = ((size_t)STAB_STATE_WORDS + STAB_REC_WORDS * (NSLOT + 1) + 2 * stab_sum_words(h->in_w, h->in_h)) * sizeof(int);
    HIPCHK(hipMalloc((void **)&h->d_stab, bytes));
    if (hipHostMalloc((void **)&h->h_stab, (size_t)STAB_REC_WORDS * (NSLOT + 1) * sizeof(int), hipHostMallocDefault) != hipSuccess) { stab_free(h); return MI355ENC_ERR_HIP; }
    memset(h->h_stab, 0, (size_t)STAB_REC_WORDS * (NSLOT + 1) * sizeof(int));
    h->stab_bytes = bytes; h->stab_w = h->in_w; h->stab_h = h->in_h; h->stab_half = 0; h->stab_primed = false;
    return MI355ENC_OK;
}

static bool stab_size_ok(const mi355enc_t *h, int range) { return h->in_w >= 4 * range && h->in_h >= 4 * range; }

int stab_latch(mi355enc_t *h, slot_t *s, bool own) {
    { std::lock_guard<std::mutex> g(h->stab_mu); s->stab = h->stab_cur; }
    s->stab_done = false;
    if (!own) return MI355ENC_OK;
    if (!s->stab.range) { h->stab_primed = false; return MI355ENC_OK; } // (off: the next picture it is on for primes)
    if (!h->geom_on) return MI355ENC_ERR_STATE;
    return stab_size_ok(h, s->stab.range) ? MI355ENC_OK : MI355ENC_ERR_ARG;
}

// this picture's bounds {lo_x, hi_x, lo_y, hi_y}: from the crop as it is set now (the tables the launch runs with are that crop's)
static void stab_bounds_now(const mi355enc_t *h, const mi355enc_stabilize_t *st, int b[4]) {
    stab_bounds(st->margin_x, h->geom.crop_x, h->geom.crop_w, h->geom.in_w, &b[0], &b[1]);
    stab_bounds(st->margin_y, h->geom.crop_y, h->geom.crop_h, h->geom.in_h, &b[2], &b[3]);
}

// the luma the scale launch of `fmt` reads: first sample and byte step
static void stab_luma_of(int fmt, const uint8_t *p0, const uint8_t **luma, int *step) {
    *step = fmt >= MI355ENC_FMT_YUY2 ? 2 : 1;
    *luma = p0 + (fmt == MI355ENC_FMT_UYVY ? 1 : 0);
}

// clear + projection launch into half `half`
static int stab_run_project(mi355enc_t *h, const uint8_t *luma, int stride, int step, int half, hipStream_t st) {
    HIPCHK(hipMemsetAsync(stab_sums(h, half), 0, stab_sum_words(h->stab_w, h->stab_h) * sizeof(unsigned), st));
    if (k_launch_stab_project(luma, stride, step, h->stab_w, h->stab_h, stab_sums(h, half), st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}
// match launch of half `half` against the other one into record i, and the record's copy to pinned memory
static int stab_run_match(mi355enc_t *h, const mi355enc_stabilize_t *set, int half, bool prime, int i, hipStream_t st) {
    int b[4];
    stab_bounds_now(h, set, b);
    if (k_launch_stab_match(stab_sums(h, half ^ 1), stab_sums(h, half), h->stab_w, h->stab_h, set->range, set->leak, prime ? 1 : 0, b, h->d_stab, stab_rec(h, i), st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->h_stab + STAB_REC_WORDS * i, stab_rec(h, i), STAB_REC_WORDS * sizeof(int), hipMemcpyDeviceToHost, st));
    return MI355ENC_OK;
}

int input_scale(mi355enc_t *h, slot_t *s, int fmt, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2, int s0, int s1, int s2, const in_target_t *t, const scale_plan_t *pl, hipStream_t up) {
    const int *off = nullptr;
    if (s->stab.range > 0 && h->geom_on && fmt >= MI355ENC_FMT_NV12 && fmt <= MI355ENC_FMT_UYVY) {
        const int i = (int)(s - h->slot);
        { int r = stab_alloc(h); if (r) return r; }
        const uint8_t *luma;
        int step;
        stab_luma_of(fmt, p0, &luma, &step);
        int r = stab_run_project(h, luma, s0, step, h->stab_half, up);
        if (!r) r = stab_run_match(h, &s->stab, h->stab_half, !h->stab_primed, i, up);
        if (r) return r;
        h->stab_half ^= 1; h->stab_primed = true; s->stab_done = true;
        off = stab_rec(h, i) + 4; // {ox, oy}
    }
    return k_launch_scale(fmt, p0, p1, p2, s0, s1, s2, t->y, t->uv, t->W, t->H, pl, up, off) ? MI355ENC_ERR_ARG : MI355ENC_OK;
}

void stab_collected(mi355enc_t *h, slot_t *s) {
    h->stab_last_have = true;
    h->stab_last = s->stab;
    memset(&h->stab_last_info, 0, sizeof h->stab_last_info);
    if (s->stab_done && h->h_stab) memcpy(&h->stab_last_info, h->h_stab + STAB_REC_WORDS * (int)(s - h->slot), sizeof h->stab_last_info); // (the copy was enqueued in front of everything the collect has waited for)
}

bool stab_time_ready(mi355enc_t *h, int) {
    std::lock_guard<std::mutex> g(h->stab_mu);
    return h->stab_cur.range > 0 && h->geom_on && stab_size_ok(h, h->stab_cur.range);
}
int stab_time_prepare(mi355enc_t *h, slot_t *, ts_ctx_t *) {
    { int r = stab_alloc(h); if (r) return r; }
    HIPCHK(hipMemsetAsync(h->d_stab, 0, h->stab_bytes, h->stream)); // (sums of no picture: the match launch's time does not depend on them)
    return MI355ENC_OK;
}
int stab_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x) {
    if (x->stage == 29) return stab_run_project(h, s->d_raw, (h->in_w + 15) & ~15, 1, 0, h->stream); // (an NV12 picture in the raw staging buffer, as stage 14's)
    mi355enc_stabilize_t set;
    { std::lock_guard<std::mutex> g(h->stab_mu); set = h->stab_cur; }
    return stab_run_match(h, &set, 0, false, NSLOT, h->stream);
}
void stab_time_done(mi355enc_t *h) { h->stab_primed = false; }

static_assert(sizeof(mi355enc_stabilize_info_t) == STAB_REC_WORDS * sizeof(int), "the record is the info struct");

extern "C" {

int mi355enc_set_stabilize(mi355enc_t *h, const mi355enc_stabilize_t *s) {
    if (!h) return MI355ENC_ERR_ARG;
    mi355enc_stabilize_t off;
    mi355enc_stabilize_default(&off);
    if (!s) s = &off;
    if (mi355enc_stabilize_check(s)) return MI355ENC_ERR_ARG;
    std::lock_guard<std::mutex> g(h->stab_mu);
    h->stab_cur = *s;
    return MI355ENC_OK;
}

int mi355enc_get_stabilize(const mi355enc_t *h, mi355enc_stabilize_t *s) {
    if (!h || !s) return MI355ENC_ERR_ARG;
    mi355enc_t *m = const_cast<mi355enc_t *>(h);
    std::lock_guard<std::mutex> g(m->stab_mu);
    *s = h->stab_cur;
    return MI355ENC_OK;
}

int mi355enc_last_stabilize(mi355enc_t *h, mi355enc_stabilize_t *s, mi355enc_stabilize_info_t *info) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!h->stab_last_have) return MI355ENC_ERR_STATE;
    if (s) *s = h->stab_last;
    if (info) *info = h->stab_last_info;
    return MI355ENC_OK;
}

size_t mi355enc_debug_stabilize_bytes(const mi355enc_t *h) { return h ? h->stab_bytes : 0; }

int mi355enc_stabilize_probe_project(mi355enc_t *h, const uint8_t *luma, int stride, int step, int w, int ht, uint32_t *sums) {
    if (!h || !luma || !sums || w < 1 || ht < 1 || w > 8192 || ht > 8192 || (step != 1 && step != 2) || stride < (w - 1) * step + 1) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; }
    const size_t bytes = (size_t)stride * (ht - 1) + (size_t)(w - 1) * step + 1, words = stab_sum_words(w, ht);
    const size_t lead = (size_t)((uintptr_t)luma & 3); // the plane keeps its address modulo 4 on the device
    stage_tmp_t pic(h->stream), out(h->stream);
    if (pic.alloc(lead + bytes + 8) || out.alloc(words * sizeof(unsigned))) return MI355ENC_ERR_HIP;
    HIPCHK(hipMemcpyAsync(pic.as<uint8_t>() + lead, luma, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(out.p, 0, words * sizeof(unsigned), h->stream));
    if (k_launch_stab_project(pic.as<uint8_t>() + lead, stride, step, w, ht, out.as<unsigned>(), h->stream)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sums, out.p, words * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}

int mi355enc_stabilize_probe_match(mi355enc_t *h, const uint32_t *prev, const uint32_t *cur, int w, int ht, const mi355enc_stabilize_t *s, const int bounds[4],
                                   const int state[2], int prime, mi355enc_stabilize_info_t *info) {
    if (!h || !prev || !cur || !s || !bounds || !state || !info || mi355enc_stabilize_check(s) || s->range < 1 || w > 8192 || ht > 8192 || w < 4 * s->range || ht < 4 * s->range) return MI355ENC_ERR_ARG;
    for (int a = 0; a < 2; a++) { // bounds and state as the rule makes them
        const int lo = bounds[2 * a], hi = bounds[2 * a + 1];
        if (lo > 0 || hi < 0 || lo < -MI355ENC_STABILIZE_MARGIN_MAX || hi > MI355ENC_STABILIZE_MARGIN_MAX || ((lo | hi) & 1) || state[a] < -256 * MI355ENC_STABILIZE_MARGIN_MAX || state[a] > 256 * MI355ENC_STABILIZE_MARGIN_MAX) return MI355ENC_ERR_ARG;
    }
    { int r = stage_enter(h); if (r) return r; }
    const size_t words = stab_sum_words(w, ht);
    stage_tmp_t buf(h->stream);
    if (buf.alloc((2 * words + STAB_STATE_WORDS + STAB_REC_WORDS) * sizeof(int))) return MI355ENC_ERR_HIP;
    int *d_state = buf.as<int>(), *d_rec = d_state + STAB_STATE_WORDS;
    unsigned *d_prev = (unsigned *)(d_rec + STAB_REC_WORDS), *d_cur = d_prev + words;
    HIPCHK(hipMemcpyAsync(d_state, state, 2 * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_prev, prev, words * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_cur, cur, words * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    if (k_launch_stab_match(d_prev, d_cur, w, ht, s->range, s->leak, prime ? 1 : 0, bounds, d_state, d_rec, h->stream)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(info, d_rec, sizeof *info, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}

} // extern "C"
