// enc_quality.cpp -- quality metrics of the coded pictures (mi355enc_set_quality_metrics): the per-slot accumulator and result blocks,
// the launch behind a picture's deblocking (enc_schedule.cpp says where), what collect() books, and the getters.  The kernel is k_quality.hip; everything
// derived from its five integers (PSNR, mean SSIM) is computed here on the host.
#include "enc_internal.hpp"

#include <cmath>

static const size_t k_qblock = QUALITY_WORDS * sizeof(unsigned long long), k_qacc = QUALITY_ACC_WORDS * sizeof(unsigned long long);

int quality_alloc(mi355enc_t *h) {
    if (h->d_qacc && h->h_qres) return 0;
    if (!h->d_qacc) HIPCHK(hipMalloc((void **)&h->d_qacc, (NSLOT + 1) * k_qacc));
    if (!h->h_qres) HIPCHK(hipHostMalloc((void **)&h->h_qres, (NSLOT + 1) * k_qblock, hipHostMallocDefault));
    memset(h->h_qres, 0, (NSLOT + 1) * k_qblock);
    HIPCHK(hipMemsetAsync(h->d_qacc, 0, (NSLOT + 1) * k_qacc, h->stream)); // once: every launch leaves its block clear for the next one
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
void quality_free(mi355enc_t *h) {
    for (int i = 0; i < NSLOT; i++) if (h->ev_q[i]) { (void)hipEventDestroy(h->ev_q[i]); h->ev_q[i] = nullptr; }
    if (h->d_qacc) (void)hipFree(h->d_qacc);
    if (h->h_qres) (void)hipHostFree(h->h_qres);
    h->d_qacc = h->h_qres = nullptr;
}

// the derived figures of a filled-in set of integers
static void quality_derive(const mi355enc_t *h, mi355enc_quality_t *q, uint64_t pictures) {
    const uint64_t ny = (uint64_t)h->cfg.width * h->cfg.height, nc = (uint64_t)(h->cfg.width / 2) * (h->cfg.height / 2);
    q->samples[0] = ny * pictures; q->samples[1] = q->samples[2] = nc * pictures;
    for (int c = 0; c < 3; c++) q->psnr[c] = q->sse[c] ? 10.0 * std::log10(65025.0 * (double)q->samples[c] / (double)q->sse[c]) : 100.0;
    q->ssim = q->ssim_windows ? (double)q->ssim_sum / ((double)q->ssim_windows * 1073741824.0) : 0.0;
}
static void quality_take(const mi355enc_t *h, const unsigned long long *res, mi355enc_quality_t *q) {
    memset(q, 0, sizeof *q);
    for (int c = 0; c < 3; c++) q->sse[c] = res[c];
    q->ssim_sum = (int64_t)res[3]; q->ssim_windows = res[4];
    quality_derive(h, q, 1);
}

int quality_enqueue(mi355enc_t *h, slot_t *s, const uint8_t *src_y, const uint8_t *src_uv, int src_stride, int rec, hipStream_t st) {
    const int k = (int)(s - h->slot);
    k_launch_quality(src_y, src_uv, src_stride, h->d_rec_y[rec], h->d_rec_uv[rec], h->W, h->cfg.width, h->cfg.height, h->d_qacc + (size_t)k * QUALITY_ACC_WORDS,
                     h->h_qres + (size_t)k * QUALITY_WORDS, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_q[k], st));
    return 0;
}

int quality_collect(mi355enc_t *h, slot_t *s) {
    const int k = (int)(s - h->slot);
    HIPCHK(hipEventSynchronize(h->ev_q[k])); // the hand-over event fires before deblocking ends: this wait is the metrics' own
    quality_take(h, h->h_qres + (size_t)k * QUALITY_WORDS, &h->q_last);
    h->q_last.pts = s->pts;
    h->q_have = true;
    for (int c = 0; c < 3; c++) h->q_tot.sse[c] += h->q_last.sse[c];
    h->q_tot.ssim_sum += h->q_last.ssim_sum; h->q_tot.ssim_windows += h->q_last.ssim_windows;
    h->q_tot.pictures++; h->q_tot.pts = s->pts;
    return 0;
}

int quality_run(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, int src_stride, const uint8_t *rec_y, const uint8_t *rec_uv, mi355enc_quality_t *q) {
    { int r = quality_alloc(h); if (r) return r; }
    k_launch_quality(src_y, src_uv, src_stride, rec_y, rec_uv, h->W, h->cfg.width, h->cfg.height, h->d_qacc + (size_t)NSLOT * QUALITY_ACC_WORDS,
                     h->h_qres + (size_t)NSLOT * QUALITY_WORDS, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    quality_take(h, h->h_qres + (size_t)NSLOT * QUALITY_WORDS, q);
    return 0;
}

extern "C" {

int mi355enc_set_quality_metrics(mi355enc_t *h, int on) {
    if (!h) return MI355ENC_ERR_ARG;
    if (h->n_submitted) return MI355ENC_ERR_STATE; // (before the first submit: every picture of the stream is measured, or none)
    if (!on) { h->q_on = false; return MI355ENC_OK; }
    HIPCHK(hipSetDevice(h->cfg.device_id));
    { int r = quality_alloc(h); if (r) return r; }
    for (int i = 0; i < NSLOT; i++) if (!h->ev_q[i]) HIPCHK(hipEventCreateWithFlags(&h->ev_q[i], hipEventDisableTiming));
    h->q_on = true;
    return MI355ENC_OK;
}

int mi355enc_last_quality(mi355enc_t *h, mi355enc_quality_t *q) {
    if (!h || !q) return MI355ENC_ERR_ARG;
    if (!h->q_on || !h->q_have) return MI355ENC_ERR_STATE;
    *q = h->q_last;
    return MI355ENC_OK;
}

int mi355enc_quality_totals(mi355enc_t *h, mi355enc_quality_t *q) {
    if (!h || !q) return MI355ENC_ERR_ARG;
    if (!h->q_on) return MI355ENC_ERR_STATE;
    *q = h->q_tot;
    quality_derive(h, q, q->pictures);
    return MI355ENC_OK;
}

} // extern "C"
