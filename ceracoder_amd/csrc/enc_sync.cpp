// enc_sync.cpp -- the wait words' owner (enc_sync.hpp): allocation, the one clear that open() and recover() share, the debug entry points' part, fetch.
#include "enc_internal.hpp"

static size_t row_words_bytes(int mbh) { return (size_t)mbh * MI355_PROG_STRIDE * sizeof(unsigned); } // one word per macroblock row, on different memory channels

// the four words of d_progress_: [0] the error word, then the three counts (the only place that knows)
dev_count_t dev_words_t::started() const { return {d_progress_ + 1, tot_.started}; }
dev_count_t dev_words_t::ip_done() const { return {d_progress_ + 2, tot_.ip_done}; }
dev_count_t dev_words_t::qpc() const { return {d_progress_ + 3, tot_.qpc}; }

int dev_words_t::alloc(int mbh, hipStream_t s) {
    mbh_ = mbh;
    HIPCHK(hipMalloc((void **)&d_progress_, 4 * sizeof(unsigned)));
    if (!getenv("MI355ENC_NO_SPLIT") && k_deblock_part_bytes(mbh)) HIPCHK(hipMalloc((void **)&d_db_part_, k_deblock_part_bytes(mbh))); // (A/B switch, read once per encoder)
    HIPCHK(hipMalloc((void **)&d_iband_done_, 2 * (size_t)mbh * sizeof(unsigned))); // (intra_mode 2: one word per band)
    HIPCHK(hipMalloc((void **)&d_row_done_, row_words_bytes(mbh)));
    HIPCHK(hipMalloc((void **)&d_db_done_, 2 * k_deblock_done_bytes()));
    HIPCHK(hipMalloc((void **)&d_ip_progress_, row_words_bytes(mbh)));
    HIPCHK(hipMemsetAsync(d_ip_progress_, 0, row_words_bytes(mbh), s)); // epoch-tagged: the epoch starts at 1
    return clear(s);
}
void dev_words_t::release() {
    for (unsigned **p : {&d_progress_, &d_row_done_, &d_db_part_, &d_db_done_, &d_iband_done_, &d_ip_progress_}) { if (*p) (void)hipFree(*p); *p = nullptr; }
}
int dev_words_t::clear(hipStream_t s) {
    HIPCHK(hipMemsetAsync(d_progress_, 0, 4 * sizeof(unsigned), s)); // (the error word is sticky: only cleared here)
    HIPCHK(hipMemsetAsync(d_row_done_, 0, row_words_bytes(mbh_), s));
    if (d_db_part_) HIPCHK(hipMemsetAsync(d_db_part_, 0, k_deblock_part_bytes(mbh_), s));
    HIPCHK(hipMemsetAsync(d_db_done_, 0, 2 * k_deblock_done_bytes(), s)); // epoch 0 is never used
    HIPCHK(hipMemsetAsync(d_iband_done_, 0, 2 * (size_t)mbh_ * sizeof(unsigned), s));
    tot_ = word_totals_t();
    forget();
    return 0;
}
int dev_words_t::set(const mi355enc_counters_t *in) {
    if (!(in->keep & 2u)) {
        uint32_t *rows = (uint32_t *)malloc((size_t)mbh_ * sizeof(uint32_t));
        if (!rows) return MI355ENC_ERR_NOMEM;
        for (int r = 0; r < mbh_; r++) rows[r] = in->pmb_rows_total;
        const hipError_t e = hipMemcpy2D(d_row_done_, MI355_PROG_STRIDE * sizeof(unsigned), rows, sizeof(uint32_t), sizeof(uint32_t), (size_t)mbh_, hipMemcpyHostToDevice);
        free(rows);
        HIPCHK(e);
        tot_.rows = in->pmb_rows_total;
    }
    const struct { unsigned bit; unsigned *word; uint32_t *total; uint32_t v; } counts[3] = {
        {4u, started().word, &tot_.started, in->db_started_total}, {8u, ip_done().word, &tot_.ip_done, in->ip_done_total}, {16u, qpc().word, &tot_.qpc, in->qpc_total}};
    for (const auto &c : counts)
        if (!(in->keep & c.bit)) { HIPCHK(hipMemcpy(c.word, &c.v, sizeof(uint32_t), hipMemcpyHostToDevice)); *c.total = c.v; }
    return 0;
}
int dev_words_t::trip(unsigned code) {
    HIPCHK(hipMemcpy(d_progress_, &code, sizeof code, hipMemcpyHostToDevice));
    return 0;
}
// The progress words of a P picture's intra macroblock rows carry 20 bits of the epoch (IP_EPOCH, intra_mb.hpp).  Every launch of the rows rewrites every row's
// word, so the words are those of the last launch, and a launch's deblocker can take a stale word for its own picture's only when that launch was a multiple of
// 2^20 epochs ago with no launch of the rows in between: a run of IDR pictures (force_idr, or stage calls, which stamp epochs of their own) of 4 h 51 min at 60
// pictures/s, then a P picture.  There the words are cleared first (a zero word reports no macroblock final under any tag).  No launch that reads or writes them
// is in flight then: a picture in flight is at most three epochs old.
int dev_words_t::ip_rows_stamp(uint32_t epoch, hipStream_t s) {
    if (ip_epoch_ && ip_epoch_ != epoch && ((ip_epoch_ ^ epoch) & 0xFFFFFu) == 0) {
        HIPCHK(hipMemsetAsync(d_ip_progress_, 0, row_words_bytes(mbh_), s));
        HIPCHK(hipStreamSynchronize(s));
    }
    ip_epoch_ = epoch;
    return 0;
}
size_t dev_words_t::fetch_bytes(int what) const {
    return what == 102 ? (d_db_part_ ? k_deblock_part_bytes(mbh_) : 0) : what == 103 ? sizeof(unsigned) : what == 104 ? (size_t)(3 + mbh_) * sizeof(unsigned) : 0;
}
int dev_words_t::fetch(int what, void *dst) const {
    if (what != 104) { HIPCHK(hipMemcpy(dst, what == 102 ? d_db_part_ : d_progress_, fetch_bytes(what), hipMemcpyDeviceToHost)); return 0; }
    HIPCHK(hipMemcpy(dst, started().word, 3 * sizeof(unsigned), hipMemcpyDeviceToHost)); // (started, ip_done, qpc: adjacent)
    HIPCHK(hipMemcpy2D((unsigned *)dst + 3, sizeof(unsigned), d_row_done_, MI355_PROG_STRIDE * sizeof(unsigned), sizeof(unsigned), (size_t)mbh_, hipMemcpyDeviceToHost));
    return 0;
}
