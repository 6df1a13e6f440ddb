// enc_sync.hpp -- the words kernels wait on, and the host's account of them, under one owner (the table of the words: DESIGN.md section 5, "The wait words").
// Device side: the sticky error word, three counts that only grow, one count per macroblock row, and the epoch-tagged flags of the bands and rows.  Host
// side: what each count reaches with the last launch enqueued -- the kernels compare the two, so a count's word and its total move together, in book(),
// set() and clear() and nowhere else.  Only this struct's functions touch its fields (the handle holds one, mi355enc::words).
#ifndef MI355_ENC_SYNC_HPP
#define MI355_ENC_SYNC_HPP
#include "enc_plan.hpp"

// The host's totals: uint32, they wrap with the device's words (every comparison on the device is a signed difference).  Plain C++, no HIP: the stand-alone
// driver of tests/test_plan_cpu.py books into one of these.
struct word_totals_t {
    uint32_t rows = 0, started = 0, ip_done = 0, qpc = 0;
    void book(const launch_counts_t &c) { rows += c.rows; started += c.started; ip_done += c.ip_done; qpc += c.qpc; } // the only place a total grows
};

#ifdef __HIPCC__
#include "../../include/mi355enc.h"
struct dev_count_t { unsigned *word; uint32_t total; }; // a growing count: where the device counts, and what it reaches with everything enqueued so far

class dev_words_t {
  public:
    int alloc(int mbh, hipStream_t s); // open(): allocates and clears (MI355ENC_NO_SPLIT, read here once: no parts' words)
    void release();                    // close()
    // Every count and flag to zero, on stream s, which must be idle with every other stream of the handle -- what open() starts from and recover() returns
    // to.  Deliberately NOT cleared: the intra macroblock rows' progress words and ip_epoch.  Those words are tagged with the picture's epoch, every launch
    // of the rows rewrites all of them, and ip_rows_stamp() clears them in the one case a stale tag could pass for a new one.
    int clear(hipStream_t s);
    void forget() { rec_epoch_[0] = rec_epoch_[1] = 0; } // a stage call wrote the reconstruction buffers: no band-done words stand for them
    // the debug entry points: the four totals of mi355enc_counters_t, under its keep bits 2, 4, 8, 16; set() writes word and total together (streams idle)
    void get(mi355enc_counters_t *out) const { out->pmb_rows_total = tot_.rows; out->db_started_total = tot_.started; out->ip_done_total = tot_.ip_done; out->qpc_total = tot_.qpc; }
    int set(const mi355enc_counters_t *in);
    void book(const launch_counts_t &c) { tot_.book(c); }
    int trip(unsigned code); // mi355enc_debug_trip_wait: a code into the error word, as a wait that ran out would leave it (streams idle)
    // in front of every launch of a P picture's intra macroblock rows (on stream s: whichever stream carries the rows and their deblocker is behind it)
    int ip_rows_stamp(uint32_t epoch, hipStream_t s);

    unsigned *err() const { return d_progress_; } // the sticky error word of every bounded wait
    dev_count_t started() const; // workgroups of band-deblocking launches placed
    dev_count_t ip_done() const; // intra macroblock rows of fused launches complete
    dev_count_t qpc() const;     // macroblock rows whose QP_Y chain is resolved
    dev_count_t row_done() const { return {d_row_done_, tot_.rows}; }       // per macroblock row (MI355_PROG_STRIDE words apart): macroblocks of gated P-stage launches complete
    unsigned *band_done(int rec) const { return d_db_done_ + (size_t)rec * (k_deblock_done_bytes() / sizeof(unsigned)); } // reconstruction buffer rec: its bands' done words
    unsigned *iband_done(int rec) const { return d_iband_done_ + (size_t)rec * mbh_; }                                    // ... and its intra rows' (bands') flags
    unsigned *ip_progress() const { return d_ip_progress_; }
    unsigned *part_cnt() const { return d_db_part_; } // null: bands are walked whole
    uint32_t rec_epoch(int rec) const { return rec_epoch_[rec]; }        // the epoch buffer rec's band-done words carry once its picture is deblocked (0: none stand for it)
    void stamp_rec(int rec, uint32_t epoch) { rec_epoch_[rec] = epoch; }
    // mi355enc_fetch 102 (the parts' words), 103 (the error word), 104 (started, ip_done, qpc, then every row's row_done word): bytes (0: not there), and the copy
    size_t fetch_bytes(int what) const;
    int fetch(int what, void *dst) const;

  private:
    int mbh_ = 0;
    unsigned *d_progress_ = nullptr;    // [0] error word, [1] started, [2] ip_done, [3] qpc
    unsigned *d_row_done_ = nullptr;
    unsigned *d_db_part_ = nullptr;     // k_deblock_part_bytes(): per band the parts' counters and {cut, epoch} granules
    unsigned *d_db_done_ = nullptr;     // per reconstruction buffer k_deblock_done_bytes()
    unsigned *d_iband_done_ = nullptr;  // per reconstruction buffer one word per macroblock row
    unsigned *d_ip_progress_ = nullptr; // one word per macroblock row, MI355_PROG_STRIDE words apart
    word_totals_t tot_;
    uint32_t rec_epoch_[2] = {0, 0};
    uint32_t ip_epoch_ = 0;             // epoch of the last launch that wrote d_ip_progress_ (0: none since they were cleared)
};
#endif
#endif
