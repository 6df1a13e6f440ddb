// enc_schedule.cpp -- the picture pipeline of the C-ABI shim: the stream schedule of one picture (enqueue_picture), the entropy worker, recovery, collect.
// What stands in front of the search on the front stream -- the bracketed steps below -- is enqueued by the submit entry points (enc_input.cpp).
//
// Per picture:
//   front stream: [H2D source | conversion | JPEG coefficients + inverse DCT | scale] -> [image layers, if one is set] -> [text overlay, if a text is set] -> P: me_kernel (SAD surfaces + first selection) -> me_select_kernel x ME_ITERS
//                 -> intra analysis of the badly predicted macroblocks;  IDR: the source copy the next search runs against
//   back stream:  IDR: intra analysis (flat) -> intra wavefront (persistent bands) | P: pmb_kernel -> intra_p_kernel
//                 -> deblocking (persistent band kernel)
//   hand-over stream, from the moment records and levels are final: scan + pack into pinned host memory -> event
//   host, when the event has fired: CAVLC slice coding (h264_host.c).
// With pipeline_depth = 1 the host codes picture n while the device works on n+1; with 2 a third picture is in flight.
// Which of these run beside each other, on which stream, waiting for what on the device, is the picture's plan (enc_plan.hpp; the table of its flags:
// DESIGN.md section 5, "The plan of a picture"): enqueue_picture() decides, plans, then enqueues from the plan.
#include "enc_internal.hpp"

static void worker_push(mi355enc_t *h, int slot_index);

static void launch_intra_all(mi355enc_t *h, int ci) {
    int n = k_intra_diags(h->mbw, h->mbh);
    for (int d = 0; d < n; d++) k_launch_intra_diag(h->d_ctx2[ci], h->mbw, h->mbh, d, h->stream);
}
static void launch_deblock_all(mi355enc_t *h, int ci) {
    int n = k_deblock_diags(h->mbw, h->mbh);
    for (int d = 0; d < n; d++) k_launch_deblock_diag(h->d_ctx2[ci], h->mbw, h->mbh, d, h->stream);
}
static int build_graph(mi355enc_t *h, int which, int ci, hipGraphExec_t *out) {
    hipGraph_t g;
    HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    if (which == 0) launch_intra_all(h, ci); else launch_deblock_all(h, ci);
    HIPCHK(hipStreamEndCapture(h->stream, &g));
    HIPCHK(hipGraphInstantiate(out, g, nullptr, nullptr, 0));
    HIPCHK(hipGraphDestroy(g));
    return 0;
}
int run_intra(mi355enc_t *h, int ci, const frame_ctx_t *hc, unsigned *band_done) {
    k_launch_intra_analyse(hc, h->mbw, h->mbh, 0, h->stream); // open-loop mode analysis + decisions: one flat launch
    if (h->cfg.intra_mode == 0 || h->cfg.intra_mode == 2) { // one persistent launch: dataflow per macroblock row (0) / the lock-step band kernel (2, kept for A/B)
        if (h->cfg.intra_mode == 0) k_launch_intra_rows(hc, h->mbh, h->d_ib_gran, h->words.err(), band_done, h->stream);
        else k_launch_intra_band(hc, h->mbh, h->d_ib_gran, h->words.err(), band_done, h->stream);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (h->cfg.use_graphs) {
        if (!h->g_intra[ci]) { int r = build_graph(h, 0, ci, &h->g_intra[ci]); if (r) return r; }
        HIPCHK(hipGraphLaunch(h->g_intra[ci], h->stream));
    } else launch_intra_all(h, ci);
    return 0;
}
static hipStream_t plan_stream(const mi355enc_t *h, plan_stream_t which) { return which == PS_MAIN ? h->stream : which == PS_FRONT ? h->fstream : which == PS_INTRA ? h->istream : h->cstream; }
// whole picture; hc: host copy of the context (by-value kernels), ci: which device copy holds the same (graph kernels); p: the picture's plan -- the stream and what the
// launch waits for on the device (the stage entry points: the in-order plan); rec: the reconstruction buffer whose band-done words the launch publishes (-1: none)
int run_deblock(mi355enc_t *h, int ci, const frame_ctx_t *hc, const pic_plan_t &p, int rec) {
    if (h->cfg.deblock_mode == 0) { // the persistent band kernel (its prologue derives the boundary strengths from the records)
        const dev_words_t &w = h->words;
        const launch_shape_t shape = plan_launches(p, hc->all_intra != 0, hc->qp_off != nullptr, w.part_cnt() != nullptr, h->mbw, h->mbh);
        db_launch_t l;
        l.variant = shape.db; l.parts = shape.parts; l.qpc = shape.qpc; l.ib_rows = h->cfg.intra_mode == 2 ? k_intra_band_rows() : 1;
        l.err = w.err(); l.gran = h->d_db_gran; l.partab = h->d_db_par;
        l.band_done = rec >= 0 ? w.band_done(rec) : nullptr; l.started = w.started().word;
        l.iband_done = p.isplit ? w.iband_done(rec) : nullptr;
        l.row_done = p.db_rows ? w.row_done().word : nullptr; l.row_need = w.row_done().total;
        l.ip_progress = w.ip_progress(); l.ip_strips = h->d_ip_strips; l.ip_done = w.ip_done().word;
        l.qpc_word = w.qpc().word; l.qpc_base = w.qpc().total; l.part_cnt = w.part_cnt();
        if (k_launch_deblock_bands(hc, &l, plan_stream(h, p.deblock))) return MI355ENC_ERR_ARG;
        h->words.book({0, shape.inc.started, shape.inc.ip_done, shape.inc.qpc}); // (the rows were booked with the fused P stage: run_pmb)
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (h->cfg.use_graphs) {
        if (!h->g_deblock[ci]) { int r = build_graph(h, 1, ci, &h->g_deblock[ci]); if (r) return r; }
        HIPCHK(hipGraphLaunch(h->g_deblock[ci], h->stream));
    } else launch_deblock_all(h, ci);
    return 0;
}
// scene-cut recovery: the decision taken with picture k's hand-over lands on picture k + lag, the first one that cannot have been
// submitted yet (depth 0 behaves as depth 1, so that the stream is the same for both)
static int sc_lag(const mi355enc_t *h) { return h->cfg.pipeline_depth >= 2 ? h->cfg.pipeline_depth + 1 : 2; }

// rate control's ladder below QP 51 (oracle: k_drop_sad): the SAD under which a P macroblock carries no residual / takes the skip vector
static const uint32_t k_drop_sad[DROP_MAX + 1] = {0, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192, 12288, 0xFFFFFFFFu};
// ... and its counterpart for I pictures (oracle: k_idrop_ac): the sum of level magnitudes up to which a macroblock's luma / chroma residual is not sent
#define I8_QP_MAX 37 /* Intra_8x8 is tried up to this picture quantiser (oracle: ORC_I8_QP_MAX) */
static const int32_t k_idrop_ac[DROP_MAX + 1] = {0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 64, 0x7FFFFFFF};

void fill_ctx(mi355enc_t *h, frame_ctx_t *c, int qp, int drop, int idr, int set, int roi) {
    c->mbi = h->d_mbi; c->levels = h->d_levels; c->isad = h->d_isad; c->dbrec = h->d_dbrec; c->idec = h->d_idec2[set];
    c->stride = h->W; c->mbw = h->mbw; c->mbh = h->mbh;
    c->slice_rows = idr ? h->islice_rows : h->pslice_rows; c->slice_dbf = h->slice_dbf;
    c->partitions = (!idr && h->cfg.partitions && !h->cfg.transform8x8 && h->cfg.deblock_mode == 0) ? 1 : 0;
    c->qp = qp; c->me_range = h->cfg.me_range; c->lambda = k_lambda[qp < 0 ? 0 : qp > 51 ? 51 : qp]; c->i4x4 = h->cfg.i4x4; c->t8 = h->cfg.transform8x8; c->all_intra = idr ? 1 : 0;
    c->surf = h->d_surf[set]; c->imv_a = h->d_imv[set][0]; c->imv_b = h->d_imv[set][1]; c->imv_c = h->d_imv[set][2];
    c->me_ref_y = h->d_psrc[h->psrc_cur]; c->psrc_out = h->d_psrc[h->psrc_cur ^ 1];
    if (++h->epoch == 0) h->epoch = 1;
    c->epoch = h->epoch;
    c->drop_sad = (!idr && drop > 0 && drop <= DROP_MAX) ? k_drop_sad[drop] : 0;
    c->iac_drop = (idr && drop > 0 && drop <= DROP_MAX) ? k_idrop_ac[drop] : 0;
    if (c->iac_drop) c->i4x4 = 0; // on the ladder: Intra_16x16 only
    c->i8 = (idr && h->cfg.transform8x8 && h->cfg.i8x8 && h->cfg.intra_mode == 0 && !c->iac_drop && qp <= I8_QP_MAX) ? 1 : 0;
    c->qp_off = (h->cfg.aq_mode || roi) ? h->d_qp_off[set] : nullptr; // (roi: this picture latched an active region-of-interest map)
    c->intra_p = h->cfg.intra_in_p ? (h->cfg.i4x4 && h->cfg.intra_in_p > 1 ? 2 : 1) : 0; // 2: Intra_4x4 as well
    c->ir_c0 = 0; c->ir_c1 = 0; c->ir_clean = -1; // (enqueue_picture sets the refresh columns of a picture of an intra-refresh stream)
}
// The fused P stage as the plan gates it: gated on the reference picture's band-done words, behind wait_started_kernel (not before the reference's deblocking
// launch is on the chip); with rows, every macroblock counted for the picture's own deblocking launch
int run_pmb(mi355enc_t *h, const frame_ctx_t *hc, int refine, const pic_plan_t &p, hipStream_t st) {
    const dev_words_t &w = h->words;
    const launch_shape_t shape = plan_launches(p, false, hc->qp_off != nullptr, w.part_cnt() != nullptr, h->mbw, h->mbh);
    pmb_launch_t l;
    l.gate = shape.gate; l.refine = refine; l.err = w.err();
    l.gate_done = shape.gate != PMB_IN_ORDER ? w.band_done(h->cur) : nullptr; l.ref_epoch = w.rec_epoch(h->cur);
    l.row_done = shape.gate == PMB_GATED_ROWS ? w.row_done().word : nullptr;
    if (shape.gate != PMB_IN_ORDER) k_launch_wait_started(w.started().word, w.started().total, w.err(), st);
    if (k_launch_pmb(hc, h->mbw, &l, st)) return MI355ENC_ERR_ARG;
    h->words.book({shape.inc.rows, 0, 0, 0});
    return 0;
}
// P picture, front part (front stream): nothing here depends on the coding of the picture before
static int run_p_front(mi355enc_t *h, const frame_ctx_t *hc, slot_t *s, int prof) {
    hipStream_t st = h->fstream;
    if (prof) HIPCHK(hipEventRecord(s->ev[0], st));
    k_launch_me(hc, h->mbw, st);
    if (prof) HIPCHK(hipEventRecord(s->ev[6], st));
    k_launch_me_select_all(hc, h->mbw, st);
    if (prof) HIPCHK(hipEventRecord(s->ev[1], st));
    if (hc->intra_p) k_launch_intra_analyse(hc, h->mbw, h->mbh, 1, st);
    if (prof) HIPCHK(hipEventRecord(s->ev[7], st));
    HIPCHK(hipGetLastError());
    return 0;
}
// ... and back part (the plan's back stream): needs the deblocked picture before it
// p.pgate: gated on the reference picture's band-done words (the fused stage then runs on the intra stream, beside that picture's deblocking)
// p.prows: the picture's deblocking launch will sit directly behind the previous one and wait on the device for this stage's rows (no event)
static int run_p_back(mi355enc_t *h, const frame_ctx_t *hc, slot_t *s, int prof, const pic_plan_t &p) {
    hipStream_t st = plan_stream(h, p.back);
    unsigned *const ip_progress = h->words.ip_progress();
    if (prof) HIPCHK(hipEventRecord(s->ev[8], st));
    { int r = run_pmb(h, hc, h->cfg.subpel, p, st); if (r) return r; }
    if (prof) HIPCHK(hipEventRecord(s->ev[5], st));
    if (p.pgate) { // the main stream carries nothing but deblocking launches, back to back: with prows this picture's bands wait on the device for the fused
        // stage's rows (row counts, no event between the streams), and its movers follow intra_p_kernel
        if (!p.prows) { HIPCHK(hipEventRecord(h->ev_pmb, st)); HIPCHK(hipStreamWaitEvent(h->stream, h->ev_pmb, 0)); } // (fewer than three pictures in flight: by event)
        if (hc->intra_p && !p.fip) k_launch_intra_p(hc, h->mbw, h->mbh, ip_progress, h->d_ip_strips, h->words.err(), st); // (fip: the deblocking launch carries the rows)
    } else if (p.split) { // intra_p_kernel leaves the chain: prep + the band deblocker follow the fused stage directly and overtake it row by row
        HIPCHK(hipEventRecord(h->ev_pmb, st));
        HIPCHK(hipStreamWaitEvent(h->istream, h->ev_pmb, 0));
        k_launch_intra_p(hc, h->mbw, h->mbh, ip_progress, h->d_ip_strips, h->words.err(), h->istream);
    } else if (hc->intra_p) k_launch_intra_p(hc, h->mbw, h->mbh, ip_progress, h->d_ip_strips, h->words.err(), st);
    if (prof) HIPCHK(hipEventRecord(s->ev[11], st));
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- one picture: decide (host state) -> plan (enc_plan.hpp) -> enqueue from the plan -> book.  No decision is taken behind the picture's first launch.
// what decide_picture() settles about a picture on the host
struct pic_t { const uint8_t *src_y, *src_uv; int src_stride, idr, qp, drop, ir_j, all_skip, nxt, set, prof, roi; }; // nxt: the reconstruction buffer it writes; set: its device set and context copy; roi: it carries an active region-of-interest map

// Decide: IDR or P, rate control's pick, the position in the intra-refresh cycle, all-skip, buffers and device set, whether the stage timers are sampled
static pic_t decide_picture(mi355enc_t *h, slot_t *s, const uint8_t *src_y, const uint8_t *src_uv, int src_stride, int force_idr) {
    const int idr = force_idr || !h->have_ref || (!h->ir_on && h->frames_since_idr >= h->cfg.gop) || // (intra refresh: no periodic IDR picture)
                    (h->n_submitted == h->sc_force_at && h->frames_since_idr >= sc_lag(h)); // scene-cut recovery, see collect(): not when an IDR picture came in between
    if (idr) { h->frames_since_idr = 0; h->ir_pos = 0; h->ir_R = 0; h->ir_skip_owed = 0; }
    // rate control: latch the setpoint written by the control thread, pick this picture's QP (and, below QP 51, its drop level)
    rc_set_bitrate(&h->rc, h->want_bps.load(std::memory_order_relaxed));
    int fq = h->fixed_qp.load(std::memory_order_relaxed);
    int qp, drop;
    s->fixed_qp = fq; s->fixed_drop = 0;
    if (fq >= 0) { qp = fq; drop = s->fixed_drop = h->fixed_drop.load(std::memory_order_relaxed); s->rc_picked = 0; } // (no pick: collect() / recover() then leave rate control alone for this picture)
    else { rc_pick(&h->rc, idr, &qp, &drop); s->rc_picked = 1; }
    if (idr && drop == DROP_SKIP) drop = 0; // an IDR picture is never skipped; it has a ladder of its own
    // Periodic intra refresh: P picture p >= 1 after the IDR picture is picture j = (p - 1) mod N of a cycle (N = cfg.gop) and
    // refreshes the columns [max(R - 1, 0), a(j + 1)), a(j) = floor(j * mbw / N), R the first column the cycle has not refreshed yet (= a(j) unless an
    // all-skip picture refreshed nothing).  The last picture of a cycle is never an all-skip picture: that moves to the next one.
    const int ir_j = (h->ir_on && !idr) ? h->ir_pos : -1; // (= (p - 1) mod N, kept as a counter of its own: p itself is unbounded on a live stream)
    if (ir_j >= 0) {
        if (ir_j == 0) h->ir_R = 0;
        const bool last = ir_j == h->cfg.gop - 1;
        if (drop == DROP_SKIP && last) { drop = DROP_MAX; h->ir_skip_owed = 1; }
        else if (h->ir_skip_owed && !last) { drop = DROP_SKIP; h->ir_skip_owed = 0; }
    }
    const int all_skip = !idr && drop == DROP_SKIP;
    // stage timers: an event record costs ~5 us of queue time, so profile_events = k samples every k-th picture (IDR pictures always)
    // (a sampled picture runs its stages strictly in order; IDR pictures: every other one, or at the P pictures' cadence in an all-intra stream)
    const int prof = !all_skip && h->cfg.profile_events > 0 &&
                     ((idr && h->cfg.gop > 1) ? (h->idr_count & 1) == 0 : h->n_submitted % (uint64_t)h->cfg.profile_events == 0);
    return {src_y, src_uv, src_stride, idr, qp, drop, ir_j, all_skip, all_skip ? h->cur : (h->cur ^ 1) /* an all-skip picture IS its reference: nothing is written */, (int)(h->n_submitted % NSET), prof, s->roi_on ? 1 : 0};
}
// Plan: what plan_picture() is asked with
static plan_in_t plan_inputs(const mi355enc_t *h, const pic_t &p) {
    plan_in_t in;
    in.idr = p.idr != 0; in.all_skip = p.all_skip != 0; in.prof = p.prof != 0;
    in.pipeline_depth = h->cfg.pipeline_depth; in.intra_mode = h->cfg.intra_mode; in.deblock_mode = h->cfg.deblock_mode; in.aq_mode = h->cfg.aq_mode || p.roi; // (the plan's aq_mode: "offsets are present for this picture")
    in.intra_in_p = h->cfg.intra_in_p; in.i4x4 = h->cfg.i4x4; in.profile_overlap = h->cfg.profile_overlap;
    in.overlap_allowed = overlap_allowed(h); in.exclusive_device = exclusive_device(h); in.wait_room[0] = h->wait_room[0]; in.wait_room[1] = h->wait_room[1];
    in.keep_prefilter = h->d_pre_y != nullptr; in.ref_flags = h->words.rec_epoch(h->cur) != 0; in.pgate = h->pgate; in.fip_rows = h->fip_rows;
    return in;
}
// Enqueue, all-skip: one run of P_Skip macroblocks with the zero vector (8.4.1.1 infers it: every neighbour's vector is zero): the host
// writes the records itself; no source sample is read, no kernel runs, the reference stays where it is
static int enqueue_all_skip(mi355enc_t *h, slot_t *s, const pic_t &p) {
    memset(s->h_mbi, 0, (size_t)h->nmb * sizeof(mb_info_t));
    for (int i = 0; i < h->nmb; i++) { s->h_mbi[i].mb_type = 1; s->h_mbi[i].qp = (uint8_t)p.qp; }
    s->h_hdr[0] = 0; s->h_hdr[1] = 0;
    for (int r = 0; r < h->mbh; r++) s->h_hdr[2 + r] = 0;
    s->h_hdr[2 + h->mbh] = s->h_hdr[3 + h->mbh] = 0;
    if (h->d_pre_y) {
        HIPCHK(hipMemcpyAsync(h->d_pre_y, h->d_rec_y[p.nxt], h->ysz, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_pre_uv, h->d_rec_uv[p.nxt], h->csz, hipMemcpyDeviceToDevice, h->stream));
    }
    // The readers of the reconstruction (below) read the reference the picture repeats -- that is what the source is measured against, and what a decoder shows: on the main
    // stream, behind the reference's deblocking (an IDR picture's may have run on the intra stream); the metrics also behind the source's arrival on the front stream, which
    // nothing else of this picture waits for
    if (h->q_on) { HIPCHK(hipEventRecord(s->ev_front, h->fstream)); HIPCHK(hipStreamWaitEvent(h->stream, s->ev_front, 0)); }
    if ((h->q_on || (s->snap && s->snap_req.what == 1)) && h->dbI_busy[p.nxt]) { HIPCHK(hipStreamWaitEvent(h->stream, h->ev_dbI[p.nxt], 0)); h->dbI_busy[p.nxt] = 0; }
    return 0;
}
// the picture's context: the host copy every kernel of the default path takes by value
static int picture_ctx(mi355enc_t *h, frame_ctx_t *c, const pic_t &p) {
    c->src_y = p.src_y; c->src_uv = p.src_uv; c->src_stride = p.src_stride;
    c->ref_y = h->d_rec_y[h->cur]; c->ref_uv = h->d_rec_uv[h->cur];
    c->rec_y = h->d_rec_y[p.nxt]; c->rec_uv = h->d_rec_uv[p.nxt];
    c->vis_h = h->cfg.height;
    fill_ctx(h, c, p.qp, p.drop, p.idr, p.set, p.roi);
    c->mbi = h->d_mbi_set[p.set]; c->levels = h->d_levels_set[p.set];
    if (!p.idr && c->intra_p) { int r = h->words.ip_rows_stamp(c->epoch, h->stream); if (r) return r; }
    if (p.ir_j >= 0) {
        const int R = h->ir_R;
        c->ir_c0 = R > 0 ? R - 1 : 0; // (one column of overlap: deblocking left the last columns of column R - 1 dirty in the reference)
        c->ir_c1 = (int)((long long)(p.ir_j + 1) * h->mbw / h->cfg.gop);
        c->ir_clean = R > 0 ? 16 * R - 4 : -1;
        h->ir_R = c->ir_c1;
    }
    return 0;
}
// Enqueue, front stream: the source is in place (upload / conversion were enqueued there); P pictures: search, selection, gated intra
// analysis; I pictures: only the padded source copy the next picture's search will run against.  Then what the back stage has to wait for.
static int enqueue_front(mi355enc_t *h, slot_t *s, const pic_t &p, const pic_plan_t &plan) {
    frame_ctx_t *c = s->h_ctx;
    { int r = picture_ctx(h, c, p); if (r) return r; }
    if (plan.upload_ctx) HIPCHK(hipMemcpyAsync(h->d_ctx2[p.set], c, sizeof *c, hipMemcpyHostToDevice, h->stream));
    if (h->cfg.aq_mode) k_launch_aq(c, h->d_qp_off[p.set], h->fstream); // adaptive quantisation: the offsets of this picture's macroblocks
    if (p.roi) roi_compose(h, s, p.set, h->fstream); // ... moved by the picture's region-of-interest map (alone: the map is the offsets)
    if (p.idr) k_launch_copy_luma(c, h->fstream);
    else { int r = run_p_front(h, c, s, p.prof); if (r) return r; }
    HIPCHK(hipEventRecord(s->ev_front, h->fstream));
    h->psrc_cur ^= 1;
    HIPCHK(hipStreamWaitEvent(plan_stream(h, plan.back), s->ev_front, 0));
    for (int b = 0; b < 2; b++) // an IDR picture's deblocking on the intra stream: a P picture reads the whole reference, and whoever writes the buffer it works on waits too
        if (h->dbI_busy[b] && (!p.idr || b == p.nxt)) { HIPCHK(hipStreamWaitEvent(h->stream, h->ev_dbI[b], 0)); h->dbI_busy[b] = 0; }
    return 0;
}
// Enqueue, back stage of an IDR picture: the intra wavefront on the main stream (isplit: its bands publish their flags for the deblocker beside it)
static int enqueue_idr(mi355enc_t *h, slot_t *s, const pic_t &p, const pic_plan_t &plan) {
    if (plan.isplit) { HIPCHK(hipEventRecord(h->ev_pmb, h->stream)); HIPCHK(hipStreamWaitEvent(h->istream, h->ev_pmb, 0)); } // behind everything enqueued so far (a P picture's deblocker, its tables)
    if (p.prof) HIPCHK(hipEventRecord(s->ev[0], h->stream));
    int r = run_intra(h, p.set, s->h_ctx, plan.isplit ? h->words.iband_done(p.nxt) : nullptr); if (r) return r;
    if (p.prof) HIPCHK(hipEventRecord(s->ev[1], h->stream));
    return 0;
}
// ... of a P picture: the fused stage; fip: the deblocking launch follows at once, the intra macroblock rows inside it
static int enqueue_p(mi355enc_t *h, slot_t *s, const pic_t &p, const pic_plan_t &plan) {
    int r = run_p_back(h, s->h_ctx, s, p.prof, plan); if (r) return r;
    if (plan.fip) {
        r = run_deblock(h, p.set, s->h_ctx, plan, p.nxt); if (r) return r;
        k_launch_wait_started(h->words.ip_done().word, h->words.ip_done().total, h->words.err(), h->istream); // records and levels are final once the rows have all counted themselves
    }
    return 0;
}
// Enqueue, behind the back stage: "records and levels are final", then the deblocking launch (unless the P stage carried it)
static int enqueue_deblock(mi355enc_t *h, slot_t *s, const pic_t &p, const pic_plan_t &plan) {
    const frame_ctx_t *c = s->h_ctx;
    if (p.prof) HIPCHK(hipEventRecord(s->ev[2], h->stream));
    HIPCHK(hipGetLastError());
    if (c->qp_off && h->cfg.deblock_mode != 0) k_launch_qp_chain(h->d_mbi_set[p.set], h->nmb, p.qp, c->slice_rows * h->mbw, h->stream); // 7.4.5: QP_Y of the macroblocks without mb_qp_delta, for the deblocker (everything runs on the main stream here)
    HIPCHK(hipEventRecord(s->gpu_done, plan_stream(h, plan.gpu_done))); // records and levels are final here; they do not depend on deblocking
    if (h->d_pre_y) {
        HIPCHK(hipMemcpyAsync(h->d_pre_y, h->d_rec_y[p.nxt], h->ysz, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_pre_uv, h->d_rec_uv[p.nxt], h->csz, hipMemcpyDeviceToDevice, h->stream));
        if (p.prof) HIPCHK(hipEventRecord(s->ev[2], h->stream));
    }
    if (!plan.fip) { int r = run_deblock(h, p.set, c, plan, p.nxt); if (r) return r; }
    if (p.prof) { HIPCHK(hipEventRecord(s->ev[3], h->stream)); HIPCHK(hipEventRecord(s->ev[4], h->stream)); } // (never an isplit picture: a sampled IDR picture may not wait)
    return 0;
}
// Readers of the reconstruction: quality metrics and a still of what a decoder shows (DESIGN.md sections 12, 18), directly behind the picture's deblocking launch, on its
// stream.  Whatever writes this reconstruction buffer next (the picture after next) is either behind them in the main stream's order, or a gated fused P stage on the intra
// stream, which starts only when the deblocking launch of the picture between the two is on the chip -- a launch that sits behind this one in the main stream.  An isplit
// picture's deblocking runs on the intra stream: the event the buffer's next writer waits for is recorded here, behind the readers.
static int enqueue_rec_readers(mi355enc_t *h, slot_t *s, const pic_t &p, const pic_plan_t &plan) {
    hipStream_t st = plan_stream(h, plan.deblock);
    if (h->q_on) { int r = quality_enqueue(h, s, p.src_y, p.src_uv, p.src_stride, p.nxt, st); if (r) return r; }
    if (s->snap && s->snap_req.what == 1) { int r = snapshot_enqueue(h, s, h->d_rec_y[p.nxt], h->d_rec_uv[p.nxt], h->W, st); if (r) return r; }
    if (plan.isplit) { HIPCHK(hipEventRecord(h->ev_dbI[p.nxt], st)); h->dbI_busy[p.nxt] = 1; }
    return 0;
}
// Hand-over, enqueued after the deblocking launches so that it cannot be dispatched ahead of them: the device packs the non-zero
// blocks straight into the pinned host buffer while the band deblocker runs.
static int enqueue_handover(mi355enc_t *h, slot_t *s, const pic_t &p) {
    HIPCHK(hipStreamWaitEvent(h->cstream, s->gpu_done, 0));
    k_launch_pack(h->d_mbi_set[p.set], h->d_levels_set[p.set], h->nmb, h->mbw, h->d_off, s->h_mbi, s->h_levels, s->h_hdr, h->words.err(), h->cstream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->done, h->cstream));
    return 0;
}
// Book: the picture on its slot, the handle moved on to the next one
static void book_picture(mi355enc_t *h, slot_t *s, const pic_t &p, int64_t pts, int force_idr) {
    if (!p.all_skip) h->words.stamp_rec(p.nxt, h->cfg.deblock_mode == 0 ? s->h_ctx->epoch : 0); // the epoch the buffer's band-done words carry once its deblocking is through
    h->n_submitted++;
    s->is_idr = p.idr; s->qp = p.qp; s->drop = p.drop; s->frame_num = h->frames_since_idr; s->idr_pic_id = h->idr_count & 0xFFFF; s->ir_start = p.ir_j == 0;
    s->src_y = p.src_y; s->src_uv = p.src_uv; s->src_stride = p.src_stride; s->force_idr = force_idr;
    s->pts = pts; s->rec_index = p.nxt; s->set = p.set; s->prof = p.prof; s->index = h->n_submitted - 1; s->all_skip = p.all_skip;
    if (p.idr) h->idr_count++;
    h->frames_since_idr++;
    if (p.ir_j >= 0) h->ir_pos = p.ir_j + 1 < h->cfg.gop ? p.ir_j + 1 : 0;
    // intra refresh: no periodic IDR picture resets the count, so it is kept bounded; frame_num is sent modulo MaxFrameNum = 256 (h264_host.c), and the
    // count stays >= 256, past the scene-cut rule's sc_lag()
    if (h->ir_on && h->frames_since_idr >= 512) h->frames_since_idr -= 256;
    h->cur = p.nxt; h->have_ref = 1; h->prev_slot = s;
    h->head = (h->head + 1) % NSLOT; h->pending++;
    if (h->wk_on) worker_push(h, (int)(s - h->slot));
}

// Enqueue every device step of one picture whose source is described by (src_y, src_uv, src_stride).  Anything the caller
// uploaded for this picture was enqueued on the same stream.
int enqueue_picture(mi355enc_t *h, slot_t *s, const uint8_t *src_y, const uint8_t *src_uv, int src_stride, int64_t pts, int force_idr) {
    if (!h->recovering) snapshot_latch(h, s); // stills: an armed request becomes this picture's (a picture recover() enqueues again keeps what it had)
    if (!h->recovering) { int r = roi_latch(h, s); if (r) return r; } // the region-of-interest map set last likewise
    const pic_t p = decide_picture(h, s, src_y, src_uv, src_stride, force_idr);
    const pic_plan_t plan = plan_picture(plan_inputs(h, p)); // streams and device-side waits: all of them, before the first launch
    int r = p.all_skip ? enqueue_all_skip(h, s, p) : enqueue_front(h, s, p, plan);
    if (!r && !p.all_skip) r = p.idr ? enqueue_idr(h, s, p, plan) : enqueue_p(h, s, p, plan);
    if (!r && !p.all_skip) r = enqueue_deblock(h, s, p, plan);
    if (!r) r = enqueue_rec_readers(h, s, p, plan);
    if (!r && !p.all_skip) r = enqueue_handover(h, s, p);
    // A still of the coded source: on the front stream, where the source is in place, behind everything of this picture that runs there (it delays none of it);
    // the source stays valid until the picture's collect() returns, and collect() waits for the still.
    if (!r && s->snap && s->snap_req.what == 0) r = snapshot_enqueue(h, s, src_y, src_uv, src_stride, h->fstream);
    if (r) return r;
    book_picture(h, s, p, pts, force_idr);
    return MI355ENC_OK;
}

// ---- the entropy-coding worker: one picture at a time, in submission order
static size_t code_access_unit(mi355enc_t *h, slot_t *s, uint8_t *out, size_t cap) {
    size_t n = 0;
    if (s->is_idr || s->ir_start) {
        n = h264_write_headers_vui(out, cap, h->cfg.width, h->cfg.height, h->cfg.fps_num, h->cfg.fps_den, h->cfg.transform8x8, h->sar_w, h->sar_h,
                                   h->col_full, h->col_prim, h->col_trc, h->col_mat);
        if (!n) return 0;
    }
    if (s->ir_start) { // a refresh cycle starts: a decoder that joins here outputs exact pictures from the cycle's last one on
        const size_t k = h264_write_recovery_sei(out + n, cap - n, h->cfg.gop - 1);
        if (!k) return 0;
        n += k;
    }
    h264_writer_set_p_slices(h->writer, s->all_skip ? 0 : h->pslice_rows, h->slice_dbf); // (an all-skip picture is one run of P_Skip macroblocks in one slice)
    const size_t m = h264_write_slice_packed_rows(h->writer, out + n, cap - n, s->is_idr, s->frame_num, s->idr_pic_id, s->qp, s->h_mbi, s->h_levels, s->h_hdr + 2);
    return m ? n + m : 0;
}
void entropy_worker(mi355enc_t *h) {
    (void)hipSetDevice(h->cfg.device_id);
    for (;;) {
        int k;
        {
            std::unique_lock<std::mutex> g(h->wk_mu);
            h->wk_cv.wait(g, [&] { return h->wk_stop || h->wk_qh != h->wk_qt; });
            if (h->wk_stop) return;
            k = h->wk_q[h->wk_qh];
        }
        slot_t *s = &h->slot[k];
        int state = 2;
        if (!s->all_skip && hipEventSynchronize(s->done) != hipSuccess) state = 3;
        const double t0 = now_ms();
        if (state == 2 && s->h_hdr[1]) state = 3; // a device-side wait ran out: collect() recovers (and queues the pictures again)
        if (state == 2) s->au_len = code_access_unit(h, s, s->au, h->au_cap);
        s->au_ms = now_ms() - t0;
        {
            std::lock_guard<std::mutex> g(h->wk_mu);
            h->wk_qh = (h->wk_qh + 1) % (NSLOT + 1);
            s->au_state = state;
        }
        h->wk_done_cv.notify_all();
    }
}
static void worker_push(mi355enc_t *h, int slot_index) {
    { std::lock_guard<std::mutex> g(h->wk_mu); h->slot[slot_index].au_state = 1; h->wk_q[h->wk_qt] = slot_index; h->wk_qt = (h->wk_qt + 1) % (NSLOT + 1); }
    h->wk_cv.notify_one();
}
// waits until the worker has nothing queued or in hand (recover() re-enqueues pictures behind its back)
static void worker_drain(mi355enc_t *h) {
    std::unique_lock<std::mutex> g(h->wk_mu);
    h->wk_done_cv.wait(g, [&] { return h->wk_qh == h->wk_qt; });
}

static const char *wait_name(unsigned code) {
    switch (code & 255u) { // (the upper bits say where: band << 8, chroma << 15, macroblock column << 16)
    case 3: return "pmb_kernel waiting for the reference's deblocking bands";
    case 4: return "wait_started_kernel";
    case 11: return "deblocker waiting for the intra bands";
    case 12: return "deblocker waiting for the strips of the band above";
    case 13: return "deblocker waiting for intra_p_kernel";
    case 14: return "intra band waiting for the lines of the band above";
    case 15: return "intra_p_kernel waiting for the row above";
    case 16: return "progress counter";
    case 17: return "deblocker waiting for pmb_kernel's rows";
    case 22: return "QP_Y chain waiting for a macroblock row";
    case 23: return "deblocker waiting for the QP_Y chain";
    default: return "injected / unknown";
    }
}
// A bounded wait on the device ran out (the kernels report it in the sticky error word, which the hand-over copies into h_hdr[1]; once
// it is set nobody waits any more, so everything in flight completes, possibly from data that was not final).  Nothing that was produced since
// can be trusted, but nothing needs to be lost either: the sources of the pictures in flight are still where submit() put them (the slots'
// staging surfaces, or the caller's device memory, which stays valid until the matching collect()).  So: drain, clear the device-side words,
// step one level down the ladder of mi355enc::safe_level, and enqueue the pictures in flight again, the first one as an IDR picture.  The
// stream continues without a gap; the decoder re-synchronises at that IDR picture.
static int recover(mi355enc_t *h, unsigned code) {
    h->safe_level++;
    h->n_recoveries++; h->last_error_word = code;
    fprintf(stderr, "mi355enc: a device-side wait timed out (error word %u: %s); %s\n", code, wait_name(code),
            h->safe_level == 1 ? "re-encoding the pictures in flight from an IDR picture; kernels run in stream order from now on" :
            h->safe_level == 2 ? "again: one launch per wavefront step from now on (no waits on the device at all)" : "giving up");
    if (h->safe_level > 2) return MI355ENC_ERR_HIP;
    if (h->wk_on) worker_drain(h); // (the pictures behind the failing one are coded and thrown away: they are enqueued again below)
    HIPCHK(hipStreamSynchronize(h->cstream));
    { int r = sync_compute(h); if (r) return r; }
    { int r = h->words.clear(h->stream); if (r) return r; }
    if (h->d_qacc) HIPCHK(hipMemsetAsync(h->d_qacc, 0, (size_t)(NSLOT + 1) * QUALITY_ACC_WORDS * sizeof(unsigned long long), h->stream)); // (every launch has completed and left its block clear; kept with the other device-side words)
    HIPCHK(hipStreamSynchronize(h->stream));
    h->dbI_busy[0] = h->dbI_busy[1] = 0;
    if (h->safe_level == 2) { h->cfg.deblock_mode = 1; h->cfg.intra_mode = 1; }
    const int n = h->pending;
    struct { const uint8_t *y, *uv; int stride, force_idr; int64_t pts; int fixed_qp, fixed_drop; } again[NSLOT];
    for (int i = 0; i < n; i++) {
        slot_t *p = &h->slot[(h->tail + i) % NSLOT];
        again[i] = {p->src_y, p->src_uv, p->src_stride, p->force_idr, p->pts, p->fixed_qp, p->fixed_drop};
        if (p->is_idr) h->idr_count--;
        p->h_hdr[1] = 0;
        if (p->rc_picked) rc_cancel(&h->rc); // their rate-control bookings (rc_cancel takes back the newest one outstanding: only the count matters)
    }
    h->n_submitted -= (uint64_t)n; h->head = h->tail; h->pending = 0; h->have_ref = 0;
    // a picture submitted under a constant-QP override is coded again under that one, not under whatever mi355enc_set_fixed_qp() has said since
    const int now_qp = h->fixed_qp.load(std::memory_order_relaxed), now_drop = h->fixed_drop.load(std::memory_order_relaxed);
    h->recovering = true;
    for (int i = 0; i < n; i++) {
        if (again[i].fixed_qp >= 0) { h->fixed_qp.store(again[i].fixed_qp, std::memory_order_relaxed); h->fixed_drop.store(again[i].fixed_drop, std::memory_order_relaxed); }
        int r = enqueue_picture(h, &h->slot[h->head], again[i].y, again[i].uv, again[i].stride, again[i].pts, i == 0 ? 1 : again[i].force_idr);
        h->fixed_qp.store(now_qp, std::memory_order_relaxed); h->fixed_drop.store(now_drop, std::memory_order_relaxed);
        if (r) { h->recovering = false; return r; }
    }
    h->recovering = false;
    return MI355ENC_OK;
}

// a sampled picture's stage timers into the statistics
static int book_stage_timers(mi355enc_t *h, slot_t *s) {
    float a = 0, b = 0, c = 0, tot = 0, sel = 0, an = 0, ip = 0;
    HIPCHK(hipEventSynchronize(s->ev[4])); // the access unit is ready before deblocking ends; the stage timers are not
    if (s->is_idr) { (void)hipEventElapsedTime(&a, s->ev[0], s->ev[1]); (void)hipEventElapsedTime(&tot, s->ev[0], s->ev[4]); }
    else { // front-stream stages and back-stream stages are timed on their own streams; the picture's total is their sum
        float fe = 0, be = 0;
        (void)hipEventElapsedTime(&a, s->ev[0], s->ev[6]);
        (void)hipEventElapsedTime(&sel, s->ev[6], s->ev[1]);
        (void)hipEventElapsedTime(&an, s->ev[1], s->ev[7]);
        (void)hipEventElapsedTime(&fe, s->ev[0], s->ev[7]);
        (void)hipEventElapsedTime(&be, s->ev[8], s->ev[4]);
        tot = fe + be;
        (void)hipEventElapsedTime(&b, s->ev[8], s->ev[11]); b += an; (void)hipEventElapsedTime(&ip, s->ev[5], s->ev[11]); // analysis + fused stage + intra macroblocks, booked as inter
        h->st.ms_select += sel; h->st.ms_analyse_p += an; h->st.ms_intra_p += ip;
    }
    (void)hipEventElapsedTime(&c, s->ev[2], s->ev[3]);
    if (s->is_idr) { h->st.ms_intra += a; h->st.n_intra++; }
    else { h->st.ms_me += a; h->st.n_me++; h->st.ms_inter += b; h->st.n_inter++; } // (ms_subpel stays 0: the refinement is part of the fused stage)
    h->st.ms_deblock += c; h->st.n_deblock++;
    if (s->is_idr) { h->st.ms_deblock_idr += c; h->st.n_deblock_idr++; }
    h->st.ms_total_gpu += tot; h->st.n_total_gpu++;
    return 0;
}

extern "C" {

int mi355enc_collect(mi355enc_t *h, uint8_t *out, size_t out_cap, size_t *out_len, int *is_keyframe, int64_t *pts, int *qp) {
    if (!h || !out || !out_len) return MI355ENC_ERR_ARG;
    if (h->pending <= 0) return MI355ENC_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    slot_t *s = &h->slot[h->tail];
    double t0 = now_ms();
    size_t m = 0;
    if (h->wk_on) { // the worker codes the access unit; here it is only copied out
        for (int attempt = 0;; attempt++) {
            { std::unique_lock<std::mutex> g(h->wk_mu); h->wk_done_cv.wait(g, [&] { return s->au_state >= 2; }); }
            if (s->au_state == 2) break;
            if (attempt >= 2 || !s->h_hdr[1]) return MI355ENC_ERR_HIP;
            int r = recover(h, s->h_hdr[1]);
            if (r) return r;
            s = &h->slot[h->tail];
        }
        h->st.ms_wait += now_ms() - t0 - s->au_ms > 0 ? now_ms() - t0 - s->au_ms : 0;
        h->st.ms_entropy += s->au_ms;
        if (!s->au_len || s->au_len > out_cap) return MI355ENC_ERR_OVERFLOW;
        memcpy(out, s->au, s->au_len);
        m = s->au_len;
        s->au_state = 0;
    } else {
        if (!s->all_skip) HIPCHK(hipEventSynchronize(s->done));
        double t1 = now_ms();
        h->st.ms_wait += t1 - t0;
        for (int attempt = 0; s->h_hdr[1]; attempt++) { // set by a kernel of this or an earlier picture that gave up waiting on the device
            if (attempt >= 2) return MI355ENC_ERR_HIP;
            int r = recover(h, s->h_hdr[1]);
            if (r) return r;
            s = &h->slot[h->tail];
            if (!s->all_skip) HIPCHK(hipEventSynchronize(s->done));
        }
        m = code_access_unit(h, s, out, out_cap);
        if (!m) return MI355ENC_ERR_OVERFLOW;
        h->st.ms_entropy += now_ms() - t1;
    }
    if (h->q_on) { int r = quality_collect(h, s); if (r) return r; } // (a picture that came back through recover(): the re-encode's)
    if (s->snap) { int r = snapshot_collect(h, s); if (r) return r; } // an armed picture: its still becomes the one mi355enc_take_snapshot codes
    *out_len = m;
    if (is_keyframe) *is_keyframe = s->is_idr || s->ir_start; // (intra refresh: a cycle's first picture is a recovery point)
    if (pts) *pts = s->pts;
    if (qp) *qp = s->qp;
    if (s->rc_picked) rc_update(&h->rc, s->is_idr, s->qp, s->drop, m); // picks and updates stay paired: a picture coded at a fixed QP booked nothing
    // Scene-cut recovery (cfg.scenecut; the oracle's orc_enc_frame applies the same rule): the summed cost of the picture's
    // macroblocks came with the hand-over.  The decision lands on picture index + 2, the first one not submitted yet whatever
    // the pipeline depth, and is skipped there if picture index + 1 turned out to be an IDR: the stream does not depend on
    // the order of submit() and collect() calls.
    if (s->is_idr) { h->sc_sum = 0; h->sc_cnt = 0; }
    else if (!s->all_skip && !h->sc_prev_skip) { // (a picture that follows P_Skip-run pictures is searched against an older source: its cost says nothing about a cut)
        const uint64_t cost = (uint64_t)s->h_hdr[2 + h->mbh] | ((uint64_t)s->h_hdr[3 + h->mbh] << 32);
        const bool pending = h->sc_force_at != ~0ull && h->sc_force_at > s->index; // a decision not yet carried out stands
        if (h->cfg.scenecut && !pending && h->sc_cnt >= 2 && cost > 3 * (h->sc_sum / (uint64_t)h->sc_cnt)) h->sc_force_at = s->index + (uint64_t)sc_lag(h);
        h->sc_sum += cost; h->sc_cnt++;
    }
    h->sc_prev_skip = s->all_skip;
    if (s->prof) { int r = book_stage_timers(h, s); if (r) return r; }
    h->st.frames++; h->st.idr_frames += s->is_idr; h->st.bytes += m;
    h->st.last_qp = (uint32_t)s->qp; h->st.last_drop = (uint32_t)s->drop; h->n_skip_pictures += s->all_skip; h->st.last_bytes = (uint32_t)m; h->st.target_bps = h->want_bps.load();
    h->last_slot = s; h->last_collected_rec = s->rec_index;
    steps_collected(h, s); // what the picture carried through the input steps becomes the last picture's (each step books its own fields; the layers let go of their images)
    roi_collected(h, s);
    h->tail = (h->tail + 1) % NSLOT; h->pending--;
    return MI355ENC_OK;
}

int mi355enc_encode(mi355enc_t *h, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride, int64_t pts, int force_idr,
                    uint8_t *out, size_t out_cap, size_t *out_len, int *is_keyframe) {
    if (!h) return MI355ENC_ERR_ARG;
    if (h->pending || h->rate.mode) return MI355ENC_ERR_STATE; // (frame-rate conversion: a submit yields any number of pictures, this call returns one)
    int r = mi355enc_submit(h, y, y_stride, uv, uv_stride, pts, force_idr);
    if (r) return r;
    return mi355enc_collect(h, out, out_cap, out_len, is_keyframe, nullptr, nullptr);
}

} // extern "C"
