// enc_plan.hpp -- the stream schedule of one picture as a value: every decision that guards a device-side wait, taken by one pure function before the
// picture's first launch; enqueue_picture() (enc_schedule.cpp) only reads it.  Plain C++, no HIP: tests/test_plan_cpu.py walks every input through
// plan_driver.cpp and holds the result against tests/planref.py.  The flags as a table: DESIGN.md section 5, "The plan of a picture".
#ifndef MI355_ENC_PLAN_HPP
#define MI355_ENC_PLAN_HPP
#include "mi355enc_dev.h" // (its plain C part: db_variant_t, pmb_gate_t, db_launch_wgs(), DB_CUT_MIN_MBW)

enum plan_stream_t { PS_MAIN, PS_FRONT, PS_INTRA, PS_HANDOVER }; // mi355enc::stream / fstream / istream / cstream

// everything the schedule depends on
struct plan_in_t {
    bool idr, all_skip, prof;                           // the picture: IDR or P, one run of P_Skip macroblocks (nothing is enqueued), stage timers sampled
    int pipeline_depth, intra_mode, deblock_mode, aq_mode, intra_in_p, i4x4, profile_overlap; // cfg
    bool overlap_allowed, exclusive_device;             // overlap_allowed(h) (safe_level, single_stream, MI355ENC_SERIAL, one open encoder), exclusive_device(h)
    bool wait_room[2];                                  // mi355enc::wait_room
    bool keep_prefilter, ref_flags;                     // d_pre_y != nullptr; rec_epoch[cur] != 0: the reference's deblocking publishes band-done words
    bool pgate, fip_rows;                               // latched at open(): pgate_on(), fip_on()
};
struct pic_plan_t {
    bool may_wait = false, split = false, pgate = false, prows = false, isplit = false, fip = false;
    plan_stream_t back = PS_MAIN;     // carries the back stage (fused P stage / intra wavefront) and waits for the front stream's event
    plan_stream_t deblock = PS_MAIN;  // carries the deblocking launch and, behind it, the readers of the reconstruction
    plan_stream_t gpu_done = PS_MAIN; // where "records and levels are final" is recorded
    bool upload_ctx = false;          // the device copy of the context is uploaded
    bool db_follows_ip = false;       // the deblocker's movers follow the intra macroblock rows' progress words (d_ip_progress)
    bool db_rows = false;             // the deblocking launch waits on the device for the fused stage's row counts (d_row_done)
};

// (a default-constructed plan is the in-order one of the single-stage entry points: everything on the main stream, no wait on the device)
inline pic_plan_t plan_picture(const plan_in_t &in) {
    pic_plan_t p;
    if (in.all_skip) return p; // the host writes the records itself: no kernel runs, the reference stays where it is
    const int intra_p = in.intra_in_p ? (in.i4x4 && in.intra_in_p > 1 ? 2 : 1) : 0; // = frame_ctx_t::intra_p as fill_ctx() sets it
    const bool qp_off = in.aq_mode != 0;                                           // = frame_ctx_t::qp_off is present
    // Every kernel of the default path takes the context by value; only the kernels replayed from a hipGraph
    // (intra_mode 1, deblock_mode 1) read the device copy, so only those pictures pay for an upload.
    p.upload_ctx = (in.idr && in.intra_mode == 1) || in.deblock_mode != 0;
    // P picture with intra macroblocks: intra_p_kernel (a chain along rows, 10..80 us) and the band deblocker (a chain along
    // x + y) overlap -- intra_p_kernel runs on a stream of its own and the deblocker's movers follow its per-row progress words
    // (GATED, k_deblock.hip); the chain pmb -> prep -> deblocker -> next pmb stays on one stream (a cross-stream event on the
    // chain costs 10-17 us).  Not on pictures whose stage timers are sampled (a gated launch's duration includes its waiting).
    // Every kernel-waits-for-kernel overlap below is opt-in (cfg.exclusive_device): next to another process's kernels on the same GPU a
    // kernel that waits on the device for a kernel that has not been placed yet can run into the bound of its wait.
    // (adaptive quantisation with Intra_4x4 in P pictures: the QP_Y chain over the whole picture sits between a picture's records and its deblocking)
    p.may_wait = in.overlap_allowed && in.exclusive_device && in.wait_room[in.idr ? 1 : 0] && in.deblock_mode == 0 && !in.keep_prefilter &&
                 !(in.prof && (in.idr || !in.profile_overlap)) && !(in.aq_mode && in.intra_in_p == 2);
    // (r03: the High-profile stream goes through the fused stage too; the two-kernel form remains behind the single-stage entry points)
    p.split = !in.idr && intra_p && p.may_wait;
    // IDR picture: the band deblocker runs on the intra stream BESIDE the intra wavefront, each of its bands waiting for the intra bands
    // of the same rows (flags + acquire); in an all-intra stream the next picture's wavefront then starts while this one is still
    // being deblocked.  What has to wait for such a deblocking: a P picture (it reads the whole reference), and whoever writes
    // the reconstruction buffer it works on (the picture after next).
    // (r04 tried the IDR picture's open-loop analysis on the front stream as well -- it needs nothing but the source: all-intra 3 469 -> 3 463 frames/s, the flat analysis
    // launch beside the previous picture's rows kernel slows that kernel by what it saves; not kept.)
    p.isplit = in.idr && in.intra_mode != 1 && p.may_wait;
    // P picture whose reference is still being deblocked: the fused stage leaves the chain too.  It runs on the intra stream, each of
    // its waves waiting for the reference's bands it reads (pmb_kernel<GATED>), so it is all but done when that deblocking ends.
    p.pgate = !in.idr && p.may_wait && in.ref_flags && in.pgate;
    // ... and with three pictures in flight (the next picture's front stages are done long before this launch ends) the deblocking launches go back
    // to back, each waiting on the device for its picture's rows; with fewer the host sits on the chain and a launch waiting on the chip only
    // gets in the way (1080p depth 1: 4465 -> 3980 frames/s, 2160p: 2050 -> 1615)
    // (Round 3 also built consecutive pictures' deblocking launches on two streams, the next picture's upper bands beside this one's lower
    // ones: +2 % at 1080p, slower at 2160p, and a bounded wait that ran out in two of four runs without a cause found -- removed in round 4;
    // what shortens the chain instead is slices with slice-local deblocking)
    p.prows = p.pgate && in.pipeline_depth >= 2;
    // One launch in flight, the intra macroblock rows inside it: the rows no longer queue behind the END of pmb_kernel (stream order) -- each starts when pmb_kernel
    // has completed its row and the row above, so the upper bands find them done when the launch starts.  Behind pmb_kernel in host order: nothing here waits for a
    // kernel that is not on the chip or in front of it in its own stream.  Not on sampled pictures (the timers bracket the launches in stream order).
    p.fip = p.prows && !qp_off && intra_p && !in.prof && in.fip_rows;
    p.back = p.pgate ? PS_INTRA : PS_MAIN;
    p.deblock = p.isplit ? PS_INTRA : PS_MAIN;
    p.gpu_done = (p.split || p.pgate) ? PS_INTRA : PS_MAIN; // records and levels are final behind intra_p_kernel / the gated fused stage; they do not depend on deblocking
    p.db_follows_ip = p.split || (p.pgate && intra_p);
    p.db_rows = p.prows;
    return p;
}

// ---- the picture's two launches that wait on the device, as they follow from its plan: which kernel, how many workgroups, and what the launches add to the
// counts that device and host keep in step (enc_sync.hpp: dev_words_t::book).  run_p_back() and run_deblock() fill pmb_launch_t / db_launch_t from here.
struct launch_counts_t { uint32_t rows = 0, started = 0, ip_done = 0, qpc = 0; }; // per row of row_done; the started, ip_done and qpc words
struct launch_shape_t {
    db_variant_t db; bool parts, qpc; // the deblocking launch: db_launch_t's variant, parts and qpc
    pmb_gate_t gate;                  // the fused P stage's gate (P pictures)
    int grid;                         // workgroups of the deblocking launch
    launch_counts_t inc;
};
// idr: frame_ctx_t::all_intra; qp_off: frame_ctx_t::qp_off is present; part_words: the handle has the parts' words (k_deblock_part_bytes(), MI355ENC_NO_SPLIT)
inline launch_shape_t plan_launches(const pic_plan_t &p, bool idr, bool qp_off, bool part_words, int mbw, int mbh) {
    launch_shape_t l;
    l.db = idr ? DB_ALL_INTRA : p.fip ? DB_P_FUSED_IP : p.db_follows_ip ? DB_P_FOLLOWS_IP : DB_P;
    l.parts = !idr && mbw >= DB_CUT_MIN_MBW && part_words; // P pictures walk every band as two workgroups (k_deblock.hip: the cut)
    l.qpc = qp_off;                                        // the QP_Y chain rides in the launch and counts the rows it has resolved
    l.gate = p.prows ? PMB_GATED_ROWS : p.pgate ? PMB_GATED : PMB_IN_ORDER;
    const db_wgs_t w = db_launch_wgs(mbh, l.db, l.parts, l.qpc);
    l.grid = w.grid;
    l.inc.rows = p.prows ? (uint32_t)mbw : 0u; // the picture's deblocking launch waits for its rows
    l.inc.started = (uint32_t)w.counted;
    l.inc.ip_done = p.fip ? (uint32_t)mbh : 0u;
    l.inc.qpc = qp_off ? (uint32_t)mbh : 0u;
    return l;
}
// open()'s wait_room: the workgroups of a picture's deblocking launch at its largest -- a P picture's bands in two parts wherever rows are long enough (whether
// the handle has the parts' words or not), its intra rows inside wherever fip_rows allows; the QP_Y chain's one small workgroup is not counted
inline int wait_room_wgs(int mbw, int mbh, bool idr, bool fip_rows) {
    return db_launch_wgs(mbh, idr ? DB_ALL_INTRA : fip_rows ? DB_P_FUSED_IP : DB_P, !idr && mbw >= DB_CUT_MIN_MBW, 0).grid;
}
#endif
