// enc_stages.cpp -- single-stage entry points of the C ABI (the same kernels the encoder launches, one stage at a time: parity
// tests and probes), mi355enc_time_stage and its table of stages, and the host-only stages (parameter sets, slice writer, rate-control model: no device needed).
// Every device entry point runs in the frame of enc_stage.hpp.
#include "enc_internal.hpp"

#include <utility>

// ---------------------------------------------------------------- single-stage entry points
// A single-stage call overwrites the reconstruction buffers, the previous-source planes and the record sets behind the encoder's back: the
// next picture submitted through the pipeline must not predict from any of it, so it is coded as an IDR picture and nothing of the
// previous picture's on-device progress words is trusted.
static void stage_touched(mi355enc_t *h) { h->have_ref = 0; h->words.forget(); h->dbI_busy[0] = h->dbI_busy[1] = 0; }
// slot 0's context for a single-stage call, on the host and on the device (behind stage_enter)
static int stage_ctx(mi355enc_t *h, int qp, bool src_is_staging, int drop = 0, int idr = 0) {
    // slice-local deblocking: a band of the deblocker never spans two slices (mi355enc_dev.h); the two settings are made separately, so the pair is checked here
    if (h->stage_slice_dbf == 2 && h->stage_slice_rows % MI355_BAND_ROWS != 0) return MI355ENC_ERR_ARG;
    slot_t *s = &h->slot[0];
    frame_ctx_t *c = s->h_ctx;
    c->src_y = src_is_staging ? s->d_src_y : nullptr; c->src_uv = src_is_staging ? s->d_src_uv : nullptr; c->src_stride = h->W;
    c->ref_y = h->d_rec_y[0]; c->ref_uv = h->d_rec_uv[0]; c->rec_y = h->d_rec_y[1]; c->rec_uv = h->d_rec_uv[1];
    c->vis_h = h->H;
    fill_ctx(h, c, qp, drop, idr);
    c->slice_rows = h->stage_slice_rows; c->slice_dbf = h->stage_slice_dbf;
    c->all_intra = 0; // the single-stage deblocking entry point takes records of either picture type
    { int r = roi_stage_ctx(h, c); if (r) return r; } // (single stages: one QP per picture, or the map of mi355enc_roi_probe_set_map)
    HIPCHK(hipMemcpyAsync(h->d_ctx, c, sizeof *c, hipMemcpyHostToDevice, h->stream));
    stage_touched(h);
    return 0;
}
// host planes of the coded size -> a reconstruction buffer (0: what a P stage predicts from, 1: what a stage reconstructs into)
static int upload_rec(mi355enc_t *h, int i, const uint8_t *y, const uint8_t *uv) {
    HIPCHK(hipMemcpyAsync(h->d_rec_y[i], y, h->ysz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_rec_uv[i], uv, h->csz, hipMemcpyHostToDevice, h->stream));
    return 0;
}
static int download_picture(mi355enc_t *h, void *mbinfo, uint8_t *rec_y, uint8_t *rec_uv, int16_t *levels) {
    HIPCHK(hipMemcpyAsync(mbinfo, h->d_mbi, (size_t)h->nmb * sizeof(mb_info_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(rec_y, h->d_rec_y[1], h->ysz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(rec_uv, h->d_rec_uv[1], h->csz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(levels, h->d_levels, (size_t)h->nmb * MB_LEVELS * 2, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---------------------------------------------------------------- the timed stages: one row per stage of mi355enc_time_stage (the numbers are the ABI's)
enum {
    TS_ME = 0, TS_INTER, TS_INTRA, TS_DEBLOCK, TS_SUBPEL, TS_CSC_I420, TS_CSC_YUY2, TS_CSC_UYVY, TS_ME_SELECT, TS_PMB, TS_INTRA_P, TS_QUALITY, TS_JPEG, TS_ORIENT, TS_SCALE,
    TS_IMAGE, TS_SNAPSHOT, TS_YUV_CONVERT, TS_RATE, TS_HDR_P010, TS_HDR_I420_10, TS_HDR_V210, TS_DEEP_P010, TS_ADJUST_POINT, TS_ADJUST_SHARPEN, TS_DENOISE,
    TS_DENOISE_PRIME, TS_DENOISE_SEARCH, TS_DENOISE_MC, TS_STAB_PROJECT, TS_STAB_MATCH, TS_WARP, TS_AL_MEASURE, TS_AL_DECIDE, TS_AL_APPLY, TS_LUT3D, TS_DSPATIAL, TS_DSPATIAL_AUTO, TS_MASK_CELLS, TS_MASK_BLUR, TS_COUNT
};
// ready: the precondition (false: MI355ENC_ERR_STATE); prepare: once, outside the timed loop; launch: the body of the loop; done: behind the timed loop;
// needs_raw: slot 0's raw staging buffer must exist (any bytes will do as a source: 0x55).  Null: nothing.
struct ts_row_t {
    int stage;
    bool (*ready)(mi355enc_t *h, int stage);
    int (*prepare)(mi355enc_t *h, slot_t *s, ts_ctx_t *x);
    int (*launch)(mi355enc_t *h, slot_t *s, ts_ctx_t *x);
    void (*done)(mi355enc_t *h);
    bool needs_raw;
};
static bool ts_has_scale(mi355enc_t *h, int) { return h->d_scale_tab != nullptr; } // (mi355enc_set_input_size or mi355enc_set_input_geometry first)
static bool ts_has_yuv(mi355enc_t *h, int) { return h->yuv_on; }                   // (the handle has no conversion)
static bool ts_has_keep(mi355enc_t *h, int) { return h->d_keep != nullptr; }       // (frame-rate conversion off, or hold mode without a keep buffer: there is no mix)
static bool ts_has_hdr(mi355enc_t *h, int) { return h->hdr_on && !hdr_refuses(h, MI355ENC_FMT_P010); } // (mi355enc_set_hdr_input first, and an output matrix it converts to)
static int ts_me(mi355enc_t *h, slot_t *s, ts_ctx_t *) { k_launch_me(s->h_ctx, h->mbw, h->stream); return 0; }
static int ts_inter(mi355enc_t *h, slot_t *s, ts_ctx_t *) { k_launch_inter(s->h_ctx, h->mbw, h->stream); return 0; }
static int ts_subpel(mi355enc_t *h, slot_t *s, ts_ctx_t *) { k_launch_subpel(s->h_ctx, h->mbw, h->stream); return 0; }
static int ts_me_select(mi355enc_t *h, slot_t *s, ts_ctx_t *) { k_launch_me_select(s->h_ctx, h->mbw, h->d_imv[0][0], h->d_imv[0][1], nullptr, 0, h->stream); return 0; }
static int ts_pmb(mi355enc_t *h, slot_t *s, ts_ctx_t *) { return run_pmb(h, s->h_ctx, 1, pic_plan_t(), h->stream); }
// a fresh stamp per launch: the lines / strips between bands are epoch-tagged
static void ts_stamp(mi355enc_t *h, slot_t *s) { if (++h->epoch == 0) h->epoch = 1; s->h_ctx->epoch = h->epoch; }
static int ts_intra(mi355enc_t *h, slot_t *s, ts_ctx_t *) { ts_stamp(h, s); return run_intra(h, 0, s->h_ctx); }
static int ts_deblock(mi355enc_t *h, slot_t *s, ts_ctx_t *) { ts_stamp(h, s); return run_deblock(h, 0, s->h_ctx); }
static int ts_intra_p_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *) { return h->words.ip_rows_stamp(s->h_ctx->epoch, h->stream); }
static int ts_intra_p(mi355enc_t *h, slot_t *s, ts_ctx_t *) { k_launch_intra_p(s->h_ctx, h->mbw, h->mbh, h->words.ip_progress(), h->d_ip_strips, h->words.err(), h->stream); return 0; }
static int ts_quality_prepare(mi355enc_t *h, slot_t *, ts_ctx_t *) { return quality_alloc(h); } // (the block of the stage entry points)
static int ts_quality(mi355enc_t *h, slot_t *s, ts_ctx_t *) {
    unsigned long long *acc = h->d_qacc + (size_t)NSLOT * QUALITY_ACC_WORDS, *res = h->h_qres + (size_t)NSLOT * QUALITY_WORDS;
    k_launch_quality(s->d_src_y, s->d_src_uv, h->W, h->d_rec_y[1], h->d_rec_uv[1], h->W, h->cfg.width, h->cfg.height, acc, res, h->stream); return 0;
}
static int ts_jpeg_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *) { return jpeg_alloc(h, s); }
// the conversion launch of a picture of the coded visible size in the raw staging buffer: 5 I420, 6 YUY2, 7 UYVY; 19 P010, 20 I420_10, 21 V210 tone-mapped
// (DESIGN.md section 22); 22 P010 plain (section 20)
static int ts_convert(mi355enc_t *h, slot_t *s, ts_ctx_t *x) {
    const int t = x->stage, fmt = t <= TS_CSC_UYVY ? MI355ENC_FMT_I420 + t - TS_CSC_I420 : t == TS_DEEP_P010 ? MI355ENC_FMT_P010 : MI355ENC_FMT_P010 + t - TS_HDR_P010;
    const int w = h->cfg.width, ht = h->cfg.height;
    fmt_plane_t pl[3];
    const uint8_t *p[3];
    int st[3];
    raw_layout(fmt, w, ht, s->d_raw, p, st, pl);
    const int r = t <= TS_CSC_UYVY ? k_launch_csc(fmt, p[0], p[1], p[2], st[0], st[1], st[2], s->d_src_y, s->d_src_uv, w, ht, h->W, h->H, h->stream)
                : t == TS_DEEP_P010 ? k_launch_csc2(fmt, p[0], p[1], p[2], st[0], st[1], st[2], s->d_src_y, s->d_src_uv, w, ht, h->W, h->H, h->csc_coef, h->stream)
                                    : hdr_convert(h, fmt, p, st, s->d_src_y, s->d_src_uv, w, ht, h->W, h->H, h->stream);
    return !r ? 0 : r < -1 ? r : MI355ENC_ERR_ARG;
}
// orientation: an NV12 picture of the pre-orientation size in the raw staging buffer -> the coded surfaces
static int ts_orient(mi355enc_t *h, slot_t *s, ts_ctx_t *) {
    const int m = h->orient ? h->orient : MI355ENC_ORIENT_90R, pw = orient_transposes(m) ? h->cfg.height : h->cfg.width, ph = orient_transposes(m) ? h->cfg.width : h->cfg.height;
    const int ps = (pw + 15) & ~15;
    return k_launch_orient(m, s->d_raw, ps, s->d_raw + (size_t)ps * ph, ps, pw, ph, s->d_src_y, s->d_src_uv, h->W, h->H, h->stream) ? MI355ENC_ERR_ARG : 0;
}
// the scale / geometry launch: an NV12 picture of the input size in the raw staging buffer -> the input target (a stale slot copy of the tables travels in prepare)
static int ts_scale_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *x) { return (x->scale = scale_plan_for(h, s, h->stream)) ? 0 : MI355ENC_ERR_HIP; }
static int ts_scale(mi355enc_t *h, slot_t *s, ts_ctx_t *x) {
    const int ds = (h->in_w + 15) & ~15;
    in_target_t t;
    { int r = input_target(h, s, &t); if (r) return r; }
    return k_launch_scale(MI355ENC_FMT_NV12, s->d_raw, s->d_raw + (size_t)ds * h->in_h, nullptr, ds, ds, 0, t.y, t.uv, t.W, t.H, x->scale, h->stream) ? MI355ENC_ERR_ARG : 0;
}
static int ts_image(mi355enc_t *h, slot_t *, ts_ctx_t *x) { k_launch_image_blend(&x->img, h->stream); return 0; }
static int ts_yuv(mi355enc_t *h, slot_t *s, ts_ctx_t *) { return yuv_run(h, s, h->stream); }            // the colour step, in place on slot 0's surfaces (whatever they hold)
static int ts_rate(mi355enc_t *h, slot_t *s, ts_ctx_t *) { return rate_mix(h, s, s, 128, true, h->stream); } // the mix of the keep buffer and slot 0's surfaces, in place as the encoder runs it
static constexpr ts_row_t k_ts[] = {
    // stage                ready               prepare                 launch                 done               needs_raw
    {TS_ME,             nullptr,            nullptr,                ts_me,                 nullptr,           false},
    {TS_INTER,          nullptr,            nullptr,                ts_inter,              nullptr,           false},
    {TS_INTRA,          nullptr,            nullptr,                ts_intra,              nullptr,           false},
    {TS_DEBLOCK,        nullptr,            nullptr,                ts_deblock,            nullptr,           false},
    {TS_SUBPEL,         nullptr,            nullptr,                ts_subpel,             nullptr,           false},
    {TS_CSC_I420,       nullptr,            nullptr,                ts_convert,            nullptr,           true},
    {TS_CSC_YUY2,       nullptr,            nullptr,                ts_convert,            nullptr,           true},
    {TS_CSC_UYVY,       nullptr,            nullptr,                ts_convert,            nullptr,           true},
    {TS_ME_SELECT,      nullptr,            nullptr,                ts_me_select,          nullptr,           false},
    {TS_PMB,            nullptr,            nullptr,                ts_pmb,                nullptr,           false},
    {TS_INTRA_P,        nullptr,            ts_intra_p_prepare,     ts_intra_p,            nullptr,           false},
    {TS_QUALITY,        nullptr,            ts_quality_prepare,     ts_quality,            nullptr,           false},
    {TS_JPEG,           nullptr,            ts_jpeg_prepare,        jpeg_time_launch,      nullptr,           false},
    {TS_ORIENT,         nullptr,            nullptr,                ts_orient,             nullptr,           true},
    {TS_SCALE,          ts_has_scale,       ts_scale_prepare,       ts_scale,              nullptr,           true},
    {TS_IMAGE,          nullptr,            image_time_prepare,     ts_image,              nullptr,           false}, // (prepare: ERR_STATE without an image on layer 0)
    {TS_SNAPSHOT,       nullptr,            snapshot_time_prepare,  snapshot_time_launch,  nullptr,           false},
    {TS_YUV_CONVERT,    ts_has_yuv,         nullptr,                ts_yuv,                nullptr,           false},
    {TS_RATE,           ts_has_keep,        nullptr,                ts_rate,               nullptr,           false},
    {TS_HDR_P010,       ts_has_hdr,         nullptr,                ts_convert,            nullptr,           true},
    {TS_HDR_I420_10,    ts_has_hdr,         nullptr,                ts_convert,            nullptr,           true},
    {TS_HDR_V210,       ts_has_hdr,         nullptr,                ts_convert,            nullptr,           true},
    {TS_DEEP_P010,      nullptr,            nullptr,                ts_convert,            nullptr,           true},
    {TS_ADJUST_POINT,   adjust_time_ready,  nullptr,                adjust_time_launch,    nullptr,           false}, // (mi355enc_set_adjust first: 23 with sharpen 0, 24 with sharpen set)
    {TS_ADJUST_SHARPEN, adjust_time_ready,  nullptr,                adjust_time_launch,    nullptr,           false},
    {TS_DENOISE,        denoise_time_ready, nullptr,                denoise_time_launch,   denoise_time_done, false}, // (mi355enc_set_denoise first; 27 / 28: and mi355enc_set_denoise_motion)
    {TS_DENOISE_PRIME,  denoise_time_ready, nullptr,                denoise_time_launch,   denoise_time_done, false},
    {TS_DENOISE_SEARCH, denoise_time_ready, nullptr,                denoise_time_launch,   denoise_time_done, false},
    {TS_DENOISE_MC,     denoise_time_ready, nullptr,                denoise_time_launch,   denoise_time_done, false},
    {TS_STAB_PROJECT,   stab_time_ready,    stab_time_prepare,      stab_time_launch,      stab_time_done,    true},  // (mi355enc_set_stabilize and a geometry first)
    {TS_STAB_MATCH,     stab_time_ready,    stab_time_prepare,      stab_time_launch,      stab_time_done,    false},
    {TS_WARP,           warp_time_ready,    warp_time_prepare,      warp_time_launch,      warp_time_done,    false}, // (mi355enc_set_warp first)
    {TS_AL_MEASURE,     autolevel_time_ready, autolevel_time_prepare, autolevel_time_launch, autolevel_time_done, false}, // (mi355enc_set_autolevel first)
    {TS_AL_DECIDE,      autolevel_time_ready, autolevel_time_prepare, autolevel_time_launch, autolevel_time_done, false},
    {TS_AL_APPLY,       autolevel_time_ready, autolevel_time_prepare, autolevel_time_launch, autolevel_time_done, false},
    {TS_LUT3D,          lut3d_time_ready,   lut3d_time_prepare,     lut3d_time_launch,     lut3d_time_done,   false}, // (mi355enc_set_lut3d first)
    {TS_DSPATIAL,       dspatial_time_ready, nullptr,               dspatial_time_launch,  dspatial_time_done, false}, // (mi355enc_set_denoise_spatial first: a manual setting)
    {TS_DSPATIAL_AUTO,  dspatial_time_ready, nullptr,               dspatial_time_launch,  dspatial_time_done, false}, // (... an automatic one)
    {TS_MASK_CELLS,     mask_time_ready,    mask_time_prepare,      mask_time_launch,      nullptr,           false}, // (mi355enc_set_mask first: 38 with a fill or pixelate region, 39 with a blur region)
    {TS_MASK_BLUR,      mask_time_ready,    mask_time_prepare,      mask_time_launch,      nullptr,           false},
};
static_assert(sizeof k_ts / sizeof k_ts[0] == 40 && TS_COUNT == 40, "one row per stage 0 .. 39");
template <size_t... I> static constexpr bool ts_rows_in_order(std::index_sequence<I...>) { return ((k_ts[I].stage == (int)I) && ...); }
static_assert(ts_rows_in_order(std::make_index_sequence<TS_COUNT>()), "row i describes stage i");

extern "C" {

int mi355enc_stage_me(mi355enc_t *h, const uint8_t *cur_y, const uint8_t *ref_y, int qp, uint16_t *surf_out, void *imv_out) {
    if (!h || !cur_y || !ref_y || !imv_out || qp < 0 || qp > 51) return MI355ENC_ERR_ARG;
    int r = stage_enter(h); if (r) return r;
    HIPCHK(hipMemcpyAsync(h->slot[0].d_src_y, cur_y, h->ysz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_psrc[h->psrc_cur], ref_y, h->ysz, hipMemcpyHostToDevice, h->stream)); // what the search runs against (in the encoder: the previous source)
    r = stage_ctx(h, qp, true); if (r) return r;
    k_launch_me(h->slot[0].h_ctx, h->mbw, h->stream);
    HIPCHK(hipMemcpyAsync(imv_out, h->d_imv[0][0], (size_t)h->nmb * sizeof(imv_t), hipMemcpyDeviceToHost, h->stream));
    if (surf_out) HIPCHK(hipMemcpyAsync(surf_out, h->d_surf[0], (size_t)h->nmb * SURF_U16 * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}
// imv_prev null: the first selection.  Otherwise the form the encoder's later iterations use (me_select_sparse_kernel): imv_prev is the field imv_in was selected
// from -- a macroblock whose predictors are the same in both copies its entry of imv_in.  Must equal the first form whenever imv_in really is the selection over imv_prev.
static int me_select(mi355enc_t *h, const uint16_t *surf, const void *imv_in, const void *imv_prev, int qp, void *imv_out) {
    if (!h || !surf || !imv_in || !imv_out || qp < 0 || qp > 51) return MI355ENC_ERR_ARG;
    int r = stage_enter(h); if (r) return r;
    r = stage_ctx(h, qp, true); if (r) return r;
    HIPCHK(hipMemcpyAsync(h->d_surf[0], surf, (size_t)h->nmb * SURF_U16 * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_imv[0][0], imv_in, (size_t)h->nmb * sizeof(imv_t), hipMemcpyHostToDevice, h->stream));
    if (imv_prev) HIPCHK(hipMemcpyAsync(h->d_imv[0][2], imv_prev, (size_t)h->nmb * sizeof(imv_t), hipMemcpyHostToDevice, h->stream));
    k_launch_me_select(h->slot[0].h_ctx, h->mbw, h->d_imv[0][0], h->d_imv[0][1], imv_prev ? h->d_imv[0][2] : nullptr, imv_prev ? 2 : 0, h->stream);
    HIPCHK(hipMemcpyAsync(imv_out, h->d_imv[0][1], (size_t)h->nmb * sizeof(imv_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}
int mi355enc_stage_me_select(mi355enc_t *h, const uint16_t *surf, const void *imv_in, int qp, void *imv_out) { return me_select(h, surf, imv_in, nullptr, qp, imv_out); }
int mi355enc_stage_me_select_next(mi355enc_t *h, const uint16_t *surf, const void *imv_in, const void *imv_prev, int qp, void *imv_out) { return imv_prev ? me_select(h, surf, imv_in, imv_prev, qp, imv_out) : MI355ENC_ERR_ARG; }
int mi355enc_stage_subpel(mi355enc_t *h, const uint8_t *cur_y, const uint8_t *ref_y, int qp, void *mbinfo_inout) {
    if (!h || !cur_y || !ref_y || !mbinfo_inout || qp < 0 || qp > 51) return MI355ENC_ERR_ARG;
    int r = stage_enter(h); if (r) return r;
    HIPCHK(hipMemcpyAsync(h->slot[0].d_src_y, cur_y, h->ysz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_rec_y[0], ref_y, h->ysz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_mbi, mbinfo_inout, (size_t)h->nmb * sizeof(mb_info_t), hipMemcpyHostToDevice, h->stream));
    r = stage_ctx(h, qp, true); if (r) return r;
    k_launch_subpel(h->slot[0].h_ctx, h->mbw, h->stream);
    HIPCHK(hipMemcpyAsync(mbinfo_inout, h->d_mbi, (size_t)h->nmb * sizeof(mb_info_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}
int mi355enc_stage_inter(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, const uint8_t *ref_y, const uint8_t *ref_uv,
                         int qp, void *mbinfo_inout, uint8_t *rec_y, uint8_t *rec_uv, int16_t *levels) {
    if (!h || !src_y || !src_uv || !ref_y || !ref_uv || !mbinfo_inout || !rec_y || !rec_uv || !levels || qp < 0 || qp > 51) return MI355ENC_ERR_ARG;
    if (h->cfg.transform8x8 == 2) return MI355ENC_ERR_ARG; // the two-kernel form has no per-macroblock transform choice (the fused stage has: mi355enc_stage_pmb)
    int r = stage_enter(h); if (r) return r;
    r = stage_in(h, &h->slot[0], src_y, src_uv); if (r) return r;
    r = upload_rec(h, 0, ref_y, ref_uv); if (r) return r;
    HIPCHK(hipMemcpyAsync(h->d_mbi, mbinfo_inout, (size_t)h->nmb * sizeof(mb_info_t), hipMemcpyHostToDevice, h->stream));
    r = stage_ctx(h, qp, true); if (r) return r;
    k_launch_inter(h->slot[0].h_ctx, h->mbw, h->stream);
    return download_picture(h, mbinfo_inout, rec_y, rec_uv, levels) ? MI355ENC_ERR_HIP : MI355ENC_OK;
}
int mi355enc_stage_pmb(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, const uint8_t *ref_y, const uint8_t *ref_uv,
                       int qp, int drop, int refine, const void *imv, const uint16_t *surf, const void *idec, int run_intra_p,
                       void *mbinfo_out, uint8_t *rec_y, uint8_t *rec_uv, int16_t *levels) {
    if (!h || !src_y || !src_uv || !ref_y || !ref_uv || !imv || !surf || !mbinfo_out || !rec_y || !rec_uv || !levels || qp < 0 || qp > 51 || drop < 0 || drop > DROP_MAX)
        return MI355ENC_ERR_ARG;
    int r = stage_enter(h); if (r) return r;
    r = stage_in(h, &h->slot[0], src_y, src_uv); if (r) return r;
    r = upload_rec(h, 0, ref_y, ref_uv); if (r) return r;
    r = stage_ctx(h, qp, true, drop); if (r) return r;
    frame_ctx_t *c = h->slot[0].h_ctx;
    c->intra_p = idec ? 1 : 0;
    HIPCHK(hipMemcpyAsync((void *)k_final_imv(c), imv, (size_t)h->nmb * sizeof(imv_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_surf[0], surf, (size_t)h->nmb * SURF_U16 * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    if (idec) HIPCHK(hipMemcpyAsync(h->d_idec, idec, (size_t)h->nmb * IDEC_BYTES, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->d_rec_y[1], 0, h->ysz, h->stream)); // macroblocks decided intra stay untouched unless run_intra_p
    HIPCHK(hipMemsetAsync(h->d_rec_uv[1], 0, h->csz, h->stream));
    HIPCHK(hipMemsetAsync(h->d_levels, 0, (size_t)h->nmb * MB_LEVELS * 2, h->stream));
    r = run_pmb(h, c, refine ? 1 : 0, pic_plan_t(), h->stream); if (r) return r;
    if (idec && run_intra_p) { r = h->words.ip_rows_stamp(c->epoch, h->stream); if (r) return r; }
    if (idec && run_intra_p) k_launch_intra_p(c, h->mbw, h->mbh, h->words.ip_progress(), h->d_ip_strips, h->words.err(), h->stream);
    HIPCHK(hipGetLastError());
    return download_picture(h, mbinfo_out, rec_y, rec_uv, levels) ? MI355ENC_ERR_HIP : MI355ENC_OK;
}
int mi355enc_stage_intra(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, int qp, int drop, void *mbinfo_out, uint8_t *rec_y,
                         uint8_t *rec_uv, int16_t *levels) {
    if (!h || !src_y || !src_uv || !mbinfo_out || !rec_y || !rec_uv || !levels || qp < 0 || qp > 51 || drop < 0 || drop > DROP_MAX) return MI355ENC_ERR_ARG;
    int r = stage_enter(h); if (r) return r;
    r = stage_in(h, &h->slot[0], src_y, src_uv); if (r) return r;
    r = stage_ctx(h, qp, true, drop, 1); if (r) return r;
    r = run_intra(h, 0, h->slot[0].h_ctx); if (r) return r;
    return download_picture(h, mbinfo_out, rec_y, rec_uv, levels) ? MI355ENC_ERR_HIP : MI355ENC_OK;
}
int mi355enc_stage_intra_analyse(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, int qp, uint16_t *isad_out, void *idec_out) {
    if (!h || !src_y || !src_uv || !isad_out || qp < 0 || qp > 51) return MI355ENC_ERR_ARG;
    int r = stage_enter(h); if (r) return r;
    r = stage_in(h, &h->slot[0], src_y, src_uv); if (r) return r;
    r = stage_ctx(h, qp, true); if (r) return r;
    k_launch_intra_analyse(h->slot[0].h_ctx, h->mbw, h->mbh, 0, h->stream);
    HIPCHK(hipMemcpyAsync(isad_out, h->d_isad, (size_t)h->nmb * ISAD_PER_MB * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
    if (idec_out) HIPCHK(hipMemcpyAsync(idec_out, h->d_idec, (size_t)h->nmb * IDEC_BYTES, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}
int mi355enc_stage_deblock(mi355enc_t *h, uint8_t *rec_y, uint8_t *rec_uv, const void *mbinfo) {
    if (!h || !rec_y || !rec_uv || !mbinfo) return MI355ENC_ERR_ARG;
    int r = stage_enter(h); if (r) return r;
    r = upload_rec(h, 1, rec_y, rec_uv); if (r) return r;
    HIPCHK(hipMemcpyAsync(h->d_mbi, mbinfo, (size_t)h->nmb * sizeof(mb_info_t), hipMemcpyHostToDevice, h->stream));
    r = stage_ctx(h, 26, false); if (r) return r;
    r = run_deblock(h, 0, h->slot[0].h_ctx); if (r) return r;
    HIPCHK(hipMemcpyAsync(rec_y, h->d_rec_y[1], h->ysz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(rec_uv, h->d_rec_uv[1], h->csz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}
// quality metrics, the kernel alone: host planes of the coded size through the encoder's own surfaces ...
int mi355enc_stage_quality(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, const uint8_t *rec_y, const uint8_t *rec_uv, mi355enc_quality_t *q) {
    if (!h || !src_y || !src_uv || !rec_y || !rec_uv || !q) return MI355ENC_ERR_ARG;
    slot_t *s = &h->slot[0];
    int r = stage_enter(h); if (r) return r;
    r = stage_in(h, s, src_y, src_uv); if (r) return r;
    r = upload_rec(h, 1, rec_y, rec_uv); if (r) return r;
    stage_touched(h);
    return quality_run(h, s->d_src_y, s->d_src_uv, h->W, h->d_rec_y[1], h->d_rec_uv[1], q);
}
// ... and planes that lie on the device, where they lie
int mi355enc_stage_quality_device(mi355enc_t *h, const void *d_src_y, const void *d_src_uv, int src_stride, const void *d_rec_y, const void *d_rec_uv, mi355enc_quality_t *q) {
    if (!h || !d_src_y || !d_src_uv || !d_rec_y || !d_rec_uv || !q || src_stride < h->cfg.width) return MI355ENC_ERR_ARG;
    int r = stage_enter(h); if (r) return r;
    return quality_run(h, (const uint8_t *)d_src_y, (const uint8_t *)d_src_uv, src_stride, (const uint8_t *)d_rec_y, (const uint8_t *)d_rec_uv, q);
}
int mi355enc_debug_trip_wait(mi355enc_t *h, unsigned code) {
    if (!h || !code) return MI355ENC_ERR_ARG;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    { int r = sync_compute(h); if (r) return r; }
    return h->words.trip(code);
}
int mi355enc_debug_get_counters(mi355enc_t *h, mi355enc_counters_t *out) {
    if (!h || !out) return MI355ENC_ERR_ARG;
    *out = {h->epoch, 0u, 0u, 0u, 0u, (uint32_t)h->idr_count, (uint32_t)h->frames_since_idr, 0u};
    h->words.get(out);
    return MI355ENC_OK;
}
// The four counts go through their owner (dev_words_t::set: word and total together); the band-done words and their epochs, the strips and progress words
// tagged with an epoch, and the parity of the band parts' counters stay as the last picture left them.
int mi355enc_debug_set_counters(mi355enc_t *h, const mi355enc_counters_t *in) {
    if (!h || !in || (!(in->keep & 64u) && in->frames_since_idr > 0x7FFFFFFFu) || (!(in->keep & 32u) && in->idr_count > 0x7FFFFFFFu)) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; }
    if (!(in->keep & 1u)) h->epoch = in->epoch;
    { int r = h->words.set(in); if (r) return r; }
    if (!(in->keep & 32u)) h->idr_count = (int)in->idr_count;
    if (!(in->keep & 64u)) h->frames_since_idr = (int)in->frames_since_idr;
    return MI355ENC_OK;
}
int mi355enc_time_stage(mi355enc_t *h, int stage, int iters, double *avg_ms) {
    if (!h || !avg_ms || iters < 1 || stage < 0 || stage >= TS_COUNT) return MI355ENC_ERR_ARG;
    const ts_row_t &row = k_ts[stage];
    if (row.ready && !row.ready(h, stage)) return MI355ENC_ERR_STATE;
    { int r = stage_enter(h); if (r) return r; }
    slot_t *s = &h->slot[0];
    // a valid context in both places: the LAST COLLECTED picture's host copy (the slots rotate: it is slot 0's only one time in three), brought
    // to slot 0 and re-uploaded -- or a fresh stage context.  The stages run on that picture's surfaces in place (stage 3 filters its
    // reconstruction again), so the next picture through the pipeline starts a new GOP.
    if (!h->have_ref || !h->last_slot) { int r = stage_ctx(h, 26, true); if (r) return r; }
    else {
        if (h->last_slot != s) *s->h_ctx = *h->last_slot->h_ctx;
        HIPCHK(hipMemcpyAsync(h->d_ctx, s->h_ctx, sizeof(frame_ctx_t), hipMemcpyHostToDevice, h->stream));
        stage_touched(h);
    }
    if (row.needs_raw && !s->d_raw) {
        HIPCHK(hipMalloc((void **)&s->d_raw, raw_bytes(h)));
        HIPCHK(hipMemsetAsync(s->d_raw, 0x55, raw_bytes(h), h->stream));
    }
    ts_ctx_t x; x.stage = stage; x.scale = nullptr; // what prepare hands to launch
    if (row.prepare) { int r = row.prepare(h, s, &x); if (r) return r; }
    for (int warm = 0; warm < 2; warm++) {
        if (warm) HIPCHK(hipEventRecord(s->ev[0], h->stream));
        for (int i = 0; i < (warm ? iters : 1); i++) { int r = row.launch(h, s, &x); if (r) return r; }
        if (warm) HIPCHK(hipEventRecord(s->ev[1], h->stream));
    }
    HIPCHK(hipEventSynchronize(s->ev[1]));
    if (row.done) row.done(h); // (the noise filter: a stream that follows primes, it does not filter against what the probe left)
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
    *avg_ms = (double)ms / iters;
    return MI355ENC_OK;
}

// ---------------------------------------------------------------- host-only stages
int mi355enc_host_write_headers(int width, int height, int fps_num, int fps_den, int t8, uint8_t *out, size_t cap, size_t *out_len) {
    if (!out || !out_len || width < 16 || height < 16 || fps_num <= 0 || fps_den <= 0) return MI355ENC_ERR_ARG;
    size_t n = h264_write_headers(out, cap, width, height, fps_num, fps_den, t8);
    if (!n) return MI355ENC_ERR_OVERFLOW;
    *out_len = n;
    return MI355ENC_OK;
}
static int g_host_slice_rows = 0;
static int g_host_pslice_rows = 0, g_host_dbf_idc = 0;
void mi355enc_host_set_slice_rows(int rows) { g_host_slice_rows = rows > 0 ? rows : 0; }
void mi355enc_host_set_p_slices(int rows, int dbf_idc) { g_host_pslice_rows = rows > 0 ? rows : 0; g_host_dbf_idc = dbf_idc == 2 ? 2 : 0; }
int mi355enc_stage_set_slice_rows(mi355enc_t *h, int rows) { if (!h || rows < 0) return MI355ENC_ERR_ARG; h->stage_slice_rows = rows; return MI355ENC_OK; }
int mi355enc_slice_rows(const mi355enc_t *h) { return h ? h->islice_rows : 0; }
int mi355enc_p_slice_rows(const mi355enc_t *h) { return h ? h->pslice_rows : 0; }
int mi355enc_stage_set_slice_deblock(mi355enc_t *h, int idc) { if (!h || (idc != 0 && idc != 2)) return MI355ENC_ERR_ARG; h->stage_slice_dbf = idc; return MI355ENC_OK; }
int mi355enc_host_write_slice(int mbw, int mbh, int is_idr, int frame_num, int idr_pic_id, int qp, int t8, const void *mbinfo,
                              const int16_t *levels, uint8_t *out, size_t cap, size_t *out_len) {
    if (!out || !out_len || !mbinfo || !levels || mbw < 1 || mbh < 1 || qp < 0 || qp > 51) return MI355ENC_ERR_ARG;
    h264_writer_t *w = h264_writer_new(mbw, mbh, t8);
    if (!w) return MI355ENC_ERR_NOMEM;
    h264_writer_set_slice_rows(w, g_host_slice_rows);
    h264_writer_set_p_slices(w, g_host_pslice_rows, g_host_dbf_idc);
    size_t n = h264_write_slice(w, out, cap, is_idr, frame_num, idr_pic_id, qp, (const mb_info_t *)mbinfo, levels);
    h264_writer_free(w);
    if (!n) return MI355ENC_ERR_OVERFLOW;
    *out_len = n;
    return MI355ENC_OK;
}
// Host statement of what levels_pack_kernel + levels_scan_kernel hand over (same block order), then the slice writer on
// `threads` host threads: lets the row-parallel coder be checked against the dense single-thread one without a device.
int mi355enc_host_write_slice_packed(int mbw, int mbh, int is_idr, int frame_num, int idr_pic_id, int qp, int t8, int threads, const void *mbinfo,
                                     const int16_t *levels, uint8_t *out, size_t cap, size_t *out_len) {
    if (!out || !out_len || !mbinfo || !levels || mbw < 1 || mbh < 1 || qp < 0 || qp > 51 || threads < 1) return MI355ENC_ERR_ARG;
    const mb_info_t *mbi = (const mb_info_t *)mbinfo;
    const size_t nmb = (size_t)mbw * mbh;
    int16_t *packed = (int16_t *)malloc(nmb * PACK_BLOCKS_MAX * 32 + 32);
    uint32_t *row_off = (uint32_t *)malloc((size_t)mbh * sizeof(uint32_t));
    h264_writer_t *w = h264_writer_new(mbw, mbh, t8);
    int rc = MI355ENC_ERR_NOMEM;
    if (packed && row_off && w && h264_writer_set_threads(w, threads) == 0) {
        h264_writer_set_slice_rows(w, g_host_slice_rows);
        h264_writer_set_p_slices(w, g_host_pslice_rows, g_host_dbf_idc);
        h264_pack_levels(mbw, mbh, mbi, levels, packed, row_off);
        size_t n = h264_write_slice_packed_rows(w, out, cap, is_idr, frame_num, idr_pic_id, qp, mbi, packed, row_off);
        rc = n ? MI355ENC_OK : MI355ENC_ERR_OVERFLOW;
        *out_len = n;
    }
    h264_writer_free(w); free(packed); free(row_off);
    return rc;
}
int mi355enc_host_cavlc_block(const int16_t *coef, int maxnum, int nC, uint8_t *out, size_t cap) {
    if (!coef || !out) return MI355ENC_ERR_ARG;
    return h264_cavlc_block_bits(coef, maxnum, nC, out, cap);
}
static_assert(sizeof(rc_state_t) <= MI355ENC_RC_BYTES, "MI355ENC_RC_BYTES too small");
void mi355enc_rc_init(void *rc, double fps, int gop, uint32_t bps, int qp_min, int qp_max) { rc_init((rc_state_t *)rc, fps, gop, bps, qp_min, qp_max); }
void mi355enc_rc_set_bitrate(void *rc, uint32_t bps) { rc_set_bitrate((rc_state_t *)rc, bps); }
void mi355enc_rc_pick(void *rc, int is_idr, int *qp, int *drop) { int q = 0, d = 0; rc_pick((rc_state_t *)rc, is_idr, &q, &d); if (qp) *qp = q; if (drop) *drop = d; }
void mi355enc_rc_update(void *rc, int is_idr, int qp, int drop, size_t bytes) { rc_update((rc_state_t *)rc, is_idr, qp, drop, bytes); }

} // extern "C"
