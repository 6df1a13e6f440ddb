// enc_input.cpp -- the input path of the C-ABI shim: from "the caller hands over a picture" to "the slot's NV12 source surfaces are ready".
//
// Every submit entry point is four steps ("The input path"):
//   its own argument checks
//   ingest_begin   the pipeline-full check (with frame-rate conversion: the rule's step, which says how many pictures the submit yields), the slot, the steps' latches
//   fill           its own way of filling the input target: copy | convert | decode | scale, ending in input_finish (the orientation launch)
//   ingest_end     the per-input steps' draws -> [frame-rate conversion: mix / keep / repeat, per output picture] -> the per-output steps' draws -> upload event ->
//                  enqueue_picture (enc_schedule.cpp) on the slot's own surfaces
// Which steps there are, and in which order, is k_steps below and nowhere else: latch, draw, the in-place exit's test, collect and close all walk it.
// The one exception to the sequence is the in-place exit of mi355enc_submit_device.  A new step on the way in is a row of k_steps (one that works on the coded
// surfaces) or goes in front of input_finish (one that works on the pre-orientation picture), never into a submit.
// Also here: what the fills share -- a format's planes, the raw staging upload, the two-launch form, the staging helper threads -- and mi355enc_stage_csc.
#include "enc_internal.hpp"

static hipStream_t upload_stream(const mi355enc_t *h) { return h->ustream ? h->ustream : h->fstream; }
// the front stream's kernels read the source: behind the upload, if that went to a stream of its own
static int upload_done(mi355enc_t *h, slot_t *s) {
    if (h->ustream) { HIPCHK(hipEventRecord(s->ev_up, h->ustream)); HIPCHK(hipStreamWaitEvent(h->fstream, s->ev_up, 0)); }
    return 0;
}

// ---- the sequence around every fill
// the slot the next picture goes into; ERR_STATE with the pipeline full.  With frame-rate conversion the rule is asked first: a submit that
// yields n pictures needs n free slots, its input goes into the last of them (the repeats / earlier mixes are enqueued in front of it, from the queue's head
// on), and one that yields none and transfers nothing answers INGEST_DROP
static int ingest_slot(mi355enc_t *h, slot_t **s, int64_t pts, int force_idr) {
    int ahead = 0;
    if (h->rate.mode) { int r = rate_begin(h, pts, force_idr, &ahead); if (r) return r; }
    else if (h->pending > h->cfg.pipeline_depth) return MI355ENC_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    *s = &h->slot[(h->head + ahead) % NSLOT];
    (*s)->yuv_step = h->yuv_on;
    return MI355ENC_OK;
}

// ---- the input steps ("The input path"): one row per step, in chain order.  Null: the step has nothing of that kind.
//   latch      what the control thread set last becomes the slot's; own: the slot the step is applied on (false: the picture only reports the setting)
//   draw       the step on the slot's coded surfaces, behind everything enqueued on the stream so far; nothing where the slot latched none
//   active     the slot's picture is changed by the step: it goes into the encoder's own surfaces, never through the in-place exit
//   collected  mi355enc_collect: books what the picture carried as the last picture's
//   free       mi355enc_close: everything of the step
// PER_INPUT: applied once, to the slot the input goes into; the other pictures of the same submit (frame-rate conversion) latch with own == false.  PER_OUTPUT:
// latched and drawn afresh for every picture the submit yields -- holds and blends keep their undrawn source.  The mix sits between the two phases.
enum step_phase_t { PER_INPUT, PER_OUTPUT };
struct step_t {
    const char *name;
    int (*latch)(mi355enc_t *, slot_t *, bool own);
    int (*draw)(mi355enc_t *, slot_t *, hipStream_t);
    bool (*active)(const slot_t *);
    void (*collected)(mi355enc_t *, slot_t *);
    void (*free)(mi355enc_t *);
    step_phase_t phase;
};
static constexpr step_t k_steps[] = {
    // the stabiliser: measured on the input, once; its launches sit in front of the scale launch (input_scale), and it runs only under a geometry, where the in-place exit is not taken anyway
    {"stabiliser", stab_latch, nullptr, nullptr, stab_collected, stab_free, PER_INPUT},
    // geometry first: colours, filter, controls, mix, layers and text follow, so layers and text stay straight
    {"warp", warp_latch, warp_draw, [](const slot_t *s) { return s->warp_on; }, warp_collected, warp_close, PER_INPUT},
    // the colour step: layers and text are drawn in the output's colours.  Latched with the slot (ingest_slot); an RGB submit clears it
    {"colour step", nullptr, yuv_draw, [](const slot_t *s) { return s->yuv_step; }, nullptr, nullptr, PER_INPUT},
    // the spatial noise filter and its estimate: measured on the camera's picture, filtered in front of the temporal filter, whose block measure then sees less noise
    {"spatial filter", dspatial_latch, dspatial_draw, [](const slot_t *s) { return s->ds_on; }, dspatial_collected, dspatial_free, PER_INPUT},
    // the temporal noise filter: in front of the picture controls, so that sharpening never amplifies noise; only the input's own slot launches and needs the tables
    {"temporal filter", denoise_latch, denoise_draw, [](const slot_t *s) { return s->dn.parts != 0; }, denoise_collected, denoise_free, PER_INPUT},
    // the 3D LUT: behind the noise filter, whose history stays in the camera's domain; automatic levels measure the graded picture
    {"3D LUT", lut3d_latch, lut3d_draw, [](const slot_t *s) { return s->lut_on; }, lut3d_collected, lut3d_close, PER_INPUT},
    // automatic levels and white balance: measured on the filtered picture, and the manual controls trim on top of it
    {"automatic levels", autolevel_latch, autolevel_draw, [](const slot_t *s) { return s->al_on; }, autolevel_collected, autolevel_free, PER_INPUT},
    // picture controls: behind the colour step, in front of the mix, the layers and the text
    {"picture controls", adjust_latch, adjust_draw, [](const slot_t *s) { return s->adj.parts != 0; }, adjust_collected, adjust_free, PER_INPUT},
    // the privacy masks first of what is drawn on top: logos and the stats line stay sharp on top of them
    {"masks", mask_latch, mask_draw, [](const slot_t *s) { return s->mask_on; }, mask_collected, mask_free, PER_OUTPUT},
    // image layers, in index order; collected lets go of the slot's images
    {"layers", image_latch, image_draw, image_active, image_collected, image_free, PER_OUTPUT},
    // the text on top of everything
    {"text", overlay_latch, overlay_draw, [](const slot_t *s) { return s->ov_len != 0; }, overlay_collected, nullptr, PER_OUTPUT},
};
// one slot's latches; own: the slot the input goes into (every other picture of the submit is latched afresh by the per-output steps alone)
static int latch_slot(mi355enc_t *h, slot_t *s, bool own) {
    for (const step_t &st : k_steps)
        if (st.latch) { int r = st.latch(h, s, own || st.phase == PER_OUTPUT); if (r) return r; }
    return MI355ENC_OK;
}
static int draw_steps(mi355enc_t *h, slot_t *s, hipStream_t up, step_phase_t phase) {
    for (const step_t &st : k_steps)
        if (st.draw && st.phase == phase) {
            int r = st.draw(h, s, up);
            if (r) { fprintf(stderr, "mi355enc: input step '%s' failed: %d\n", st.name, r); return r; }
        }
    return MI355ENC_OK;
}
bool steps_active(const slot_t *s) {
    for (const step_t &st : k_steps) if (st.active && st.active(s)) return true;
    return false;
}
void steps_collected(mi355enc_t *h, slot_t *s) { for (const step_t &st : k_steps) if (st.collected) st.collected(h, s); }
void steps_free(mi355enc_t *h) { for (const step_t &st : k_steps) if (st.free) st.free(h); }

// what the control thread set last becomes the picture's -- every picture's that the submit yields: the rate conversion's earlier ticks first, then the input's own slot
static int ingest_latch(mi355enc_t *h, slot_t *s) {
    for (int i = 0; h->rate.mode && i < h->rate_n - 1; i++) { int r = latch_slot(h, &h->slot[(h->head + i) % NSLOT], false); if (r) return r; }
    return latch_slot(h, s, true);
}
// (apart only for mi355enc_submit_jpeg, which decodes into the slot between the two: after the state check -- with the pipeline full the slot's buffers
// belong to a picture in flight -- and before anything is latched)
static int ingest_begin(mi355enc_t *h, slot_t **s, int64_t pts, int force_idr) {
    int r = ingest_slot(h, s, pts, force_idr);
    return r ? r : ingest_latch(h, *s);
}
// everything that is drawn into a picture on top of its samples (the per-output steps), then the schedule
static int draw_and_enqueue(mi355enc_t *h, slot_t *s, hipStream_t up, int64_t pts, int force_idr) {
    int r = draw_steps(h, s, up, PER_OUTPUT);
    if (!r) r = upload_done(h, s);
    return r ? r : enqueue_picture(h, s, s->d_src_y, s->d_src_uv, h->W, pts, force_idr);
}
// frame-rate conversion: the slot's surfaces hold the input after the colour step; the pictures the plan's step yields, in tick order (s is the last one's slot)
static int ingest_end_rate(mi355enc_t *h, slot_t *s, hipStream_t up, int force_idr) {
    const int n = h->rate_n, idr = force_idr || h->rate_idr_owed;
    if (n == 0) { // blend: the input is the next pair's `a` and nothing is coded.  The slot (and a pinned staging buffer or the caller's pinned picture behind it) is free
        int r = rate_keep(h, s, up); // again when this returns, so the transfer is waited for here
        if (r) return r;
        HIPCHK(hipStreamSynchronize(up));
        rate_commit(h, force_idr);
        return MI355ENC_OK;
    }
    for (int i = 0; i < n - 1; i++) { // the ticks in front of the input's own: hold -- the previous output picture again; blend -- mixes of the same pair, b read where it lies
        slot_t *t = &h->slot[h->head];
        int r = h->rate.mode == 1 ? rate_repeat(h, t, up) : rate_mix(h, s, t, h->rate_w[i], false, up);
        if (!r) r = draw_and_enqueue(h, t, up, h->rate_pts[i], i == 0 ? idr : 0);
        if (r) return r;
    }
    int r = h->rate.mode == 1 ? rate_keep(h, s, up) : rate_mix(h, s, s, h->rate_w[n - 1], true, up); // (hold: kept before layers and text, and only with max_fill > 0)
    if (!r) r = draw_and_enqueue(h, s, up, h->rate_pts[n - 1], n == 1 ? idr : 0);
    if (!r) rate_commit(h, force_idr);
    return r;
}
// the slot's surfaces hold the oriented picture: the per-input steps, the mix or nothing, then the per-output steps and the schedule
static int ingest_end(mi355enc_t *h, slot_t *s, hipStream_t up, int64_t pts, int force_idr) {
    int r = draw_steps(h, s, up, PER_INPUT);
    if (r) return r;
    if (h->rate.mode) return ingest_end_rate(h, s, up, force_idr); // (the mix sits here: between the picture controls and the masks)
    r = draw_and_enqueue(h, s, up, pts, force_idr);
    if (!r) h->last_count = 1;
    return r;
}
// a submit's answer to ingest_begin's: a dropped input is a successful submit
static inline int begin_answer(int r) { return r == INGEST_DROP ? MI355ENC_OK : r; }

// ---- a format's planes
int fmt_planes(int fmt, int w, int h, fmt_plane_t pl[3]) {
    pl[0] = {w, h};
    switch (fmt) {
    case MI355ENC_FMT_NV12: case MI355ENC_FMT_NV21: pl[1] = {w, h / 2}; return 2;
    case MI355ENC_FMT_I420: pl[1] = pl[2] = {w / 2, h / 2}; return 3;
    case MI355ENC_FMT_Y42B: pl[1] = pl[2] = {w / 2, h}; return 3;
    case MI355ENC_FMT_Y444: pl[1] = pl[2] = {w, h}; return 3;
    case MI355ENC_FMT_YUY2: case MI355ENC_FMT_UYVY: pl[0].row = 2 * w; return 1;
    case MI355ENC_FMT_BGRX: case MI355ENC_FMT_RGBX: case MI355ENC_FMT_XRGB: case MI355ENC_FMT_XBGR: pl[0].row = 4 * w; return 1;
    case MI355ENC_FMT_BGR: case MI355ENC_FMT_RGB: pl[0].row = 3 * w; return 1;
    case MI355ENC_FMT_P010: pl[0].row = 2 * w; pl[1] = {2 * w, h / 2}; return 2;
    case MI355ENC_FMT_I420_10: pl[0].row = 2 * w; pl[1] = pl[2] = {w, h / 2}; return 3;
    case MI355ENC_FMT_V210: pl[0].row = (w + 5) / 6 * 16; return 1;
    case MI355ENC_FMT_GRAY8: return 1;
    default: return 0; // (YV12 too: it arrives here as I420, yv12_as_i420)
    }
}
bool planes_fit(int n, const fmt_plane_t pl[3], const uint8_t *const planes[3], const int strides[3]) {
    for (int i = 0; i < n; i++) if (!planes[i] || strides[i] < pl[i].row) return false;
    return true;
}
int yv12_as_i420(int fmt, const uint8_t *p[3], int st[3]) {
    if (fmt != MI355ENC_FMT_YV12) return fmt;
    const uint8_t *v = p[1]; p[1] = p[2]; p[2] = v;
    const int sv = st[1]; st[1] = st[2]; st[2] = sv;
    return MI355ENC_FMT_I420;
}

// A picture's planes tightly in a raw staging buffer (rows at multiples of 16 bytes), one behind the other from d on.
int raw_layout(int fmt, int w, int h, const uint8_t *d, const uint8_t *p[3], int st[3], fmt_plane_t pl[3]) {
    const int n = fmt_planes(fmt, w, h, pl);
    p[0] = p[1] = p[2] = nullptr; st[0] = st[1] = st[2] = 0;
    for (int i = 0; i < n; i++) { st[i] = (pl[i].row + 15) & ~15; p[i] = d; d += (size_t)st[i] * pl[i].rows; }
    return n;
}
// Upload the planes of a picture of the input size into the slot's raw staging buffer, laid out so.
int upload_raw(mi355enc_t *h, slot_t *s, int fmt, const uint8_t *const planes[3], const int strides[3], hipStream_t up, const uint8_t *p[3], int st[3]) {
    fmt_plane_t pl[3];
    const int n = fmt_planes(fmt, h->in_w, h->in_h, pl);
    if (!planes || !strides || !n || !planes_fit(n, pl, planes, strides)) return MI355ENC_ERR_ARG; // (nothing is allocated for or transferred of a picture that is refused)
    if (!s->d_raw) HIPCHK(hipMalloc((void **)&s->d_raw, raw_bytes(h)));
    raw_layout(fmt, h->in_w, h->in_h, s->d_raw, p, st, pl);
    for (int i = 0; i < n; i++) HIPCHK(hipMemcpy2DAsync((void *)p[i], st[i], planes[i], strides[i], pl[i].row, pl[i].rows, hipMemcpyHostToDevice, up));
    return MI355ENC_OK;
}

// ---- the two-launch form: a launch that makes NV12 at the input size, then the scale launch from there
int input_nv12(mi355enc_t *h, slot_t *s, nv12_pic_t *c) {
    c->stride = (h->in_w + 15) & ~15;
    if (!s->d_csc) HIPCHK(hipMalloc((void **)&s->d_csc, (size_t)c->stride * h->in_h * 3 / 2 + SURF_PAD));
    c->y = s->d_csc; c->uv = c->y + (size_t)c->stride * h->in_h;
    return MI355ENC_OK;
}
int scale_nv12(mi355enc_t *h, slot_t *s, const nv12_pic_t *c, const in_target_t *t, const scale_plan_t *pl, hipStream_t up) {
    return input_scale(h, s, MI355ENC_FMT_NV12, c->y, c->uv, nullptr, c->stride, c->stride, 0, t, pl, up);
}

// ... and convert (or, with an input size of its own, scale) it into the slot's NV12 staging surfaces.  NV12 only when scaling: unscaled, it is
// transferred straight into the surfaces (mi355enc_submit).
int upload_and_convert(mi355enc_t *h, slot_t *s, int fmt, const uint8_t *const planes[3], const int strides[3], hipStream_t up) {
    if (fmt == MI355ENC_FMT_NV12 && !h->scaling) return MI355ENC_ERR_ARG;
    if (!planes || !strides) return MI355ENC_ERR_ARG;
    if (fmt == MI355ENC_FMT_YV12) {
        const uint8_t *pl[3] = {planes[0], planes[1], planes[2]};
        int sl[3] = {strides[0], strides[1], strides[2]};
        return upload_and_convert(h, s, yv12_as_i420(fmt, pl, sl), pl, sl, up);
    }
    if (fmt_is_rgb(fmt) && !h->csc_ok) return MI355ENC_ERR_ARG; // (a matrix code RGB cannot be converted with: before anything is uploaded)
    if (hdr_refuses(h, fmt)) return MI355ENC_ERR_ARG;           // (a handle that tone-maps takes the three 10-bit formats only)
    const uint8_t *p[3];
    int st[3];
    int r = upload_raw(h, s, fmt, planes, strides, up, p, st);
    if (r) return r;
    in_target_t t; // the coded surfaces, or with an orientation the slot's pre-orientation picture
    r = input_target(h, s, &t);
    if (r) return r;
    const scale_plan_t *pl = h->scaling ? scale_plan_for(h, s, up) : nullptr;
    if (h->scaling && !pl) return MI355ENC_ERR_HIP;
    if (fmt >= MI355ENC_FMT_Y42B) { // the formats of k_csc.hip; with an input size of its own: converted at that size, then scaled as NV12
        if (h->hdr_on && !h->scaling) r = hdr_convert(h, fmt, p, st, t.y, t.uv, t.vw, t.vh, t.W, t.H, up); // (tone-mapped in the conversion launch: DESIGN.md section 22)
        else if (!h->scaling) r = k_launch_csc2(fmt, p[0], p[1], p[2], st[0], st[1], st[2], t.y, t.uv, t.vw, t.vh, t.W, t.H, h->csc_coef, up);
        else {
            nv12_pic_t c;
            r = input_nv12(h, s, &c);
            if (r) return r;
            if (h->hdr_on) r = hdr_convert(h, fmt, p, st, c.y, c.uv, h->in_w, h->in_h, c.stride, h->in_h, up);
            else r = k_launch_csc2(fmt, p[0], p[1], p[2], st[0], st[1], st[2], c.y, c.uv, h->in_w, h->in_h, c.stride, h->in_h, h->csc_coef, up);
            if (!r) r = scale_nv12(h, s, &c, &t, pl, up);
        }
    } else if (h->scaling) r = input_scale(h, s, fmt, p[0], p[1], p[2], st[0], st[1], st[2], &t, pl, up);
    else r = k_launch_csc(fmt, p[0], p[1], p[2], st[0], st[1], st[2], t.y, t.uv, t.vw, t.vh, t.W, t.H, up);
    if (r) return r < -1 ? r : MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return input_finish(h, s, up);
}

// one piece of a pageable source picture: into the pinned staging buffer, then on its way to the device
static int stage_piece(mi355enc_t *h, const mi355enc::stage_job &j, hipStream_t up) {
    if (j.src_stride == (int)j.dst_stride) memcpy(j.dst, j.src, j.dst_stride * (size_t)(j.rows - 1) + (size_t)j.width);
    else for (int r = 0; r < j.rows; r++) memcpy(j.dst + (size_t)r * j.dst_stride, j.src + (size_t)r * j.src_stride, (size_t)j.width);
    return hipMemcpyAsync(j.dev, j.dst, j.dst_stride * (size_t)(j.rows - 1) + (size_t)j.width, hipMemcpyHostToDevice, up) == hipSuccess ? 0 : 1;
}
void stage_helper(mi355enc_t *h) {
    (void)hipSetDevice(h->cfg.device_id);
    unsigned long long seen = 0;
    for (;;) {
        {
            std::unique_lock<std::mutex> g(h->stg_mu);
            h->stg_cv.wait(g, [&] { return h->stg_stop || (h->stg_gen != seen && h->stg_next < h->stg_n); });
            if (h->stg_stop) return;
        }
        const hipStream_t up = upload_stream(h);
        for (;;) {
            int i;
            { std::lock_guard<std::mutex> g(h->stg_mu); seen = h->stg_gen; i = h->stg_next < h->stg_n ? h->stg_next++ : -1; }
            if (i < 0) break;
            const int e = stage_piece(h, h->stg_job[i], up);
            bool last;
            { std::lock_guard<std::mutex> g(h->stg_mu); if (e) h->stg_err = e; last = ++h->stg_done >= h->stg_n; }
            if (last) h->stg_done_cv.notify_all();
        }
    }
}

extern "C" {

int mi355enc_stage_csc(mi355enc_t *h, int fmt, const uint8_t *const planes[3], const int strides[3], uint8_t *out_y, uint8_t *out_uv) {
    if (!h || !out_y || !out_uv) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r == MI355ENC_ERR_STATE ? MI355ENC_ERR_ARG : r; } // (with pictures in flight too: ERR_ARG, not the other stages' ERR_STATE)
    slot_t *s = &h->slot[0];
    int r = upload_and_convert(h, s, fmt, planes, strides, h->stream);
    return r ? r : stage_out(h, s, out_y, out_uv);
}

// Host input.  A picture in memory from mi355enc_host_alloc() is DMA'd from where it lies (the call returns at once; the memory is the
// caller's again after the matching collect()).  Anything else is pageable as far as HIP knows: a stream-ordered copy from pageable memory
// blocks the calling thread while the runtime stages it chunk by chunk through its own pinned buffers -- so the picture is copied once, by
// this thread, into the slot's pinned staging buffer and leaves from there in one asynchronous transfer per plane, on the front stream,
// beside the kernels of the pictures before it.
int mi355enc_submit(mi355enc_t *h, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride, int64_t pts, int force_idr) {
    if (!h || !y || !uv || y_stride < h->in_w || uv_stride < h->in_w || h->yuv_bad || hdr_refuses(h, MI355ENC_FMT_NV12)) return MI355ENC_ERR_ARG; // (yuv_bad: YUV samples that cannot be converted to the output's matrix; a handle that tone-maps takes 10-bit input only)
    slot_t *s;
    { int r = ingest_begin(h, &s, pts, force_idr); if (r) return begin_answer(r); }
    const int w = h->in_w, ht = h->in_h;
    hipStream_t up = upload_stream(h);
    // where the planes go: the staging surfaces at the coded stride, or -- to be scaled -- the raw staging buffer at the input's
    // (with an orientation, `the staging surfaces' are the slot's pre-orientation picture at its own stride: input_target)
    if (h->scaling && !s->d_raw) HIPCHK(hipMalloc((void **)&s->d_raw, raw_bytes(h)));
    in_target_t t;
    { int r = input_target(h, s, &t); if (r) return r; }
    const int ds = h->scaling ? (w + 15) & ~15 : t.W;
    uint8_t *dev_y = h->scaling ? s->d_raw : t.y, *dev_uv = h->scaling ? s->d_raw + (size_t)ds * ht : t.uv;
    const bool pinned = host_range_pinned(y, (size_t)y_stride * (ht - 1) + w) && host_range_pinned(uv, (size_t)uv_stride * (ht / 2 - 1) + w);
    if (pinned || h->cfg.pipeline_depth == 0) {
        // pinned: transferred in place.  pipeline_depth 0 (the latency mode: collect() follows at once, there is nothing to run beside): the
        // runtime's own pageable path, which stages and transfers in chunks on its side of the call (measured 0.06 ms less per 1080p picture
        // than staging here and transferring afterwards)
        HIPCHK(hipMemcpy2DAsync(dev_y, ds, y, y_stride, w, ht, hipMemcpyHostToDevice, up));
        HIPCHK(hipMemcpy2DAsync(dev_uv, ds, uv, uv_stride, w, ht / 2, hipMemcpyHostToDevice, up));
        h->st.pinned_inputs += pinned ? 1 : 0;
    } else {
        if (!s->h_src) HIPCHK(hipHostMalloc((void **)&s->h_src, (h->scaling || h->orient) ? (size_t)ds * ht * 3 / 2 : h->ysz + h->csz, hipHostMallocDefault));
        // rows at the coded stride, so that a range of rows is one contiguous transfer; in pieces (luma thirds or sixths, the chroma plane in one or two), each
        // sent as soon as it is staged: the transfer of one piece runs beside the staging of the next, and with the helper threads three pieces are
        // staged side by side (a single thread copies 3.1 MB in 0.15-0.2 ms, as long as the device needs for the whole picture)
        uint8_t *hy = s->h_src, *huv = s->h_src + (size_t)ds * ht;
        mi355enc::stage_job jobs[8];
        int nj = 0;
        const int ny = h->stg_on ? 6 : 3, nc = h->stg_on ? 2 : 1;
        for (int k = 0; k < ny; k++) {
            const int r0 = (ht * k / ny) & ~1, r1 = k == ny - 1 ? ht : (ht * (k + 1) / ny) & ~1;
            if (r1 > r0) jobs[nj++] = {y + (size_t)r0 * y_stride, hy + (size_t)r0 * ds, dev_y + (size_t)r0 * ds, y_stride, r1 - r0, w, (size_t)ds};
        }
        for (int k = 0; k < nc; k++) {
            const int r0 = (ht / 2) * k / nc, r1 = (ht / 2) * (k + 1) / nc;
            if (r1 > r0) jobs[nj++] = {uv + (size_t)r0 * uv_stride, huv + (size_t)r0 * ds, dev_uv + (size_t)r0 * ds, uv_stride, r1 - r0, w, (size_t)ds};
        }
        if (h->stg_on) {
            { std::lock_guard<std::mutex> g(h->stg_mu); for (int i = 0; i < nj; i++) h->stg_job[i] = jobs[i]; h->stg_n = nj; h->stg_next = 0; h->stg_done = 0; h->stg_err = 0; h->stg_gen++; }
            h->stg_cv.notify_all();
            for (;;) { // the caller takes pieces too
                int i;
                { std::lock_guard<std::mutex> g(h->stg_mu); i = h->stg_next < h->stg_n ? h->stg_next++ : -1; }
                if (i < 0) break;
                const int e = stage_piece(h, h->stg_job[i], up);
                { std::lock_guard<std::mutex> g(h->stg_mu); if (e) h->stg_err = e; h->stg_done++; }
            }
            { std::unique_lock<std::mutex> g(h->stg_mu); h->stg_done_cv.wait(g, [&] { return h->stg_done >= h->stg_n; }); if (h->stg_err) return MI355ENC_ERR_HIP; }
        } else
            for (int i = 0; i < nj; i++) if (stage_piece(h, jobs[i], up)) return MI355ENC_ERR_HIP;
    }
    if (h->scaling) {
        const scale_plan_t *pl = scale_plan_for(h, s, up);
        if (!pl) return MI355ENC_ERR_HIP;
        const nv12_pic_t raw = {dev_y, dev_uv, ds};
        { int r = scale_nv12(h, s, &raw, &t, pl, up); if (r) return r; }
        HIPCHK(hipGetLastError());
    }
    else if (!h->orient && (w != h->W || (s->dn.parts && (ht & 7)))) k_launch_pad(s->d_src_y, s->d_src_uv, h->W, w, ht, h->W, h->H, up); // (the orientation launch writes the margin itself; the bottom margin alone is padded only for the noise filter, the one step that reads it, and only where a block row is partly visible: its block measure takes such a block as it lies)
    { int r = input_finish(h, s, up); if (r) return r; }
    return ingest_end(h, s, up, pts, force_idr);
}

int mi355enc_submit_fmt(mi355enc_t *h, int fmt, const uint8_t *const planes[3], const int strides[3], int64_t pts, int force_idr) {
    if (!h || !planes || !strides) return MI355ENC_ERR_ARG;
    if (fmt == MI355ENC_FMT_NV12) return mi355enc_submit(h, planes[0], strides[0], planes[1], strides[1], pts, force_idr);
    if ((!fmt_is_rgb(fmt) && h->yuv_bad) || hdr_refuses(h, fmt)) return MI355ENC_ERR_ARG;
    slot_t *s;
    int r = ingest_begin(h, &s, pts, force_idr);
    if (r) return begin_answer(r);
    if (fmt_is_rgb(fmt)) s->yuv_step = false; // (RGB is converted straight to the output's matrix and range)
    r = upload_and_convert(h, s, fmt, planes, strides, upload_stream(h));
    return r ? r : ingest_end(h, s, upload_stream(h), pts, force_idr);
}

// MJPEG input: the host decodes the entropy-coded data into the slot's pinned coefficient buffer first -- a picture that is refused or does not decode has
// touched nothing else -- then the transfer and the JPEG launch take the place of the conversion launch.
int mi355enc_submit_jpeg(mi355enc_t *h, const uint8_t *data, size_t len, int64_t pts, int force_idr) {
    if (!h || !data || h->yuv_bad || hdr_refuses(h, -1)) return MI355ENC_ERR_ARG;
    slot_t *s;
    int r = ingest_slot(h, &s, pts, force_idr);
    if (r) return begin_answer(r); // (a dropped picture is not entropy-decoded)
    mi355enc_jpeg_info_t info;
    r = jpeg_decode_host(h, s, data, len, &info);
    if (!r) r = ingest_latch(h, s);
    if (!r) r = jpeg_enqueue(h, s, &info, upload_stream(h));
    return r ? r : ingest_end(h, s, upload_stream(h), pts, force_idr);
}

// Device input.  The in-place exit is the one exception to the sequence: the kernels read the caller's planes where they lie, nothing is drawn (with a
// colour step, a text or an active layer the exit is not taken) and nothing was uploaded, so enqueue_picture follows the latches directly.
int mi355enc_submit_device(mi355enc_t *h, const void *d_y, int y_stride, const void *d_uv, int uv_stride, int64_t pts, int force_idr) {
    if (!h || !d_y || !d_uv || y_stride < h->in_w || uv_stride < h->in_w || h->yuv_bad || hdr_refuses(h, -1)) return MI355ENC_ERR_ARG;
    slot_t *s;
    int r = ingest_begin(h, &s, pts, force_idr);
    if (r) return begin_answer(r);
    hipStream_t up = upload_stream(h);
    if (h->scaling) { // scaled from where the planes lie into the slot's staging surfaces
        in_target_t t;
        r = input_target(h, s, &t);
        if (r) return r;
        const scale_plan_t *pl = scale_plan_for(h, s, up);
        if (!pl) return MI355ENC_ERR_HIP;
        r = input_scale(h, s, MI355ENC_FMT_NV12, (const uint8_t *)d_y, (const uint8_t *)d_uv, nullptr, y_stride, uv_stride, 0, &t, pl, up); // (stabilised: the whole submitted luma is read, not only the crop)
        if (r) return r;
        HIPCHK(hipGetLastError());
        r = input_finish(h, s, up);
    } else if (h->orient) { // oriented from where the planes lie, at their stride and address, into the slot's staging surfaces: never in place, the caller's planes are only read
        r = input_finish(h, s, up, (const uint8_t *)d_y, y_stride, (const uint8_t *)d_uv, uv_stride);
    } else {
        const int w = h->cfg.width, ht = h->cfg.height;
        // in place -- unless the frame rate is converted (the picture may be kept, repeated or mixed) or a step changes the samples (steps_active): that goes into the encoder's own surfaces, never into the caller's planes
        const bool direct = !h->rate.mode && !steps_active(s) && w == h->W && y_stride == uv_stride && (y_stride & 15) == 0 && (((uintptr_t)d_y | (uintptr_t)d_uv) & 15) == 0;
        if (direct) return enqueue_picture(h, s, (const uint8_t *)d_y, (const uint8_t *)d_uv, y_stride, pts, force_idr);
        HIPCHK(hipMemcpy2DAsync(s->d_src_y, h->W, d_y, y_stride, w, ht, hipMemcpyDeviceToDevice, up));
        HIPCHK(hipMemcpy2DAsync(s->d_src_uv, h->W, d_uv, uv_stride, w, ht / 2, hipMemcpyDeviceToDevice, up));
        if (w != h->W || (s->dn.parts && (ht & 7))) k_launch_pad(s->d_src_y, s->d_src_uv, h->W, w, ht, h->W, h->H, up); // (as in mi355enc_submit)
    }
    return r ? r : ingest_end(h, s, up, pts, force_idr);
}

} // extern "C"
