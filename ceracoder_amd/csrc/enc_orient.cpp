// enc_orient.cpp -- orientation of the input picture: the host's statement of the rule, the setter, the slot's
// pre-orientation picture and the launch of k_orient.hip that every submit path ends in, and the entry points that expose the kernel to tests.
#include "enc_internal.hpp"

// method -> transpose, mirror of the source column, mirror of the source row (k_orient.hip's table)
static bool orient_fx(int m) { return m == MI355ENC_ORIENT_180 || m == MI355ENC_ORIENT_90L || m == MI355ENC_ORIENT_HORIZ || m == MI355ENC_ORIENT_UR_LL; }
static bool orient_fy(int m) { return m == MI355ENC_ORIENT_90R || m == MI355ENC_ORIENT_180 || m == MI355ENC_ORIENT_VERT || m == MI355ENC_ORIENT_UR_LL; }
static bool orient_ok(int m) { return m >= MI355ENC_ORIENT_IDENTITY && m <= MI355ENC_ORIENT_UR_LL; }

static size_t pre_stride(const mi355enc_t *h) { return (size_t)((pre_w(h) + 15) & ~15); }
static size_t pre_bytes(const mi355enc_t *h) { return pre_stride(h) * pre_h(h) * 3 / 2 + SURF_PAD; }

void orient_free(slot_t *s) {
    if (s->d_pre) { (void)hipFree(s->d_pre); s->d_pre = nullptr; }
}

int input_target(mi355enc_t *h, slot_t *s, in_target_t *t) {
    if (!h->orient) { *t = {s->d_src_y, s->d_src_uv, h->cfg.width, h->cfg.height, h->W, h->H}; return MI355ENC_OK; }
    if (!s->d_pre) HIPCHK(hipMalloc((void **)&s->d_pre, pre_bytes(h)));
    const int ps = (int)pre_stride(h);
    *t = {s->d_pre, s->d_pre + (size_t)ps * pre_h(h), pre_w(h), pre_h(h), ps, pre_h(h)}; // no margin rows: the orientation launch makes the coded margin
    return MI355ENC_OK;
}

int input_finish(mi355enc_t *h, slot_t *s, hipStream_t up, const uint8_t *src_y, int y_stride, const uint8_t *src_uv, int uv_stride) {
    if (!h->orient) return MI355ENC_OK;
    if (!src_y) {
        in_target_t t;
        int r = input_target(h, s, &t);
        if (r) return r;
        src_y = t.y; src_uv = t.uv; y_stride = uv_stride = t.W;
    }
    if (k_launch_orient(h->orient, src_y, y_stride, src_uv, uv_stride, pre_w(h), pre_h(h), s->d_src_y, s->d_src_uv, h->W, h->H, up)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}

extern "C" {

int mi355enc_orient_size(int method, int in_w, int in_h, int *out_w, int *out_h) {
    if (!orient_ok(method) || in_w <= 0 || in_h <= 0 || !out_w || !out_h) return MI355ENC_ERR_ARG;
    *out_w = orient_transposes(method) ? in_h : in_w;
    *out_h = orient_transposes(method) ? in_w : in_h;
    return MI355ENC_OK;
}

int mi355enc_orient_source(int method, int out_w, int out_h, int x, int y, int *sx, int *sy) {
    if (!orient_ok(method) || out_w <= 0 || out_h <= 0 || x < 0 || y < 0 || x >= out_w || y >= out_h || !sx || !sy) return MI355ENC_ERR_ARG;
    const bool tr = orient_transposes(method);
    const int in_w = tr ? out_h : out_w, in_h = tr ? out_w : out_h, u = tr ? y : x, v = tr ? x : y;
    *sx = orient_fx(method) ? in_w - 1 - u : u;
    *sy = orient_fy(method) ? in_h - 1 - v : v;
    return MI355ENC_OK;
}

int mi355enc_set_orientation(mi355enc_t *h, int method) {
    if (!h) return MI355ENC_ERR_ARG;
    return geometry_apply(h, method, h->in_set, h->in_w, h->in_h, h->geom_on ? &h->geom : nullptr);
}

int mi355enc_get_orientation(const mi355enc_t *h) { return h ? h->orient : MI355ENC_ERR_ARG; }

size_t mi355enc_debug_orient_bytes(const mi355enc_t *h) {
    size_t n = 0;
    if (h) for (int i = 0; i < NSLOT; i++) if (h->slot[i].d_pre) n += pre_bytes(h);
    return n;
}

// the kernel alone: the pre-orientation size is that of `method` at the handle's coded size, whatever the handle's own method and input size
static int stage_sizes(const mi355enc_t *h, int method, int *pw, int *ph) {
    if (method < MI355ENC_ORIENT_90R || method > MI355ENC_ORIENT_UR_LL) return MI355ENC_ERR_ARG;
    *pw = orient_transposes(method) ? h->cfg.height : h->cfg.width;
    *ph = orient_transposes(method) ? h->cfg.width : h->cfg.height;
    return MI355ENC_OK;
}

int mi355enc_stage_orient(mi355enc_t *h, int method, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride, uint8_t *out_y, uint8_t *out_uv) {
    int pw, ph;
    if (!h || !y || !uv || !out_y || !out_uv || stage_sizes(h, method, &pw, &ph) || y_stride < pw || uv_stride < pw) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; }
    slot_t *s = &h->slot[0];
    const int ps = (pw + 15) & ~15;
    stage_tmp_t tmp(h->stream); // (a buffer of its own: the handle's pre-orientation picture has the size of the handle's method)
    if (tmp.alloc((size_t)ps * ph * 3 / 2 + SURF_PAD)) return MI355ENC_ERR_HIP;
    uint8_t *d = tmp.as<uint8_t>();
    HIPCHK(hipMemcpy2DAsync(d, ps, y, y_stride, pw, ph, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpy2DAsync(d + (size_t)ps * ph, ps, uv, uv_stride, pw, ph / 2, hipMemcpyHostToDevice, h->stream));
    if (k_launch_orient(method, d, ps, d + (size_t)ps * ph, ps, pw, ph, s->d_src_y, s->d_src_uv, h->W, h->H, h->stream)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return stage_out(h, s, out_y, out_uv);
}

int mi355enc_stage_orient_device(mi355enc_t *h, int method, const void *d_y, int y_stride, const void *d_uv, int uv_stride, void *d_out_y, void *d_out_uv) {
    int pw, ph;
    if (!h || !d_y || !d_uv || !d_out_y || !d_out_uv || stage_sizes(h, method, &pw, &ph) || y_stride < pw || uv_stride < pw) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; }
    if (k_launch_orient(method, (const uint8_t *)d_y, y_stride, (const uint8_t *)d_uv, uv_stride, pw, ph, (uint8_t *)d_out_y, (uint8_t *)d_out_uv, h->W, h->H, h->stream)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}

} // extern "C"
