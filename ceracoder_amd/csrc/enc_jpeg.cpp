// enc_jpeg.cpp -- MJPEG input: a slot's coefficient buffers, the host's entropy decode into them (jpeg_host.c), the
// transfer and the launch of k_jpeg.hip into the slot's NV12 staging surfaces, and the single-stage entry points.  The submit entry point
// itself sits beside the other submits in enc_input.cpp.
#include "enc_internal.hpp"

#include "jpeg_host.h"

#define JPEG_QT_BYTES 512 /* the three tables (384 bytes) lead the buffer: one transfer carries both */

// room for the largest accepted layout of a picture of the input size: three components at full size, padded to whole 16 x 16 MCUs
static size_t jpeg_coef_cap(const mi355enc_t *h) { return 3 * (size_t)((h->in_w + 15) & ~15) * (size_t)((h->in_h + 15) & ~15); }

int jpeg_alloc(mi355enc_t *h, slot_t *s) {
    if (s->h_jpeg) return MI355ENC_OK;
    const size_t bytes = JPEG_QT_BYTES + jpeg_coef_cap(h) * sizeof(int16_t);
    HIPCHK(hipHostMalloc((void **)&s->h_jpeg, bytes, hipHostMallocDefault));
    memset(s->h_jpeg, 0, bytes);
    HIPCHK(hipMalloc((void **)&s->d_jpeg, bytes));
    HIPCHK(hipMemset(s->d_jpeg, 0, bytes)); // (mi355enc_time_stage runs the launch on whatever the buffer holds)
    HIPCHK(hipStreamSynchronize(nullptr));  // the fill runs on the null stream, which the handle's streams do not wait for: through before the first transfer into the buffer is enqueued
    HIPCHK(hipMalloc((void **)&s->d_jpeg_planar, 3 * (size_t)((h->in_w + 15) & ~15) * h->in_h + SURF_PAD));
    return MI355ENC_OK;
}
void jpeg_free(slot_t *s) {
    if (s->h_jpeg) { (void)hipHostFree(s->h_jpeg); s->h_jpeg = nullptr; }
    if (s->d_jpeg) { (void)hipFree(s->d_jpeg); s->d_jpeg = nullptr; }
    if (s->d_jpeg_planar) { (void)hipFree(s->d_jpeg_planar); s->d_jpeg_planar = nullptr; }
}

// the picture must be one this handle takes: even, of the input size
static int jpeg_check(const mi355enc_t *h, const mi355enc_jpeg_info_t *info) {
    if (((info->width | info->height) & 1) || info->width != h->in_w || info->height != h->in_h) return MI355ENC_ERR_ARG;
    return MI355ENC_OK;
}

// Host part: parse, check the size, decode into the slot's pinned buffer.  Touches nothing else of the handle: a picture refused here leaves no trace.
int jpeg_decode_host(mi355enc_t *h, slot_t *s, const uint8_t *data, size_t len, mi355enc_jpeg_info_t *info) {
    if (!data) return MI355ENC_ERR_ARG;
    int r = mi355enc_jpeg_info(data, len, info);
    if (!r) r = jpeg_check(h, info);
    if (r) return r;
    r = jpeg_alloc(h, s);
    if (r) return r;
    r = mi355enc_jpeg_entropy_decode(data, len, (int16_t *)(s->h_jpeg + JPEG_QT_BYTES), jpeg_coef_cap(h), (uint16_t(*)[64])s->h_jpeg, nullptr);
    return r == MI355ENC_ERR_OVERFLOW ? MI355ENC_ERR_ARG : r;
}

// Device part, on stream `up`: tables and coefficients to the device, the JPEG launch into the slot's staging surfaces -- or, with an input size of its own,
// into the slot's NV12 picture of the input size and from there through the scale kernel (section 11's two-launch form).
int jpeg_enqueue(mi355enc_t *h, slot_t *s, const mi355enc_jpeg_info_t *info, hipStream_t up) {
    int bw[3], bh[3];
    size_t first[3];
    const size_t bytes = JPEG_QT_BYTES + jpeg_host_layout(info, bw, bh, first) * 64 * sizeof(int16_t);
    HIPCHK(hipMemcpyAsync(s->d_jpeg, s->h_jpeg, bytes, hipMemcpyHostToDevice, up));
    const int16_t *dc = (const int16_t *)(s->d_jpeg + JPEG_QT_BYTES);
    const uint16_t *dq = (const uint16_t *)s->d_jpeg;
    in_target_t t;
    int r = input_target(h, s, &t);
    if (r) return r;
    if (!h->scaling) r = k_launch_jpeg(dc, dq, info->hs, info->vs, info->components, t.vw, t.vh, t.y, t.uv, t.W, t.H, s->d_jpeg_planar, up);
    else {
        nv12_pic_t c;
        r = input_nv12(h, s, &c);
        if (r) return r;
        r = k_launch_jpeg(dc, dq, info->hs, info->vs, info->components, h->in_w, h->in_h, c.y, c.uv, c.stride, h->in_h, s->d_jpeg_planar, up);
        const scale_plan_t *pl = scale_plan_for(h, s, up);
        if (!pl) return MI355ENC_ERR_HIP;
        if (r) return MI355ENC_ERR_ARG;
        r = scale_nv12(h, s, &c, &t, pl, up);
        if (r) return r;
    }
    if (r) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return input_finish(h, s, up);
}

// the launch alone for mi355enc_time_stage: the coded size as 4:2:2, on whatever slot 0's coefficient buffer holds
int jpeg_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *) {
    in_target_t t;
    int r = input_target(h, s, &t);
    if (r) return r;
    return k_launch_jpeg((const int16_t *)(s->d_jpeg + JPEG_QT_BYTES), (const uint16_t *)s->d_jpeg, 2, 1, 3, t.vw, t.vh, t.y, t.uv, t.W, t.H,
                         s->d_jpeg_planar, h->stream) ? MI355ENC_ERR_ARG : MI355ENC_OK;
}

extern "C" {

int mi355enc_stage_jpeg(mi355enc_t *h, const uint8_t *data, size_t len, uint8_t *out_y, uint8_t *out_uv) {
    if (!h || !data || !out_y || !out_uv) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; }
    slot_t *s = &h->slot[0];
    mi355enc_jpeg_info_t info;
    int r = jpeg_decode_host(h, s, data, len, &info);
    if (!r) r = jpeg_enqueue(h, s, &info, h->stream);
    return r ? r : stage_out(h, s, out_y, out_uv);
}

int mi355enc_stage_jpeg_blocks(mi355enc_t *h, int hs, int vs, int components, const int16_t *coef, const uint16_t qt[3][64], uint8_t *out_y, uint8_t *out_uv) {
    if (!h || !coef || !qt || !out_y || !out_uv) return MI355ENC_ERR_ARG;
    if (!((components == 1 && hs == 1 && vs == 1) || (components == 3 && (hs == 1 || hs == 2) && (vs == 1 || (vs == 2 && hs == 2))))) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; }
    slot_t *s = &h->slot[0];
    const mi355enc_jpeg_info_t info = {h->in_w, h->in_h, components, hs, vs, 0, 0};
    int r = jpeg_check(h, &info);
    if (!r) r = jpeg_alloc(h, s);
    if (r) return r;
    int bw[3], bh[3];
    size_t first[3];
    memcpy(s->h_jpeg, qt, 3 * 64 * sizeof(uint16_t));
    memcpy(s->h_jpeg + JPEG_QT_BYTES, coef, jpeg_host_layout(&info, bw, bh, first) * 64 * sizeof(int16_t));
    r = jpeg_enqueue(h, s, &info, h->stream);
    return r ? r : stage_out(h, s, out_y, out_uv);
}

} // extern "C"
