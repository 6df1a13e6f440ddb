// enc_stage.hpp -- the frame every single-stage entry point runs in ("The stage entry points"; included at the end of enc_internal.hpp):
// own argument checks -> stage_enter -> stage_in -> the step -> stage_out, with stage_tmp_t for whatever a call allocates for itself.
#ifndef MI355_ENC_STAGE_HPP
#define MI355_ENC_STAGE_HPP

// A single-stage call made with pictures in flight would overwrite what they use: refused before anything is touched (the caller collects first).  Otherwise the
// handle's device is current and every stream of the handle has run dry (with nothing in flight they are idle or draining).
static inline int stage_enter(mi355enc_t *h) {
    if (h->pending) return MI355ENC_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    for (int i = 0; i < NSLOT; i++) { h->slot[i].stab.range = 0; h->slot[i].stab_done = false; } // (a stage call is no part of the stream: it runs the geometry as set, unstabilised -- DESIGN.md section 26)
    return sync_compute(h);
}
// host planes of the coded size -> the slot's source surfaces, on the main stream
static inline int stage_in(mi355enc_t *h, slot_t *s, const uint8_t *y, const uint8_t *uv) {
    HIPCHK(hipMemcpyAsync(s->d_src_y, y, h->ysz, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(s->d_src_uv, uv, h->csz, hipMemcpyHostToDevice, h->stream));
    return MI355ENC_OK;
}
// ... and back: the slot's source surfaces to the host, once everything enqueued on the main stream is done
static inline int stage_out(mi355enc_t *h, slot_t *s, uint8_t *out_y, uint8_t *out_uv) {
    HIPCHK(hipMemcpyAsync(out_y, s->d_src_y, h->ysz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(out_uv, s->d_src_uv, h->csz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}
// A device buffer that lives for one call (never one of the handle's): freed when the call returns, on every path, behind everything the stream it was used on
// still has to do with it.
struct stage_tmp_t {
    void *p = nullptr;
    const hipStream_t st;
    explicit stage_tmp_t(hipStream_t used_on) : st(used_on) {}
    stage_tmp_t(const stage_tmp_t &) = delete; // (and with it the assignment: the member below)
    ~stage_tmp_t() { if (p) { (void)hipStreamSynchronize(st); (void)hipFree(p); } }
    int alloc(size_t bytes) { HIPCHK(hipMalloc(&p, bytes)); return MI355ENC_OK; } // (nonzero: MI355ENC_ERR_HIP)
    template <class T> T *as() const { return (T *)p; }
};
#endif
