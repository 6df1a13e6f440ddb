// enc_hdr.cpp -- HDR input of a handle (mi355enc_set_hdr_input): the state, the parameter block's way to the device, and the launch that
// takes k_launch_csc2's place for the three 10-bit formats.  The block itself is built by hdr_host.c, which needs no device.
#include "enc_internal.hpp"

#include <cstdlib>

// the output matrix the block is built for: the handle's, 2 resolved by the coded size as for RGB input; 0: not one of 1, 5, 6
static int hdr_out_matrix(const mi355enc_t *h) {
    const int m = h->col_mat != 2 ? h->col_mat : (h->cfg.width > 1024 || h->cfg.height > 576) ? 1 : 6;
    return m == 1 || m == 5 || m == 6 ? m : 0;
}

bool hdr_refuses(const mi355enc_t *h, int fmt) {
    if (!h->hdr_on) return false;
    return (fmt != MI355ENC_FMT_P010 && fmt != MI355ENC_FMT_I420_10 && fmt != MI355ENC_FMT_V210) || !hdr_out_matrix(h);
}

int hdr_convert(mi355enc_t *h, int fmt, const uint8_t *const p[3], const int st[3], uint8_t *dy, uint8_t *duv, int vw, int vh, int W, int H, hipStream_t s) {
    const int m = hdr_out_matrix(h);
    if (!m) return MI355ENC_ERR_ARG;
    const int key = m * 2 + h->col_full;
    if (key != h->hdr_key) { // the first conversion (or the output's colorimetry was changed since the last one): build, and upload on this stream
        if (!h->h_hdr && !(h->h_hdr = (int32_t *)malloc(HDR_WORDS * sizeof(int32_t)))) return MI355ENC_ERR_NOMEM;
        if (!h->d_hdr) HIPCHK(hipMalloc((void **)&h->d_hdr, HDR_WORDS * sizeof(int32_t)));
        if (h->hdr_stream) HIPCHK(hipStreamSynchronize(h->hdr_stream)); // (a launch that still reads the old block; only stage calls, which end synchronised, can lie before a rebuild)
        hdr_build(h->hdr_transfer, h->hdr_full, h->hdr_peak, h->hdr_target, m, h->col_full, h->h_hdr);
        HIPCHK(hipMemcpyAsync(h->d_hdr, h->h_hdr, HDR_WORDS * sizeof(int32_t), hipMemcpyHostToDevice, s));
        h->hdr_key = key; h->hdr_stream = s; h->hdr_arrived = false;
    } else if (s != h->hdr_stream && !h->hdr_arrived) { // another stream than the one the block went up on: waited for once, then it is there for every stream
        HIPCHK(hipStreamSynchronize(h->hdr_stream));
        h->hdr_arrived = true;
    }
    if (k_launch_hdr(fmt, h->hdr_transfer == 18, p, st, dy, duv, vw, vh, W, H, h->d_hdr, s)) return MI355ENC_ERR_ARG;
    return MI355ENC_OK;
}

void hdr_free(mi355enc_t *h) {
    if (h->d_hdr) (void)hipFree(h->d_hdr);
    free(h->h_hdr);
    h->d_hdr = h->h_hdr = nullptr;
}

extern "C" {

int mi355enc_set_hdr_input(mi355enc_t *h, int transfer, int full_range, int peak_nits, int target_nits) {
    if (!h || hdr_check(transfer, full_range, peak_nits, target_nits)) return MI355ENC_ERR_ARG;
    if (h->n_submitted || h->in_col_set) return MI355ENC_ERR_STATE; // (fixed from the stream's first picture on; one meaning of the input per handle)
    h->hdr_on = true; h->hdr_transfer = transfer; h->hdr_full = full_range; h->hdr_peak = peak_nits; h->hdr_target = target_nits;
    h->hdr_key = -1;
    return MI355ENC_OK;
}

} // extern "C"
