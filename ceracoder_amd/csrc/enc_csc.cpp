// enc_csc.cpp -- colorimetry of a handle (mi355enc_set_colorimetry): the code points every SPS carries, the integer RGB -> Y'CbCr matrix
// that follows from them (DESIGN.md section 11 states the rule; built on the host in double), and the entry points that expose both to tests.
#include "enc_internal.hpp"

#include <cmath>

// The ten words of mi355enc_csc_coefficients for a matrix code RGB can be converted with (1, 5, 6, 9); false otherwise.
static bool csc_matrix(int matrix, int full_range, int *c) {
#pragma clang fp contract(off) // bit for bit the plain IEEE double restatement (tests/cscref.py): no fused multiply-adds
    double kr, kb;
    switch (matrix) {
    case 1: kr = 0.2126; kb = 0.0722; break;
    case 5: case 6: kr = 0.299; kb = 0.114; break;
    case 9: kr = 0.2627; kb = 0.0593; break;
    default: return false;
    }
    const double sy = full_range ? 1.0 : 219.0 / 255.0, sc = full_range ? 1.0 : 224.0 / 255.0;
    auto r = [](double x) { return (int)std::floor(x + 0.5); };
    c[0] = r(kr * sy * 65536.0); c[2] = r(kb * sy * 65536.0); c[1] = r(sy * 65536.0) - c[0] - c[2];
    c[5] = r(0.5 * sc * 65536.0); c[3] = -r(kr / (2.0 * (1.0 - kb)) * sc * 65536.0); c[4] = -c[5] - c[3];
    c[6] = r(0.5 * sc * 65536.0); c[8] = -r(kb / (2.0 * (1.0 - kr)) * sc * 65536.0); c[7] = -c[6] - c[8];
    c[9] = full_range ? 0 : 16;
    return true;
}

void csc_resolve(mi355enc_t *h) {
    // unspecified: what `videoconvert` would have negotiated for a picture of this size -- BT.709 for HD, BT.601 below
    const int m = h->col_mat != 2 ? h->col_mat : (h->cfg.width > 1024 || h->cfg.height > 576) ? 1 : 6;
    h->csc_ok = csc_matrix(m, h->col_full, h->csc_coef);
}

extern "C" {

int mi355enc_csc_coefficients(int matrix, int full_range, int32_t coef[10]) {
    int c[10];
    if (!coef || (full_range | 1) != 1 || !csc_matrix(matrix, full_range, c)) return MI355ENC_ERR_ARG;
    for (int i = 0; i < 10; i++) coef[i] = c[i];
    return MI355ENC_OK;
}

int mi355enc_set_colorimetry(mi355enc_t *h, int full_range, int primaries, int transfer, int matrix) {
    if (!h || (full_range | 1) != 1 || ((primaries | transfer | matrix) & ~255)) return MI355ENC_ERR_ARG;
    if (h->n_submitted) return MI355ENC_ERR_STATE; // (what the samples mean is fixed from the stream's first picture on)
    h->col_full = full_range; h->col_prim = primaries; h->col_trc = transfer; h->col_mat = matrix;
    csc_resolve(h);
    return MI355ENC_OK;
}

int mi355enc_host_write_headers_vui(int width, int height, int fps_num, int fps_den, int t8, int sar_w, int sar_h, int full_range, int primaries, int transfer,
                                    int matrix, uint8_t *out, size_t cap, size_t *out_len) {
    if (!out || !out_len || width < 16 || height < 16 || fps_num <= 0 || fps_den <= 0 || sar_w < 0 || sar_h < 0 || sar_w > 65535 || sar_h > 65535 ||
        (full_range | 1) != 1 || ((primaries | transfer | matrix) & ~255)) return MI355ENC_ERR_ARG;
    const size_t n = h264_write_headers_vui(out, cap, width, height, fps_num, fps_den, t8, sar_w, sar_h, full_range, primaries, transfer, matrix);
    if (!n) return MI355ENC_ERR_OVERFLOW;
    *out_len = n;
    return MI355ENC_OK;
}

int mi355enc_stage_csc_device(mi355enc_t *h, int fmt, const void *const d_planes[3], const int strides[3], void *d_out_y, void *d_out_uv) {
    if (!h || !d_planes || !strides || !d_planes[0] || !d_out_y || !d_out_uv || (((uintptr_t)d_out_y | (uintptr_t)d_out_uv) & 7)) return MI355ENC_ERR_ARG;
    if (h->pending) return MI355ENC_ERR_STATE;
    const int w = h->cfg.width, ht = h->cfg.height;
    const uint8_t *p[3] = {(const uint8_t *)d_planes[0], (const uint8_t *)d_planes[1], (const uint8_t *)d_planes[2]};
    int st[3] = {strides[0], strides[1], strides[2]};
    fmt = yv12_as_i420(fmt, p, st);
    // every plane the format reads is there and as wide as the picture: the kernels stay inside rows of these lengths (NV12 is not converted: refused)
    fmt_plane_t pl[3];
    const int nplanes = fmt == MI355ENC_FMT_NV12 ? 0 : fmt_planes(fmt, w, ht, pl);
    if (!nplanes || !planes_fit(nplanes, pl, p, st)) return MI355ENC_ERR_ARG;
    if (fmt >= MI355ENC_FMT_BGRX && !h->csc_ok) return MI355ENC_ERR_ARG;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    int r;
    if (fmt <= MI355ENC_FMT_UYVY) r = k_launch_csc(fmt, p[0], p[1], p[2], st[0], st[1], st[2], (uint8_t *)d_out_y, (uint8_t *)d_out_uv, w, ht, h->W, h->H, h->stream);
    else r = k_launch_csc2(fmt, p[0], p[1], p[2], st[0], st[1], st[2], (uint8_t *)d_out_y, (uint8_t *)d_out_uv, w, ht, h->W, h->H, h->csc_coef, h->stream);
    if (r) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}

} // extern "C"
