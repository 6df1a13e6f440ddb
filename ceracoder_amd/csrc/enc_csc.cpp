// enc_csc.cpp -- colorimetry of a handle (mi355enc_set_colorimetry): the code points every SPS carries, the integer RGB -> Y'CbCr matrix
// that follows from them (DESIGN.md section 11 states the rule; built on the host in double), and the entry points that expose both to tests.
// Also: what submitted YUV samples mean (mi355enc_set_input_colorimetry), the YUV -> YUV table and the colour step's launch.
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

static bool matrix_k(int matrix, double *kr, double *kb) {
    switch (matrix) {
    case 1: *kr = 0.2126; *kb = 0.0722; return true;
    case 5: case 6: *kr = 0.299; *kb = 0.114; return true;
    case 9: *kr = 0.2627; *kb = 0.0593; return true;
    default: return false;
    }
}
// The nine words of mi355enc_yuv_coefficients (DESIGN.md section 20 states the rule); false for a matrix code outside 1, 5, 6, 9.
static bool yuv_matrix(int in_m, int in_full, int out_m, int out_full, int *c) {
#pragma clang fp contract(off) // bit for bit the plain IEEE double restatement (tests/yuvref.py)
    double kr, kb, kr2, kb2;
    if (!matrix_k(in_m, &kr, &kb) || !matrix_k(out_m, &kr2, &kb2)) return false;
    const double kg = 1.0 - kr - kb, kg2 = 1.0 - kr2 - kb2;
    const double ys = in_full ? 255.0 : 219.0, cs = in_full ? 255.0 : 224.0, ys2 = out_full ? 255.0 : 219.0, cs2 = out_full ? 255.0 : 224.0;
    const double lb = 2.0 * (1.0 - kb) * (kb2 - kg2 * kb / kg), lr = 2.0 * (1.0 - kr) * (kr2 - kg2 * kr / kg);
    auto r = [](double x) { return (int)std::floor(x + 0.5); };
    c[0] = r(ys2 / ys * 65536.0);
    c[1] = r(lb * ys2 / cs * 65536.0);
    c[2] = r(lr * ys2 / cs * 65536.0);
    c[3] = r((2.0 * (1.0 - kb) - lb) / (2.0 * (1.0 - kb2)) * cs2 / cs * 65536.0);
    c[4] = r(-lr / (2.0 * (1.0 - kb2)) * cs2 / cs * 65536.0);
    c[5] = r(-lb / (2.0 * (1.0 - kr2)) * cs2 / cs * 65536.0);
    c[6] = r((2.0 * (1.0 - kr) - lr) / (2.0 * (1.0 - kr2)) * cs2 / cs * 65536.0);
    c[7] = in_full ? 0 : 16;
    c[8] = out_full ? 0 : 16;
    return true;
}

void csc_resolve(mi355enc_t *h) {
    // unspecified: what `videoconvert` would have negotiated for a picture of this size -- BT.709 for HD, BT.601 below
    const int by_size = (h->cfg.width > 1024 || h->cfg.height > 576) ? 1 : 6;
    const int m = h->col_mat != 2 ? h->col_mat : by_size;
    h->csc_ok = csc_matrix(m, h->col_full, h->csc_coef);
    // the colour step: none unless the input's meaning was given and differs from the output's (5 and 6 are one matrix)
    h->yuv_on = h->yuv_bad = false;
    if (!h->in_col_set) return;
    const int im = h->in_col_mat != 2 ? h->in_col_mat : by_size;
    h->yuv_bad = !yuv_matrix(im, h->in_col_full, m, h->col_full, h->yuv_coef);
    h->yuv_on = !h->yuv_bad && (h->in_col_full != h->col_full || (im == 5 ? 6 : im) != (m == 5 ? 6 : m));
}

// the part of the coded surfaces that is picture: everything, or with a geometry the destination rectangle mapped through the orientation -- up to the surfaces'
// edge where it reaches the visible picture's (a margin sample is what its clamped visible source is)
void yuv_rect(const mi355enc_t *h, int rect[4]) {
    rect[0] = 0; rect[1] = h->W; rect[2] = 0; rect[3] = h->H;
    if (!h->geom_on) return;
    const int m = h->orient;
    const bool tr = orient_transposes(m);
    const bool fx = m == MI355ENC_ORIENT_180 || m == MI355ENC_ORIENT_90L || m == MI355ENC_ORIENT_HORIZ || m == MI355ENC_ORIENT_UR_LL;
    const bool fy = m == MI355ENC_ORIENT_90R || m == MI355ENC_ORIENT_180 || m == MI355ENC_ORIENT_VERT || m == MI355ENC_ORIENT_UR_LL;
    const mi355enc_geometry_t &g = h->geom;
    // mi355enc_orient_source: output (x, y) reads pre-orientation (fx ? pw - 1 - u : u, fy ? ph - 1 - v : v) with (u, v) = tr ? (y, x) : (x, y)
    const int u0 = fx ? pre_w(h) - g.dst_x - g.dst_w : g.dst_x, v0 = fy ? pre_h(h) - g.dst_y - g.dst_h : g.dst_y;
    rect[0] = tr ? v0 : u0; rect[1] = rect[0] + (tr ? g.dst_h : g.dst_w);
    rect[2] = tr ? u0 : v0; rect[3] = rect[2] + (tr ? g.dst_w : g.dst_h);
    if (rect[1] == h->cfg.width) rect[1] = h->W;
    if (rect[3] == h->cfg.height) rect[3] = h->H;
}

int yuv_run(mi355enc_t *h, slot_t *s, hipStream_t st) {
    int rect[4];
    yuv_rect(h, rect);
    if (k_launch_yuv_convert(s->d_src_y, s->d_src_uv, h->W, h->H, rect, h->yuv_coef, st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}
int yuv_draw(mi355enc_t *h, slot_t *s, hipStream_t st) { return s->yuv_step ? yuv_run(h, s, st) : MI355ENC_OK; }

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
    adjust_retable(h); // (black level and scale of the picture controls are the output range's)
    return MI355ENC_OK;
}

int mi355enc_yuv_coefficients(int in_matrix, int in_full, int out_matrix, int out_full, int32_t coef[9]) {
    int c[9];
    if (!coef || (in_full | 1) != 1 || (out_full | 1) != 1 || !yuv_matrix(in_matrix, in_full, out_matrix, out_full, c)) return MI355ENC_ERR_ARG;
    for (int i = 0; i < 9; i++) coef[i] = c[i];
    return MI355ENC_OK;
}

int mi355enc_set_input_colorimetry(mi355enc_t *h, int full_range, int matrix) {
    if (!h || (full_range | 1) != 1 || (matrix != 1 && matrix != 2 && matrix != 5 && matrix != 6 && matrix != 9)) return MI355ENC_ERR_ARG;
    if (h->n_submitted || h->hdr_on) return MI355ENC_ERR_STATE; // (like the output's: fixed from the stream's first picture on; not beside mi355enc_set_hdr_input)
    h->in_col_set = true; h->in_col_full = full_range; h->in_col_mat = matrix;
    csc_resolve(h);
    return MI355ENC_OK;
}

int mi355enc_stage_yuv_convert(mi355enc_t *h, uint8_t *y, uint8_t *uv) {
    if (!h || !y || !uv) return MI355ENC_ERR_ARG;
    if (!h->yuv_on) return MI355ENC_ERR_STATE;
    slot_t *s = &h->slot[0];
    int r = stage_enter(h);
    if (!r) r = stage_in(h, s, y, uv);
    if (!r) r = yuv_run(h, s, h->stream);
    return r ? r : stage_out(h, s, y, uv);
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
    { int r = stage_enter(h); if (r) return r; }
    const int w = h->cfg.width, ht = h->cfg.height;
    const uint8_t *p[3] = {(const uint8_t *)d_planes[0], (const uint8_t *)d_planes[1], (const uint8_t *)d_planes[2]};
    int st[3] = {strides[0], strides[1], strides[2]};
    fmt = yv12_as_i420(fmt, p, st);
    // every plane the format reads is there and as wide as the picture: the kernels stay inside rows of these lengths (NV12 is not converted: refused)
    fmt_plane_t pl[3];
    const int nplanes = fmt == MI355ENC_FMT_NV12 ? 0 : fmt_planes(fmt, w, ht, pl);
    if (!nplanes || !planes_fit(nplanes, pl, p, st)) return MI355ENC_ERR_ARG;
    if ((fmt_is_rgb(fmt) && !h->csc_ok) || hdr_refuses(h, fmt)) return MI355ENC_ERR_ARG;
    int r;
    if (h->hdr_on) r = hdr_convert(h, fmt, p, st, (uint8_t *)d_out_y, (uint8_t *)d_out_uv, w, ht, h->W, h->H, h->stream); // (tone-mapped: DESIGN.md section 22)
    else if (fmt <= MI355ENC_FMT_UYVY) r = k_launch_csc(fmt, p[0], p[1], p[2], st[0], st[1], st[2], (uint8_t *)d_out_y, (uint8_t *)d_out_uv, w, ht, h->W, h->H, h->stream);
    else r = k_launch_csc2(fmt, p[0], p[1], p[2], st[0], st[1], st[2], (uint8_t *)d_out_y, (uint8_t *)d_out_uv, w, ht, h->W, h->H, h->csc_coef, h->stream);
    if (r) return r < -1 ? r : MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}

} // extern "C"
