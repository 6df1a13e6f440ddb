// enc_scale.cpp -- the input size of a handle (mi355enc_set_input_size): the downscaling tables, built once on the host in double
// (DESIGN.md section 10 states the rule), their copy on the device, and the entry points that expose them to tests.
#include "enc_internal.hpp"

#include <cmath>
#include <vector>

// Catmull-Rom (a = -0.5), support |t| < 2
static double scale_cubic(double t) {
    t = std::fabs(t);
    if (t < 1.0) return (1.5 * t - 2.5) * t * t + 1.0;
    if (t < 2.0) return ((-0.5 * t + 2.5) * t - 4.0) * t + 2.0;
    return 0.0;
}

// Table `kind` (MI355ENC_SCALE_*) for one axis, `in` -> `out` luma samples: n entries of `taps` coefficients.
// first / q may be null (only the sizes are wanted).  Returns n, or a negative error code.
static int scale_table_build(int in, int out, int kind, int *first, int16_t *q, int *taps_out) {
#pragma clang fp contract(off) // the tables are bit-for-bit those of a plain IEEE double restatement (tests/scaleref.py): no fused multiply-adds
    if (in <= 0 || out <= 0 || (in & 1) || (out & 1) || out > in || in > 8 * out || kind < 0 || kind > 3) return MI355ENC_ERR_ARG;
    const double S = (double)in / (double)out;
    const int n = kind == MI355ENC_SCALE_LUMA ? out : out / 2;
    const double st = kind == MI355ENC_SCALE_CHROMA_V422 ? 2.0 * S : S;
    std::vector<int> lo(n), hi(n);
    std::vector<double> c(n);
    int T = 0;
    for (int i = 0; i < n; i++) {
        double ci;
        if (kind == MI355ENC_SCALE_LUMA || kind == MI355ENC_SCALE_CHROMA_V) ci = (i + 0.5) * S - 0.5;
        else if (kind == MI355ENC_SCALE_CHROMA_H) ci = ((2.0 * i + 0.5) * S - 0.5) / 2.0;
        else ci = (2.0 * i + 1.0) * S - 0.5;
        c[i] = ci;
        lo[i] = (int)std::floor(ci - 2.0 * st) + 1; // the integers j with |j - c| < 2 st
        hi[i] = (int)std::ceil(ci + 2.0 * st) - 1;
        if (hi[i] - lo[i] + 1 > T) T = hi[i] - lo[i] + 1;
    }
    if (taps_out) *taps_out = T;
    if (!first || !q) return n;
    std::vector<double> w(T);
    for (int i = 0; i < n; i++) {
        const int m = hi[i] - lo[i] + 1;
        double sum = 0.0;
        for (int k = 0; k < m; k++) { w[k] = scale_cubic((lo[i] + k - c[i]) / st); sum += w[k]; }
        int tot = 0, big = 0;
        int16_t *qi = q + (size_t)i * T;
        for (int k = 0; k < T; k++) {
            const int v = k < m ? (int)std::floor(w[k] / sum * 16384.0 + 0.5) : 0;
            qi[k] = (int16_t)v;
            tot += v;
            if (k < m && v > qi[big]) big = k; // the largest quantised weight, the lowest index on a tie
        }
        qi[big] = (int16_t)(qi[big] + (16384 - tot));
        first[i] = lo[i];
    }
    return n;
}

// the most source rows (columns) one output tile reads through a table, clamped to the picture
static int scale_tile_reach(const std::vector<int> &first, int taps, int n_out, int n_in, int tile) {
    int most = 0;
    for (int t0 = 0; t0 < n_out; t0 += tile) { // tiles inside the visible picture; those in the margin read what the last one reads
        const int e0 = t0, e1 = t0 + tile - 1 < n_out ? t0 + tile - 1 : n_out - 1;
        int a = first[e0], b = first[e1] + taps - 1;
        a = a < 0 ? 0 : a > n_in - 1 ? n_in - 1 : a;
        b = b < 0 ? 0 : b > n_in - 1 ? n_in - 1 : b;
        if (b - a + 1 > most) most = b - a + 1;
    }
    return most;
}

// Builds the five tables for in_w x in_h -> the pre-orientation target (the coded visible size, exchanged under a transposing method), copies them to the
// device (one allocation per handle) and fills h->scale.
static int scale_setup(mi355enc_t *h, int in_w, int in_h) {
    const int ow = pre_w(h), oh = pre_h(h);
    const int ins[SCALE_TABLES] = {in_w, in_h, in_w, in_h, in_h}, outs[SCALE_TABLES] = {ow, oh, ow, oh, oh};
    const int kinds[SCALE_TABLES] = {MI355ENC_SCALE_LUMA, MI355ENC_SCALE_LUMA, MI355ENC_SCALE_CHROMA_H, MI355ENC_SCALE_CHROMA_V, MI355ENC_SCALE_CHROMA_V422};
    std::vector<int> first[SCALE_TABLES];
    std::vector<int16_t> q[SCALE_TABLES];
    size_t off[SCALE_TABLES], total = 0;
    scale_plan_t p;
    memset(&p, 0, sizeof p);
    for (int t = 0; t < SCALE_TABLES; t++) {
        int T = 0;
        const int n = scale_table_build(ins[t], outs[t], kinds[t], nullptr, nullptr, &T);
        if (n <= 0) return MI355ENC_ERR_ARG;
        first[t].resize(n); q[t].resize((size_t)n * T);
        scale_table_build(ins[t], outs[t], kinds[t], first[t].data(), q[t].data(), &T);
        p.taps[t] = T;
        off[t] = total;
        total += ((size_t)n * 4 + (size_t)n * T * 2 + 15) & ~(size_t)15;
    }
    std::vector<uint8_t> blob(total);
    for (int t = 0; t < SCALE_TABLES; t++) {
        memcpy(blob.data() + off[t], first[t].data(), first[t].size() * 4);
        memcpy(blob.data() + off[t] + first[t].size() * 4, q[t].data(), q[t].size() * 2);
    }
    if (h->d_scale_tab) { (void)hipFree(h->d_scale_tab); h->d_scale_tab = nullptr; h->scale_tab_bytes = 0; }
    HIPCHK(hipMalloc((void **)&h->d_scale_tab, total));
    HIPCHK(hipMemcpy(h->d_scale_tab, blob.data(), total, hipMemcpyHostToDevice));
    h->scale_tab_bytes = total;
    p.in_w = in_w; p.in_h = in_h; p.out_w = ow; p.out_h = oh;
    for (int t = 0; t < SCALE_TABLES; t++) {
        p.first[t] = (const int *)(h->d_scale_tab + off[t]);
        p.q[t] = (const int16_t *)(h->d_scale_tab + off[t] + first[t].size() * 4);
    }
    p.span[0] = scale_tile_reach(first[0], p.taps[0], ow, in_w, SCALE_TILE_W);
    p.span[1] = scale_tile_reach(first[2], p.taps[2], ow / 2, in_w / 2, SCALE_TILE_W / 2);
    p.hrows[0] = scale_tile_reach(first[1], p.taps[1], oh, in_h, SCALE_TILE_H);
    p.hrows[1] = scale_tile_reach(first[3], p.taps[3], oh / 2, in_h / 2, SCALE_TILE_H);
    p.hrows[2] = scale_tile_reach(first[4], p.taps[4], oh / 2, in_h, SCALE_TILE_H);
    h->scale = p;
    return MI355ENC_OK;
}

// SAR of a picture scaled from in_w x in_h to out_w x out_h (square source samples): (in_w * out_h) : (in_h * out_w), reduced, and
// brought into 16 bits by the last continued-fraction convergent that fits.  1:1 when the scale keeps the aspect ratio.
static void scale_sar(int in_w, int in_h, int out_w, int out_h, int *sw, int *sh) {
    unsigned long long a = (unsigned long long)in_w * out_h, b = (unsigned long long)in_h * out_w;
    unsigned long long p0 = 0, q0 = 1, p1 = 1, q1 = 0; // convergents of a / b
    unsigned long long x = a, y = b;
    while (y) {
        const unsigned long long t = x / y, p2 = t * p1 + p0, q2 = t * q1 + q0;
        if (p2 > 65535 || q2 > 65535) break;
        p0 = p1; q0 = q1; p1 = p2; q1 = q2;
        const unsigned long long r = x % y; x = y; y = r;
    }
    *sw = (int)p1; *sh = (int)q1;
}

size_t raw_bytes(const mi355enc_t *h) {
    const int w = h->in_w > h->W ? h->in_w : h->W, ht = h->in_h > h->H ? h->in_h : h->H;
    return (size_t)(4 * w + 48) * ht + 64; // the largest: four bytes per pixel, or three planes of the picture's size, rows at multiples of 16 bytes
}

// The input geometry of a handle: the method, and the input size (in_set: the one mi355enc_set_input_size gave; otherwise it follows the method).  The scaler's
// target is the pre-orientation size, so its limits hold against that; the SAR it makes is written with its terms exchanged when the picture is transposed afterwards.
int geometry_apply(mi355enc_t *h, int orient, bool in_set, int in_w, int in_h) {
    if (h->n_submitted) return MI355ENC_ERR_STATE; // (the stream's geometry is fixed from its first picture on)
    if (orient < MI355ENC_ORIENT_IDENTITY || orient > MI355ENC_ORIENT_UR_LL) return MI355ENC_ERR_ARG;
    const bool tr = orient_transposes(orient);
    const int ow = tr ? h->cfg.height : h->cfg.width, oh = tr ? h->cfg.width : h->cfg.height;
    if (!in_set) { in_w = ow; in_h = oh; }
    if (in_w > 8192 || in_h > 8192 || (in_w & 1) || (in_h & 1) || in_w < ow || in_h < oh || in_w > 8 * ow || in_h > 8 * oh) return MI355ENC_ERR_ARG;
    if (orient == h->orient && in_set == h->in_set && in_w == h->in_w && in_h == h->in_h && (!in_set || h->d_scale_tab)) return MI355ENC_OK; // nothing changes: nothing is touched
    if (h->pending) return MI355ENC_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    { int r = sync_compute(h); if (r) return r; }
    HIPCHK(hipStreamSynchronize(h->cstream));
    const int was = h->orient;
    h->orient = orient; // (scale_setup builds for the pre-orientation target)
    if (in_set) { int r = scale_setup(h, in_w, in_h); if (r) { h->orient = was; return r; } } // (a handle whose input size was never set has no tables, as before)
    h->in_set = in_set;
    h->in_w = in_w; h->in_h = in_h;
    h->scaling = in_w != ow || in_h != oh;
    if (h->scaling) scale_sar(in_w, in_h, ow, oh, &h->sar_w, &h->sar_h);
    else h->sar_w = h->sar_h = in_set ? 1 : 0;
    if (h->sar_w == h->sar_h) h->sar_w = h->sar_h = 0; // square samples: no aspect_ratio_info in the VUI (the headers of an unscaled stream)
    else if (tr) { const int t = h->sar_w; h->sar_w = h->sar_h; h->sar_h = t; } // the samples are turned with the picture
    for (int i = 0; i < NSLOT; i++) { // staging buffers follow the input size (allocated again on first use)
        slot_t *s = &h->slot[i];
        if (s->d_raw) { (void)hipFree(s->d_raw); s->d_raw = nullptr; }
        if (s->d_csc) { (void)hipFree(s->d_csc); s->d_csc = nullptr; }
        orient_free(s);
        jpeg_free(s);
        if (s->h_src) { (void)hipHostFree(s->h_src); s->h_src = nullptr; }
    }
    return MI355ENC_OK;
}

extern "C" {

int mi355enc_scale_table(int in, int out, int kind, int *first, int16_t *coef, size_t coef_cap, int *taps) {
    int T = 0;
    const int n = scale_table_build(in, out, kind, nullptr, nullptr, &T);
    if (n < 0) return n;
    if (taps) *taps = T;
    if (!first && !coef) return n;
    if (!first || !coef) return MI355ENC_ERR_ARG;
    if (coef_cap < (size_t)n * T) return MI355ENC_ERR_OVERFLOW;
    return scale_table_build(in, out, kind, first, coef, &T);
}

int mi355enc_set_input_size(mi355enc_t *h, int in_w, int in_h) {
    if (!h) return MI355ENC_ERR_ARG;
    return geometry_apply(h, h->orient, true, in_w, in_h);
}

int mi355enc_stage_scale(mi355enc_t *h, int fmt, const uint8_t *const planes[3], const int strides[3], uint8_t *out_y, uint8_t *out_uv) {
    if (!h || !out_y || !out_uv) return MI355ENC_ERR_ARG;
    if (h->pending) return MI355ENC_ERR_STATE;
    if (!h->d_scale_tab) return MI355ENC_ERR_STATE; // (mi355enc_set_input_size first)
    HIPCHK(hipSetDevice(h->cfg.device_id));
    slot_t *s = &h->slot[0];
    const uint8_t *p[3];
    int st[3];
    if (fmt >= MI355ENC_FMT_Y42B) { // converted at the input size, then scaled as NV12
        int r = upload_and_convert(h, s, fmt, planes, strides, h->stream);
        if (r) return r;
    } else {
        int r = upload_raw(h, s, fmt, planes, strides, h->stream, p, st);
        if (r) return r;
        in_target_t t;
        r = input_target(h, s, &t);
        if (r) return r;
        if (k_launch_scale(fmt, p[0], p[1], p[2], st[0], st[1], st[2], t.y, t.uv, t.W, t.H, &h->scale, h->stream)) return MI355ENC_ERR_ARG;
        HIPCHK(hipGetLastError());
        r = input_finish(h, s, h->stream);
        if (r) return r;
    }
    HIPCHK(hipMemcpyAsync(out_y, s->d_src_y, h->ysz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(out_uv, s->d_src_uv, h->csz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355ENC_OK;
}

} // extern "C"
