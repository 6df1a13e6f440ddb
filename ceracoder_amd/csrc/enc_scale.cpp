// enc_scale.cpp -- the input size of a handle (mi355enc_set_input_size): the downscaling tables, built once on the host in double
// (DESIGN.md section 10 states the rule), their copy on the device, and the entry points that expose them to tests; and the input geometry
// (mi355enc_set_input_geometry, mi355enc_set_crop; section 16): the same tables with a crop offset and upscaling, one copy per picture in flight.
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

// Table `kind` (MI355ENC_SCALE_*) for one axis: `in` luma samples from luma offset `off` on (the crop) -> `out` luma samples: n entries of `taps`
// coefficients, indices in the whole source plane.  Upscaling (in < out) uses the unstretched kernel.  first / q may be null (only the sizes are
// wanted).  Returns n, or a negative error code.  With off 0 and in >= out this is section 10's table, entry for entry (0.0 + x is x).
static int geom_table_build(int off, int in, int out, int kind, int *first, int16_t *q, int *taps_out) {
#pragma clang fp contract(off) // the tables are bit-for-bit those of a plain IEEE double restatement (tests/scaleref.py, tests/geomref.py): no fused multiply-adds
    if (off < 0 || in < 2 || out < 2 || ((off | in | out) & 1) || out > 8 * in || in > 8 * out || kind < 0 || kind > 3) return MI355ENC_ERR_ARG;
    const double S = (double)in / (double)out;
    const int n = kind == MI355ENC_SCALE_LUMA ? out : out / 2;
    const double sk = kind == MI355ENC_SCALE_CHROMA_V422 ? 2.0 * S : S;
    const double st = sk > 1.0 ? sk : 1.0;
    std::vector<int> lo(n), hi(n);
    std::vector<double> c(n);
    int T = 0;
    for (int i = 0; i < n; i++) {
        double ci;
        if (kind == MI355ENC_SCALE_LUMA) ci = off + (i + 0.5) * S - 0.5;
        else if (kind == MI355ENC_SCALE_CHROMA_V) ci = off / 2 + (i + 0.5) * S - 0.5; // (off is even)
        else if (kind == MI355ENC_SCALE_CHROMA_H) ci = off / 2 + ((2.0 * i + 0.5) * S - 0.5) / 2.0;
        else ci = off + (2.0 * i + 1.0) * S - 0.5;
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

static int scale_table_build(int in, int out, int kind, int *first, int16_t *q, int *taps_out) {
    if (in <= 0 || out <= 0 || (in & 1) || (out & 1) || out > in || in > 8 * out || kind < 0 || kind > 3) return MI355ENC_ERR_ARG; // (section 10: downscaling only)
    return geom_table_build(0, in, out, kind, first, q, taps_out);
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

// ---- the input geometry
static bool geom_rect_ok(int x, int y, int w, int h, int W, int H) {
    return x >= 0 && y >= 0 && w >= 2 && h >= 2 && !((x | y | w | h) & 1) && x <= W - w && y <= H - h;
}
static bool geom_ratio_ok(int crop, int dst) { return crop <= 8 * dst && dst <= 8 * crop; }
// the validity rule, against the pre-orientation target tw x th
static bool geom_valid(const mi355enc_geometry_t *g, int tw, int th) {
    if (g->in_w < 2 || g->in_h < 2 || g->in_w > 8192 || g->in_h > 8192 || ((g->in_w | g->in_h | tw | th) & 1)) return false;
    if (!geom_rect_ok(g->crop_x, g->crop_y, g->crop_w, g->crop_h, g->in_w, g->in_h) || !geom_rect_ok(g->dst_x, g->dst_y, g->dst_w, g->dst_h, tw, th)) return false;
    if (!geom_ratio_ok(g->crop_w, g->dst_w) || !geom_ratio_ok(g->crop_h, g->dst_h)) return false;
    if (g->border_y < 0 || g->border_y > 255 || g->border_cb < 0 || g->border_cb > 255 || g->border_cr < 0 || g->border_cr > 255) return false;
    return !(g->flags & ~(unsigned)MI355ENC_GEOM_KEEP_SAR);
}
// the most source samples a tile of `tile` target samples reads through a table whose entries start at target sample d0 (clamped into [lo, hi])
static int geom_tile_reach(const int *first, int taps, int n, int d0, int tile, int lo, int hi) {
    int most = 0;
    for (int t0 = (d0 / tile) * tile; t0 < d0 + n; t0 += tile) {
        const int e0 = t0 > d0 ? t0 - d0 : 0, e1 = t0 + tile - 1 < d0 + n ? t0 + tile - 1 - d0 : n - 1;
        int a = first[e0], b = first[e1] + taps - 1;
        a = a < lo ? lo : a > hi ? hi : a;
        b = b < lo ? lo : b > hi ? hi : b;
        if (b - a + 1 > most) most = b - a + 1;
    }
    return most;
}
// room for the largest admissible crop of an axis (section 16: crop <= 8 dst, and inside the input): taps of an entry, and samples a tile of n entries
// `step` apart reaches, for stretch factor k (2 for the chroma rows of 4:2:2 input).  Upper bounds: an entry has fewer than 4 st + 1 taps, and the centres
// of a tile's first and last entry lie (n - 1) step s apart.
static double geom_smax(int in, int dst) { const int c = in < 8 * dst ? in : 8 * dst; return (double)c / dst; }
static int geom_taps_room(double s, double k) { const double st = k * s > 1.0 ? k * s : 1.0; return (int)(4.0 * st) + 2; }
static int geom_reach_room(double s, double k, int n, double step, int limit) {
    const int r = (int)((n - 1) * step * s) + geom_taps_room(s, k) + 2;
    return r < limit ? r : limit;
}

// The tables of geometry g (valid) against target tw x th: into `blob` (room bytes), the plan's sizes, bounds and offsets into *p (pointers left null: off[t] / off[5 + t] say where
// table t's first indices / coefficients lie in the blob, and scale_plan_for points a slot's plan at its copy).  fix: also fix the LDS room from the largest admissible crop (set_input_geometry); otherwise check against
// the room fixed before (set_crop) and answer MI355ENC_ERR_ARG when a table outgrows it.
static int geom_build(const mi355enc_geometry_t *g, int tw, int th, bool fix, scale_plan_t *p, uint8_t *blob, size_t room, size_t *bytes, size_t *off) {
    const int offs[SCALE_TABLES] = {g->crop_x, g->crop_y, g->crop_x, g->crop_y, g->crop_y};
    const int ins[SCALE_TABLES] = {g->crop_w, g->crop_h, g->crop_w, g->crop_h, g->crop_h}, outs[SCALE_TABLES] = {g->dst_w, g->dst_h, g->dst_w, g->dst_h, g->dst_h};
    const int kinds[SCALE_TABLES] = {MI355ENC_SCALE_LUMA, MI355ENC_SCALE_LUMA, MI355ENC_SCALE_CHROMA_H, MI355ENC_SCALE_CHROMA_V, MI355ENC_SCALE_CHROMA_V422};
    scale_plan_t q = *p;
    q.geom = 1;
    q.in_w = g->in_w; q.in_h = g->in_h; q.out_w = tw; q.out_h = th;
    q.dx = g->dst_x; q.dy = g->dst_y; q.dw = g->dst_w; q.dh = g->dst_h;
    // whole picture over the whole target, not scaled up: section 10's launch, instruction for instruction (the plain instance of the kernel)
    q.plain = !g->crop_x && !g->crop_y && g->crop_w == g->in_w && g->crop_h == g->in_h && !g->dst_x && !g->dst_y && g->dst_w == tw && g->dst_h == th && g->crop_w >= tw && g->crop_h >= th;
    q.border[0] = g->border_y; q.border[1] = g->border_cb; q.border[2] = g->border_cr;
    q.lo[0] = g->crop_x; q.hi[0] = g->crop_x + g->crop_w - 1;
    q.lo[1] = g->crop_y; q.hi[1] = g->crop_y + g->crop_h - 1;
    q.lo[2] = g->crop_x / 2; q.hi[2] = (g->crop_x + g->crop_w) / 2 - 1;
    q.lo[3] = g->crop_y / 2; q.hi[3] = (g->crop_y + g->crop_h) / 2 - 1;
    q.lo[4] = g->crop_y; q.hi[4] = g->crop_y + g->crop_h - 1;
    if (fix) {
        const double sx = geom_smax(g->in_w, g->dst_w), sy = geom_smax(g->in_h, g->dst_h);
        q.cap_taps[0] = geom_taps_room(sx, 1); q.cap_taps[1] = geom_taps_room(sy, 1); q.cap_taps[2] = geom_taps_room(sx, 1);
        q.cap_taps[3] = geom_taps_room(sy, 1); q.cap_taps[4] = geom_taps_room(sy, 2);
        q.span[0] = geom_reach_room(sx, 1, SCALE_TILE_W, 1, g->in_w); q.span[1] = geom_reach_room(sx, 1, SCALE_TILE_W / 2, 1, g->in_w / 2);
        q.hrows[0] = geom_reach_room(sy, 1, SCALE_TILE_H, 1, g->in_h); q.hrows[1] = geom_reach_room(sy, 1, SCALE_TILE_H, 1, g->in_h / 2);
        q.hrows[2] = geom_reach_room(sy, 2, SCALE_TILE_H, 2, g->in_h);
    }
    size_t total = 0;
    for (int t = 0; t < SCALE_TABLES; t++) {
        int T = 0;
        const int n = geom_table_build(offs[t], ins[t], outs[t], kinds[t], nullptr, nullptr, &T);
        if (n <= 0 || T > q.cap_taps[t]) return MI355ENC_ERR_ARG;
        const size_t need = ((size_t)n * 4 + (size_t)n * T * 2 + 15) & ~(size_t)15;
        if (total + need > room) return MI355ENC_ERR_ARG;
        int *first = (int *)(blob + total);
        int16_t *coef = (int16_t *)(blob + total + (size_t)n * 4);
        geom_table_build(offs[t], ins[t], outs[t], kinds[t], first, coef, &T);
        q.taps[t] = T;
        q.first[t] = nullptr; q.q[t] = nullptr;
        off[t] = total; off[SCALE_TABLES + t] = total + (size_t)n * 4;
        // what a tile really reads must fit the room fixed with the geometry (it does: the room is an upper bound)
        const bool horiz = t == 0 || t == 2, chroma = t >= 2;
        const int d0 = (horiz ? g->dst_x : g->dst_y) >> (chroma ? 1 : 0), tile = horiz ? (chroma ? SCALE_TILE_W / 2 : SCALE_TILE_W) : SCALE_TILE_H;
        const int reach = geom_tile_reach(first, T, n, d0, tile, q.lo[t], q.hi[t]);
        const int have = t == 0 ? q.span[0] : t == 2 ? q.span[1] : t == 1 ? q.hrows[0] : t == 3 ? q.hrows[1] : q.hrows[2];
        if (reach > have) return MI355ENC_ERR_ARG;
        total += need;
    }
    *p = q;
    *bytes = total;
    return MI355ENC_OK;
}
// bytes of one copy of the tables at the largest admissible crop
static size_t geom_room(const mi355enc_geometry_t *g) {
    const double sx = geom_smax(g->in_w, g->dst_w), sy = geom_smax(g->in_h, g->dst_h);
    const int n[SCALE_TABLES] = {g->dst_w, g->dst_h, g->dst_w / 2, g->dst_h / 2, g->dst_h / 2};
    const int T[SCALE_TABLES] = {geom_taps_room(sx, 1), geom_taps_room(sy, 1), geom_taps_room(sx, 1), geom_taps_room(sy, 1), geom_taps_room(sy, 2)};
    size_t total = 0;
    for (int t = 0; t < SCALE_TABLES; t++) total += ((size_t)n[t] * 4 + (size_t)n[t] * T[t] * 2 + 15) & ~(size_t)15;
    return total;
}
static void geom_free(mi355enc_t *h) {
    if (h->h_geom_tab) { (void)hipHostFree(h->h_geom_tab); h->h_geom_tab = nullptr; }
    h->geom_room = 0;
}
void scale_free(mi355enc_t *h) {
    if (h->d_scale_tab) { (void)hipFree(h->d_scale_tab); h->d_scale_tab = nullptr; h->scale_tab_bytes = 0; }
    geom_free(h);
}
// Device and pinned room for NSLOT copies of the tables (a picture in flight keeps the crop it was submitted under) plus the host's current copy, and the
// tables of g as the current ones.  The caller has made sure nothing is in flight.
static int geom_setup(mi355enc_t *h, const mi355enc_geometry_t *g) {
    const size_t room = geom_room(g);
    uint8_t *hp = nullptr, *dp = nullptr;
    HIPCHK(hipHostMalloc((void **)&hp, room * (NSLOT + 2), hipHostMallocDefault)); // (the slots' copies, the current tables, and set_crop's candidate)
    scale_plan_t p;
    memset(&p, 0, sizeof p);
    size_t bytes = 0, off[2 * SCALE_TABLES];
    int r = geom_build(g, pre_w(h), pre_h(h), true, &p, hp + room * NSLOT, room, &bytes, off);
    if (!r && hipMalloc((void **)&dp, room * NSLOT) != hipSuccess) r = MI355ENC_ERR_HIP;
    if (r) { (void)hipHostFree(hp); return r; }
    scale_free(h);
    h->h_geom_tab = hp; h->geom_room = room; h->geom_bytes = bytes;
    h->d_scale_tab = dp; h->scale_tab_bytes = room * NSLOT;
    h->scale = p;
    memcpy(h->geom_off, off, sizeof off);
    h->geom_gen++;
    return MI355ENC_OK;
}

const scale_plan_t *scale_plan_for(mi355enc_t *h, slot_t *s, hipStream_t up) {
    if (!h->geom_on) return &h->scale;
    const int i = (int)(s - h->slot);
    if (h->geom_slot_gen[i] != h->geom_gen) { // the crop has changed since this slot's copy was made: the current tables follow, in stream order, in front of the launch
        uint8_t *hp = h->h_geom_tab + h->geom_room * i, *dp = h->d_scale_tab + h->geom_room * i; // (the slot's last picture has been collected, and with it the last transfer from here is done -- unless the last submit into this slot failed behind this point; such an error ends the stream)
        memcpy(hp, h->h_geom_tab + h->geom_room * NSLOT, h->geom_bytes);
        if (hipMemcpyAsync(dp, hp, h->geom_bytes, hipMemcpyHostToDevice, up) != hipSuccess) return nullptr;
        scale_plan_t p = h->scale;
        for (int t = 0; t < SCALE_TABLES; t++) {
            p.first[t] = (const int *)(dp + h->geom_off[t]);
            p.q[t] = (const int16_t *)(dp + h->geom_off[SCALE_TABLES + t]);
        }
        h->geom_plan[i] = p;
        h->geom_slot_gen[i] = h->geom_gen;
    }
    return &h->geom_plan[i];
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
    // Bounds every layout of fmt_planes() with rows at multiples of 16 bytes: no format has more than four bytes per pixel in all its planes together, plane by
    // plane at most ht rows each (4:2:0 chroma, with half the rows, counts for less), and at most three planes round a row up, by 15 bytes each: (4 w + 45) ht.
    return (size_t)(4 * w + 48) * ht + 64;
}

// The input geometry of a handle: the method, and the input size (in_set: the one mi355enc_set_input_size gave; otherwise it follows the method).  The scaler's
// target is the pre-orientation size, so its limits hold against that; the SAR it makes is written with its terms exchanged when the picture is transposed afterwards.
int geometry_apply(mi355enc_t *h, int orient, bool in_set, int in_w, int in_h, const mi355enc_geometry_t *geom) {
    if (h->n_submitted) return MI355ENC_ERR_STATE; // (the stream's geometry is fixed from its first picture on)
    if (orient < MI355ENC_ORIENT_IDENTITY || orient > MI355ENC_ORIENT_UR_LL) return MI355ENC_ERR_ARG;
    const bool tr = orient_transposes(orient);
    const int ow = tr ? h->cfg.height : h->cfg.width, oh = tr ? h->cfg.width : h->cfg.height;
    mi355enc_geometry_t g;
    memset(&g, 0, sizeof g);
    if (geom) { // (section 16) the input size is the geometry's; a copy: the setters pass the handle's own
        g = *geom;
        if (!geom_valid(&g, ow, oh)) return MI355ENC_ERR_ARG;
        in_set = false; in_w = g.in_w; in_h = g.in_h;
    }
    if (!geom && !in_set) { in_w = ow; in_h = oh; }
    if (!geom && (in_w > 8192 || in_h > 8192 || (in_w & 1) || (in_h & 1) || in_w < ow || in_h < oh || in_w > 8 * ow || in_h > 8 * oh)) return MI355ENC_ERR_ARG;
    if (!geom && !h->geom_on && orient == h->orient && in_set == h->in_set && in_w == h->in_w && in_h == h->in_h && (!in_set || h->d_scale_tab)) return MI355ENC_OK; // nothing changes: nothing is touched
    if (h->pending) return MI355ENC_ERR_STATE;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    { int r = sync_compute(h); if (r) return r; }
    HIPCHK(hipStreamSynchronize(h->cstream));
    const int was = h->orient;
    h->orient = orient; // (scale_setup builds for the pre-orientation target)
    if (geom) { int r = geom_setup(h, &g); if (r) { h->orient = was; return r; } }
    else if (in_set) { geom_free(h); int r = scale_setup(h, in_w, in_h); if (r) { h->orient = was; return r; } } // (a handle whose input size was never set has no tables, as before)
    h->geom_on = geom != nullptr;
    if (geom) h->geom = g;
    h->in_set = in_set;
    h->in_w = in_w; h->in_h = in_h;
    h->scaling = geom || in_w != ow || in_h != oh; // (a geometry always goes through the scale launch: it writes the border)
    if (geom) (void)mi355enc_geometry_sar(&g, 0, &h->sar_w, &h->sar_h); // (not yet exchanged: below, as the scaler's)
    else if (h->scaling) scale_sar(in_w, in_h, ow, oh, &h->sar_w, &h->sar_h);
    else h->sar_w = h->sar_h = in_set ? 1 : 0;
    if (h->sar_w == h->sar_h) h->sar_w = h->sar_h = 0; // square samples: no aspect_ratio_info in the VUI (the headers of an unscaled stream)
    else if (tr) { const int t = h->sar_w; h->sar_w = h->sar_h; h->sar_h = t; } // the samples are turned with the picture
    stab_free(h); // (the stabiliser's buffers too)
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

int mi355enc_geometry_table(int crop_off, int crop, int dst, int kind, int *first, int16_t *coef, size_t coef_cap, int *taps) {
    int T = 0;
    const int n = geom_table_build(crop_off, crop, dst, kind, nullptr, nullptr, &T);
    if (n < 0) return n;
    if (taps) *taps = T;
    if (!first && !coef) return n;
    if (!first || !coef) return MI355ENC_ERR_ARG;
    if (coef_cap < (size_t)n * T) return MI355ENC_ERR_OVERFLOW;
    return geom_table_build(crop_off, crop, dst, kind, first, coef, &T);
}

int mi355enc_fit_rect(int src_w, int src_h, int tw, int th, int *dx, int *dy, int *dw, int *dh) {
    if (src_w <= 0 || src_h <= 0 || tw < 2 || th < 2 || ((tw | th) & 1) || !dx || !dy || !dw || !dh) return MI355ENC_ERR_ARG;
    // the constrained axis is filled; the other one is 2 round(other / 2) in integers: other / 2 = tw src_h / (2 src_w), rounded half up
    long long w = tw, ht = th;
    if ((long long)tw * src_h <= (long long)th * src_w) ht = 2 * (((long long)tw * src_h + src_w) / (2ll * src_w));
    else w = 2 * (((long long)th * src_w + src_h) / (2ll * src_h));
    if (w > tw) w = tw;
    if (ht > th) ht = th;
    if (w < 2) w = 2;
    if (ht < 2) ht = 2;
    *dw = (int)w; *dh = (int)ht;
    *dx = ((tw - *dw) / 4) * 2; *dy = ((th - *dh) / 4) * 2;
    return MI355ENC_OK;
}

int mi355enc_geometry_check(const mi355enc_geometry_t *g, int tw, int th) {
    return g && tw >= 2 && th >= 2 && geom_valid(g, tw, th) ? MI355ENC_OK : MI355ENC_ERR_ARG;
}

// exact: (cw dh) : (ch dw) -- or nothing at all (the letterbox mode: its rounding to even sizes is not an aspect ratio anybody meant)
int mi355enc_geometry_sar(const mi355enc_geometry_t *g, int transposed, int *sar_w, int *sar_h) {
    if (!g || !sar_w || !sar_h || g->crop_w <= 0 || g->crop_h <= 0 || g->dst_w <= 0 || g->dst_h <= 0) return MI355ENC_ERR_ARG;
    int a = 0, b = 0;
    if (!(g->flags & MI355ENC_GEOM_KEEP_SAR)) scale_sar(g->crop_w, g->crop_h, g->dst_w, g->dst_h, &a, &b);
    if (a == b) a = b = 0;
    *sar_w = transposed ? b : a; *sar_h = transposed ? a : b;
    return MI355ENC_OK;
}

int mi355enc_set_input_geometry(mi355enc_t *h, const mi355enc_geometry_t *g) {
    if (!h || !g) return MI355ENC_ERR_ARG;
    return geometry_apply(h, h->orient, false, 0, 0, g);
}

int mi355enc_get_input_geometry(const mi355enc_t *h, mi355enc_geometry_t *g) {
    if (!h || !g) return MI355ENC_ERR_ARG;
    if (!h->geom_on) return MI355ENC_ERR_STATE;
    *g = h->geom;
    return MI355ENC_OK;
}

// Between submits: host work only.  The candidate tables are built beside the current ones in the pinned block; a refused crop leaves everything as it was.
// Nothing is allocated on the device or pinned, no stream is waited for; the tables travel with the next submit (scale_plan_for).
int mi355enc_set_crop(mi355enc_t *h, int cx, int cy, int cw, int ch) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!h->geom_on) return MI355ENC_ERR_STATE;
    mi355enc_geometry_t g = h->geom;
    g.crop_x = cx; g.crop_y = cy; g.crop_w = cw; g.crop_h = ch;
    if (!geom_valid(&g, pre_w(h), pre_h(h))) return MI355ENC_ERR_ARG;
    if (!(g.flags & MI355ENC_GEOM_KEEP_SAR) && (long long)cw * h->geom.crop_h != (long long)ch * h->geom.crop_w) return MI355ENC_ERR_ARG; // (the SPS would have to change)
    if (cx == h->geom.crop_x && cy == h->geom.crop_y && cw == h->geom.crop_w && ch == h->geom.crop_h) return MI355ENC_OK;
    scale_plan_t p = h->scale;
    size_t bytes = 0, off[2 * SCALE_TABLES];
    uint8_t *cur = h->h_geom_tab + h->geom_room * NSLOT, *cand = cur + h->geom_room;
    int r = geom_build(&g, pre_w(h), pre_h(h), false, &p, cand, h->geom_room, &bytes, off);
    if (r) return r;
    memcpy(cur, cand, bytes);
    h->scale = p; h->geom_bytes = bytes; h->geom = g;
    memcpy(h->geom_off, off, sizeof off);
    h->geom_gen++;
    return MI355ENC_OK;
}

int mi355enc_stage_geometry(mi355enc_t *h, int fmt, const uint8_t *const planes[3], const int strides[3], uint8_t *out_y, uint8_t *out_uv) {
    if (!h || !h->geom_on) return h ? MI355ENC_ERR_STATE : MI355ENC_ERR_ARG;
    return mi355enc_stage_scale(h, fmt, planes, strides, out_y, out_uv);
}

int mi355enc_stage_scale(mi355enc_t *h, int fmt, const uint8_t *const planes[3], const int strides[3], uint8_t *out_y, uint8_t *out_uv) {
    if (!h || !out_y || !out_uv) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; }
    if (!h->d_scale_tab) return MI355ENC_ERR_STATE; // (mi355enc_set_input_size first)
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
        const scale_plan_t *pl = scale_plan_for(h, s, h->stream);
        if (!pl) return MI355ENC_ERR_HIP;
        r = input_scale(h, s, fmt, p[0], p[1], p[2], st[0], st[1], st[2], &t, pl, h->stream);
        if (r) return r;
        HIPCHK(hipGetLastError());
        r = input_finish(h, s, h->stream);
        if (r) return r;
    }
    return stage_out(h, s, out_y, out_uv);
}

} // extern "C"
