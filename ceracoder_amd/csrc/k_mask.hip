// k_mask.hip -- privacy masks on the coded NV12 surfaces of a slot (the rule: mask_host.h and include/mi355enc.h).
// Hand-written HIP for gfx950 (CDNA4, wave64); part of libmi355enc.
//
// Rule 3 -- every region computes from the picture as it stood -- decides the shape: no launch writes the picture before every region has read it.  The mode
// launches read the picture and write a result surface of the handle's (the picture's layout), each region only the quads it owns (mask_owns: it contains the
// quad and no region in front of it does), so no two regions ever write one byte of it.  The commit launch, last, copies the owned quads into the picture --
// a fill's quads straight from its colour -- and, from a quad at the last visible column or row, stores the coded-size margin beside it as the replica of what
// it wrote (rule 7; the image layers' form: computed values, the margin is never read).
//   mask_cell_kernel    pixelate: one wave per cell, lanes across the cell's columns (at most 64), rows in a loop, the three sums by the DPP wave reduction
//   mask_blur_h_kernel  a 16-row x 256-byte tile and its halo of r samples each side staged in LDS with the positions clamped to C; a lane owns 16 consecutive
//                       bytes of a row: one window sum, then it slides; the 16 results leave as one 16-byte store into a packed ping-pong plane
//   mask_blur_v_kernel  lanes across columns, four byte columns (one dword of a packed plane's row) per lane and a run of 8 rows: one window sum of four
//                       accumulators, then it slides down; every load is a coalesced row segment.  The last pass writes the result surface, owned quads only
//   mask_commit_kernel  a lane owns a quad
// The blur's H, V, H, V go picture -> A -> B -> A -> result.  A and B hold every region of a batch packed one behind the other (rows at multiples of 16
// bytes), luma then chroma; chroma is the same kernel over byte rows whose elements are pairs (comps 2).  A batch is as many regions as fit a plane: one
// region always does, overlapping ones that do not are run in further batches, so the launch count depends on the configuration alone, never on the
// picture's size.  No inline assembly, no atomics, no wait on another workgroup.
#include "kernels_common.hpp"
#include "mask_host.h"

#define MASK_TW 256 // the horizontal pass's tile: bytes of a row ...
#define MASK_TH 16  // ... and rows
#define MASK_HALO 32 // bytes each side at most: r = 32 luma, 16 pairs of chroma
#define MASK_LW (MASK_TW + 2 * MASK_HALO + 4) // a tile row in LDS; 81 dwords: the 4 rows a wave reads start in different banks
#define MASK_VR 8   // the vertical pass's run of rows per lane

// one plane of one region in one blur pass: `rows` rows of n bytes, elements of `comps` interleaved components; px, py: the picture position of its first
// byte in luma samples, rowstep 1 (luma) or 2 (chroma) luma rows per row -- the last pass asks mask_owns with them for region k
struct mask_job { const uint8_t *src; uint8_t *dst; int sstride, dstride, n, rows, comps, r; unsigned recip; int k, px, py, rowstep; };
struct mask_blur_args { mask_job j[2 * MASK_REGIONS_MAX]; mask_tab_t tab; };
struct mask_cell_args { const uint8_t *y, *uv; uint8_t *ry, *ruv; int W, idx[MASK_REGIONS_MAX]; mask_tab_t tab; };
struct mask_commit_args { uint8_t *y, *uv; const uint8_t *ry, *ruv; int W, H, vw, vh; mask_tab_t tab; };

template <int COMPS> DEV void mask_h_run(const mask_job &j, const uint8_t *row, int seg, uint8_t *dst) {
    const int r = j.r, halo = r * COMPS;
    unsigned out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < COMPS; c++) {
        const uint8_t *p = row + halo + seg * 16 + c; // the first output's own sample
        unsigned sum = 0;
        for (int k = -r; k <= r; k++) sum += p[k * COMPS];
#pragma unroll
        for (int m = 0; m < 16 / COMPS; m++) {
            const int q = c + m * COMPS; // the byte of the 16
            out[q >> 2] |= mask_div(sum + (unsigned)r, j.recip) << (8 * (q & 3));
            if (m + 1 < 16 / COMPS) sum += (unsigned)p[(m + 1 + r) * COMPS] - (unsigned)p[(m - r) * COMPS];
        }
    }
    stg128(dst, make_uint4(out[0], out[1], out[2], out[3]));
}

__global__ __launch_bounds__(256) void mask_blur_h_kernel(mask_blur_args a) {
    const mask_job &j = a.j[blockIdx.z];
    const int tx0 = blockIdx.x * MASK_TW, ty0 = blockIdx.y * MASK_TH;
    if (tx0 >= j.n || ty0 >= j.rows) return; // (uniform: the grid is the largest job's)
    __shared__ uint8_t t[MASK_TH][MASK_LW];
    const int cm = j.comps - 1, halo = j.r * j.comps, lw = MASK_TW + 2 * halo, last = (j.n >> cm) - 1;
    for (int rr = 0; rr < MASK_TH; rr++) {
        const int row = ty0 + rr < j.rows ? ty0 + rr : j.rows - 1;
        const uint8_t *s = j.src + (size_t)row * j.sstride;
        for (int i = threadIdx.x; i < lw; i += 256) {
            const int bp = tx0 - halo + i; // the byte position in the row; its element clamped to the row, its component kept
            int e = bp >> cm;
            e = e < 0 ? 0 : e > last ? last : e;
            t[rr][i] = (uint8_t)ldg8(s + (e << cm) + (bp & cm));
        }
    }
    __syncthreads();
    const int rr = threadIdx.x >> 4, seg = threadIdx.x & 15, row = ty0 + rr;
    if (row >= j.rows || tx0 + seg * 16 >= j.n) return;
    uint8_t *dst = j.dst + (size_t)row * j.dstride + tx0 + seg * 16; // (a packed plane: 16-byte aligned, and the row's stride covers the whole 16)
    if (j.comps == 1) mask_h_run<1>(j, t[rr], seg, dst); else mask_h_run<2>(j, t[rr], seg, dst);
}

template <bool FINAL> __global__ __launch_bounds__(256) void mask_blur_v_kernel(mask_blur_args a) {
    const mask_job &j = a.j[blockIdx.z];
    const int b0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, row0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * MASK_VR;
    if (b0 >= j.n || row0 >= j.rows) return;
    const int r = j.r, lastrow = j.rows - 1;
    const uint8_t *src = j.src + b0; // (a packed plane: b0 + 3 is inside the row's stride)
    unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int k = -r; k <= r; k++) {
        const int rw = row0 + k < 0 ? 0 : row0 + k > lastrow ? lastrow : row0 + k;
        const unsigned w = ldg32(src + (size_t)rw * j.sstride);
        s0 += w & 255u; s1 += (w >> 8) & 255u; s2 += (w >> 16) & 255u; s3 += w >> 24;
    }
    for (int m = 0; m < MASK_VR; m++) {
        const int row = row0 + m;
        if (row > lastrow) break;
        const unsigned v0 = mask_div(s0 + (unsigned)r, j.recip), v1 = mask_div(s1 + (unsigned)r, j.recip), v2 = mask_div(s2 + (unsigned)r, j.recip), v3 = mask_div(s3 + (unsigned)r, j.recip);
        uint8_t *d = j.dst + (size_t)row * j.dstride + b0;
        if (!FINAL) stg32(d, v0 | (v1 << 8) | (v2 << 16) | (v3 << 24));
        else { // the result surface at the picture's own place: a byte pair is one quad's -- two luma samples of a row, or a chroma pair
            const int py = (j.py + row * j.rowstep) & ~1;
            if (mask_owns(&a.tab, j.k, j.px + b0, py)) stg16(d, (int)(v0 | (v1 << 8)));
            if (b0 + 2 < j.n && mask_owns(&a.tab, j.k, j.px + b0 + 2, py)) stg16(d + 2, (int)(v2 | (v3 << 8)));
        }
        const int ra = row + r + 1 > lastrow ? lastrow : row + r + 1, rb = row - r < 0 ? 0 : row - r;
        const unsigned wa = ldg32(src + (size_t)ra * j.sstride), wb = ldg32(src + (size_t)rb * j.sstride);
        s0 += (wa & 255u) - (wb & 255u); s1 += ((wa >> 8) & 255u) - ((wb >> 8) & 255u); s2 += ((wa >> 16) & 255u) - ((wb >> 16) & 255u); s3 += (wa >> 24) - (wb >> 24);
    }
}

__global__ __launch_bounds__(64) void mask_cell_kernel(mask_cell_args a) {
    const int k = a.idx[blockIdx.z];
    const mask_reg_t &r = a.tab.r[k];
    const int c = r.param;
    // the cells tile from (x0, y0); the grid starts at the first one that reaches C
    const int gx = r.x0 + ((r.cx0 - r.x0) / c + (int)blockIdx.x) * c, gy = r.y0 + ((r.cy0 - r.y0) / c + (int)blockIdx.y) * c;
    const int ax = gx > r.cx0 ? gx : r.cx0, ay = gy > r.cy0 ? gy : r.cy0, bx = gx + c < r.cx1 ? gx + c : r.cx1, by = gy + c < r.cy1 ? gy + c : r.cy1;
    if (ax >= bx || ay >= by) return; // (uniform)
    const int lane = threadIdx.x, col = ax + lane;
    const bool on = col < bx;
    int sl = 0, sc = 0;
    if (on) {
        for (int y = ay; y < by; y++) sl += (int)ldg8(a.y + (size_t)y * a.W + col);
        for (int y = ay >> 1; y < by >> 1; y++) sc += (int)ldg8(a.uv + (size_t)y * a.W + col);
    }
    // ax is even: an even lane holds Cb, an odd one Cr
    const int tl = wave64_sum(sl), tb = wave64_sum(lane & 1 ? 0 : sc), tr = wave64_sum(lane & 1 ? sc : 0);
    const int nl = (bx - ax) * (by - ay), nc = nl >> 2;
    const unsigned ml = (unsigned)((tl + (nl >> 1)) / nl), mb = (unsigned)((tb + (nc >> 1)) / nc), mr = (unsigned)((tr + (nc >> 1)) / nc);
    if (!on) return;
    for (int y = ay; y < by; y += 2) {
        if (!mask_owns(&a.tab, k, col & ~1, y)) continue;
        stg8(a.ry + (size_t)y * a.W + col, ml); stg8(a.ry + (size_t)(y + 1) * a.W + col, ml);
        stg8(a.ruv + (size_t)(y >> 1) * a.W + col, lane & 1 ? mr : mb);
    }
}

__global__ __launch_bounds__(256) void mask_commit_kernel(mask_commit_args a) {
    const int k = blockIdx.z;
    const mask_reg_t &r = a.tab.r[k];
    const int px = r.cx0 + 2 * (int)(blockIdx.x * 64 + threadIdx.x), py = r.cy0 + 2 * (int)(blockIdx.y * 4 + threadIdx.y);
    if (px >= r.cx1 || py >= r.cy1 || !mask_owns(&a.tab, k, px, py)) return;
    const size_t yo = (size_t)py * a.W + px, co = (size_t)(py >> 1) * a.W + px;
    unsigned v[4], cv;
    if (r.mode == MASK_MODE_FILL) {
        v[0] = v[1] = v[2] = v[3] = (unsigned)r.cy; cv = (unsigned)r.ccb | ((unsigned)r.ccr << 8);
    } else {
        const unsigned d0 = (unsigned)ldg16(a.ry + yo) & 0xFFFFu, d1 = (unsigned)ldg16(a.ry + yo + a.W) & 0xFFFFu;
        v[0] = d0 & 255u; v[1] = d0 >> 8; v[2] = d1 & 255u; v[3] = d1 >> 8; cv = (unsigned)ldg16(a.ruv + co) & 0xFFFFu;
    }
    // the quad itself and, from the last visible quad of a row / column, the coded-size margin beside / below it: quad (dx, dy) of the margin repeats the
    // quad's last column (dx > 0) and last row (dy > 0), its chroma site the quad's
    uint8_t *yp = a.y + yo, *cp = a.uv + co;
    const int nx = px + 2 == a.vw ? (a.W - a.vw) >> 1 : 0, ny = py + 2 == a.vh ? (a.H - a.vh) >> 1 : 0;
    for (int dy = 0; dy <= ny; dy++)
        for (int dx = 0; dx <= nx; dx++) {
#pragma unroll
            for (int jr = 0; jr < 2; jr++) {
                const int q = dy ? 1 : jr;
                const unsigned v0 = dx ? v[2 * q + 1] : v[2 * q], v1 = v[2 * q + 1];
                stg16(yp + (size_t)(2 * dy + jr) * a.W + 2 * dx, (int)(v0 | (v1 << 8)));
            }
            stg16(cp + (size_t)dy * a.W + 2 * dx, (int)cv);
        }
}

static int mask_stride(int n) { return (n + 15) & ~15; }
static size_t mask_packed(const mask_reg_t &r) { return (size_t)mask_stride(r.cx1 - r.cx0) * (size_t)((r.cy1 - r.cy0) * 3 / 2); }

// the four passes over the blur regions idx[0 .. n) (they fit a plane together): picture -> A -> B -> A -> result
static void mask_blur_batch(const uint8_t *y, const uint8_t *uv, int W, const mask_tab_t *tab, const int *idx, int n, uint8_t *res_y, uint8_t *res_uv, uint8_t *pa, uint8_t *pb, hipStream_t s) {
    mask_blur_args a[4];
    int maxn = 0, maxrows = 0;
    size_t off = 0;
    for (int p = 0; p < 4; p++) a[p].tab = *tab;
    for (int i = 0; i < n; i++) {
        const mask_reg_t &r = tab->r[idx[i]];
        const int cw = r.cx1 - r.cx0, ch = r.cy1 - r.cy0, st = mask_stride(cw);
        for (int c = 0; c < 2; c++) { // luma, chroma
            const int rows = c ? ch / 2 : ch, rad = c ? (r.param + 1) >> 1 : r.param;
            const uint8_t *pic = c ? uv + (size_t)(r.cy0 / 2) * W + r.cx0 : y + (size_t)r.cy0 * W + r.cx0;
            uint8_t *out = c ? res_uv + (size_t)(r.cy0 / 2) * W + r.cx0 : res_y + (size_t)r.cy0 * W + r.cx0;
            mask_job j;
            j.n = cw; j.rows = rows; j.comps = c + 1; j.r = rad; j.recip = mask_recip(2 * rad + 1); j.k = idx[i]; j.px = r.cx0; j.py = r.cy0; j.rowstep = c + 1;
            j.src = pic; j.sstride = W; j.dst = pa + off; j.dstride = st; a[0].j[2 * i + c] = j;
            j.src = pa + off; j.sstride = st; j.dst = pb + off; a[1].j[2 * i + c] = j;
            j.src = pb + off; j.dst = pa + off; a[2].j[2 * i + c] = j;
            j.src = pa + off; j.dst = out; j.dstride = W; a[3].j[2 * i + c] = j;
            off += (size_t)st * rows;
            if (rows > maxrows) maxrows = rows;
        }
        if (cw > maxn) maxn = cw;
    }
    const dim3 gh((maxn + MASK_TW - 1) / MASK_TW, (maxrows + MASK_TH - 1) / MASK_TH, 2 * n), gv((maxn + 255) / 256, (maxrows + 4 * MASK_VR - 1) / (4 * MASK_VR), 2 * n);
    hipLaunchKernelGGL(mask_blur_h_kernel, gh, dim3(256), 0, s, a[0]);
    hipLaunchKernelGGL(mask_blur_v_kernel<false>, gv, dim3(256), 0, s, a[1]);
    hipLaunchKernelGGL(mask_blur_h_kernel, gh, dim3(256), 0, s, a[2]);
    hipLaunchKernelGGL(mask_blur_v_kernel<true>, gv, dim3(256), 0, s, a[3]);
}

// y, uv: NV12 surfaces of W x H at stride W (W a multiple of 16, H even); vw x vh: the visible size, even and less than 16 short of W x H; tab: mask_resolve's
// for that visible size; res: a surface of the same layout (W H 3 / 2 bytes); pa, pb: plane_bytes each, at least W H 3 / 2, 16-byte aligned; parts: 1 the
// pixelate launch, 2 the blur launches, 4 the commit launch (a picture: 7).  -1: arguments outside that, and nothing is launched.  *launches (may be null):
// how many launches were enqueued
int k_launch_mask(uint8_t *y, uint8_t *uv, int W, int H, int vw, int vh, const mask_tab_t *tab, uint8_t *res, uint8_t *pa, uint8_t *pb, size_t plane_bytes, int parts, int *launches, hipStream_t s) {
    if (launches) *launches = 0;
    if (!y || !uv || !tab || !res || !pa || !pb || W <= 0 || H <= 0 || (W & 15) || (H & 1) || ((((uintptr_t)y) | ((uintptr_t)uv) | ((uintptr_t)res)) & 1) || ((((uintptr_t)pa) | ((uintptr_t)pb)) & 15)) return -1;
    if (((vw | vh) & 1) || vw < 2 || vh < 2 || vw > W || vw <= W - 16 || vh > H || vh <= H - 16 || plane_bytes < (size_t)W * H * 3 / 2 || tab->n < 0 || tab->n > MASK_REGIONS_MAX || (parts & ~7)) return -1;
    int cells[MASK_REGIONS_MAX], blurs[MASK_REGIONS_MAX], ncell = 0, nblur = 0, any = 0, ccx = 0, ccy = 0, qx = 0, qy = 0;
    for (int k = 0; k < tab->n; k++) {
        const mask_reg_t &r = tab->r[k];
        if (mask_empty(&r)) continue;
        // (what mask_resolve guarantees, and every index of every kernel rests on)
        if (((r.x0 | r.y0 | r.W2 | r.H2 | r.cx0 | r.cy0 | r.cx1 | r.cy1) & 1) || r.cx0 < 0 || r.cy0 < 0 || r.cx1 > vw || r.cy1 > vh || r.cx0 < r.x0 || r.cy0 < r.y0 || r.cx1 > r.x0 + r.W2 || r.cy1 > r.y0 + r.H2) return -1;
        if (r.mode == MASK_MODE_PIXELATE) {
            if (r.param < MASK_CELL_MIN || r.param > MASK_CELL_MAX || (r.param & 1)) return -1;
            const int c = r.param, nx = (r.cx1 - 1 - r.x0) / c - (r.cx0 - r.x0) / c + 1, ny = (r.cy1 - 1 - r.y0) / c - (r.cy0 - r.y0) / c + 1;
            ccx = nx > ccx ? nx : ccx; ccy = ny > ccy ? ny : ccy;
            cells[ncell++] = k;
        } else if (r.mode == MASK_MODE_BLUR) {
            if (r.param < 1 || r.param > MASK_RADIUS_MAX) return -1;
            blurs[nblur++] = k;
        } else if (r.mode != MASK_MODE_FILL) return -1;
        const int nqx = (r.cx1 - r.cx0) >> 1, nqy = (r.cy1 - r.cy0) >> 1;
        qx = nqx > qx ? nqx : qx; qy = nqy > qy ? nqy : qy;
        any = 1;
    }
    if (!any) return 0;
    uint8_t *res_y = res, *res_uv = res + (size_t)W * H;
    int count = 0;
    if ((parts & 1) && ncell) {
        mask_cell_args a;
        a.y = y; a.uv = uv; a.ry = res_y; a.ruv = res_uv; a.W = W; a.tab = *tab;
        for (int i = 0; i < MASK_REGIONS_MAX; i++) a.idx[i] = i < ncell ? cells[i] : 0;
        hipLaunchKernelGGL(mask_cell_kernel, dim3(ccx, ccy, ncell), dim3(64), 0, s, a);
        count++;
    }
    if (parts & 2)
        for (int i = 0; i < nblur;) { // a batch: as many of the regions, in order, as fit a plane together
            int n = 0;
            size_t used = 0;
            while (i + n < nblur && used + mask_packed(tab->r[blurs[i + n]]) <= plane_bytes) { used += mask_packed(tab->r[blurs[i + n]]); n++; }
            if (!n) return -1; // (a region's C is inside the visible picture: one always fits)
            mask_blur_batch(y, uv, W, tab, blurs + i, n, res_y, res_uv, pa, pb, s);
            count += 4;
            i += n;
        }
    if (parts & 4) {
        mask_commit_args a;
        a.y = y; a.uv = uv; a.ry = res_y; a.ruv = res_uv; a.W = W; a.H = H; a.vw = vw; a.vh = vh; a.tab = *tab;
        hipLaunchKernelGGL(mask_commit_kernel, dim3((qx + 63) / 64, (qy + 3) / 4, tab->n), dim3(64, 4), 0, s, a);
        count++;
    }
    if (launches) *launches = count;
    return 0;
}
