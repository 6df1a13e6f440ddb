// k_overlay.hip -- the text overlay: a few lines of an 8 x 16 bitmap font drawn into an NV12 source surface (DESIGN.md section 13 states the rule).
// Hand-written HIP for gfx950 (CDNA4, wave64); part of libmi355enc.
// One launch per picture over the visible part of the box, never the whole picture.  Text, resolved layout and style come by value in the kernel
// arguments; the font is a constant table.  A thread owns one 2 x 2 luma quad and its chroma site: it classifies the four samples (text / outline /
// box) from the glyph bits of the 4 x 4 font pixels around them, reads the picture only where the shaded background needs the old sample, and stores
// what it changes -- nothing else.  The owner of a row's / column's last visible quad also writes the coded-size margin beside / below it from the
// values it computed (at most 7 quads each way).  No LDS, no scratch, no atomics.
#include "kernels_common.hpp"
#include "overlay_font.h"

__constant__ uint8_t k_overlay_font[95 * 16] = {OVERLAY_FONT_ROWS};

// One bit of T on the font-pixel grid of the text area (origin: the first cell's top-left pixel; lines 16 pixels apart, every line shifted by its
// alignment inside the box).  Outside every cell: 0.
DEV unsigned ov_bit(const overlay_args_t &a, int fx, int fy) {
    if (fy < 0 || fy >= 16 * a.nlines) return 0;
    const int li = fy >> 4;
    const int end = a.line_end[li], start = li ? a.line_end[li - 1] + 1 : 0, len = end - start;
    const int off = a.halign == 0 ? 0 : a.halign == 1 ? 4 * (a.maxlen - len) : 8 * (a.maxlen - len);
    const int cx = fx - off;
    if (cx < 0 || cx >= 8 * len) return 0;
    unsigned ch = a.text[start + (cx >> 3)];
    if (ch < 0x20 || ch > 0x7E) ch = '?';
    return (k_overlay_font[(ch - 0x20) * 16 + (fy & 15)] >> (7 - (cx & 7))) & 1u;
}

__global__ __launch_bounds__(256) void overlay_kernel(overlay_args_t a) {
    const int qx = blockIdx.x * 64 + threadIdx.x, qy = blockIdx.y * 4 + threadIdx.y;
    const int x0 = a.gx0 + 2 * qx, y0 = a.gy0 + 2 * qy; // the visible quad this thread owns (gx1 <= vw, gy1 <= vh)
    if (x0 >= a.gx1 || y0 >= a.gy1) return;
    const int s = a.scale;
    // font pixels of the quad's samples: column (x0 + i - tx) / s rounded down, tx the text area's left edge (>= -s from any sample of the box)
    const int tx = a.bx + s, ty = a.by + s;
    int fx[2], fy[2];
#pragma unroll
    for (int i = 0; i < 2; i++) { fx[i] = (x0 + i - tx + s) / s - 1; fy[i] = (y0 + i - ty + s) / s - 1; }
    // T on the 4 x 4 font pixels fx[0] - 1 .. fx[0] + 2, fy[0] - 1 .. fy[0] + 2: bit 4 r + c
    unsigned t = 0;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) t |= ov_bit(a, fx[0] - 1 + c, fy[0] - 1 + r) << (4 * r + c);
    // the four samples (bit / byte 2 j + i): written or not, and the value -- text 235, outline 16, shaded background from the old sample
    unsigned wm = 0, val = 0;
    bool any_ink = false, any_box = false;
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int c = fx[i] - fx[0] + 1, r = fy[j] - fy[0] + 1; // 1 or 2
            const unsigned nb = (t >> (4 * (r - 1) + (c - 1))) & 0x777u; // the 3 x 3 pixels around (r, c)
            const bool self = (t >> (4 * r + c)) & 1u;
            const bool in = x0 + i >= a.bx && x0 + i < a.bx + a.bw && y0 + j >= a.by && y0 + j < a.by + a.bh; // (T and O lie inside the box by construction)
            const bool ink = in && (self || nb), shade = in && !ink && a.shaded;
            unsigned v = self ? 235u : 16u;
            if (shade) v = (ldg8(a.y + (size_t)(y0 + j) * a.stride + x0 + i) + 16u + 1u) >> 1;
            if (ink || shade) { wm |= 1u << (2 * j + i); val |= v << (8 * (2 * j + i)); }
            any_ink |= ink; any_box |= in;
        }
    // chroma of the quad's site
    uint8_t *cp = a.uv + (size_t)(y0 >> 1) * a.stride + x0;
    const bool cw = any_ink || (a.shaded && any_box);
    unsigned cv = 128u | (128u << 8);
    if (cw && !any_ink) cv = ((ldg8(cp) + 128u + 1u) >> 1) | (((ldg8(cp + 1) + 128u + 1u) >> 1) << 8);
    // The quad itself and, from the last visible quad of a row / column, the coded-size margin beside / below it: quad (dx, dy) of the margin repeats the
    // quad's last column (dx > 0) and last row (dy > 0), its chroma site the quad's -- computed values, so the margin is never read.
    const int nx = x0 + 2 == a.vw ? (a.W - a.vw) >> 1 : 0, ny = y0 + 2 == a.vh ? (a.H - a.vh) >> 1 : 0;
    for (int dy = 0; dy <= ny; dy++)
        for (int dx = 0; dx <= nx; dx++) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int k0 = 2 * (dy ? 1 : j) + (dx ? 1 : 0), k1 = 2 * (dy ? 1 : j) + 1;
                const bool w0 = (wm >> k0) & 1u, w1 = (wm >> k1) & 1u;
                const unsigned v0 = (val >> (8 * k0)) & 255u, v1 = (val >> (8 * k1)) & 255u;
                uint8_t *row = a.y + (size_t)(y0 + 2 * dy + j) * a.stride + x0 + 2 * dx;
                if (w0 && w1) stg16(row, v0 | (v1 << 8));
                else if (w0) stg8(row, v0);
                else if (w1) stg8(row + 1, v1);
            }
            if (cw) stg16(cp + (size_t)dy * a.stride + 2 * dx, cv);
        }
}

void k_launch_overlay(const overlay_args_t *a, hipStream_t s) {
    const int nqx = (a->gx1 - a->gx0) >> 1, nqy = (a->gy1 - a->gy0) >> 1;
    if (nqx <= 0 || nqy <= 0) return;
    hipLaunchKernelGGL(overlay_kernel, dim3((nqx + 63) / 64, (nqy + 3) / 4), dim3(64, 4), 0, s, *a);
}
