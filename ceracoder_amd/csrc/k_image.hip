// k_image.hip -- image layers: RGBA pictures with straight alpha blended into an NV12 source surface (DESIGN.md section 17 states the rule).
// Hand-written HIP for gfx950 (CDNA4, wave64); part of libmi355enc.
// image_prepare_kernel runs once per uploaded image: the colour matrix and the byte order are paid there, and every pixel becomes one word
// {Yi, Cbi, Cri, A}.  image_blend_kernel runs once per active layer and picture, over the visible intersection of image and picture from an even
// origin, never over the whole picture.  A thread owns one 2 x 2 luma quad and its chroma site: it loads the (up to) four image words that cover the
// quad -- consecutive lanes read consecutive pixel pairs of an image row, whatever the parity of the place -- reads the quad's two luma pairs and its
// chroma pair as 16-bit words (the widest access a quad at an even column allows), blends, and stores the same three words.  The owner of a row's /
// column's last visible quad also writes the coded-size margin beside / below it from the values it computed (at most 7 quads each way).  Nothing a
// thread reads is written by another one.  No LDS, no scratch, no atomics.
#include "kernels_common.hpp"

struct image_coef_t { int c[10]; };

// shifts: where R, G, B and A lie in a pixel's little-endian word
__global__ __launch_bounds__(256) void image_prepare_kernel(uint32_t *pix, size_t n, int rs, int gs, int bs, int as, image_coef_t k) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned p = ldg32(pix + i);
    const int r = (int)((p >> rs) & 255u), g = (int)((p >> gs) & 255u), b = (int)((p >> bs) & 255u);
    const unsigned a = (p >> as) & 255u;
    const int yi = clip255((k.c[0] * r + k.c[1] * g + k.c[2] * b + (k.c[9] << 16) + (1 << 15)) >> 16);
    const int cb = clip255((k.c[3] * r + k.c[4] * g + k.c[5] * b + (128 << 16) + (1 << 15)) >> 16);
    const int cr = clip255((k.c[6] * r + k.c[7] * g + k.c[8] * b + (128 << 16) + (1 << 15)) >> 16);
    // bytes packed by v_perm: an OR of shifted clipped values is what hipcc turns into gfx950's v_ashr_pk_u8_i32, which leaves bits 31:16 set on MI355X
    // (tests/test_abi_cpu.py, test_device_code_avoids_miscompiled_pack_instruction)
    stg32(pix + i, __builtin_amdgcn_perm(__builtin_amdgcn_perm(a, (unsigned)cr, 0x0c0c0400u), __builtin_amdgcn_perm((unsigned)cb, (unsigned)yi, 0x0c0c0400u), 0x05040100u));
}

__global__ __launch_bounds__(256) void image_blend_kernel(image_args_t a) {
    const int qx = blockIdx.x * 64 + threadIdx.x, qy = blockIdx.y * 4 + threadIdx.y;
    const int x0 = a.gx0 + 2 * qx, y0 = a.gy0 + 2 * qy; // the visible quad this thread owns (gx1 <= vw, gy1 <= vh)
    if (x0 >= a.gx1 || y0 >= a.gy1) return;
    const int px = x0 - a.x, py = y0 - a.y0; // the image pixel under the quad's first sample (-1: the image starts at the second)
    // the four image words (index 2 j + i): alpha scaled by the opacity, 0 for a sample the image does not cover
    unsigned al[4], w[4];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const bool cov = px + i >= 0 && px + i < a.iw && py + j >= 0 && py + j < a.ih;
            const unsigned p = cov ? ldg32(a.img + (size_t)(py + j) * a.iw + (px + i)) : 0u;
            w[2 * j + i] = p;
            al[2 * j + i] = ((p >> 24) * (unsigned)a.opacity + 128u) >> 8;
        }
    uint8_t *yp = a.y + (size_t)y0 * a.stride + x0, *cp = a.uv + (size_t)(y0 >> 1) * a.stride + x0;
    const unsigned d0 = (unsigned)ldg16(yp) & 0xFFFFu, d1 = (unsigned)ldg16(yp + a.stride) & 0xFFFFu, c = (unsigned)ldg16(cp) & 0xFFFFu;
    unsigned v[4]; // the blended luma samples
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned d = ((k < 2 ? d0 : d1) >> (8 * (k & 1))) & 255u;
        v[k] = (d * (255u - al[k]) + (w[k] & 255u) * al[k] + 127u) / 255u;
    }
    unsigned sa = 0, sb = 0, sr = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { sa += al[k]; sb += al[k] * ((w[k] >> 8) & 255u); sr += al[k] * ((w[k] >> 16) & 255u); }
    const unsigned cb = ((c & 255u) * (1020u - sa) + sb + 510u) / 1020u, cr = ((c >> 8) * (1020u - sa) + sr + 510u) / 1020u;
    const unsigned cv = cb | (cr << 8);
    // The quad itself and, from the last visible quad of a row / column, the coded-size margin beside / below it: quad (dx, dy) of the margin repeats the
    // quad's last column (dx > 0) and last row (dy > 0), its chroma site the quad's -- computed values, so the margin is never read.
    const int nx = x0 + 2 == a.vw ? (a.W - a.vw) >> 1 : 0, ny = y0 + 2 == a.vh ? (a.H - a.vh) >> 1 : 0;
    for (int dy = 0; dy <= ny; dy++)
        for (int dx = 0; dx <= nx; dx++) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int r = dy ? 1 : j;
                const unsigned v0 = dx ? v[2 * r + 1] : v[2 * r], v1 = v[2 * r + 1];
                stg16(yp + (size_t)(2 * dy + j) * a.stride + 2 * dx, (int)(v0 | (v1 << 8)));
            }
            stg16(cp + (size_t)dy * a.stride + 2 * dx, (int)cv);
        }
}

int k_launch_image_prepare(uint32_t *pix, size_t n, int fmt, const int *coef, hipStream_t s) {
    int rs, gs, bs, as;
    switch (fmt) {
    case 8: bs = 0; gs = 8; rs = 16; as = 24; break;  // MI355ENC_FMT_BGRX of include/mi355enc.h: B G R A
    case 9: rs = 0; gs = 8; bs = 16; as = 24; break;  // RGBX: R G B A
    case 10: as = 0; rs = 8; gs = 16; bs = 24; break; // XRGB: A R G B
    case 11: as = 0; bs = 8; gs = 16; rs = 24; break; // XBGR: A B G R
    default: return -1;
    }
    if (!n) return 0;
    image_coef_t k;
    for (int i = 0; i < 10; i++) k.c[i] = coef[i];
    hipLaunchKernelGGL(image_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pix, n, rs, gs, bs, as, k);
    return 0;
}

bool k_image_grid(image_args_t *a) {
    const int ix0 = a->x > 0 ? a->x : 0, iy0 = a->y0 > 0 ? a->y0 : 0;
    const int ix1 = a->x + a->iw < a->vw ? a->x + a->iw : a->vw, iy1 = a->y0 + a->ih < a->vh ? a->y0 + a->ih : a->vh;
    if (ix0 >= ix1 || iy0 >= iy1) return false;
    a->gx0 = ix0 & ~1; a->gy0 = iy0 & ~1; a->gx1 = (ix1 + 1) & ~1; a->gy1 = (iy1 + 1) & ~1; // (vw, vh even: still inside the visible picture)
    return true;
}

void k_launch_image_blend(const image_args_t *a, hipStream_t s) {
    const int nqx = (a->gx1 - a->gx0) >> 1, nqy = (a->gy1 - a->gy0) >> 1;
    if (nqx <= 0 || nqy <= 0) return;
    hipLaunchKernelGGL(image_blend_kernel, dim3((nqx + 63) / 64, (nqy + 3) / 4), dim3(64, 4), 0, s, *a);
}
