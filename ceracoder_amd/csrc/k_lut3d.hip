// k_lut3d.hip -- a 3D colour LUT on the coded NV12 surfaces of a slot, in place (the rule: lut3d_host.h).  One launch.
//
// k_adjust.hip's ownership: a lane owns an 8 x 2 luma patch and its four chroma pairs (8-byte loads and stores), that is four quads of the rule; per sample it
// converts to R'G'B', finds the cell and gathers the four nodes of the tetrahedron -- one dword per node, 64 gathers per lane, at addresses the sample's value
// decides.  Where the patch straddles an edge of the picture rectangle the bytes outside keep their value, per column pair, as in al_apply_kernel.
// The coded margin (rule 6): where the rectangle reaches the visible picture's right (bottom) edge, the lane that owns the patch with the last visible column pair
// (row pair) also stores the margin beside (below) it from the values it has just computed -- luma the last visible column / row, chroma the last visible pair /
// row, the corner both -- so the margin is a replica of the graded picture, is never read, and no lane of a margin patch does anything.
// Two forms, which differ only in where a node comes from:
//   direct   one lane one patch, 256-thread workgroups; the nodes come from global memory (through the vector cache and L2).  Serves every N.
//   staged   at most LUT3D_GRID workgroups of 256 .. 1024 lanes walk the patches in a grid-stride loop; each first copies the whole table into LDS (16-byte loads, 16-byte
//            LDS stores), so the copy is paid once per workgroup and not once per tile, and a node is one ds_read_b32.  N <= LUT3D_STAGED_FIT; above 64 KiB of
//            table (N >= 26) the launch asks for the raised dynamic-LDS limit and a compute unit holds one workgroup.
// No inline assembly, no atomics, no wait on another workgroup.
#include "kernels_common.hpp"
#include "lut3d_host.h"

#define LUT3D_GRID 256       // the staged form's workgroups at most: one per compute unit
#define LUT3D_STAGED_WG 1024

struct lut3d_args {
    uint8_t *y, *uv;
    int W, H, x0, x1, y0, y1; // the surfaces' stride and rows, and the picture rectangle (even) cut to the visible size
    int mx, my;               // whether the margin columns right of x1 / the margin rows below y1 are the graded picture's replica (x1 / y1 is then the visible width / height)
    int items;             // patches of 8 x 2 in the surfaces: (W >> 3) * (H >> 1)
    const unsigned *tab;   // N^3 nodes (staged: 16-byte aligned)
    int N, strength;
    int coef[LUT3D_COEF_WORDS];
};

struct lut3d_global { const unsigned *t; DEV unsigned operator()(int i) const { return ldg32(t + i); } };
struct lut3d_lds { const unsigned *t; DEV unsigned operator()(int i) const { return t[i]; } };

// a patch's two luma rows and its chroma row at row pair ry; part: its column pairs that are written (15: all four, as whole words; a margin row under a patch
// that holds a letterbox border writes the rectangle's pairs alone, the border keeps its bytes); fill: also the whole patches right of it up to the stride, every
// sample the patch's last (chroma: pair)
DEV void lut3d_store(const lut3d_args &a, int ry, int x0, uint64_t o0, uint64_t o1, uint64_t oc, unsigned part, bool fill) {
    const unsigned co = (unsigned)ry * (unsigned)a.W + (unsigned)x0, yo = co + (unsigned)ry * (unsigned)a.W; // (below 2^30: k_launch_lut3d refuses a larger surface)
    uint8_t *py = a.y + yo, *puv = a.uv + co;
    if (part == 15u) {
        stg64(py, make_uint2((unsigned)o0, (unsigned)(o0 >> 32))); stg64(py + a.W, make_uint2((unsigned)o1, (unsigned)(o1 >> 32))); stg64(puv, make_uint2((unsigned)oc, (unsigned)(oc >> 32)));
    } else {
#pragma unroll 1
        for (int k = 0; k < 4; k++)
            if (part >> k & 1u) {
                *(uint16_t *)(py + 2 * k) = (uint16_t)(o0 >> (16 * k)); *(uint16_t *)(py + a.W + 2 * k) = (uint16_t)(o1 >> (16 * k)); *(uint16_t *)(puv + 2 * k) = (uint16_t)(oc >> (16 * k));
            }
    }
    if (!fill) return;
    const unsigned f0 = (unsigned)(o0 >> 56) * 0x01010101u, f1 = (unsigned)(o1 >> 56) * 0x01010101u, fc = (unsigned)(oc >> 48) * 0x00010001u;
    for (int x = x0 + 8; x < a.W; x += 8) { // (the margin is less than 16 columns: at most one patch)
        stg64(py + (x - x0), make_uint2(f0, f0)); stg64(py + a.W + (x - x0), make_uint2(f1, f1)); stg64(puv + (x - x0), make_uint2(fc, fc));
    }
}

// patch tx: the four quads of it inside the rectangle
template <class TAB> DEV void lut3d_patch(const lut3d_args &a, const TAB tab, int tx) {
    const int per_row = a.W >> 3, ry = tx / per_row, x0 = (tx - ry * per_row) * 8;
    if (2 * ry < a.y0 || 2 * ry >= a.y1 || x0 + 8 <= a.x0 || x0 >= a.x1) return;
    const unsigned co = (unsigned)ry * (unsigned)a.W + (unsigned)x0, yo = co + (unsigned)ry * (unsigned)a.W;
    const uint2 s0 = ldg64(a.y + yo), s1 = ldg64(a.y + yo + a.W), sc = ldg64(a.uv + co);
    const uint64_t in0 = s0.x | (uint64_t)s0.y << 32, in1 = s1.x | (uint64_t)s1.y << 32, inc = sc.x | (uint64_t)sc.y << 32;
    uint64_t o0 = 0, o1 = 0, oc = 0;
    const int N = a.N, st = a.strength, yoff = a.coef[18];
#pragma unroll 1
    for (int q = 0; q < 4; q++) { // a quad: its 16 gathers are in flight together; the four quads one after another keep the lane's registers few
        const unsigned l0 = (unsigned)(in0 >> (16 * q)) & 0xffffu, l1 = (unsigned)(in1 >> (16 * q)) & 0xffffu, c = (unsigned)(inc >> (16 * q)) & 0xffffu;
        const unsigned luma = l0 | l1 << 16;
        const int cb = (int)(c & 255u), cr = (int)(c >> 8);
        int su = 0, sv = 0;
        unsigned out = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int yy = (int)((luma >> (8 * k)) & 255u), vy = yy - yoff;
            int idx[4], wt[4];
            lut3d_cell(N, lut3d_rgb(a.coef, vy, cb - 128, cr - 128), lut3d_rgb(a.coef + 3, vy, cb - 128, cr - 128), lut3d_rgb(a.coef + 6, vy, cb - 128, cr - 128), idx, wt);
            const unsigned g = lut3d_blend(tab(idx[0]), tab(idx[1]), tab(idx[2]), tab(idx[3]), wt);
            su += lut3d_dot(a.coef + 12, g); sv += lut3d_dot(a.coef + 15, g);
            out |= (unsigned)lut3d_mix(yy, lut3d_luma(a.coef, g), st) << (8 * k);
        }
        o0 |= (uint64_t)(out & 0xffffu) << (16 * q); o1 |= (uint64_t)(out >> 16) << (16 * q);
        oc |= (uint64_t)((unsigned)lut3d_mix(cb, lut3d_chroma(su), st) | (unsigned)lut3d_mix(cr, lut3d_chroma(sv), st) << 8) << (16 * q);
    }
    if (x0 < a.x0 || x0 + 8 > a.x1) { // straddles an edge of the picture rectangle: per column pair, graded inside, the original bytes outside
        uint64_t m = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) m |= x0 + 2 * k >= a.x0 && x0 + 2 * k < a.x1 ? (uint64_t)0xffffu << (16 * k) : 0;
        o0 = (o0 & m) | (in0 & ~m); o1 = (o1 & m) | (in1 & ~m); oc = (oc & m) | (inc & ~m);
    }
    // rule 6.  right: the patch holds the last visible column pair (x0 < x1 here), so the margin columns of its rows are this lane's; below: it holds the last
    // visible row pair, so the margin rows under it are -- luma the last visible row, chroma the last visible chroma row
    const bool right = a.mx && x0 + 8 >= a.x1, below = a.my && 2 * ry + 2 == a.y1;
    if (right && x0 + 8 > a.x1) { // the patch's own columns from x1 on: the luma of column x1 - 1, the chroma pair of columns x1 - 2, x1 - 1
        const int n = a.x1 - x0; // 2, 4 or 6 visible columns
        const uint64_t keep = ((uint64_t)1 << (8 * n)) - 1, ones = 0x0101010101010101ull & ~keep, pairs = 0x0001000100010001ull & ~keep;
        o0 = (o0 & keep) | ((o0 >> (8 * n - 8)) & 255u) * ones; o1 = (o1 & keep) | ((o1 >> (8 * n - 8)) & 255u) * ones;
        oc = (oc & keep) | ((oc >> (8 * n - 16)) & 0xffffu) * pairs;
    }
    // one store site, in one loop, for the patch's own rows (whole words: outside the rectangle they hold the bytes that were there) and the margin rows under
    // them, where a letterbox border beside the rectangle keeps its own bytes: only the rectangle's column pairs, and with `right` the margin's, are written
    unsigned part = 15u;
    if (below && (x0 < a.x0 || (!a.mx && x0 + 8 > a.x1))) {
        part = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) part |= x0 + 2 * k >= a.x0 && (a.mx || x0 + 2 * k < a.x1) ? 1u << k : 0u;
    }
    const int rows = below ? (a.H >> 1) : ry + 1;
#pragma unroll 1
    for (int r = ry; r < rows; r++) { lut3d_store(a, r, x0, o0, o1, oc, r == ry ? 15u : part, right); o0 = o1; }
}

__global__ __launch_bounds__(256) void lut3d_direct_kernel(lut3d_args a) {
    const int tx = blockIdx.x * 256 + threadIdx.x;
    if (tx < a.items) lut3d_patch(a, lut3d_global{a.tab}, tx);
}

__global__ __launch_bounds__(LUT3D_STAGED_WG) void lut3d_staged_kernel(lut3d_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned lut3d_tab[];
    const int n = a.N * a.N * a.N;
    for (int i = 4 * (int)threadIdx.x; i + 3 < n; i += 4 * (int)blockDim.x) *(uint4 *)(lut3d_tab + i) = ldg128(a.tab + i);
    if ((int)threadIdx.x < (n & 3)) lut3d_tab[(n & ~3) + threadIdx.x] = ldg32(a.tab + (n & ~3) + threadIdx.x);
    __syncthreads();
    for (int tx = blockIdx.x * blockDim.x + threadIdx.x; tx < a.items; tx += gridDim.x * blockDim.x) lut3d_patch(a, lut3d_lds{lut3d_tab}, tx);
}

// y, uv: NV12 surfaces of W x H at stride W (W a multiple of 8, H even, 8-byte aligned); vw x vh: the visible size, even and less than 16 short of W x H; rect {x0,
// x1, y0, y1} even and inside the surfaces, its right (bottom) edge inside the visible size or at W (H): there it reaches the visible edge and the margin beside
// (below) it becomes the graded picture's replica; nodes: N^3 checked words on the device; strength 1 .. 256; coef: mi355enc_lut3d_coefficients'; form 0 direct,
// 1 staged (N <= LUT3D_STAGED_FIT, nodes 16-byte aligned).  -1: arguments outside that, and nothing is launched.
int k_launch_lut3d(uint8_t *y, uint8_t *uv, int W, int H, int vw, int vh, const int rect[4], const uint32_t *nodes, int N, int strength, const int32_t coef[LUT3D_COEF_WORDS], int form, hipStream_t s) {
    if (!y || !uv || !rect || !nodes || !coef || W <= 0 || H <= 0 || (W & 7) || (H & 1) || ((((uintptr_t)y) | ((uintptr_t)uv)) & 7) || (((uintptr_t)nodes) & 3)) return -1;
    if (((rect[0] | rect[1] | rect[2] | rect[3]) & 1) || rect[0] < 0 || rect[2] < 0 || rect[1] > W || rect[3] > H || rect[0] >= rect[1] || rect[2] >= rect[3]) return -1;
    if ((size_t)W * (size_t)H > ((size_t)1 << 30)) return -1; // (the kernels address a surface with 32-bit offsets)
    if (((vw | vh) & 1) || vw > W || vw <= W - 16 || vh > H || vh <= H - 16 || rect[0] >= vw || rect[2] >= vh || (rect[1] > vw && rect[1] != W) || (rect[3] > vh && rect[3] != H)) return -1;
    if (N < LUT3D_N_MIN || N > LUT3D_N_MAX || strength < 1 || strength > 256 || (form != 0 && form != 1)) return -1;
    if (form == 1 && (N > LUT3D_STAGED_FIT || (((uintptr_t)nodes) & 15))) return -1;
    lut3d_args a;
    a.y = y; a.uv = uv; a.W = W; a.H = H; a.x0 = rect[0]; a.y0 = rect[2];
    a.mx = rect[1] > vw; a.x1 = a.mx ? vw : rect[1];
    a.my = rect[3] > vh; a.y1 = a.my ? vh : rect[3];
    a.items = (W >> 3) * (H >> 1);
    a.tab = nodes; a.N = N; a.strength = strength;
    for (int i = 0; i < LUT3D_COEF_WORDS; i++) a.coef[i] = coef[i];
    if (form == 0) {
        hipLaunchKernelGGL(lut3d_direct_kernel, dim3((a.items + 255) / 256), dim3(256), 0, s, a);
        return 0;
    }
    const size_t bytes = (((size_t)N * N * N * 4) + 15) & ~(size_t)15;
    // (per launch: the limit belongs to the function on the current device, and a process may hold handles on several)
    if (bytes > 65536 && hipFuncSetAttribute((const void *)lut3d_staged_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return -1;
    // every compute unit gets a workgroup before any workgroup gets a second patch per lane: the workgroup is as large as a LUT3D_GRID-th of the patches asks
    // for, in whole waves, from 256 lanes (below that, fewer workgroups) up to LUT3D_STAGED_WG (beyond that, the loop)
    int wg = ((a.items + LUT3D_GRID - 1) / LUT3D_GRID + 63) & ~63;
    wg = wg < 256 ? 256 : wg > LUT3D_STAGED_WG ? LUT3D_STAGED_WG : wg;
    const int wgs = (a.items + wg - 1) / wg;
    hipLaunchKernelGGL(lut3d_staged_kernel, dim3(wgs < LUT3D_GRID ? wgs : LUT3D_GRID), dim3(wg), bytes, s, a);
    return 0;
}
