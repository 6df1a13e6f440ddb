// k_scale.hip -- scaling of the input picture to the coded size, on the way in (NV12, I420, YUY2, UYVY -> NV12): the downscale of DESIGN.md
// section 10, and the input geometry of section 16 (a crop rectangle resampled into a destination rectangle, border colour around it)
// Hand-written HIP for gfx950 (CDNA4, wave64); part of libmi355enc (see kernels_common.hpp).
#include "kernels_common.hpp"

// One launch per picture.  A workgroup owns an output tile of SCALE_TILE_W bytes x SCALE_TILE_H rows of one NV12 plane (luma: 64
// samples; chroma: 32 (U,V) pairs) and runs the separable filter of DESIGN.md section 10 in two passes:
//   1. horizontal: the source rows the tile's vertical support needs, SCALE_CHUNK rows at a time -- the row segments the tile's
//      horizontal taps cover are fetched as aligned dwords into LDS (a byte-wise fetch where a row's end or its alignment does not allow
//      it), then every (row, output column) is filtered from LDS into an int16 intermediate, also in LDS;
//   2. vertical: every output byte of the tile from the intermediate rows.
// Source indices outside the picture are clamped to its edge; output positions in the coded-size margin take the table entry of the
// last visible row / column / chroma pair, so the margin repeats them (as csc_kernel's does).  The tables are read once per tile
// into LDS.  Arithmetic: h = (sum q * src + 2^7) >> 8 (int16), out = clip((sum q * h + 2^19) >> 20).
// GEOM (section 16): the tables hold one entry per sample of the destination rectangle, with indices in the whole source plane; a tap index is
// clamped into the crop rectangle [lo, hi] of its table, and no byte outside the crop rectangle is fetched (the dwords that straddle its left or right
// edge go byte by byte).  A target position outside the destination rectangle takes the border colour, in the same full-width store; a tile that
// lies wholly outside it skips both passes.  Without GEOM the kernel is the downscale as it was, instruction for instruction.
// GEOM with a.stab (section 26): every table index and the clamp rectangle are displaced by the offset read there -- luma by (ox, oy), chroma columns by ox / 2,
// chroma rows by oy / 2 (4:2:2 input: oy); weights, reach and LDS room are those of the crop as set, since indices and bounds move together.
#define DEV_HOST_SCALE static __host__ __device__ __forceinline__
struct scale_args {
    const uint8_t *p0, *p1, *p2; // NV12: Y, UV; I420: Y, U, V; packed formats: p0 only
    int s0, s1, s2;              // their strides in bytes
    uint8_t *dy, *duv;           // NV12 destination, coded size W x H, stride W
    int W, H;
    int ltiles_x, ltiles;        // tiles per row, luma tiles (the chroma tiles follow them in the grid)
    int rawb;                    // bytes per staged source row in LDS
    int hmax;                    // intermediate rows the LDS holds
    int tmax_h, tmax_v;          // LDS room for coefficients per output column / row
    scale_plan_t p;
    const int *stab;             // GEOM: the stabiliser's {ox, oy} for this picture on the device; null: none
};

// one contiguous byte range of a source row, fetched into LDS
struct span_t {
    const uint8_t *base; int stride, rowbytes; // plane, its stride, the bytes a row holds
    int a0, nw, lds;                           // first byte (multiple of 4), dwords, offset in the staged row
    int b0;                                    // GEOM: the first byte of a row that may be read (rowbytes: the end)
};

// int16 coefficients of a tile in LDS, rounded up to 8 bytes
DEV_HOST_SCALE int scale_coef_room(int tmh, int tmv) { return (SCALE_TILE_W * tmh + SCALE_TILE_H * tmv + 3) & ~3; }

template <int FMT, bool GEOM> // 0 NV12, 1 I420, 2 YUY2 (Y0 U Y1 V), 3 UYVY (U Y0 V Y1)
__global__ __launch_bounds__(256) void scale_kernel(const scale_args a) {
    extern __shared__ __align__(16) uint8_t lds[];
    const int tid = threadIdx.x;
    const bool luma = (int)blockIdx.x < a.ltiles;
    const int tile = luma ? blockIdx.x : blockIdx.x - a.ltiles;
    const int tx = tile % a.ltiles_x, ty = tile / a.ltiles_x;
    const int th = luma ? 0 : 2, tv = luma ? 1 : (FMT >= 2 ? 4 : 3); // tables
    const int *__restrict__ fh = a.p.first[th];
    const int *__restrict__ fv = a.p.first[tv];
    const int16_t *__restrict__ qh = a.p.q[th];
    const int16_t *__restrict__ qv = a.p.q[tv];
    const int nth = a.p.taps[th], ntv = a.p.taps[tv];
    // geometry of this plane: output samples per row / rows, source samples per row / rows
    const int nout_x = luma ? a.p.out_w : a.p.out_w >> 1, nout_y = luma ? a.p.out_h : a.p.out_h >> 1;
    const int nin_x = luma ? a.p.in_w : a.p.in_w >> 1, nin_y = luma || FMT >= 2 ? a.p.in_h : a.p.in_h >> 1;
    const int rows_here = luma ? a.H : a.H >> 1; // coded rows of this plane
    // output index of element e (0 .. 63) of a tile row, clamped into the visible picture (the margin repeats the last one)
    auto col_of = [&](int e) { const int c = luma ? tx * SCALE_TILE_W + e : tx * (SCALE_TILE_W / 2) + (e >> 1); return c < nout_x ? c : nout_x - 1; };
    auto row_of = [&](int o) { const int r = ty * SCALE_TILE_H + o; return r < nout_y ? r : nout_y - 1; };
    // clamp bounds of the source indices (the crop rectangle), and the destination rectangle in this plane's samples
    int ofx = 0, ofy = 0; // the stabiliser's displacement in this plane's samples (even luma offsets: the halves are exact)
    if (GEOM && a.stab) { ofx = luma ? a.stab[0] : a.stab[0] / 2; ofy = luma || FMT >= 2 ? a.stab[1] : a.stab[1] / 2; }
    const int xlo = GEOM ? a.p.lo[th] + ofx : 0, xhi = GEOM ? a.p.hi[th] + ofx : nin_x - 1;
    const int ylo = GEOM ? a.p.lo[tv] + ofy : 0, yhi = GEOM ? a.p.hi[tv] + ofy : nin_y - 1;
    const int ddx = !GEOM ? 0 : luma ? a.p.dx : a.p.dx >> 1, ddy = !GEOM ? 0 : luma ? a.p.dy : a.p.dy >> 1;
    const int ndx = !GEOM ? nout_x : luma ? a.p.dw : a.p.dw >> 1, ndy = !GEOM ? nout_y : luma ? a.p.dh : a.p.dh >> 1;
    auto clamp3 = [](int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; };
    // table entry of tile element e / tile row o: counted from the destination rectangle's first sample (outside it: the nearest one, never used for output)
    auto tcol = [&](int e) { return GEOM ? clamp3(col_of(e) - ddx, 0, ndx - 1) : col_of(e); };
    auto trow = [&](int o) { return GEOM ? clamp3(row_of(o) - ddy, 0, ndy - 1) : row_of(o); };
    // (block-uniform) does the tile hold any sample of the destination rectangle?
    const bool any = !GEOM || (col_of(SCALE_TILE_W - 1) >= ddx && col_of(0) < ddx + ndx && row_of(SCALE_TILE_H - 1) >= ddy && row_of(0) < ddy + ndy);

    // LDS: [horizontal coefficients 64 x tmax_h][vertical coefficients 16 x tmax_v][first source column per element 64]
    //      [intermediate hmax x 64 int16][staged source rows SCALE_CHUNK x rawb]
    int16_t *cq_h = (int16_t *)lds;
    int16_t *cq_v = cq_h + SCALE_TILE_W * a.tmax_h;
    int *cf_h = (int *)(cq_h + scale_coef_room(a.tmax_h, a.tmax_v)); // (8-byte aligned: the vertical pass reads the intermediate as uint2)
    int16_t *hbuf = (int16_t *)(cf_h + SCALE_TILE_W);
    uint8_t *raw = (uint8_t *)(hbuf + (size_t)a.hmax * SCALE_TILE_W);

    // rows and columns of the source this tile reads
    const int ya = clamp3(fv[trow(0)] + ofy, ylo, yhi), yb = clamp3(fv[trow(SCALE_TILE_H - 1)] + ofy + ntv - 1, ylo, yhi);
    const int nh = yb - ya + 1;
    const int xa = clamp3(fh[tcol(0)] + ofx, xlo, xhi), xb = clamp3(fh[tcol(SCALE_TILE_W - 1)] + ofx + nth - 1, xlo, xhi);
    if (nh > a.hmax) return; // (cannot happen: the host sized the LDS for the largest tile; wave-uniform)
    if (GEOM && (nth > a.tmax_h || ntv > a.tmax_v)) return; // (nor this: mi355enc_set_crop refuses a crop whose tables outgrow the room fixed with the geometry)

    // where component c of source sample x lies: plane (span), byte step and offset
    constexpr int ystep = FMT >= 2 ? 2 : 1, yoff = FMT == 3 ? 1 : 0;
    constexpr int cstep = FMT == 0 ? 2 : FMT == 1 ? 1 : 4;
    constexpr int uoff = FMT == 2 ? 1 : 0, voff = FMT == 0 ? 1 : FMT == 1 ? 0 : FMT == 2 ? 3 : 2;
    span_t sp[2];
    int nsp = 1;
    if (luma) {
        sp[0].base = a.p0; sp[0].stride = a.s0; sp[0].rowbytes = GEOM ? (xhi + 1) * ystep : a.p.in_w * ystep; sp[0].b0 = xlo * ystep;
        sp[0].a0 = (xa * ystep) & ~3; sp[0].nw = ((((xb + 1) * ystep + 3) & ~3) - sp[0].a0) >> 2; sp[0].lds = 0;
    } else {
        const uint8_t *cb = FMT == 0 || FMT == 1 ? a.p1 : a.p0;
        const int cs = FMT == 0 || FMT == 1 ? a.s1 : a.s0;
        sp[0].base = cb; sp[0].stride = cs; sp[0].rowbytes = GEOM ? (xhi + 1) * cstep : nin_x * cstep; sp[0].b0 = xlo * cstep;
        sp[0].a0 = (xa * cstep) & ~3; sp[0].nw = ((((xb + 1) * cstep + 3) & ~3) - sp[0].a0) >> 2; sp[0].lds = 0;
        if (FMT == 1) { sp[1] = sp[0]; sp[1].base = a.p2; sp[1].stride = a.s2; sp[1].lds = sp[0].nw * 4; nsp = 2; }
    }
    const int nwt = sp[0].nw + (nsp == 2 ? sp[1].nw : 0);
    if (GEOM && nwt * 4 > a.rawb) return; // (as above: the staged rows were sized for the largest crop)

    // the tile's coefficients into LDS
    for (int i = tid; i < SCALE_TILE_W * nth; i += 256) { const int e = i / nth, k = i - e * nth; cq_h[e * a.tmax_h + k] = qh[(size_t)tcol(e) * nth + k]; }
    for (int i = tid; i < SCALE_TILE_H * ntv; i += 256) { const int o = i / ntv, k = i - o * ntv; cq_v[o * a.tmax_v + k] = qv[(size_t)trow(o) * ntv + k]; }
    if (tid < SCALE_TILE_W) cf_h[tid] = fh[tcol(tid)] + ofx;
    __syncthreads();

    // ---- pass 1: horizontal, SCALE_CHUNK source rows at a time
    const int e = tid & (SCALE_TILE_W - 1);
    const int comp = luma ? 0 : 1 + (e & 1); // 0 Y, 1 U, 2 V
    const int step = luma ? ystep : cstep, off = luma ? yoff : comp == 1 ? uoff : voff;
    const span_t &mys = sp[FMT == 1 && comp == 2 ? 1 : 0];
    const int lbase = mys.lds + off - mys.a0; // + x * step: the sample's byte in a staged row
    const int f0 = cf_h[e];
    const int16_t *myq = cq_h + e * a.tmax_h;
    for (int c0 = 0; c0 < (any ? nh : 0); c0 += SCALE_CHUNK) {
        const int nr = nh - c0 < SCALE_CHUNK ? nh - c0 : SCALE_CHUNK;
        for (int i = tid; i < nr * nwt; i += 256) {
            const int r = i / nwt, wi = i - r * nwt;
            const span_t &s = wi < sp[0].nw ? sp[0] : sp[1];
            const int k = wi < sp[0].nw ? wi : wi - sp[0].nw;
            const uint8_t *rp = s.base + (size_t)(ya + c0 + r) * s.stride;
            const int g = s.a0 + 4 * k;
            unsigned w;
            if (((((uintptr_t)s.base) | (unsigned)s.stride) & 3) == 0 && (!GEOM || g >= s.b0) && g + 4 <= s.rowbytes) w = ldg32(rp + g);
            else { // the row's last bytes, or a misaligned plane: byte by byte, never past the row (GEOM: nor outside the crop rectangle)
                w = 0;
                for (int b = 0; b < 4; b++) if ((!GEOM || g + b >= s.b0) && g + b < s.rowbytes) w |= ldg8(rp + g + b) << (8 * b);
            }
            *(unsigned *)(raw + r * a.rawb + s.lds + 4 * k) = w;
        }
        __syncthreads();
        for (int r = tid >> 6; r < nr; r += 4) {
            const uint8_t *rr = raw + r * a.rawb + lbase;
            int acc = 0;
            for (int k = 0; k < nth; k++) acc += (int)myq[k] * (int)rr[clamp3(f0 + k, xlo, xhi) * step];
            hbuf[(c0 + r) * SCALE_TILE_W + e] = (int16_t)((acc + 128) >> 8);
        }
        __syncthreads();
    }

    // ---- pass 2: vertical; a thread writes 4 bytes of one output row
    const int o = tid >> 4, e4 = (tid & 15) * 4;
    const int orow = ty * SCALE_TILE_H + o;
    const int xbyte = tx * SCALE_TILE_W + e4;
    if (orow >= rows_here || xbyte >= a.W) return; // (W is a multiple of 16: a dword is all inside or all outside)
    const int fo = fv[trow(o)] + ofy;
    const int16_t *vq = cq_v + o * a.tmax_v;
    int acc[4] = {0, 0, 0, 0};
    for (int k = 0; k < (any ? ntv : 0); k++) {
        const int hr = clamp3(fo + k, ylo, yhi) - ya;
        const uint2 hv = *(const uint2 *)(hbuf + hr * SCALE_TILE_W + e4);
        const int q = vq[k];
        acc[0] += q * (int)(int16_t)(hv.x & 0xFFFF); acc[1] += q * ((int)hv.x >> 16);
        acc[2] += q * (int)(int16_t)(hv.y & 0xFFFF); acc[3] += q * ((int)hv.y >> 16);
    }
    unsigned v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { const int t = (acc[i] + (1 << 19)) >> 20; v[i] = (unsigned)(t < 0 ? 0 : t > 255 ? 255 : t); }
    if (GEOM) { // outside the destination rectangle: the border colour (a margin position is judged as the last visible one it repeats)
        const bool rin = any && row_of(o) >= ddy && row_of(o) < ddy + ndy;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int c = col_of(e4 + i);
            if (!rin || c < ddx || c >= ddx + ndx) v[i] = (unsigned)(luma ? a.p.border[0] : a.p.border[1 + (i & 1)]);
        }
    }
    // bytes packed by v_perm: an OR of shifted clipped values is what hipcc turns into gfx950's v_ashr_pk_u8_i32, which leaves bits 31:16
    // set on MI355X (tests/test_abi_cpu.py, test_device_code_avoids_miscompiled_pack_instruction)
    const unsigned w = __builtin_amdgcn_perm(__builtin_amdgcn_perm(v[3], v[2], 0x0c0c0400u), __builtin_amdgcn_perm(v[1], v[0], 0x0c0c0400u), 0x05040100u);
    stg32((luma ? a.dy : a.duv) + (size_t)orow * a.W + xbyte, w);
}

// LDS bytes of one workgroup for `fmt`
static size_t scale_lds_bytes(int fmt, const scale_plan_t *p, int *rawb, int *hmax, int *tmh, int *tmv) {
    const int ystep = fmt >= 2 ? 2 : 1, cstep = fmt == 0 ? 2 : fmt == 1 ? 1 : 4;
    const int rl = p->span[0] * ystep + 8, rc = fmt == 1 ? 2 * (p->span[1] + 8) : p->span[1] * cstep + 8;
    *rawb = ((rl > rc ? rl : rc) + 3) & ~3;
    *hmax = p->hrows[0] > p->hrows[fmt >= 2 ? 2 : 1] ? p->hrows[0] : p->hrows[fmt >= 2 ? 2 : 1];
    const int *tp = p->geom ? p->cap_taps : p->taps; // (with a geometry the room is that of the largest admissible crop)
    *tmh = tp[0] > tp[2] ? tp[0] : tp[2];
    const int tv = tp[fmt >= 2 ? 4 : 3];
    *tmv = tp[1] > tv ? tp[1] : tv;
    return (size_t)scale_coef_room(*tmh, *tmv) * 2 + SCALE_TILE_W * 4 + (size_t)*hmax * SCALE_TILE_W * 2 + (size_t)SCALE_CHUNK * *rawb;
}

int k_launch_scale(int fmt, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2, int s0, int s1, int s2, uint8_t *dy, uint8_t *duv,
                   int W, int H, const scale_plan_t *plan, hipStream_t s, const int *stab) {
    if (fmt < 0 || fmt > 3 || !plan) return -1;
    scale_args a;
    a.p0 = p0; a.p1 = p1; a.p2 = p2; a.s0 = s0; a.s1 = s1; a.s2 = s2; a.dy = dy; a.duv = duv; a.W = W; a.H = H; a.p = *plan; a.stab = stab;
    a.ltiles_x = (W + SCALE_TILE_W - 1) / SCALE_TILE_W;
    a.ltiles = a.ltiles_x * ((H + SCALE_TILE_H - 1) / SCALE_TILE_H);
    const int ctiles = a.ltiles_x * ((H / 2 + SCALE_TILE_H - 1) / SCALE_TILE_H);
    const size_t lds = scale_lds_bytes(fmt, plan, &a.rawb, &a.hmax, &a.tmax_h, &a.tmax_v);
    if (lds > 64 * 1024) return -1; // (s <= 8: at most about 55 KB, for 4:2:2 chroma)
    const dim3 grid(a.ltiles + ctiles), blk(256);
    switch (fmt + (plan->geom && !plan->plain ? 4 : 0)) {
    case 0: hipLaunchKernelGGL((scale_kernel<0, false>), grid, blk, lds, s, a); break;
    case 1: hipLaunchKernelGGL((scale_kernel<1, false>), grid, blk, lds, s, a); break;
    case 2: hipLaunchKernelGGL((scale_kernel<2, false>), grid, blk, lds, s, a); break;
    case 3: hipLaunchKernelGGL((scale_kernel<3, false>), grid, blk, lds, s, a); break;
    case 4: hipLaunchKernelGGL((scale_kernel<0, true>), grid, blk, lds, s, a); break;
    case 5: hipLaunchKernelGGL((scale_kernel<1, true>), grid, blk, lds, s, a); break;
    case 6: hipLaunchKernelGGL((scale_kernel<2, true>), grid, blk, lds, s, a); break;
    default: hipLaunchKernelGGL((scale_kernel<3, true>), grid, blk, lds, s, a); break;
    }
    return 0;
}
