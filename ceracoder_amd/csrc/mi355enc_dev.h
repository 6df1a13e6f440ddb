/* Internal: types shared by the host orchestration (enc_*.cpp), the host entropy coder
 * (h264_host.c) and the HIP kernels (k_*.hip, kernels_common.hpp).  Not part of the C ABI. */
#ifndef MI355ENC_DEV_H
#define MI355ENC_DEV_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 16-byte per-macroblock record (DESIGN.md "HBM layout") */
typedef struct {
    int16_t mvx, mvy;     /* luma motion vector, quarter-sample units               */
    uint8_t mb_type;      /* 0 I16x16, 1 P_L0_16x16, 2 I4x4 (modes in levels[L_LDC..]) */
    uint8_t i16_mode;     /* 0 V 1 H 2 DC 3 Plane                                   */
    uint8_t chroma_mode;  /* 0 DC 1 H 2 V 3 Plane                                   */
    uint8_t qp;
    uint32_t nzmask;      /* b0-15 luma blkIdx, b16-23 chroma AC, b24 luma DC, b25 Cb DC, b26 Cr DC */
    uint32_t cost;
} mb_info_t;

/* 8-byte result of the whole-sample motion search per macroblock (me_kernel / me_select_kernel) */
typedef struct {
    int16_t mvx, mvy;     /* whole-sample vector in quarter-sample units (multiples of 4)      */
    uint16_t sad;         /* its SAD                                                            */
    uint16_t bits;        /* the vector + header bits it was charged (cost = sad + lambda*bits) */
} imv_t;

#define MB_LEVELS 408
#define ISAD_PER_MB 152
#define IDEC_BYTES 32 /* intra decisions per macroblock: u8 modes4[16] (by blkIdx); u8 mode16, cmode, use_i4, 0; u32 cost (luma + chroma), cost_luma, 0 */
/* SAD surface of the motion search: per macroblock 35 rows (dy = -16 .. 18) x 36 columns (dx = -16 .. 19) of uint16; the search
 * range is the 33 x 33 upper-left part, the rest is what the lanes' 5 x 4 candidate tiles compute beyond it */
#define SURF_COLS 36
#define SURF_ROWS 35
#define SURF_U16 (SURF_ROWS * SURF_COLS)
#ifndef MI355_BAND_ROWS
#define MI355_BAND_ROWS 4 /* macroblock rows per band of the band deblocker (the intra band kernel has bands of its own height, k_intra_band_rows()) */
#endif
#ifndef DB_CUT_MIN_MBW
#define DB_CUT_MIN_MBW 60 /* rows at least this long are walked in two parts (A/B, alternating processes: 2160p +6...9 %, 1080p +2 %, 720p +5 %, 640 x 368 -3 %: two workgroups' prologues cost more than twenty columns save) */
#endif
/* Words that one workgroup publishes and others poll (pmb_kernel's row counts, intra_p_kernel's progress words) lie this many words apart: one
 * per 4 KB, i.e. on different memory channels -- dozens of waves polling neighbouring words of one cache line make its channel a hot spot. */
#ifndef MI355_PROG_STRIDE
#define MI355_PROG_STRIDE 1024
#endif
/* Per macroblock of a P picture, the bottom lines an intra macroblock leaves for the row below: eight 8-byte {4 samples, epoch} granules (four of
 * the luma line, four of the interleaved chroma line) */
#define IP_STRIP_BYTES 64
#define ME_ITERS 3          /* Jacobi iterations of the vector selection after the search's own (oracle: ORC_ME_ITERS) */
#define SEL_BONUS 2         /* oracle: ORC_SEL_BONUS */
#define SKIP_MARGIN_BITS 4  /* oracle: ORC_SKIP_MARGIN_BITS */
#define INTRA_GATE(lambda) (768u + 8u * (unsigned)(lambda)) /* oracle: ORC_INTRA_GATE */
#define DROP_MAX 12
#define DROP_SKIP 255
#define L_LUMA 0
#define L_LDC 256
#define L_CDC 272
#define L_CAC 280
#define NZ_LDC (1u << 24)
#define NZ_CBDC (1u << 25)
#define NZ_CRDC (1u << 26)
#define NZ_T8 (1u << 27) /* transform_size_8x8_flag of a P macroblock */
#define PACK_BLOCKS_MAX 27 /* 32-byte blocks a macroblock can contribute to the packed level stream */

/* Device-resident description of the picture being encoded; kernels read it through one
 * pointer so that the per-picture launch sequence can be replayed as a hipGraph. */
typedef struct {
    const uint8_t *src_y, *src_uv; /* source NV12 (visible rows only; rows clamp to vis_h-1) */
    const uint8_t *ref_y, *ref_uv; /* previous reconstructed, deblocked picture (coded size) */
    uint8_t *rec_y, *rec_uv;       /* picture being reconstructed (coded size)               */
    mb_info_t *mbi;
    int16_t *levels;
    uint16_t *isad;                /* intra analysis: 152 u16 per macroblock {i16[4], chroma[4], i4[16][9]}, 0xFFFF = mode unavailable */
    uint8_t *idec;                 /* intra decisions of intra_analyse_kernel, IDEC_BYTES per macroblock */
    uint8_t *dbrec;                /* deblocking: 64 B per macroblock {bS nibbles V, H; alpha/beta/tc0 of 6 edge classes} */
    int32_t src_stride;            /* bytes per source luma row (= chroma row, NV12)          */
    int32_t stride;                /* coded-surface stride = 16*mbw                           */
    int32_t mbw, mbh, vis_h;
    int32_t qp, me_range, lambda;
    int32_t i4x4;                  /* try Intra_4x4 in I pictures */
    int32_t t8;                    /* P macroblocks use the 8x8 transform (High profile stream) */
    int32_t all_intra;             /* every macroblock of the picture is intra (IDR): the deblocker runs all edges without per-edge tests */
    /* P pictures */
    const uint8_t *me_ref_y;       /* what the whole-sample search runs against: the padded SOURCE luma of the last coded picture (coded size, stride `stride`) */
    uint8_t *psrc_out;             /* where this picture's padded source luma goes for the next picture's search (written by me_kernel / copy_luma_kernel) */
    uint16_t *surf;                /* SAD surfaces, SURF_U16 per macroblock */
    imv_t *imv_a, *imv_b, *imv_c;  /* whole-sample vector fields: the search writes imv_a, selection iteration k reads field k % 3 and writes (k + 1) % 3 */
    uint32_t epoch;                /* picture stamp (never 0): tags the progress words of intra_p_kernel so that nothing needs clearing */
    uint32_t drop_sad;             /* rate control's ladder below QP 51: 0 off, else the SAD below which a P macroblock carries no residual / takes the skip vector */
    int32_t iac_drop;              /* I pictures on rate control's ladder: 0 off, else the sum of level magnitudes up to which a macroblock's luma / chroma
                                      residual is not sent */
    int32_t intra_p;               /* P macroblocks may be intra (the analysis of this picture's source is in isad / idec) */
    const int8_t *qp_off;          /* adaptive quantisation and / or a region-of-interest map: one QP offset per macroblock (aq_kernel, roi_compose_kernel), or null: one QP per picture */
    int32_t partitions;            /* P macroblocks may be split (shape in the record's i16_mode: 1 16x8, 2 8x16, 3 8x8; the vectors of partitions 1 .. 3 in the
                                      luma-DC slot of the macroblock's levels); the deblocker then takes boundary strengths per 8x8 quadrant */
    int32_t slice_rows;            /* a new slice every so many macroblock rows (0: one slice); the row above a slice's first row is not available (6.4.8): intra prediction,
                                      mode and vector predictors, nC, QP_Y,PRED */
    int32_t slice_dbf;             /* disable_deblocking_filter_idc of the picture's slices: 0 the deblocking filter runs across slice boundaries, 2 it stops at them
                                      (slice_rows is then a multiple of MI355_BAND_ROWS: a band of the deblocker never spans two slices) */
    int32_t i8;                    /* I pictures: try Intra_8x8 (High profile; intra_mode 0 only: the macroblock above-right has to be complete) */
    /* periodic intra refresh (P pictures of a stream with mi355enc_set_intra_refresh; all three 0 / 0 / -1 otherwise): the macroblocks of columns
       [ir_c0, ir_c1) are intra whatever they cost, and every inter macroblock of a column < ir_c0 predicts from reference luma columns <= ir_clean
       and chroma columns <= ir_clean / 2 only (the clean part: DESIGN.md section 9) */
    int32_t ir_c0, ir_c1;
    int32_t ir_clean;
} frame_ctx_t;

/* ---- the two launches that wait on the device for other kernels, described by value (the decisions: plan_launches(), enc_plan.hpp) */
/* the band deblocker's kernel: an IDR picture (every edge has work) | a P picture | ... whose movers follow the intra macroblock rows' progress words
 * (intra_p_kernel beside it) | ... whose intra macroblock rows lead the launch itself, one workgroup per row */
typedef enum { DB_ALL_INTRA, DB_P, DB_P_FOLLOWS_IP, DB_P_FUSED_IP } db_variant_t;
/* the fused P stage: in stream order | each workgroup waits for the reference's band-done words | ... and counts every macroblock for its row */
typedef enum { PMB_IN_ORDER, PMB_GATED, PMB_GATED_ROWS } pmb_gate_t;
/* The workgroups of one deblocking launch over a whole picture.  counted: two per band (luma, chroma), four where every band is walked as two parts (the cut) --
 * twelve waves at more than 100 VGPRs each, a compute unit's worth, and each counts itself in the `started` word as it is placed.  grid: those behind what leads
 * the launch -- the picture's intra macroblock rows (DB_P_FUSED_IP: one workgroup per row), or the QP_Y chain's workgroup.  The launcher's grid, what a launch
 * adds to the host's `started` total and open()'s wait_room all come from here. */
typedef struct { int counted, grid; } db_wgs_t;
static inline db_wgs_t db_launch_wgs(int mbh, db_variant_t v, int parts, int qpc) {
    db_wgs_t w;
    w.counted = (parts ? 4 : 2) * ((mbh + MI355_BAND_ROWS - 1) / MI355_BAND_ROWS);
    w.grid = w.counted + (v == DB_P_FUSED_IP ? mbh : qpc ? 1 : 0);
    return w;
}
/* One deblocking launch.  The launcher chooses its kernel by `variant` and nothing else; a pointer marked "may be null" switches one wait or one publication off,
 * every other one the variant names must be there. */
typedef struct {
    db_variant_t variant;
    int parts;                    /* P pictures: every band as two workgroups, cut at a column where the filter does nothing (part_cnt) */
    int qpc;                      /* adaptive quantisation: the launch's first workgroup resolves the QP_Y chain and counts the rows in *qpc_word from qpc_base */
    int ib_rows;                  /* rows per intra band (iband_done's granularity; 0: the deblocker's own bands) */
    unsigned *err;                /* the sticky error word */
    void *gran;                   /* uint2: the strips between bands, epoch-tagged granules */
    unsigned *partab;             /* per-edge parameter words (prologue -> movers) */
    unsigned *band_done;          /* may be null: DB_DONE_COPIES x {luma, chroma} per band = the picture's epoch once the band is final in memory */
    unsigned *started;            /* may be null: counts the workgroups placed */
    const unsigned *iband_done;   /* may be null (DB_ALL_INTRA): the picture's intra wavefront is still running; a band waits for its flags */
    const unsigned *row_done;     /* may be null unless DB_P_FUSED_IP: pmb_kernel<GATED, ROWS> of this picture is still running; per macroblock row, it counts up to row_need */
    unsigned row_need;
    unsigned *ip_progress;        /* DB_P_FOLLOWS_IP, DB_P_FUSED_IP: the intra macroblock rows' progress words */
    uint8_t *ip_strips;           /* DB_P_FUSED_IP: ... the bottom lines they publish */
    unsigned *ip_done;            /* DB_P_FUSED_IP: ... and each row counts itself here when its records and levels are in memory */
    unsigned *qpc_word; unsigned qpc_base;
    unsigned *part_cnt;           /* parts: k_deblock_part_bytes() of words, zeroed once -- 2 counters per band ({luma, chroma}: each part adds one when its lines are in
                                     memory; the counts only grow), then 2 uint2 granules {cut column, picture epoch} per band that the band below reads
                                     (cut 0: an idle band, mbw: walked whole) */
} db_launch_t;
/* One launch of the fused P stage */
typedef struct {
    pmb_gate_t gate;
    int refine;
    const unsigned *gate_done; unsigned ref_epoch; /* PMB_GATED*: the reference's band-done words; a wave waits until the bands it reads carry ref_epoch */
    unsigned *row_done;                            /* PMB_GATED_ROWS: one count per macroblock row, + mbw per launch */
    unsigned *err;
} pmb_launch_t;

#ifdef __cplusplus
}
#endif

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include "mask_host.h"
/* launchers (k_*.hip); all asynchronous on `s`.  h_ctx: HOST copy of the context, passed to the kernel by value
 * (kernarg segment); d_ctx: device copy, for the kernels that are replayed from a hipGraph. */
/* (the P-picture launchers cover the whole picture: mbw x h_ctx->mbh macroblocks) */
void k_launch_me(const frame_ctx_t *h_ctx, int mbw, hipStream_t s);
void k_launch_copy_luma(const frame_ctx_t *h_ctx, hipStream_t s); /* I pictures: source luma -> psrc_out (rows beyond the visible picture repeat its last row) */
void k_launch_me_select(const frame_ctx_t *h_ctx, int mbw, const imv_t *in, imv_t *out, const imv_t *prev, int mode, hipStream_t s); /* mode 0: recompute all; 1 / 2: copy where the predictors equal zeros / those of `prev` */
void k_launch_me_select_all(const frame_ctx_t *h_ctx, int mbw, hipStream_t s); /* the ME_ITERS iterations */
void k_launch_intra_p(const frame_ctx_t *h_ctx, int mbw, int mbh, unsigned *d_progress /* one word per macroblock row */, uint8_t *d_strips /* 32 bytes per macroblock */,
                      unsigned *d_err, hipStream_t s);
const imv_t *k_final_imv(const frame_ctx_t *h_ctx); /* where the last selection iteration leaves the field */
void k_launch_subpel(const frame_ctx_t *h_ctx, int mbw, hipStream_t s);
int k_launch_pmb(const frame_ctx_t *h_ctx, int mbw, const pmb_launch_t *l, hipStream_t s); // fused refinement + inter; -1: a word the gate needs is missing (nothing is launched)
void k_launch_inter(const frame_ctx_t *h_ctx, int mbw, hipStream_t s);
void k_launch_intra_analyse(const frame_ctx_t *h_ctx, int mbw, int mbh, int gate_p, hipStream_t s); /* gate_p: P picture -- only macroblocks whose search cost reaches INTRA_GATE */
void k_launch_intra_diag(const frame_ctx_t *d_ctx, int mbw, int mbh, int diag, hipStream_t s);
void k_launch_deblock_diag(const frame_ctx_t *d_ctx, int mbw, int mbh, int diag, hipStream_t s);
int k_deblock_bands16(int mbh);
int k_launch_deblock_bands(const frame_ctx_t *h_ctx, const db_launch_t *l, hipStream_t s); /* all the picture's bands in one launch; -1: a word the variant needs is missing (nothing is launched) */
size_t k_deblock_part_bytes(int mbh); /* db_launch_t::part_cnt: 6 words per band (0: this build walks every band whole) */
int k_intra_band_rows(void);
size_t k_deblock_partab_bytes(int mbw, int mbh); // scratch of the band kernel: one parameter word per (edge, segment) of every macroblock
size_t k_deblock_gran_bytes(int mbw, int mbh);
void k_launch_wait_started(const unsigned *d_started, unsigned count, unsigned *d_err, hipStream_t s);
size_t k_deblock_done_bytes(void); /* band-done words of one picture (all copies) */ // the strips between bands: 8-byte {samples, epoch} granules
void k_launch_pad(uint8_t *y, uint8_t *uv, int stride, int vis_w, int vis_h, int W, int H, hipStream_t s);
int k_intra_diags(int mbw, int mbh);
int k_intra_bands(int mbh);
void k_launch_intra_band(const frame_ctx_t *h_ctx, int mbh, uint2 *d_gran, unsigned *d_err, unsigned *d_band_done, hipStream_t s);
/* I pictures, dataflow at 4x4-block granularity: one workgroup per macroblock row; d_gran: 8 granules per macroblock; d_row_done (may be null): one tagged word per row */
void k_launch_intra_rows(const frame_ctx_t *h_ctx, int mbh, uint2 *d_gran, unsigned *d_err, unsigned *d_row_done, hipStream_t s);
int k_launch_csc(int fmt, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2, int s0, int s1, int s2, uint8_t *dy, uint8_t *duv,
                 int vw, int vh, int W, int H, hipStream_t s);
/* the formats csc_kernel does not take (k_csc.hip; the rule: DESIGN.md section 11): fmt MI355ENC_FMT_Y42B .. MI355ENC_FMT_GRAY8 except YV12 (k_launch_csc with
 * the chroma planes exchanged); coef: the ten words of mi355enc_csc_coefficients, RGB formats only.  -1: not one of them */
int k_launch_csc2(int fmt, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2, int s0, int s1, int s2, uint8_t *dy, uint8_t *duv,
                  int vw, int vh, int W, int H, const int *coef, hipStream_t s);
/* HDR input tone-mapped to SDR NV12 (k_hdr.hip; the model and the rule: DESIGN.md section 22): fmt MI355ENC_FMT_P010, _I420_10 or _V210, planes and strides
 * as k_launch_csc2's, d_tables the words of mi355enc_hdr_tables on the device, hlg whether their transfer is 18 (the kernel with the OOTF step) and not 16.  -1: another format, or arguments outside what the kernel's addressing holds for */
int k_launch_hdr(int fmt, int hlg, const uint8_t *const planes[3], const int strides[3], uint8_t *dy, uint8_t *duv, int vw, int vh, int W, int H, const int *d_tables, hipStream_t s);
/* the colour step (k_csc.hip; the rule: DESIGN.md section 20), in place on NV12 surfaces of W x H at stride W: the samples inside rect (x0, x1, y0, y1; even)
 * go from one (range, matrix) to another with the nine words of mi355enc_yuv_coefficients; everything outside keeps its bytes.  -1: arguments outside that */
int k_launch_yuv_convert(uint8_t *y, uint8_t *uv, int W, int H, const int rect[4], const int *coef, hipStream_t s);
/* picture controls (k_adjust.hip; the rule: DESIGN.md section 23), pointwise form, in place on NV12 surfaces of W x H at stride W: the samples inside rect (as
 * k_launch_yuv_convert's) go through the luma table (256 bytes; null: the luma plane is not touched) and the chroma rotation {cu, su} (null: the chroma plane
 * is not touched); everything outside keeps its bytes.  -1: arguments outside that, or both null */
int k_launch_adjust(uint8_t *y, uint8_t *uv, int W, int H, const int rect[4], const uint8_t *luma, const int *chroma, hipStream_t s);
/* ... stencil form, luma only, from y into another plane `out` of the same layout (W, H multiples of 16; vw x vh the visible size, less than 16 short of them):
 * table (null: neutral, none), then the 3 x 3 unsharp mask with amount (-16 .. 64, not 0) and threshold thr (0 .. 32), neighbours clamped to the visible part of rect, a margin sample
 * the result of its clamped visible position.  Writes rect's samples of `out` and at most two bytes beside its left and right edge.  -1: arguments outside that */
int k_launch_adjust_sharpen(const uint8_t *y, uint8_t *out, int W, int H, int vw, int vh, const int rect[4], const uint8_t *luma, int amount, int thr, hipStream_t s);
/* temporal noise reduction (k_denoise.hip; the rule: DESIGN.md section 24), in place on NV12 surfaces of W x H (multiples of 16) at stride W and on their
 * histories hy, huv (uint16 per sample, the same layout, 16-byte aligned; huv null with cmode 0); vw x vh the visible size (even, less than 16 short of W x H).
 * lmode 1: the luma is filtered, 0: it primes / follows (H' = 16 c, the luma surface is not written); cmode 2: the chroma is filtered, 1: it primes, 0: neither
 * read nor written.  tabs: 768 bytes -- B, the luma's P, the chroma's P (mi355enc_denoise_tables) --, needed when anything is filtered.  -1: arguments outside that */
int k_launch_denoise(uint8_t *y, uint8_t *uv, uint16_t *hy, uint16_t *huv, int W, int H, int vw, int vh, int lmode, int cmode, const uint8_t *tabs, hipStream_t s);
/* ... with motion compensation.  The search: per aligned 8 x 8 luma block with a visible sample the vector into the history hy within
 * `range` (1 .. 16) whose key is smallest, lambda (0 .. 128) the penalty per sample of vector length; vec: (W / 8) (H / 8) words in raster order -- dx in byte 0,
 * dy in byte 1 (int8), the vector's cost M in the high half; zero for a block without a visible sample.  The compensated filter: k_launch_denoise with the
 * histories read (hy, huv) and written (ny, nuv: other buffers) apart, the history read at the block's vector; something is filtered (lmode 1 or cmode 2). */
int k_launch_denoise_search(const uint8_t *y, const uint16_t *hy, unsigned *vec, int W, int H, int vw, int vh, int range, int lambda, hipStream_t s);
int k_launch_denoise_mc(uint8_t *y, uint8_t *uv, const uint16_t *hy, const uint16_t *huv, uint16_t *ny, uint16_t *nuv, const unsigned *vec, int W, int H, int vw, int vh,
                        int lmode, int cmode, const uint8_t *tabs, hipStream_t s);
/* Downscaling of the input picture to the coded size (k_scale.hip; the rule: DESIGN.md section 10).  Tables built on the host
 * (enc_scale.cpp), five of them: 0 luma horizontal, 1 luma vertical, 2 chroma horizontal, 3 chroma vertical from 4:2:0 input, 4 chroma
 * vertical from 4:2:2 input.  Entry i of table t: first[t][i] (first source index, not clamped) and q[t][i * taps[t] + k]. */
#define SCALE_TABLES 5
#define SCALE_TILE_W 64 /* output bytes per tile row: 64 luma samples, or 32 chroma pairs */
#define SCALE_TILE_H 16 /* output rows per tile */
#define SCALE_CHUNK 8   /* source rows staged in LDS at a time by the horizontal pass */
typedef struct {
    int in_w, in_h, out_w, out_h;
    const int *first[SCALE_TABLES];
    const int16_t *q[SCALE_TABLES];
    int taps[SCALE_TABLES];
    int hrows[3]; /* most source rows one tile's vertical pass reads: luma, chroma from 4:2:0, chroma from 4:2:2 */
    int span[2];  /* most source samples one tile's horizontal pass reads per row: luma, chroma (per component) */
    /* the input geometry; geom 0: a plain downscale of the whole picture over the whole target, and everything below is unused */
    int geom, plain;                        /* plain: the geometry is that plain downscale after all (the tables are section 10's): the plain instance runs */
    int lo[SCALE_TABLES], hi[SCALE_TABLES]; /* source indices are clamped into [lo, hi] per table: the crop rectangle (chroma tables in chroma samples / rows) */
    int dx, dy, dw, dh;                     /* destination rectangle inside out_w x out_h, luma samples; everything else is border */
    int border[3];                          /* Y, Cb, Cr */
    int cap_taps[SCALE_TABLES];             /* LDS room for coefficients, fixed when the geometry was set (taps[] changes with the crop) */
} scale_plan_t;
int k_launch_scale(int fmt, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2, int s0, int s1, int s2, uint8_t *dy, uint8_t *duv,
                   int W, int H, const scale_plan_t *plan, hipStream_t s, const int *stab = nullptr); /* stab: with a geometry, {ox, oy} on the device (section 26); null: none */
/* Electronic image stabilisation (k_stab.hip; the rule: DESIGN.md section 26, stab_host.h).  The projection launch: the luma samples of a w x h picture (first
 * one at `luma`, `step` = 1 or 2 bytes apart, any address and stride) -> sums: C_0 .. C_3 (w words each), then R_0 .. R_3 (h each); added with atomics, so the
 * 4 (w + h) words are cleared on the same stream in front of it.  The match launch: votes of the eight projections `cur` against `prev` (range 1 .. 32,
 * w, h >= 4 range), medians and the trajectory step under bounds {lo_x, hi_x, lo_y, hi_y}; state {Sx, Sy} is read and written, rec gets the record's eight
 * words (mx, my, votes_x, votes_y, ox, oy, Sx, Sy).  prime: no vote is taken, state and record are zero.  -1: arguments outside that */
/* Lens, roll and keystone correction (k_warp.hip; the rule: DESIGN.md section 27, warp_host.h): the coded NV12 surfaces (stride W, visible w x h, even) resampled
 * through the mesh (warp_nodes(w) x warp_nodes(h) valid nodes, on the device) into another pair of surfaces, margin up to W x H included: every byte of both
 * is written.  kind 0 bilinear, 1 bicubic; fill: Y, Cb, Cr of the samples outside; staging 0: no workgroup stages its source window in LDS (measurements).  -1: arguments outside that */
int k_launch_warp(const uint8_t *sy, const uint8_t *suv, uint8_t *dy, uint8_t *duv, int w, int h, int W, int H, const int32_t *mesh, int kind, const uint8_t fill[3], hipStream_t s, int staging = 1);
int k_launch_stab_project(const uint8_t *luma, int stride, int step, int w, int h, unsigned *sums, hipStream_t s);
int k_launch_stab_match(const unsigned *prev, const unsigned *cur, int w, int h, int range, int leak, int prime, const int bounds[4], int *state, int *rec, hipStream_t s);
/* Automatic levels and white balance (k_autolevel.hip; the rule: DESIGN.md section 28, autolevel_host.h), three launches on one stream.  measure: the visible
 * samples of rect on NV12 surfaces of W x H at stride W (visible vw x vh) -> one slab of AL_SLAB_WORDS words per workgroup (plain stores: nothing to clear);
 * returns their number (1 .. AL_SLABS_MAX).  decide: the slabs, NC visible chroma samples and the setting's seven fields -> the state (4 words, read and
 * written; prime: only written), the record and the table (AL_SLOT_WORDS words at rec).  apply: the table and offsets at rec onto the samples inside rect, in
 * place; luma / chroma: the setting's levels / balance are above 0.  -1: arguments outside that */
int k_launch_autolevel_measure(const uint8_t *y, const uint8_t *uv, int W, int H, const int rect[4], int vw, int vh, int full_range, int reach, unsigned *slabs, hipStream_t s);
int k_launch_autolevel_decide(const unsigned *slabs, int nslabs, unsigned NC, const int set[7], int full_range, int prime, int *state, int *rec, hipStream_t s);
int k_launch_autolevel_apply(uint8_t *y, uint8_t *uv, int W, int H, const int rect[4], int luma, int chroma, const int *rec, hipStream_t s);
/* The spatial noise filter and its noise estimate (k_dspatial.hip; the rule: DESIGN.md section 30, dspatial_host.h).  filter: one plane (chroma 0: luma, 1: the
 * interleaved chroma plane) of NV12 surfaces of W x H (visible vw x vh) into another plane, inside rect; its weights R_s by value (weight, 256 bytes) or, with
 * weight null, the strength from the device word rec and R_s from the device's 33 tables.  measure: the candidate blocks of the luma plane -> one slab of
 * DS_SLAB_WORDS words per workgroup (plain stores: nothing to clear); returns their number (1 .. DS_SLABS_MAX).  decide: the slabs, NC candidates and the
 * automatic setting's five fields -> the state (one word, read and written; prime: only written) and the record (DS_REC_WORDS words).  -1: arguments outside that */
int k_launch_dspatial_filter(const uint8_t *src, uint8_t *out, int W, int H, int vw, int vh, const int rect[4], int chroma, const uint8_t *weight, const int *rec, const uint8_t *tabs, hipStream_t s);
int k_launch_dspatial_measure(const uint8_t *y, int W, int H, const int rect[4], int vw, int vh, int full_range, unsigned *slabs, hipStream_t s);
int k_launch_dspatial_decide(const unsigned *slabs, int nslabs, unsigned NC, const int set[5], int prime, int *state, int *rec, hipStream_t s);
/* A 3D colour LUT (k_lut3d.hip; the rule: DESIGN.md section 29, lut3d_host.h) on NV12 surfaces of W x H at stride W inside rect, in place: nodes N^3 checked
 * words on the device, strength 1 .. 256, coef mi355enc_lut3d_coefficients', form 0 direct (nodes from global memory) or 1 staged (the table in LDS: N up to
 * LUT3D_STAGED_FIT, nodes 16-byte aligned).  -1: arguments outside that, and nothing is launched */
int k_launch_lut3d(uint8_t *y, uint8_t *uv, int W, int H, int vw, int vh, const int rect[4], const uint32_t *nodes, int N, int strength, const int32_t coef[19], int form, hipStream_t s);
void k_launch_pack(const mb_info_t *d_mbi, const int16_t *d_levels, int nmb, int mbw, unsigned *d_off, mb_info_t *h_mbi, int16_t *h_packed,
                   unsigned *h_hdr, const unsigned *d_err, hipStream_t s);
int k_deblock_diags(int mbw, int mbh);
/* adaptive quantisation: per-macroblock QP offsets from the source's luma variance (oracle: orc_aq_offsets), and -- once a picture's records are
 * final -- the QP_Y of macroblocks that send no mb_qp_delta (7.4.5: that of the macroblock before them), which the deblocker reads (orc_qp_chain) */
void k_launch_aq(const frame_ctx_t *h_ctx, int8_t *d_off, hipStream_t s);
void k_launch_qp_chain(mb_info_t *d_mbi, int nmb, int slice_qp, int slice_mbs, hipStream_t s);
/* region-of-interest quantisation (k_roi.hip; the rule: DESIGN.md section 31, roi_host.h): d_off[m] = clamp(aq + t[m], -12, 12) for the nmb macroblocks of a
 * picture -- aq what d_off holds (have_aq: aq_kernel ran in front on the same stream) or 0; t: nmb bytes the device can read (pinned host or device memory),
 * 4-byte aligned like d_off */
void k_launch_roi_compose(const int8_t *t, int8_t *d_off, int nmb, int have_aq, hipStream_t s);
/* Privacy masks (k_mask.hip; the rule: DESIGN.md section 32, mask_host.h) on NV12 surfaces of W x H at stride W whose visible part is vw x vh, in place: tab
 * mask_resolve's for that visible size; res a surface of the same layout, pa and pb plane_bytes (at least W H 3 / 2) each, 16-byte aligned, all three the
 * caller's and used by no other stream; parts: 1 the pixelate launch, 2 the blur launches, 4 the commit launch (which is also the fill) -- a picture is 7.
 * *launches (may be null): how many were enqueued.  -1: arguments outside that, and nothing is launched */
int k_launch_mask(uint8_t *y, uint8_t *uv, int W, int H, int vw, int vh, const mask_tab_t *tab, uint8_t *res, uint8_t *pa, uint8_t *pb, size_t plane_bytes, int parts, int *launches, hipStream_t s);
/* Quality metrics of one picture (k_quality.hip; the rule: DESIGN.md section 12): NV12 source against NV12 reconstruction over the visible width x height.
 * d_acc: QUALITY_ACC_WORDS 64-bit words on the device, zero before the first launch (every launch leaves them zero again): QUALITY_SHARDS sets of five
 * accumulators, QUALITY_SHARD_STRIDE words (4 KB: another memory channel) apart, and the ticket; out: five words (a block of QUALITY_WORDS) -- SSE of Y, Cb, Cr,
 * the sum of the windows' q, the number of windows -- written by the launch's last workgroup (device or pinned host memory, 8-byte aligned). */
#define QUALITY_WORDS 8
#define QUALITY_SHARDS 32
#define QUALITY_SHARD_STRIDE 512
#define QUALITY_TICKET_WORD 8
#define QUALITY_ACC_WORDS (QUALITY_SHARDS * QUALITY_SHARD_STRIDE)
/* Text overlay (k_overlay.hip; the rule: DESIGN.md section 13).  Everything the launch needs, by value: the surface, the visible size, the box
 * (bx, by: origin, even, >= 0; bw x bh: its unclipped size), the quads the grid covers ([gx0, gx1) x [gy0, gy1), even: the visible part of the
 * box; where it reaches the last visible column / row, the owners of the last quads write the margin up to the coded size W x H as well), the resolved style and the text:
 * nlines lines, line i = text[(i ? line_end[i - 1] + 1 : 0) .. line_end[i]), the longest of maxlen bytes. */
typedef struct {
    uint8_t *y, *uv;
    int32_t stride, vw, vh, W, H;
    int32_t bx, by, bw, bh;
    int32_t gx0, gy0, gx1, gy1;
    int32_t scale, halign, shaded, nlines, maxlen;
    uint8_t text[256];
    uint8_t line_end[256];
} overlay_args_t;
void k_launch_overlay(const overlay_args_t *a, hipStream_t s);
/* Image layers (k_image.hip; the rule: DESIGN.md section 17).  prepare: n pixels of 4 bytes in byte order fmt (MI355ENC_FMT_BGRX .. MI355ENC_FMT_XBGR, X = A) at
 * `pix` become one word {Yi, Cbi << 8, Cri << 16, A << 24} each, in place; coef: the ten words of mi355enc_csc_coefficients.  blend: one layer -- iw x ih
 * prepared words, rows adjacent, top-left at (x, y) of the visible picture vw x vh, opacity 0 .. 256 -- into NV12 surfaces of stride `stride` and coded size
 * W x H.  The grid covers the quads [gx0, gx1) x [gy0, gy1) (even, inside the visible picture): the visible intersection from an even origin; where it reaches the
 * last visible column / row, the owners of the last quads write the margin up to W / H as well. */
typedef struct {
    uint8_t *y, *uv;
    const uint32_t *img;
    int32_t stride, vw, vh, W, H;
    int32_t iw, ih, x, y0, opacity;
    int32_t gx0, gy0, gx1, gy1;
} image_args_t;
int k_launch_image_prepare(uint32_t *pix, size_t n, int fmt, const int *coef, hipStream_t s); /* -1: not one of the four orders */
bool k_image_grid(image_args_t *a);  /* fills gx0 .. gy1 from the place and the sizes; false: nothing of the image is visible (no launch) */
void k_launch_image_blend(const image_args_t *a, hipStream_t s);
/* MJPEG input (k_jpeg.hip; the rule: DESIGN.md section 14): a picture of vw x vh (even) with luma sampling hs x vs and `comps` components, coefficient blocks and
 * quantisation tables on the device as mi355enc_jpeg_entropy_decode lays them out, into NV12 surfaces of stride W and coded size W x H (the margin repeats the last
 * visible row, column and chroma pair).  d_planar: scratch of 3 * ((vw + 15) & ~15) * vh bytes, read and written for 4:4:4 only.  -1: not a sampling it takes. */
int k_launch_jpeg(const int16_t *d_coef, const uint16_t *d_qt, int hs, int vs, int comps, int vw, int vh, uint8_t *dy, uint8_t *duv, int W, int H,
                  uint8_t *d_planar, hipStream_t s);
/* Orientation of the input picture (k_orient.hip; the rule: DESIGN.md section 15): NV12 planes of the pre-orientation visible size in_w x in_h (even), at any
 * address and stride, by method 1 .. 7 (MI355ENC_ORIENT_*) into NV12 surfaces of stride W and coded size W x H of the oriented picture, margin included.
 * -1: not such a method, or sizes that do not fit each other. */
int k_launch_orient(int method, const uint8_t *sy, int ssy, const uint8_t *suv, int ssuv, int in_w, int in_h, uint8_t *dy, uint8_t *duv, int W, int H, hipStream_t s);
/* JPEG stills (k_snapshot.hip; the rule: DESIGN.md section 18): NV12 planes of w x h (even) at any address and stride, reduced by 2^log2s, as the quantised
 * levels of a 4:2:0 still: 64 int16 per block in jpeg_host_layout's layout (16-byte aligned) and one hint byte per block (the zigzag index of its last non-zero
 * level), device or pinned host memory; d_tab: the quality's snapshot_tab_t on the device.  -1: sizes or a reduction it does not take. */
int k_launch_snapshot(const uint8_t *sy, int ys, const uint8_t *suv, int uvs, int w, int h, int log2s, const void *d_tab, int16_t *levels, uint8_t *hint, hipStream_t s);
/* Frame-rate conversion (k_rate.hip; the rule: DESIGN.md section 21): out = (a (256 - w256) + b w256 + 128) >> 8 per byte over NV12 surfaces of W x H at stride W
 * (multiples of 16, every pointer 16-byte aligned), margins included; k_y / k_uv (both or neither): b is stored there as well.  Works in place index for index
 * (a == k, b == out).  -1: arguments outside that. */
int k_launch_rate_mix(const uint8_t *a_y, const uint8_t *a_uv, const uint8_t *b_y, const uint8_t *b_uv, uint8_t *o_y, uint8_t *o_uv, uint8_t *k_y, uint8_t *k_uv,
                      int W, int H, int w256, hipStream_t s);
void k_launch_quality(const uint8_t *src_y, const uint8_t *src_uv, int src_stride, const uint8_t *rec_y, const uint8_t *rec_uv, int rec_stride,
                      int width, int height, unsigned long long *d_acc, unsigned long long *out, hipStream_t s);
#endif
#endif
