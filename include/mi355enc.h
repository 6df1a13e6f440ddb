/*
 * include/mi355enc.h -- C ABI of the MI355X-native H.264 encoder (libmi355enc.so).
 *
 * This is the drop-in boundary under ceracoder's GStreamer graph.  It replaces what the
 * reference obtains from the third-party `x264enc` element named in its pipeline text
 * (/root/reference/pipeline/generic/x264_superfast_camlink:5,
 *  /root/reference/pipeline/generic/x264_superfast_v4l_mjpeg_720p30:6,
 *  /root/reference/bindings/typescript/src/pipeline/generic-builder.ts:50-55),
 * instantiated by gst_parse_launch at /root/reference/src/io/pipeline_loader.c:59.
 * The reference has no FFI of its own for this path: the binding a maintainer adds is the
 * GStreamer element in ceracoder_amd/csrc/gstmi355h264enc.c, which
 * calls exactly these entry points.
 *
 * Conventions follow the reference's C modules (int return, 0 = ok, negative = error,
 * message on stderr; cf. /root/reference/src/gst/encoder_control.h:42-50,
 * /root/reference/src/net/srt_client.c:40-55): no exceptions, no abort(), plain pointers
 * and sizes only.  There is NO CPU fallback: without a usable HIP device
 * mi355enc_open() fails with MI355ENC_ERR_NO_DEVICE.
 */
#ifndef MI355ENC_H
#define MI355ENC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355ENC_ABI_VERSION 4

enum {
    MI355ENC_OK = 0,
    MI355ENC_ERR_ARG = -1,        /* bad argument / unsupported geometry            */
    MI355ENC_ERR_NO_DEVICE = -2,  /* no HIP device, or device-id out of range       */
    MI355ENC_ERR_HIP = -3,        /* a HIP runtime call failed (text on stderr)     */
    MI355ENC_ERR_NOMEM = -4,
    MI355ENC_ERR_OVERFLOW = -5,   /* caller's output buffer too small               */
    MI355ENC_ERR_STATE = -6,      /* call order violated (e.g. collect with nothing pending) */
};

typedef struct mi355enc mi355enc_t; /* opaque; owns all device memory, streams, graphs */

typedef struct {
    int width, height;        /* visible picture, even, 16..8192                          */
    int fps_num, fps_den;
    int gop;                  /* IDR period; x264enc `key-int-max` (pipelines pass 60)     */
    int me_range;             /* full-search radius in integer pels, 1..16                 */
    uint32_t bitrate_bps;     /* initial target; what encoder_control.c:53 later rewrites  */
    int device_id;            /* HIP device ordinal (one stream per GPU)        */
    int fixed_qp;             /* >= 0: constant QP, rate control off (tests, bench); -1: CBR */
    int qp_min, qp_max;       /* rate-control clamp; 0,0 -> defaults 10..51                */
    int pipeline_depth;       /* 0: encode() returns this frame's AU; 1: host entropy coding
                                 of frame n overlaps device work of frame n+1; 2: ... and the
                                 device never waits for the host (three pictures in flight; rate
                                 control sees a picture's size two pictures later, scene-cut
                                 recovery lands one picture later than at depth 0/1)       */
    int profile_events;       /* k > 0: bracket the kernel stages of every k-th picture (and every IDR) with HIP events
                                 for the stage statistics; an event record costs ~5 us of queue time, so k = 1 slows
                                 the stream by several per cent */
    int use_graphs;           /* 1: replay the per-picture launch sequence as a hipGraph  */
    int keep_prefilter;       /* 1: keep a copy of the picture before deblocking (tests)  */
    int transform8x8;         /* 0 (default): Constrained Baseline.  1: High-profile stream, every coded inter macroblock of a P picture uses the 8x8
                                 transform.  2: High-profile stream (the same SPS and PPS as 1), every coded inter macroblock chooses between the
                                 4x4 and the 8x8 transform: 8x8 iff (SA8D + 2) >> 2 < SATD >> 1 of its luma prediction residual, both unhalved
                                 Hadamard sums (x264's transform analysis for its fast presets).  I pictures, intra macroblocks of P
                                 pictures and i8x8 behave as with 1; mi355enc_stage_inter refuses 2 (MI355ENC_ERR_ARG) */
    int i4x4;                 /* 1 (default): try Intra_4x4 besides Intra_16x16 in I pictures */
    int subpel;               /* 1 (default): half- then quarter-sample refinement after the integer search */
    int deblock_mode;         /* 0: persistent band kernel (x+y order, three waves per macroblock row; boundary strengths in its prologue);
                                 1: one launch per x+2y wavefront (plain form, kept as a cross-check) */
    int intra_in_p;           /* 1 (default): macroblocks of P pictures may be coded intra (Intra_16x16) for uncovered regions and partial scene
                                 changes: decided in the fused P stage from the open-loop intra analysis, reconstructed by a short dependent pass
                                 after it.  2: Intra_4x4 as well (with i4x4) -- the part of x264 superfast's partition search that survives,
                                 `partitions i8x8,i4x4`; rate-distortion neutral on the synthetic clips (-0.2 % / +0.4 % BD-rate), ten dependent
                                 sub-steps per such macroblock.  0: P pictures hold inter macroblocks only */
    int cavlc_threads;        /* host threads that code the slice (ranges of macroblock rows, concatenated bit-exactly into the
                                 same single slice); 1: the calling thread only; 0 (default, like x264enc's threads=0): chosen
                                 from the machine -- a quarter of the online CPUs, between 1 and 8 (1 for pictures under
                                 1000 macroblocks, where waking workers costs more than it saves); mi355enc_stats_t reports it */
    int intra_mode;           /* 0 (default): one persistent launch, a workgroup per macroblock row, macroblocks overlapping at 4x4-block
                                 granularity (dataflow); 1: one launch per anti-diagonal replayed as a hipGraph (plain form, kept as a
                                 cross-check); 2: the lock-step band kernel of rounds 1-2 (x + y order, one barrier per step; kept for A/B) */
    int vbv_ms;               /* rate control's buffer model in ms of stream at the setpoint (default 600: x264enc's vbv-buf-capacity): an IDR
                                 picture is planned at most half of it, and P pictures are all-skip while the bucket is nearly full */
    int scenecut;             /* 1 (default, like x264's scenecut): when the summed motion cost of a P picture exceeds three times
                                 the mean of the P pictures since the last IDR (at least two of them), the picture two
                                 positions later is coded as IDR -- recovery within two pictures instead of a GOP, with no wait
                                 on the device (the sum arrives with the picture's hand-over).  0: IDR only every `gop`
                                 pictures or on request */
    int exclusive_device;     /* 0 (default): other processes may use the same GPU.  1: this encoder has the GPU to itself (one
                                 stream per GPU, BASELINE configs[4]; what bench.py sets): a P picture's fused stage is launched
                                 beside the deblocking of the picture before it and its workgroups wait ON the device for the
                                 bands they read -- a chip full of waiting workgroups.  With another process on the same GPU
                                 such launches can keep each other's kernels off the chip (seen: one of two processes ran into
                                 the bound of its wait), so it is opt-in.  Same stream either way.  No effect on pictures whose
                                 deblocking launch would by itself take more than three quarters of the compute units (from about
                                 4000 lines up): there the waiting workgroups would keep the kernel they wait for off the chip */
    int aq_mode;              /* 0 (default): one QP per picture.  1: adaptive quantisation -- a QP offset of -4 .. +4 per macroblock from the luma
                                 variance of its source samples (flat areas finer, busy texture coarser), coded with mb_qp_delta.  The QP_Y of
                                 macroblocks that send no mb_qp_delta is that of the macroblock before them (7.4.5), which the deblocker reads: a
                                 chain over the whole picture, resolved row by row by the first workgroup of the deblocking launch behind the same
                                 progress its bands wait for (r03; about 2 % fewer frames/s).  With intra_in_p = 2 the
                                 kernels of a picture run in stream order */
    int single_stream;        /* 0 (default): four HIP streams per encoder (front / main / intra / hand-over), so that a picture's independent stages and
                                 consecutive pictures overlap.  1: everything on ONE stream, in order -- for many encoders on one GPU (several in a
                                 process, or many processes): the GPU has a handful of hardware queues, and 8 encoders x 4 streams made the driver
                                 time-slice them (8 streams in one process: 409 frames/s in ALL; with single_stream each encoder keeps one queue busy) */
    int intra_slices;         /* slices per I picture, each its own NAL unit (x264enc: the `slices` option of libx264).  0 (default): about 17
                                 macroblock rows per slice, at most 8 slices (1080p: 4, 720p: 2, below 34 rows: 1).  Intra prediction cannot cross a
                                 slice boundary (6.4.8), so the slices of a picture are independent chains for the intra wavefront: an IDR picture's
                                 reconstruction takes about 1/n of the time (the deblocking filter still runs across the boundaries); the cost is the
                                 prediction lost along n - 1 rows, +0.5 % on the IDR pictures' bytes at 1080p with 4.  P pictures are one slice */
    int partitions;           /* 0 (default): every inter macroblock is one 16x16 partition (what x264's superfast preset searches).  1: P macroblocks may be
                                 split into 16x8, 8x16 or 8x8 partitions (x264enc: analyse / `partitions`): every partition chooses among the vectors the
                                 macroblock's sub-sample refinement visits; rate-distortion neutral on the test clips, about 3 % fewer frames/s.  Not with
                                 transform8x8, deblock_mode 1 or adaptive quantisation's in-order cases */
    int profile_overlap;      /* with profile_events: 0 (default) a sampled picture runs its stages strictly in order, so that every timer is one kernel
                                 alone (the picture costs the stream about two periods).  1: sampled P pictures keep the free-running schedule -- the
                                 event pairs sit on the streams the kernels are launched on, and a launch that waits on the device for another kernel's
                                 rows is timed with that wait, as a kernel trace would show it.  IDR pictures are always sampled in order */
    int i8x8;                 /* 0 (default): off.  1: with transform8x8, the macroblocks of I pictures may be Intra_8x8 (x264enc: dct8x8 brings the transform
                                 and the intra type together) at picture quantisers up to 37; needs intra_mode 0 (the macroblock above-right has to be
                                 complete), otherwise ignored.  Measured at 1080p: IDR pictures 1.4 - 3.9 % smaller at QP 22 - 34 at equal PSNR; an
                                 Intra_8x8 macroblock is four dependent 8x8 blocks on the intra wavefront (its neighbour to the right starts half a
                                 macroblock behind), so a stream with key-int 60 runs 1 - 3 % slower, an all-intra one by a third */
    int slices;               /* slices per P picture, each its own NAL unit (r04; what x264enc's threads do to a picture behind
                                 /root/reference/pipeline/generic/x264_superfast_camlink:5).  0 (default): as many as an I picture gets by default -- about 17
                                 macroblock rows each (1080p: 4, 720p: 2, 2160p: 7, below 34 rows: 1).  1: one slice.  n > 1: n slices of ceil(rows / n) rows.
                                 Motion-vector prediction, the P_Skip inference, intra prediction, nC and QP_Y,PRED stop at a slice's first row (6.4.8): on
                                 panning content the rows below a seam cannot be P_Skip (the inferred vector is zero there) -- Bjontegaard rate +2.4 % (S2 clip)
                                 / +3.9 % (panning S4) at 1080p with 5 slices, nothing on still content (profiles/r04_rd_slices_*.txt) */
    int slice_deblock;        /* 1 (default): the deblocking filter stops at slice boundaries (disable_deblocking_filter_idc 2, in the slices of I and P
                                 pictures alike; slice heights are then multiples of four macroblock rows, the height of the deblocker's bands): every slice is
                                 an independent dependency chain for the deblocking launch -- the launch that sets the picture period -- whose length falls from
                                 columns + rows - 1 steps to columns + rows per slice - 1 (1080p: the launch alone 146 -> 85 us; +17...20 % frames/s; the seam rows
                                 lose 0.0 - 0.2 dB at QP 36 - 42, nothing measurable below).  0: the filter runs across slice boundaries (idc 0) */
} mi355enc_cfg_t;

typedef struct {
    uint64_t frames, idr_frames, bytes;   /* pictures collected, IDR pictures among them, bytes produced */
    uint32_t last_qp, last_bytes, target_bps;
    /* accumulated device time per stage in ms and sample counts (profile_events > 0) */
    double ms_me, ms_inter, ms_intra, ms_deblock, ms_total_gpu;
    double ms_subpel;
    uint64_t n_me, n_inter, n_intra, n_deblock;
    double ms_entropy;        /* host CAVLC wall time */
    double ms_wait;           /* host time blocked on the device */
    uint64_t n_total_gpu;     /* pictures sampled into ms_total_gpu */
    double ms_deblock_idr;    /* the part of ms_deblock / n_deblock that came from IDR pictures */
    uint64_t n_deblock_idr;
    uint32_t cavlc_threads;   /* host threads in use for entropy coding (cfg.cavlc_threads resolved) */
    uint32_t last_drop;       /* drop level of the last collected picture (0: none; 1 .. 12: the ladder below QP 51; 255: all-skip picture) */
    double ms_select;         /* P pictures: the ME_ITERS vector-selection iterations (not part of ms_me), n_me samples */
    double ms_analyse_p;      /* P pictures: intra analysis of the gated macroblocks, n_inter samples (also contained in ms_inter) */
    double ms_intra_p;        /* P pictures: reconstruction of the intra macroblocks, n_inter samples (also contained in ms_inter) */
    uint64_t skip_pictures;   /* pictures coded as one P_Skip run (rate control's last resort) */
    double ms_open;           /* wall time mi355enc_open() took (device selection, allocations, stream creation): must stay far below
                                 the 1 s tick of the reference's stall watchdog, /root/reference/src/ceracoder.c:152-200; survives reset_stats */
    uint32_t recoveries;      /* times a bounded device-side wait ran out and the pictures in flight were re-encoded from an IDR picture
                                 (survives reset_stats); last_error_word: which wait it was (text on stderr); safe_level: 0 kernels may wait
                                 on the device for each other, 1 stream order only, 2 one launch per wavefront step (no device-side wait left) */
    uint32_t last_error_word, safe_level;
    uint64_t pinned_inputs;   /* pictures submitted from mi355enc_host_alloc() memory (DMA'd in place, no staging copy) */
} mi355enc_stats_t;

/* Fill cfg with the defaults of the element (gop 60, me_range 16, 2048 kbit/s like x264enc). */
void mi355enc_default_cfg(mi355enc_cfg_t *cfg, int width, int height, int fps_num, int fps_den);

int mi355enc_open(const mi355enc_cfg_t *cfg, mi355enc_t **out);
void mi355enc_close(mi355enc_t *h);

/* Thread-safe against a concurrent encode (atomic store, latched at the next picture);
 * never touches the GPU.  Mirrors g_object_set(elem, "bps", v) at encoder_control.c:53. */
int mi355enc_set_bitrate(mi355enc_t *h, uint32_t bps);
uint32_t mi355enc_get_bitrate(const mi355enc_t *h);
/* Constant-QP override for the next pictures (tests/bench); -1 returns to rate control. */
int mi355enc_set_fixed_qp(mi355enc_t *h, int qp);
/* With a constant QP: the level of rate control's ladder below QP 51 for the next P pictures (tests): 0 off .. 12: P macroblocks
 * whose prediction error is small enough carry no residual / take the P_Skip vector; 255: whole pictures as one P_Skip run. */
int mi355enc_set_fixed_drop(mi355enc_t *h, int drop);
/* Periodic intra refresh instead of periodic IDR pictures (x264's intra-refresh), off by default.  Valid only before the
 * first submit.  On: an IDR picture is coded only for the first picture, a forced key unit, a scene cut or a recovery re-encode, never because
 * cfg.gop pictures have passed.  Instead a column of intra macroblocks sweeps the picture from left to right once every cfg.gop (= N) P pictures,
 * and the inter macroblocks left of it predict only from the part of the reference it has refreshed.  The access unit of every cycle's first
 * picture carries SPS, PPS and a recovery point SEI (recovery_frame_cnt N - 1, exact_match_flag 1), and collect() reports it as a keyframe: a
 * decoder that starts there outputs exact pictures from N - 1 pictures later on.  MI355ENC_ERR_ARG after the first submit, and for `on` with
 * cfg.intra_in_p 0, cfg.partitions, cfg.gop < 2 or cfg.gop > MI355ENC_IR_MAX_PERIOD (recovery_frame_cnt = N - 1 must stay below MaxFrameNum,
 * which the SPS fixes at 256).  The single-stage entry points ignore it. */
#define MI355ENC_IR_MAX_PERIOD 256
int mi355enc_set_intra_refresh(mi355enc_t *h, int on);

/* Synchronous: one NV12 picture in host memory -> one Annex-B access unit
 * (SPS+PPS precede every IDR).  Borrowed input, caller-owned output. */
int mi355enc_encode(mi355enc_t *h, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride,
                    int64_t pts, int force_idr, uint8_t *out, size_t out_cap, size_t *out_len,
                    int *is_keyframe);

/* Pinned host memory for input pictures.  mi355enc_submit() copies a picture from ordinary (pageable) memory into a pinned staging buffer
 * first -- one pass of the calling thread over the picture, 3.1 MB at 1080p.  A picture that lies in memory obtained here is transferred
 * from where it is, asynchronously: submit() returns at once, and the memory must then stay untouched until the matching collect()
 * (the element offers such memory to its upstream through the ALLOCATION query, so a source writes its pictures straight into it).
 * Process-wide; usable on every device.  NULL when there is no HIP device or no memory. */
void *mi355enc_host_alloc(size_t bytes);
void mi355enc_host_free(void *p);

/* Split form.  submit() enqueues all device work of a picture and returns; collect()
 * entropy-codes the oldest submitted picture.  At most pipeline_depth+1 pictures may be
 * outstanding.  submit_device() takes planes already resident in this GPU's memory
 * (the bench's timed region; they must stay valid until the matching collect()).
 * Which way submit_device() takes (without mi355enc_set_input_size): the kernels read the planes where they lie,
 * at the caller's stride, when the width is a multiple of 16, y_stride == uv_stride and a multiple of 16, and
 * both addresses are 16-byte aligned; anything else is first copied on the device into the encoder's own
 * surfaces (and a width that is not a multiple of 16 padded there).  The stream is the same either way. */
int mi355enc_submit(mi355enc_t *h, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride,
                    int64_t pts, int force_idr);
/* Raw input formats other than NV12 are converted on the device (no `videoconvert` hop): I420 (planes Y, U, V), and
 * packed 4:2:2 YUY2 / UYVY (plane 0 only; chroma rows are averaged pairwise with rounding to reach 4:2:0). */
enum { MI355ENC_FMT_NV12 = 0, MI355ENC_FMT_I420 = 1, MI355ENC_FMT_YUY2 = 2, MI355ENC_FMT_UYVY = 3,
/* ... and planar 4:2:2 Y42B (planes Y, U, V; chroma half width, full height: rows averaged like YUY2's), planar 4:4:4 Y444 (chroma
 * filtered to 4:2:0 with the taps [1 2 1] x [1 1], cosited with the even luma columns), YV12 (I420 with V before U), NV21 (NV12 with V before U), and RGB
 * of 0 .. 255 in four 4-byte orders (the byte X is ignored: BGRA, RGBA, ARGB, ABGR are submitted as these) and two 3-byte orders, plane 0 only, converted
 * to Y'CbCr with the matrix and range of mi355enc_set_colorimetry.  mi355enc_submit_device stays NV12. */
       MI355ENC_FMT_Y42B = 4, MI355ENC_FMT_Y444 = 5, MI355ENC_FMT_YV12 = 6, MI355ENC_FMT_NV21 = 7,
       MI355ENC_FMT_BGRX = 8, MI355ENC_FMT_RGBX = 9, MI355ENC_FMT_XRGB = 10, MI355ENC_FMT_XBGR = 11, MI355ENC_FMT_BGR = 12, MI355ENC_FMT_RGB = 13,
/* ... and 10-bit and grey input, brought to 8 bits on the way in -- y8 = min(255, (v10 + 2) >> 2), a 4:2:0 chroma sample likewise, a
 * 4:2:2 one from the sum S of its two rows, min(255, (S + 4) >> 3).  P010 (GStreamer P010_10LE): planes Y and interleaved (Cb, Cr) of little-endian 16-bit
 * words, rows of 2 w bytes, v10 = word >> 6.  I420_10 (I420_10LE): planes Y, U, V of 16-bit words, v10 = word & 1023.  V210 (v210): plane 0 only, six pixels
 * in four little-endian 32-bit words of three 10-bit fields (bits 0-9, 10-19, 20-29): Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5; a row is read up to
 * ceil(w / 6) 16 bytes (GStreamer's stride ((w + 47) / 48) 128 holds that).  GRAY8: plane 0 only, every chroma byte becomes 128. */
       MI355ENC_FMT_P010 = 14, MI355ENC_FMT_I420_10 = 15, MI355ENC_FMT_V210 = 16, MI355ENC_FMT_GRAY8 = 17 };
/* What the samples mean: written into the VUI of every SPS the handle writes from now on (E.1.1 video_signal_type; each IDR picture, each refresh cycle's
 * start, recovery re-encodes), and -- for RGB input -- the matrix and range the device converts with.  full_range 0 / 1; primaries, transfer, matrix: code
 * points of H.264 Tables E-3 / E-4 / E-5, 0 .. 255 (2: unspecified); MI355ENC_ERR_ARG outside.  Valid only before the first submit (MI355ENC_ERR_STATE
 * after it).  A handle on which this was never called writes no video_signal_type (0, 2, 2, 2: the stream of earlier versions).  YUV input is only
 * labelled, not converted -- unless mi355enc_set_input_colorimetry says that it means something else.  RGB input: matrix 1 (BT.709), 5 / 6 (BT.601) or 9 (BT.2020 non-constant) convert with that matrix; 2 converts with 1 when the
 * coded picture is wider than 1024 or higher than 576, else with 6 (and the SPS still says 2: signal what you convert with); any other code makes the
 * submit of an RGB picture fail with MI355ENC_ERR_ARG.  full_range 0: Y' 16 .. 235, CbCr 16 .. 240; 1: 0 .. 255. */
int mi355enc_set_colorimetry(mi355enc_t *h, int full_range, int primaries, int transfer, int matrix);
/* The RGB -> Y'CbCr matrix in the device's integer arithmetic (host only): coef[0..2] yr, yg, yb; [3..5] br, bg, bb (Cb); [6..8] rr, rg, rb (Cr), in units
 * of 2^-16; coef[9] the luma offset (16 or 0).  Y' = clip((yr R + yg G + yb B + (off << 16) + 2^15) >> 16); Cb = clip((br S_R + bg S_G + bb S_B + (128 << 19)
 * + 2^18) >> 19) from the eight-weight sums S of the 2 x 2 site, Cr likewise.  matrix: 1, 5, 6 or 9, else MI355ENC_ERR_ARG. */
int mi355enc_csc_coefficients(int matrix, int full_range, int32_t coef[10]);
/* What the submitted YUV samples mean, where that differs from what the coded samples are to mean (what a caps filter behind
 * `videoconvert` does).  mi355enc_set_colorimetry keeps its meaning: the coded samples, the SPS, and what RGB input, image layers, overlay and border colours
 * are expressed in.  full_range 0 / 1; matrix 1, 5, 6, 9 or 2 (resolved by the coded size as for RGB input; the output's 2 likewise), else MI355ENC_ERR_ARG.
 * Before the first submit only (MI355ENC_ERR_STATE after it), in either order with mi355enc_set_colorimetry.  When the resolved input (range, matrix) differs
 * from the resolved output, every YUV picture -- every submit entry point, JPEG included -- is converted on the device, in place on the coded surfaces, behind
 * decode / conversion / scale / orientation and in front of image layers and text; with a geometry the border keeps its colour.  Pointwise on NV12 (a luma
 * sample uses the chroma pair of its own 2 x 2 block), 16-bit fixed point, clipped to 0 .. 255.  mi355enc_submit_device then never takes its in-place exit:
 * the caller's planes are only read.  When the two are equal, or this was never called, nothing is added.  RGB input is never touched by it.  An output
 * matrix outside 1, 5, 6, 9, 2 makes every YUV submit fail with MI355ENC_ERR_ARG once this has been called. */
int mi355enc_set_input_colorimetry(mi355enc_t *h, int full_range, int matrix);
/* The YUV -> YUV table in the device's integer arithmetic (host only): coef[0..2] cyy, cyb, cyr; [3..4] cbb, cbr; [5..6] crb, crr in units of 2^-16; [7] the
 * input's luma offset oy (16 or 0), [8] the output's oy'.  Y' = clip((cyy (Y - oy) + cyb (Cb - 128) + cyr (Cr - 128) + (oy' << 16) + 2^15) >> 16);
 * Cb' = clip((cbb (Cb - 128) + cbr (Cr - 128) + (128 << 16) + 2^15) >> 16), Cr' likewise with crb, crr.  Matrices 1, 5, 6 or 9, else MI355ENC_ERR_ARG. */
int mi355enc_yuv_coefficients(int in_matrix, int in_full, int out_matrix, int out_full, int32_t coef[9]);
/* HDR input: the submitted 10-bit pictures (MI355ENC_FMT_P010, _I420_10, _V210) are PQ (transfer 16, SMPTE ST 2084) or HLG (18,
 * BT.2100) Y'CbCr with the BT.2020 non-constant-luminance matrix, limited range (full_range 0: Y - 64 over 876, C - 512 over 896) or full; they are tone-mapped to
 * SDR BT.709 in their conversion launch and land in the coded surfaces as 8-bit Y'CbCr of mi355enc_set_colorimetry's matrix and range.  The model: linear
 * display light (PQ: the EOTF, clipped to peak_nits; HLG: the inverse OETF and the OOTF with Lw = peak_nits), the BT.2390 section 5.4.1 EETF from peak_nits to
 * target_nits on max(R, G, B) as a gain on all three, BT.2020 -> BT.709 primaries, over target_nits, clipped, the BT.709 OETF, then the output matrix; a 4:2:0
 * chroma pair from the mean R'G'B' of its four samples; a luma sample uses the chroma pair of its own 2 x 2 block; v210's chroma is first averaged over the two
 * rows, (a + b + 1) >> 1.  The device follows it in integers and table look-ups (mi355enc_hdr_tables) to within one output code.
 * transfer 16 or 18; peak_nits 0 (1000) or 400 .. 10000 (HLG: .. 2000); target_nits 0 (203, BT.2408's reference white) or 100 .. 400; else MI355ENC_ERR_ARG.
 * Before the first submit only, and not on a handle on which mi355enc_set_input_colorimetry was called (nor that call after this one): MI355ENC_ERR_STATE.
 * Once set, every entry point that takes the three formats tone-maps them (mi355enc_submit_fmt, mi355enc_stage_csc, mi355enc_stage_csc_device, the two-launch
 * form under an input size or geometry); every other input -- 8-bit YUV, RGB, GRAY8, JPEG, mi355enc_submit_device -- and an output matrix outside 1, 5, 6, 2
 * (2: resolved by the coded size as for RGB input) fail with MI355ENC_ERR_ARG before anything is latched.  Never called: nothing is allocated, uploaded or
 * launched, and every stream is byte for byte what it was. */
int mi355enc_set_hdr_input(mi355enc_t *h, int transfer, int full_range, int peak_nits, int target_nits);
/* The parameter block of the tone map in the device's integer arithmetic (host only, no device needed): *n = the block's size in words (7726); out (cap words)
 * receives it; out null: the size alone; cap too small: MI355ENC_ERR_OVERFLOW.  out_matrix 1, 5 or 6; other arguments as mi355enc_set_hdr_input's.  Words:
 * 0 layout version (1), 1 transfer, 2 full_range, 3 peak, 4 target (resolved), 5 out_matrix, 6 out_full, 7 words in all; 8 oy, 9 cy, 10 rv, 11 gu, 12 gv, 13 bu
 * (the input matrix, 2^-28 per code); 14-16 the HLG luminance weights (2^-16); 17-25 BT.2020 -> BT.709 by rows (2^-20); 26-28 yr yg yb, 29-31 br bg bb, 32-34
 * rr rg rb (2^-14 of a code per unit); 35 oy'; 36-39 zero; 40 LIN[4097] (linear light over the non-linear code in 2^-12 steps, 2^-28 of peak / of scene 1.0);
 * 4137 GA[1282] (HLG OOTF gain Ys^(g - 1), 2^-30); 5419 GB[1282] (tone gain EETF(n) / n peak / target, 2^-24); 6701 OE[1025] (BT.709 OETF over 2^-10 steps,
 * 2^-16).  GA, GB by octaves: entry 64 o + m stands for s = (64 + m) << (o + 2), entry 1280 for 2^28, 1281 repeats it.  The rule, with y = Y - oy, u = Cb - 512,
 * v = Cr - 512:  t = cy y + {rv v | gu u + gv v | bu u};  x = clip((t + 8) >> 4, 0, 2^24), k = min(x >> 12, 4095), f = x - (k << 12),
 * l = LIN[k] + (((LIN[k + 1] - LIN[k]) f + 2^11) >> 12);  HLG only: ys = (lr lR + lg lG + lb lB + 2^15) >> 16, l = (l gain(GA, ys) + 2^29) >> 30;
 * w = (l gain(GB, max l) + 2^23) >> 24;  u_i = clip((sum_j M_ij w_j + 2^19) >> 20, 0, 2^28), k = min(u >> 18, 1023), f = u - (k << 18),
 * E = OE[k] + (((OE[k + 1] - OE[k]) f + 2^17) >> 18);  Y' = clip255((yr R + yg G + yb B + (oy' << 30) + 2^29) >> 30);  with S the sums of E over a pair's
 * four samples, Cb = clip255((br SR + bg SG + bb SB + (128 << 32) + 2^31) >> 32), Cr likewise.  gain(T, s): s = max(min(s, 2^28), 256), e = floor(log2 s),
 * sh = e - 6, q = s >> sh, i = 64 (e - 8) + q - 64, f = s - (q << sh), T[i] + (((T[i + 1] - T[i]) f + (1 << (sh - 1))) >> sh).  Products wider than 32 bits
 * are taken in 64. */
int mi355enc_hdr_tables(int transfer, int full_range, int peak_nits, int target_nits, int out_matrix, int out_full, int32_t *out, size_t cap, size_t *n);
/* the colour step alone (tests): host NV12 planes of the coded size (16*mbw x 16*mbh luma, then interleaved chroma), in and out, like mi355enc_stage_image,
 * with the handle's geometry, orientation and colorimetries; MI355ENC_ERR_STATE when the handle has no conversion */
int mi355enc_stage_yuv_convert(mi355enc_t *h, uint8_t *y, uint8_t *uv);
/* Picture controls on the way in: colour balance, gamma and sharpening of the picture part of the coded surfaces, behind the colour
 * step and in front of frame-rate conversion, image layers and text.  All integers: brightness -1000 .. 1000 (thousandths of the luma scale S, added; neutral
 * 0), contrast 0 .. 2000 (thousandths, gain about black; 1000), saturation 0 .. 2000 (thousandths, chroma gain; 1000), hue -1000 .. 1000 (thousandths of pi,
 * chroma rotation with videobalance's sign; 0), gamma 100 .. 10000 (thousandths, t -> t^(1000 / gamma) on [0, 1]; 1000), sharpen -16 .. 64 (sixteenths of the
 * unsharp amount, negative softens; 0), sharpen_threshold 0 .. 32 (coring, for sharpen > 0 only; 0).  Black level B and scale S are the output range's
 * (mi355enc_set_colorimetry's full_range): 16 and 219, or 0 and 255.
 *   luma     Y' = L[Y]; gamma 1000: L[v] = clip255(B + floor((2 ((v - B) contrast + brightness S) + 1000) / 2000)); otherwise in double: t = (v - B) / S, inside
 *            [0, 1] t^(1000 / gamma), outside as it is, y = B + S (t contrast / 1000 + brightness / 1000), L[v] = clip255(floor(y + 0.5)).  Non-decreasing.
 *   chroma   cu = round(4096 sat / 1000 cos(pi hue / 1000)), su likewise with sin; a = Cb - 128, b = Cr - 128:
 *            Cb' = clip255(128 + ((cu a + su b + 2048) >> 12)), Cr' = clip255(128 + ((-su a + cu b + 2048) >> 12))
 *   sharpen  on the luma behind the table, weights 1 2 1 / 2 4 2 / 1 2 1: d = 16 Y - sum; sharpen > 0 and |d| <= 16 threshold: Y stays; otherwise
 *            Y' = clip255(Y + ((sharpen d + 128) >> 8)).  Neighbours are clamped to the visible part of the picture rectangle; a margin sample of the coded
 *            surface is the result of its clamped visible position; a letterbox border keeps its bytes. */
typedef struct {
    int brightness, contrast, saturation, hue, gamma, sharpen, sharpen_threshold;
} mi355enc_adjust_t;
void mi355enc_adjust_default(mi355enc_adjust_t *a);     /* the neutral values */
int mi355enc_adjust_check(const mi355enc_adjust_t *a); /* host only: MI355ENC_OK, or MI355ENC_ERR_ARG for a value outside its range */
/* host only, no device needed: the luma table L and {cu, su} of a parameter set for an output range */
int mi355enc_adjust_tables(const mi355enc_adjust_t *a, int full_range, uint8_t luma[256], int32_t chroma[2]);
/* At any time and from any thread, no GPU call (the tables are built here); latched once per input picture at its submit.  NULL or all neutral: off.  Off (the
 * default): nothing is allocated, uploaded or launched, and every stream is byte for byte what it was.  With an active adjustment mi355enc_submit_device
 * never encodes in place: the caller's planes are only read. */
int mi355enc_set_adjust(mi355enc_t *h, const mi355enc_adjust_t *a);
int mi355enc_get_adjust(const mi355enc_t *h, mi355enc_adjust_t *a);
int mi355enc_last_adjust(mi355enc_t *h, mi355enc_adjust_t *a); /* of the last collected picture; MI355ENC_ERR_STATE before the first collect */
/* the step alone (tests): host NV12 planes of the coded size, in and out, like mi355enc_stage_yuv_convert, with the handle's geometry, orientation and
 * output range; a: the parameters (the handle's own setting is not touched) */
int mi355enc_stage_adjust(mi355enc_t *h, const mi355enc_adjust_t *a, uint8_t *y, uint8_t *uv);
size_t mi355enc_debug_adjust_bytes(const mi355enc_t *h); /* device bytes the step holds: 0 until the first sharpened picture, then 16 mb_width x 16 mb_height */
/* Temporal noise reduction on the way in: a motion-adaptive recursive filter on the coded surfaces, behind the colour step and in front
 * of the picture controls, so that everything later -- controls, frame-rate conversion, image layers, text, metrics, stills, the encoder -- sees the filtered
 * picture, and layers and text are never filtered.  luma, chroma: 0 .. MI355ENC_DENOISE_MAX, the noise amplitude in codes that is filtered fully; 0 leaves that
 * plane's samples as they are.  All integers.  The handle keeps a history H per sample in sixteenths of a code (uint16, 0 .. 4080; the chroma's interleaved like
 * NV12); "the previous picture" is the previous one that went through the step (one that frame-rate conversion drops before transfer never does).
 *   tables   for a strength s > 0, floor of the exact quotient, then clipped:
 *            P_s[a] = clip(0, 224, floor(224 (3 s - a) / (2 s))), one for luma and one for chroma; B[i] = clip(0, 255, floor(255 (6 s - i) / (4 s))) with the
 *            luma strength, or the chroma strength when luma is 0
 *   block    per aligned 8 x 8 luma block: M = sum |c - ((H + 8) >> 4)| over its 64 luma samples, b = B[min(255, M >> 4)]; its 4 x 4 chroma pairs use the same b.
 *            (With luma 0 and chroma > 0 the luma samples are not changed, and their history follows them, H' = 16 c: M then measures against the previous picture.)
 *   sample   c the input code: d = |c - ((H + 8) >> 4)|, k = (b P[d] + 128) >> 8, H' = 16 c + ((k (H - 16 c) + 128) >> 8) (floor), out = (H' + 8) >> 4
 *   priming  a plane without a valid history -- the first picture, a strength that was 0 for the previous picture -- gets out = c, H' = 16 c
 *   margins  the step runs over the whole coded surface (a letterbox border is constant: the rule is the identity there); an 8 x 8 block without a visible
 *            sample takes out and H' of its clamped visible position, a partly visible one is computed as it lies (the input path makes the margins it reads
 *            replicas before the step; mi355enc_stage_denoise takes its surfaces as given).
 * A change between two strengths > 0 keeps the history; a scene cut needs nothing (b = 0: out = c, H' = 16 c). */
#define MI355ENC_DENOISE_MAX 32
typedef struct {
    int luma, chroma;
} mi355enc_denoise_t;
void mi355enc_denoise_default(mi355enc_denoise_t *d);     /* off: {0, 0} */
int mi355enc_denoise_check(const mi355enc_denoise_t *d); /* host only: MI355ENC_OK, or MI355ENC_ERR_ARG for a value outside 0 .. 32 */
/* host only, no device needed: B, the luma's P and the chroma's P (all zeros for a plane with strength 0) */
int mi355enc_denoise_tables(const mi355enc_denoise_t *d, uint8_t block[256], uint8_t luma[256], uint8_t chroma[256]);
/* At any time and from any thread, no GPU call; latched once per input picture at its submit.  NULL or {0, 0}: off.  Off (the default): nothing is allocated or
 * launched, and every stream is byte for byte what it was.  With an active filter mi355enc_submit_device never encodes in place: the caller's planes are only read. */
int mi355enc_set_denoise(mi355enc_t *h, const mi355enc_denoise_t *d);
int mi355enc_get_denoise(const mi355enc_t *h, mi355enc_denoise_t *d);
int mi355enc_last_denoise(mi355enc_t *h, mi355enc_denoise_t *d); /* of the last collected picture; MI355ENC_ERR_STATE before the first collect */
/* the step alone (tests): host NV12 planes of the coded size and their histories (uint16, the planes' shapes), in and out in place on the host arrays, with the
 * handle's visible size; hist_y / hist_uv NULL: that plane primes (hist_y is needed whenever anything is filtered: the block measure reads it).  hist_y_out is
 * written whenever d is not off, hist_uv_out when d->chroma > 0; either may be NULL.  The handle's own setting and history are not touched. */
int mi355enc_stage_denoise(mi355enc_t *h, const mi355enc_denoise_t *d, const uint16_t *hist_y, const uint16_t *hist_uv, uint8_t *y, uint8_t *uv,
                           uint16_t *hist_y_out, uint16_t *hist_uv_out);
size_t mi355enc_debug_denoise_bytes(const mi355enc_t *h); /* device bytes of the handle's history: 0 until the first filtered picture, then 2 per luma and per chroma sample kept (with motion compensation: twice that and 4 per 8 x 8 block) */
/* Motion compensation of the filter: per aligned 8 x 8 luma block with a visible sample, a whole-sample vector (dx, dy) into the history.
 *   search   Q = (H_luma + 8) >> 4; the candidates are all (dx, dy) with |dx|, |dy| <= range whose displaced block lies inside the coded surface (margins
 *            included); cost = sum |c(x, y) - Q(x + dx, y + dy)| over the block; key = ((cost + 4 s (|dx| + |dy|)) << 16) | rank with s the strength that builds
 *            B and rank = (|dx| + |dy|) * 1089 + (dy + 16) * 33 + (dx + 16); the block's vector is the candidate with the smallest key.  It runs whenever the
 *            block measure runs (a plane is filtered, not priming), and M is its cost.
 *   luma     the sample rule with H(x + dx, y + dy); H' and out are written at (x, y)
 *   chroma   H.264's chroma prediction for a whole-sample luma vector, on the history, per byte of the pair: the pair at (dx >> 1, dy >> 1), the rounded mean
 *            of two along an odd axis, (a + b + c + d + 2) >> 2 of four with both odd
 * Everything else is the filter's as described above; a change of range between pictures, 0 included, keeps the history.  range: 0 .. 16 luma samples, 0 (the
 * default): none, exactly the filter above.  Callable at any time from any thread, no GPU call; latched per input picture beside the strengths.  With both
 * strengths 0 the range has no effect.  The history is double-buffered from the first picture that is filtered with a range above 0. */
#define MI355ENC_DENOISE_MOTION_MAX 16
int mi355enc_set_denoise_motion(mi355enc_t *h, int range); /* MI355ENC_ERR_ARG outside 0 .. 16 */
int mi355enc_get_denoise_motion(const mi355enc_t *h, int *range);
int mi355enc_last_denoise_motion(mi355enc_t *h, int *range); /* of the last collected picture; MI355ENC_ERR_STATE before the first collect */
/* host only: the key of a candidate; 0xFFFFFFFF for arguments outside cost 0 .. 16320, |dx|, |dy| <= 16, s 0 .. 32 */
uint32_t mi355enc_denoise_motion_key(int cost, int dx, int dy, int s);
/* the search alone (tests): a luma surface of the coded size and a luma history on host arrays; vec_out: (coded width / 8) x (coded height / 8) words in raster
 * order -- dx in byte 0, dy in byte 1 (int8), the vector's cost M in the high half; zero for a block without a visible sample.  d not off, range 1 .. 16 */
int mi355enc_stage_denoise_search(mi355enc_t *h, const mi355enc_denoise_t *d, int range, const uint8_t *y, const uint16_t *hist_y, uint32_t *vec_out);
/* mi355enc_stage_denoise with a range (0: that call itself), on histories of its own; vec_out (may be NULL): the search's words as above, zeros where no search
 * ran (range 0, or nothing is filtered) */
int mi355enc_stage_denoise_mc(mi355enc_t *h, const mi355enc_denoise_t *d, int range, const uint16_t *hist_y, const uint16_t *hist_uv, uint8_t *y, uint8_t *uv,
                              uint16_t *hist_y_out, uint16_t *hist_uv_out, uint32_t *vec_out);
/* Electronic image stabilisation: the crop rectangle of the input geometry follows the camera's shake, decided per picture on the
 * device from the picture itself; off (range 0) by default, and off nothing is allocated or launched.  All integers.
 *   measured on  the luma of the submitted picture at the input size in_w x in_h (what the geometry launch reads: after conversion / tone map / JPEG decode,
 *                every second byte of YUY2 / UYVY), the whole picture, not only the crop
 *   projections  four horizontal bands k: rows [k in_h / 4, (k + 1) in_h / 4) give column sums C_k[x]; four vertical bands likewise give row sums R_k[y]
 *   vote         of a projection p (length n) against the previous picture's q: cost(d) = sum over x in [range, n - range) of |p[x] - q[x - d]| for
 *                d in -range .. range; the d of the smallest cost, valid only if that minimum is unique and |d| < range
 *   motion       mx: the lower median of the valid column-band votes (sorted v[(count - 1) / 2]; 0 with none); my likewise of the row bands
 *   trajectory   per axis, S in 1/256 sample: S = ((S (256 - leak)) >> 8) + 256 m (floor), S = clip(S, 256 lo, 256 hi), o = clip(2 ((S + 256) >> 9), lo, hi)
 *                with lo = -min(margin, crop origin), hi = min(margin, input - crop origin - crop size), both even towards zero
 *   priming      the first picture after off -> on (and after stages 29 / 30 of mi355enc_time_stage): m = 0, S = 0, o = 0
 *   the offset   the geometry launch uses the tables of the crop as set; every tap index and the clamp rectangle are displaced by (ox, oy) (chroma columns
 *                ox / 2, 4:2:0 chroma rows oy / 2, 4:2:2 chroma rows oy)
 * Needs an input geometry (otherwise a submit answers MI355ENC_ERR_STATE) and in_w, in_h >= 4 range (MI355ENC_ERR_ARG).  With it on, mi355enc_submit_device
 * reads the whole submitted luma plane, not only the crop rectangle.  The setters may be called at any time from any thread and make no GPU call; the value is
 * latched per input picture.  The single-stage entry points run the geometry as set, unstabilised. */
#define MI355ENC_STABILIZE_RANGE_MAX 32
#define MI355ENC_STABILIZE_MARGIN_MAX 1024
typedef struct {
    int range;              /* search range in input luma samples, 0 .. 32; 0: off */
    int leak;               /* 0 .. 255: how fast the trajectory returns to the crop as set (0: never) */
    int margin_x, margin_y; /* how far the crop may move per side, even, 0 .. 1024 */
} mi355enc_stabilize_t;
typedef struct {
    int mx, my;             /* measured motion against the previous measured picture */
    int votes_x, votes_y;   /* valid votes per axis, 0 .. 4 */
    int ox, oy;             /* the crop's displacement in input luma samples (pre-orientation) */
    int sx, sy;             /* the trajectory's state, 1/256 sample */
} mi355enc_stabilize_info_t;
void mi355enc_stabilize_default(mi355enc_stabilize_t *s); /* off: {0, 16, 0, 0} */
int mi355enc_stabilize_check(const mi355enc_stabilize_t *s); /* host only: MI355ENC_OK or MI355ENC_ERR_ARG */
int mi355enc_set_stabilize(mi355enc_t *h, const mi355enc_stabilize_t *s); /* NULL: off */
int mi355enc_get_stabilize(const mi355enc_t *h, mi355enc_stabilize_t *s);
/* of the last collected picture (either pointer may be NULL); MI355ENC_ERR_STATE before the first collect.  An unstabilised picture reports zeros */
int mi355enc_last_stabilize(mi355enc_t *h, mi355enc_stabilize_t *s, mi355enc_stabilize_info_t *info);
size_t mi355enc_debug_stabilize_bytes(const mi355enc_t *h); /* device bytes of the stabiliser: 0 until the first stabilised picture */
/* host only, the rule piece by piece.  project: a luma plane (first sample at `luma`, samples `step` = 1 or 2 bytes apart) -> sums: C_0 .. C_3 (w each), then
 * R_0 .. R_3 (h each).  vote: 1 valid / 0 no vote (*d: the first d of the smallest cost either way), n >= 4 range, range >= 1.  motion: the lower median of
 * `count` (0 .. 4) valid votes.  step: one trajectory step of an axis */
int mi355enc_stabilize_project(const uint8_t *luma, int stride, int step, int w, int h, uint32_t *sums);
int mi355enc_stabilize_vote(const uint32_t *p, const uint32_t *q, int n, int range, int *d);
int mi355enc_stabilize_motion(const int *votes, int count, int *m);
int mi355enc_stabilize_step(int S, int m, int leak, int lo, int hi, int *S_out, int *o);
/* the two launches alone (tests), in the frame of the single-stage entry points: MI355ENC_ERR_ARG without a handle, MI355ENC_ERR_STATE with pictures in flight.
 * probe_project: a host luma plane as above -> the 4 (w + h) sums.  probe_match: previous and current sums of a w x h picture from host arrays, the setting's
 * range and leak, bounds {lo_x, hi_x, lo_y, hi_y}, the state {Sx, Sy} going in, prime -> the record */
int mi355enc_stabilize_probe_project(mi355enc_t *h, const uint8_t *luma, int stride, int step, int w, int ht, uint32_t *sums);
int mi355enc_stabilize_probe_match(mi355enc_t *h, const uint32_t *prev, const uint32_t *cur, int w, int ht, const mi355enc_stabilize_t *s, const int bounds[4],
                                   const int state[2], int prime, mi355enc_stabilize_info_t *info);
/* Automatic levels and white balance: per picture, a black point, a white point and a chroma offset are measured on the picture's coded
 * surfaces, smoothed over time and applied to the same picture (feed-forward), all on the device: behind the noise filter and in front of the picture controls,
 * so the manual controls trim on top of it and mix, layers and text are never touched.  Off by default, and off nothing is allocated or launched.  All integers;
 * B and S are the output range's black level and scale (16 / 219 or 0 / 255).
 *   setting      levels, balance 0 .. 1000 (thousandths of the full stretch / chroma correction; both 0: off), speed 1 .. 256 (256 follows at once), clip_low,
 *                clip_high 0 .. 2000 (ten-thousandths of the samples that may fall outside the black / white point), max_gain 1000 .. 8000 (thousandths),
 *                reach 0 .. 127 (how far from 128 a chroma sample may lie and still vote)
 *   measured on  the visible samples of the picture rectangle (margins of the coded surface and a letterbox border never count): H[256] the count per luma
 *                code, N their sum; the chroma sample (cx, cy) votes if its co-sited luma y = Y(2 cx, 2 cy) has B + (S >> 3) <= y <= B + S - (S >> 3) and
 *                |Cb - 128|, |Cr - 128| <= reach; n voters, su / sv the sums of their Cb / Cr, NC the visible chroma samples
 *   points       lo = the smallest v with 10000 cum(v) > clip_low N (cum: inclusive prefix sum; none: 255), hi = the largest v with
 *                10000 (N - cum(v - 1)) > clip_high N (none: 0), both clipped into [B, B + S]; in 64 bits
 *   chroma       valid iff n > 0 and 16 n >= NC; then du = (256 su) / n - 32768, dv likewise (1/256 code)
 *   state        {Lo, Hi, Du, Dv} in 1/256 code: X = X + (((256 m - X) speed) >> 8) (floor); Du / Dv take du / dv as their 256 m and stay as they are with an
 *                invalid measurement; then Lo, Hi are clipped into [256 B, 256 (B + S)] (a no-op unless the output range changed).  Priming -- the first
 *                picture after off -> on, and the stage entry points -- sets Lo = 256 lo, Hi = 256 hi, Du = du, Dv = dv (0 when invalid)
 *   strength     L = 256 B + ((Lo - 256 B) levels) / 1000, T = 256 (B + S) - ((256 (B + S) - Hi) levels) / 1000
 *   gain limit   span = T - L, smin = ceil(256000 S / max_gain); span < smin: L = ((L + T) >> 1) - (smin >> 1), T = L + smin, then shifted into
 *                [256 B, 256 (B + S)], span = smin
 *   table        t = clip(256 v - L, 0, span), A[v] = B + (2 t S + span) / (2 span); not applied with levels 0
 *   offsets      off_u = floor((Du balance + 128000) / 256000), off_v likewise; Cb' = clip255(Cb - off_u), Cr' = clip255(Cr - off_v)
 * Applied in place over the whole picture rectangle, margins included; a border keeps its bytes. */
typedef struct {
    int levels, balance, speed, clip_low, clip_high, max_gain, reach;
} mi355enc_autolevel_t;
typedef struct {
    uint32_t hist[256]; /* H */
    uint32_t voters;    /* n */
    uint32_t chroma;    /* NC */
    uint64_t su, sv;
} mi355enc_autolevel_meas_t;
typedef struct {
    int lo, hi, voters, du, dv; /* the picture's measurement */
    int s_lo, s_hi, s_du, s_dv; /* the state behind it: Lo, Hi, Du, Dv */
    int off_u, off_v, valid;
} mi355enc_autolevel_info_t;
void mi355enc_autolevel_default(mi355enc_autolevel_t *a); /* off: {0, 0, 16, 50, 50, 2000, 48} */
int mi355enc_autolevel_check(const mi355enc_autolevel_t *a); /* host only: MI355ENC_OK or MI355ENC_ERR_ARG */
/* host only: the decision of a picture.  state: {Lo, Hi, Du, Dv} going in (Lo, Hi in 0 .. 65280, Du, Dv in -32768 .. 32767; ignored with prime) and coming
 * out; m: su, sv <= 255 voters, voters <= chroma <= 2^24, the sum of hist <= 2^26.  table: 256 bytes (also written with levels 0, where it is not applied) */
int mi355enc_autolevel_decide(const mi355enc_autolevel_meas_t *m, const mi355enc_autolevel_t *a, int full_range, int prime, int32_t state[4],
                              mi355enc_autolevel_info_t *info, uint8_t table[256]);
/* At any time and from any thread, no GPU call; latched once per input picture at its submit.  NULL or both strengths 0: off.  With an active setting
 * mi355enc_submit_device never encodes in place: the caller's planes are only read. */
int mi355enc_set_autolevel(mi355enc_t *h, const mi355enc_autolevel_t *a);
int mi355enc_get_autolevel(const mi355enc_t *h, mi355enc_autolevel_t *a);
/* of the last collected picture (any pointer may be NULL); MI355ENC_ERR_STATE before the first collect.  A picture the step did not run on reports zeros */
int mi355enc_last_autolevel(mi355enc_t *h, mi355enc_autolevel_t *a, mi355enc_autolevel_info_t *info, uint8_t table[256]);
size_t mi355enc_debug_autolevel_bytes(const mi355enc_t *h); /* device bytes of the step: 0 until the first autolevelled picture */
/* the step alone (tests): host NV12 planes of the coded size, in and out, like mi355enc_stage_adjust; the three launches on that picture, primed by it.  The
 * handle's own setting is not touched; a stream that follows primes.  info, table may be NULL */
int mi355enc_autolevel_probe_stage(mi355enc_t *h, const mi355enc_autolevel_t *a, uint8_t *y, uint8_t *uv, mi355enc_autolevel_info_t *info, uint8_t table[256]);
/* the first two launches alone (tests), in the frame of the single-stage entry points.  probe_measure: host NV12 surfaces of W x H (W a multiple of 16 up to
 * 8192, H even up to 8192) at stride W, rect {x0, x1, y0, y1} (even, inside the surfaces) and the visible size vw x vh (the rectangle's visible part not
 * empty) -> the measurement summed over the workgroups' slabs.  probe_decide: mi355enc_autolevel_decide on the device */
int mi355enc_autolevel_probe_measure(mi355enc_t *h, const uint8_t *y, const uint8_t *uv, int W, int H, const int rect[4], int vw, int vh, int full_range, int reach,
                                     mi355enc_autolevel_meas_t *m);
int mi355enc_autolevel_probe_decide(mi355enc_t *h, const mi355enc_autolevel_meas_t *m, const mi355enc_autolevel_t *a, int full_range, int prime, int32_t state[4],
                                    mi355enc_autolevel_info_t *info, uint8_t table[256]);
/* Spatial noise reduction with a measured strength: an edge-preserving stencil on the picture's coded surfaces, directly in front of the
 * temporal noise filter, and a per-picture noise estimate that can set its strength, all on the device.  Off by default, and off nothing is allocated or
 * launched.  All integers; >> and floor() are floors; B and S are the output range's black level and scale (16 / 219 or 0 / 255).
 *   setting      luma, chroma 0 .. 32 (the noise amplitude in codes that is filtered fully), auto_gain 0 (manual) or 250 .. 8000 (thousandths of the measured
 *                sigma), percentile 1 .. 50, speed 1 .. 256 (256 follows at once).  manual: luma / chroma are the strengths, both 0: off.  automatic: they are
 *                upper bounds of the measured strength; both 0: measure only -- the estimate is reported and nothing is filtered
 *   tables       R_s[a] = clip(0, 16, floor(16 (3 s - a) / (2 s))), F_s[a] = a R_s[a] for s > 0 and a = 0 .. 255; F_0 = 0
 *   luma         5 x 5, w = [1 4 6 4 1] x [1 4 6 4 1]; d_j = n_j - c: out = c + ((sum w_j sgn(d_j) F_s[|d_j|] + 2048) >> 12)
 *   chroma       Cb and Cr each for itself, 3 x 3, w = 1 2 1 / 2 4 2 / 1 2 1: out = c + ((sum + 128) >> 8) with the chroma strength's table
 *   edges        over the picture rectangle; neighbours are clamped to its visible part, a margin sample takes the result of its clamped visible position, a
 *                letterbox border keeps its bytes
 *   estimate     on the luma in front of the filter.  Candidates: the aligned 8 x 8 blocks wholly inside the rectangle's visible part (NC of them).  Per
 *                block: L = the mask 1 -2 1 / -2 4 -2 / 1 -2 1 on its 36 interior samples, A = sum |L|, bin = min(255, (95 A + 1024) >> 11) (sigma in eighths
 *                of a code); it votes iff its sample sum m has 64 (B + (S >> 4)) <= m <= 64 (B + S - (S >> 4)).  H[256] the voters' histogram, N their count;
 *                v = the smallest bin with 100 cum(v) >= percentile N; valid iff N > 0 and 16 N >= NC
 *   state        X in 1/256 bin: X += ((256 v - X) speed) >> 8; an invalid measurement leaves it.  Priming -- the first picture after off -> on or manual ->
 *                automatic, and the stage calls -- sets X = 256 v (0 when invalid)
 *   strength     s = floor((X auto_gain + 1024000) / 2048000); s_luma = min(luma, s), s_chroma = min(chroma, s)
 * In automatic mode a plane whose bound is above 0 goes through the filter launch whatever s turns out to be (s = 0 copies it, margins as above): only the
 * device knows s.  In manual mode a plane with strength 0 is neither read nor written. */
#define MI355ENC_DENOISE_SPATIAL_MAX 32
typedef struct {
    int luma, chroma, auto_gain, percentile, speed;
} mi355enc_denoise_spatial_t;
typedef struct {
    uint32_t hist[256]; /* H */
    uint32_t candidates; /* NC */
    uint32_t voters;     /* N */
} mi355enc_denoise_spatial_meas_t;
typedef struct {
    int candidates, voters, v, valid; /* the picture's measurement (zeros in manual mode) */
    int x;                            /* the state behind it */
    int s_luma, s_chroma;             /* the strengths the picture was filtered with */
    int reserved;
} mi355enc_denoise_spatial_info_t;
void mi355enc_denoise_spatial_default(mi355enc_denoise_spatial_t *a); /* off: {0, 0, 0, 25, 32} */
int mi355enc_denoise_spatial_check(const mi355enc_denoise_spatial_t *a); /* host only: MI355ENC_OK or MI355ENC_ERR_ARG */
/* host only: R_s and F_s of a strength 0 .. 32 (either pointer may be NULL, not both) */
int mi355enc_denoise_spatial_tables(int s, uint8_t weight[256], uint16_t filter[256]);
/* host only: the filter in place on NV12 surfaces of W x H (W a multiple of 16 up to 8192, H even up to 8192) at stride W; rect {x0, x1, y0, y1} (even, inside
 * the surfaces), vw x vh the visible size (the rectangle's visible part not empty); s_luma, s_chroma 0 .. 32, or -1: the plane is not touched */
int mi355enc_denoise_spatial_apply_host(uint8_t *y, uint8_t *uv, int W, int H, const int rect[4], int vw, int vh, int s_luma, int s_chroma);
/* host only: the estimate's measurement of a luma plane (arguments as above) */
int mi355enc_denoise_spatial_measure_host(const uint8_t *y, int W, int H, const int rect[4], int vw, int vh, int full_range, mi355enc_denoise_spatial_meas_t *m);
/* host only: the decision of a picture (a: automatic).  *x: the state going in (0 .. 65280; ignored with prime) and coming out; m: candidates <= 2^20, the sum
 * of hist = voters <= candidates */
int mi355enc_denoise_spatial_decide(const mi355enc_denoise_spatial_meas_t *m, const mi355enc_denoise_spatial_t *a, int prime, int32_t *x, mi355enc_denoise_spatial_info_t *info);
/* At any time and from any thread, no GPU call; latched once per input picture at its submit.  NULL or a setting that neither filters nor measures: off.  With
 * an active setting mi355enc_submit_device never encodes in place: the caller's planes are only read. */
int mi355enc_set_denoise_spatial(mi355enc_t *h, const mi355enc_denoise_spatial_t *a);
int mi355enc_get_denoise_spatial(const mi355enc_t *h, mi355enc_denoise_spatial_t *a);
/* of the last collected picture (either pointer may be NULL); MI355ENC_ERR_STATE before the first collect.  A picture the step did not run on reports zeros; a
 * manual one zeros and its strengths */
int mi355enc_last_denoise_spatial(mi355enc_t *h, mi355enc_denoise_spatial_t *a, mi355enc_denoise_spatial_info_t *info);
size_t mi355enc_debug_denoise_spatial_bytes(const mi355enc_t *h); /* device bytes of the step: 0 until the first picture it runs on */
/* the step alone (tests): host NV12 planes of the coded size, in and out, like mi355enc_stage_adjust; an automatic setting is primed by that picture.  The
 * handle's own setting is not touched; a stream that follows primes.  info may be NULL */
int mi355enc_denoise_spatial_probe_stage(mi355enc_t *h, const mi355enc_denoise_spatial_t *a, uint8_t *y, uint8_t *uv, mi355enc_denoise_spatial_info_t *info);
/* the measure and the decide launch alone (tests), in the frame of the single-stage entry points: mi355enc_denoise_spatial_measure_host / _decide on the device */
int mi355enc_denoise_spatial_probe_measure(mi355enc_t *h, const uint8_t *y, int W, int H, const int rect[4], int vw, int vh, int full_range, mi355enc_denoise_spatial_meas_t *m);
int mi355enc_denoise_spatial_probe_decide(mi355enc_t *h, const mi355enc_denoise_spatial_meas_t *m, const mi355enc_denoise_spatial_t *a, int prime, int32_t *x, mi355enc_denoise_spatial_info_t *info);
/* Lens, roll and keystone correction: the coded picture is resampled through a coarse mesh of source positions, the first step on the
 * coded surfaces (in front of the colour step, the noise filter, the picture controls, the mix, layers and text; behind the geometry and the stabiliser's
 * crop); off by default, and off nothing is allocated or launched.  All integers; >> is a floor.
 *   mesh       for the coded visible size w x h: nx = (w + 15) / 16 + 1 by ny = (h + 15) / 16 + 1 nodes; node (i, j) at int32 index 2 (j nx + i) holds the
 *              source position {sx, sy} of the output luma sample (16 i, 16 j) in 1/256 luma sample, each inside [-2048 * 256, 10240 * 256]
 *   position   luma (x, y): i = x >> 4, j = y >> 4, xf = x & 15, yf = y & 15; per coordinate
 *              P = (16 - yf) ((16 - xf) N[j][i] + xf N[j][i + 1]) + yf ((16 - xf) N[j + 1][i] + xf N[j + 1][i + 1]) (1/65536 sample), p = (P + 1024) >> 11;
 *              the chroma pair (cx, cy): P at the luma point (2 cx, 2 cy), p = (P + 2048) >> 12 (1/32 chroma sample; siting is ignored).  ix = p >> 5, f = p & 31
 *   filter     kind 0 bilinear: taps {0, 4 (32 - f), 4 f, 0}; kind 1 Catmull-Rom: c-1 = (-f^3 + 64 f^2 - 1024 f + 256) >> 9,
 *              c1 = (-3 f^3 + 128 f^2 + 1024 f + 256) >> 9, c2 = (f^3 - 32 f^2 + 256) >> 9, c0 = 128 - c-1 - c1 - c2.
 *              a = sum_r cy[r] sum_k cx[k] S[clamp(iy - 1 + r)][clamp(ix - 1 + k)], out = clip((a + 8192) >> 14, 0, 255); tap positions clamp to the visible
 *              plane; Cb and Cr of a pair take the same taps
 *   outside    ix < -1, ix above the last column, or the same of iy and the rows: the fill value, unfiltered (fill[0] luma, fill[1], fill[2] a chroma pair)
 *   margin     up to whole macroblocks the last visible column / row (chroma: pair) is repeated, as by every other input launch
 * The setters may be called at any time from any thread; the value is latched per input picture, and pictures in flight keep the mesh they latched. */
typedef struct {
    int kind;        /* 0 bilinear, 1 bicubic (Catmull-Rom) */
    uint8_t fill[3]; /* Y, Cb, Cr of the samples whose source lies outside the picture */
} mi355enc_warp_t;
typedef struct {     /* Q16 */
    int k1, k2;      /* radial terms, -65536 .. 65536; neutral 0 */
    int zoom;        /* 16384 .. 262144; neutral 65536 (above: the source is read further out, the picture shrinks) */
    int cos, sin;    /* roll, -65536 .. 65536 each; neutral 65536, 0 */
    int kh, kv;      /* keystone, -32768 .. 32768; neutral 0 */
} mi355enc_warp_params_t;
void mi355enc_warp_params_default(mi355enc_warp_params_t *p); /* the neutral values: their mesh is the identity (4096 i, 4096 j) */
/* host only.  coeff: the four taps of fraction f (0 .. 31).  mesh_size: nx, ny of a w x h picture (2 .. 8192 each).  mesh_check: every node inside the range.
 * build: the mesh of a parameter set into mesh[cap] (cap >= 2 nx ny), in 64-bit arithmetic, for node (i, j):
 *   u = 32 i - (w - 1), v = 32 j - (h - 1);  U = (zoom (cos u - sin v)) >> 16, V = (zoom (sin u + cos v)) >> 16
 *   d = 65536 + fdiv(kh U, (w - 1) << 16) + fdiv(kv V, (h - 1) << 16) (fdiv: rounded towards minus infinity; d < 16384: MI355ENC_ERR_ARG)
 *   U = fdiv(U << 16, d), V likewise;  r2 = ((U >> 8)^2 + (V >> 8)^2) >> 16, q = fdiv(r2 << 16, (w - 1)^2 + (h - 1)^2) (q > 4194304: MI355ENC_ERR_ARG; it keeps U g inside 64 bits)
 *   g = 65536 + ((k1 q) >> 16) + ((k2 ((q q) >> 16)) >> 16);  sx = ((w - 1) 65536 + ((U g) >> 16) + 256) >> 9, sy likewise with h and V
 * and MI355ENC_ERR_ARG for a parameter outside its range or a node outside the mesh's.
 * apply_host: the scalar form of the whole rule on NV12 planes of the visible size w x h (even), no margin */
int mi355enc_warp_coeff(int kind, int f, int16_t c[4]);
int mi355enc_warp_mesh_size(int w, int h, int *nx, int *ny);
int mi355enc_warp_mesh_check(const int32_t *mesh, int nx, int ny);
int mi355enc_warp_build(const mi355enc_warp_params_t *p, int w, int h, int32_t *mesh, size_t cap);
/* host only: how many of the launch's 32 x 32 output tiles (of the coded size) take which of the kernel's two forms, by the test the kernel makes -- staged:
 * the tile's source window, floor(smallest node) - 1 .. floor(largest node) + 2 per axis over the tile's cells, clamped to the picture, fits 64 x 64 luma
 * samples and 36 x 36 chroma pairs of LDS; direct: it does not, and the taps come from global memory.  Both forms give the same picture */
int mi355enc_warp_plan(const int32_t *mesh, int nx, int ny, int w, int h, int *staged, int *direct);
int mi355enc_warp_apply_host(const mi355enc_warp_t *s, const int32_t *mesh, int w, int h, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride,
                             uint8_t *out_y, int out_y_stride, uint8_t *out_uv, int out_uv_stride);
/* set_warp builds the mesh of `p` for the handle's coded visible size; set_warp_mesh takes the caller's (nx, ny must be that size's, every node valid).  A null
 * setting: off.  Every successful set that turns the warp on counts one generation up */
int mi355enc_set_warp(mi355enc_t *h, const mi355enc_warp_t *s, const mi355enc_warp_params_t *p);
int mi355enc_set_warp_mesh(mi355enc_t *h, const mi355enc_warp_t *s, const int32_t *mesh, int nx, int ny);
int mi355enc_get_warp(const mi355enc_t *h, int *on, mi355enc_warp_t *s); /* what was set last (s is untouched when off; either pointer may be NULL) */
/* the generation the last collected picture was warped with, 0 for an unwarped one; MI355ENC_ERR_STATE before the first collect */
int mi355enc_last_warp(mi355enc_t *h, unsigned *generation);
size_t mi355enc_debug_warp_bytes(const mi355enc_t *h); /* device bytes of the warp: 0 until the first warped picture is submitted */
int mi355enc_debug_warp_staging(mi355enc_t *h, int on); /* measurements: 0 -- every tile takes the direct form (the picture is the same); on by default */
/* the launch alone (tests), in the frame of the single-stage entry points (named as the stabiliser's probes are): y / uv are host planes of the coded size (16 mbw x 16 mbh, chroma interleaved),
 * warped in place through `mesh` (the handle's coded visible size's nx x ny); the handle's own setting plays no part */
int mi355enc_warp_probe(mi355enc_t *h, const mi355enc_warp_t *s, const int32_t *mesh, uint8_t *y, uint8_t *uv);
/* A 3D colour LUT: a camera-log-to-Rec.709 transform, a house grade or a film emulation, as shipped in a .cube file, applied to the
 * picture part of the coded surfaces in place -- behind the noise filter (whose history stays in the camera's domain), in front of automatic levels (which
 * measure the graded picture) and the picture controls; mix, layers and text are never touched.  Off by default, and off nothing is allocated, uploaded or
 * launched.  All integers; >> is a floor.
 *   table     N nodes per axis, 2 <= N <= 65; N^3 words R | G << 10 | B << 20, each field 0 .. 1023 (1023 is 1.0); node (r, g, b) is word r + N (g + N b)
 *   per 2 x 2 luma quad and its chroma pair, with the output's matrix (1, 5, 6, 9; unspecified resolved by the picture's size) and range:
 *   1  v = (Y - yoff, Cb - 128, Cr - 128) with the quad's own chroma pair for all four samples; c = clamp((Minv . v + 2^13) >> 14, 0, 4096), Q12,
 *      Minv = floor(M^-1 4096 2^14 + 0.5), M^-1 the inverse from Kr / Kb and the range's scales (219 / 224 with yoff 16, 255 / 255 with yoff 0)
 *   2  per channel p = c (N - 1), i = min(p >> 12, N - 2), f = p - (i << 12) in 0 .. 4096
 *   3  tetrahedral: the fractions in descending order f0 >= f1 >= f2 (ties in the order R, G, B), nodes n0 .. n3 walking from node i one step at a time along
 *      the axes in that order; per channel g = (n0 (4096 - f0) + n1 (f0 - f1) + n2 (f1 - f2) + n3 f2 + 2048) >> 12, ten bits
 *   4  Mf = floor(M / 1023 2^20 + 0.5); Y' = clamp((Mf[0] . g + (yoff << 20) + 2^19) >> 20, 0, 255) per sample; Cb' = clamp((the sum of the four samples'
 *      Mf[1] . g + (128 << 22) + 2^21) >> 22, 0, 255), Cr' likewise
 *   5  out = in + (((graded - in) strength + 128) >> 8) per luma and per chroma sample, strength 0 .. 256 (0: the step is off for that picture)
 *   6  the coded margin: where the picture rectangle reaches the visible picture's right (bottom) edge, a margin sample takes the graded value of its clamped
 *      visible position -- luma the last visible column / row, chroma the last visible pair / row, the corner both -- so the margin is the replica of the graded
 *      picture, as every other step of the input chain leaves it (a quad's chroma comes from its own four samples, so a margin graded as samples would be no
 *      replica, and a margin left alone is the replica of the ungraded picture: a stripe of the camera's picture coded beside the graded one).  A letterbox
 *      border keeps its bytes.  Rule 6 is the handle's and the probe's; mi355enc_lut3d_apply_host grades the rectangle it is given and knows no margin
 * Host only, no device: */
typedef struct {
    int size;     /* N */
    int strength; /* 0 .. 256 */
} mi355enc_lut3d_t;
/* the 18 coefficients and yoff, from exact rationals: Minv row-major (R', G', B' from v), then Mf row-major (Y, Cb, Cr from g), then yoff.  matrix 1, 5, 6, 9 */
int mi355enc_lut3d_coefficients(int matrix, int full_range, int32_t out[19]);
int mi355enc_lut3d_check(const uint32_t *nodes, int N);  /* MI355ENC_ERR_ARG: N outside 2 .. 65, or a node with one of its top two bits set */
int mi355enc_lut3d_identity(int N, uint32_t *nodes);     /* field i of a node: round(i 1023 / (N - 1)) */
/* A .cube text of `len` bytes -> N^3 nodes (cap: the room at nodes in words) and N.  Accepted: TITLE, # comments, blank lines, CR LF line ends, LUT_3D_SIZE,
 * DOMAIN_MIN / DOMAIN_MAX (three numbers: the lo / hi per channel that the rows' values are normalised with; 0 / 1 without), LUT_3D_INPUT_RANGE lo hi.  The
 * rule has no pre-scale of its input, so an input range other than 0 1 is refused rather than folded in.  Refused (MI355ENC_ERR_ARG): LUT_1D_SIZE and any
 * other keyword, a keyword behind the first row, a size outside 2 .. 65 or beyond cap, too few or too many rows, a row that is not three numbers,
 * |value| >= 10^6, hi <= lo.  Numbers are decimals with optional sign, fraction and exponent, read without the C library (no locale) into 64-bit integers in
 * units of 10^-9, further digits truncated; a node's field is clamp(((v - lo) 2046 + (hi - lo)) / (2 (hi - lo)), 0, 1023), the division a floor of
 * non-negative operands (a negative numerator gives 0) */
int mi355enc_lut3d_parse_cube(const char *text, size_t len, uint32_t *nodes, size_t cap, int *N);
/* the rule on host NV12 planes at `stride` (even) with `height` (even) rows of luma, inside rect {x0, x1, y0, y1} (even, inside the planes), in place */
int mi355enc_lut3d_apply_host(const uint32_t *nodes, int N, int strength, int matrix, int full_range, uint8_t *y, uint8_t *uv, int stride, int height, const int rect[4]);
/* which of the kernel's two forms serves N: 0 direct (the nodes gathered from global memory), 1 staged (the table copied into LDS once per workgroup by a grid
 * of persistent workgroups); MI355ENC_ERR_ARG for N outside 2 .. 65.  Both forms give the same picture; decided by measurement (profiles/lut3d_price.md) */
int mi355enc_lut3d_plan(int N);
/* On a handle.  set: at any time and from any thread, no GPU call; the nodes (set->size^3 words, checked) are copied; latched once per input picture at its
 * submit, so pictures in flight keep the table they were submitted with, and the size may change while the stream runs.  NULL: off.  Every successful set
 * that turns it on counts one generation up.  With the step on mi355enc_submit_device never encodes in place: the caller's planes are only read */
int mi355enc_set_lut3d(mi355enc_t *h, const mi355enc_lut3d_t *set, const uint32_t *nodes);
int mi355enc_get_lut3d(const mi355enc_t *h, int *on, mi355enc_lut3d_t *set); /* what was set last (set is untouched when off; either pointer may be NULL) */
/* of the last collected picture: its setting and the generation of its table (zeros for an ungraded one); MI355ENC_ERR_STATE before the first collect */
int mi355enc_last_lut3d(mi355enc_t *h, mi355enc_lut3d_t *set, unsigned *generation);
size_t mi355enc_debug_lut3d_bytes(const mi355enc_t *h); /* device bytes of the step: 0 until the first graded picture is submitted */
/* measurements: the form of the handle's own launches -- -1 the plan's (the default), 0 direct, 1 staged, with which a picture whose table the staged form
 * cannot hold fails its submit (the picture is the same in both forms) */
int mi355enc_debug_lut3d_form(mi355enc_t *h, int form);
/* the launch alone (tests, measurements), in the frame of the single-stage entry points: y / uv are host planes of the coded size (16 mbw x 16 mbh, chroma
 * interleaved), graded in place inside the handle's picture rectangle (rule 6 included) with the handle's output matrix and range; form -1: the plan's, 0 / 1: that form
 * (MI355ENC_ERR_ARG, and nothing launched, for the staged form with an N it cannot hold).  The handle's own setting plays no part */
int mi355enc_lut3d_probe(mi355enc_t *h, const mi355enc_lut3d_t *set, const uint32_t *nodes, uint8_t *y, uint8_t *uv, int form);
/* Region-of-interest quantisation: the application says where the bits go -- a face, a scoreboard, the road ahead -- as up to eight
 * rectangles with a QP offset each, optionally a map of its own, and the encoder quantises every macroblock with the picture's QP moved by its offset.  Off by
 * default, and off nothing is allocated, launched or planned differently.  All integers; / of non-negative operands.
 *   per macroblock m = (mx, my) of the mbw x mbh picture:
 *   1  rectangle k: mx0 = x >> 4, mx1 = (x + w - 1) >> 4 (floors), rows likewise; d = max(mx0 - mx, mx - mx1, my0 - my, my - my1, 0), the Chebyshev distance in
 *      macroblocks; c_k = delta for d = 0, sign(delta) ((|delta| (feather + 1 - d)) / (feather + 1)) for 1 <= d <= feather, 0 beyond.  A rectangle wholly
 *      outside the 16 mbw x 16 mbh picture contributes nothing (feather included) and is no error
 *   2  emphasis wins: e = min(0, min_k c_k), p = max(0, max_k c_k); the rectangle part is e where e < 0, else p
 *   3  the caller's map (optional, mbw mbh values of -12 .. +12): t[m] = clamp(rectangle part + user[m], -12, 12)
 *   4  balance ("move bits, do not add them"): with balance > 0, S = sum t[m] < 0 and N0 = #{m: t[m] = 0} > 0, every macroblock with t[m] = 0 gets
 *      b = min(balance, (-S + N0 / 2) / N0); nothing changes otherwise
 *   5  the map is active iff some t[m] != 0; an inactive map is the same as no map
 *   6  on the device off[m] = clamp(aq[m] + t[m], -12, 12), aq[m] the adaptive-quantisation offset (0 without aq_mode); QP_Y = clamp(qp + off[m], 0, 51).  Two
 *      macroblocks differ by at most 24, inside mb_qp_delta's -26 .. +25 (7.4.5).  Only quantisation and QP_Y change: search, refinement and mode decisions
 *      keep the picture's lambda, and rate control is not told -- it sees the bytes
 * Host only, no device: */
typedef struct {
    int x, y, w, h; /* luma samples of the coded picture's visible area; may reach beyond it (clipped).  |x|, |y| <= 65536, 1 <= w, h <= 65536 */
    int delta;      /* -12 .. +12, not 0: the QP offset inside (negative: finer) */
    int feather;    /* 0 .. 8: macroblocks over which the offset ramps to 0 outside */
} mi355enc_roi_rect_t;
typedef struct {
    int n_rects;    /* 0 .. 8 */
    mi355enc_roi_rect_t rect[8];
    int balance;    /* 0: off; 1 .. 12: the cap of the background offset of rule 4 */
} mi355enc_roi_t;
void mi355enc_roi_default(mi355enc_roi_t *cfg);      /* no rectangle, no balance */
int mi355enc_roi_check(const mi355enc_roi_t *cfg);   /* MI355ENC_ERR_ARG for any field outside its range */
/* rules 1 .. 5 into out[mbw mbh] (1 <= mbw, mbh <= 512); cfg NULL: no rectangle and no balance; user NULL: none (a value outside -12 .. +12: MI355ENC_ERR_ARG,
 * out untouched).  *active: rule 5; *background: the b rule 4 applied (0: none).  Either may be NULL */
int mi355enc_roi_map(const mi355enc_roi_t *cfg, const int8_t *user, int mbw, int mbh, int8_t *out, int *active, int *background);
/* the element's string form: rectangles "x,y,w,h,delta[,feather]" joined by ';', decimal integers, blanks around them allowed; an empty string: no rectangle.
 * cfg->balance stays.  MI355ENC_ERR_ARG (cfg untouched) for anything else, a ninth rectangle or a value mi355enc_roi_check refuses */
int mi355enc_roi_parse(const char *text, mi355enc_roi_t *cfg);
/* On a handle.  set: at any time and from any thread, with pictures in flight, no GPU call: the map t is computed here (cfg and user as for mi355enc_roi_map;
 * both NULL: off) and latched by the next submitted picture; pictures already submitted keep the map they were submitted with.  A picture with an active map is
 * planned exactly as an aq_mode 1 picture is; one without is planned and coded as if the call had never been made */
int mi355enc_set_roi(mi355enc_t *h, const mi355enc_roi_t *cfg, const int8_t *user_map);
int mi355enc_get_roi(const mi355enc_t *h, int *on, mi355enc_roi_t *cfg); /* what was set last (the configuration: the caller's map is not kept apart; either pointer may be NULL) */
/* of the last collected picture: whether its map was active, the background offset rule 4 gave it and the sum of its t (zeros for a picture without);
 * MI355ENC_ERR_STATE before the first collect */
int mi355enc_last_roi(mi355enc_t *h, int *active, int *background, int *sum);
size_t mi355enc_debug_roi_bytes(const mi355enc_t *h); /* device bytes the feature holds: 0 until the first picture with an active map is submitted (and always with aq_mode, whose offsets it shares) */
/* parity tests (named as the other features' probes are; both in the frame of the single-stage entry points).  probe_set_map: a setting of the handle like
 * mi355enc_stage_set_slice_rows, no device work -- the single-stage entry points then quantise with this map of mbw mbh offsets (-12 .. +12; copied) instead
 * of one QP per picture; NULL: as before.  probe_offsets: the offsets a picture of the stream would be coded with under the map set last (mi355enc_set_roi)
 * -- aq_kernel on the coded-size host luma src_y if aq_mode, then the compose launch -- into off_out[mbw mbh] */
int mi355enc_roi_probe_set_map(mi355enc_t *h, const int8_t *map);
int mi355enc_roi_probe_offsets(mi355enc_t *h, const uint8_t *src_y, int8_t *off_out);
/* Privacy masks: up to eight regions of the coded picture are made unreadable -- filled, pixelated or blurred -- on the device, in front
 * of the image layers and the text, so that everything that leaves the handle shows them: the access units, the "coded picture" stills and the quality
 * metrics' source.  Off by default, and off nothing is allocated or launched.  All integers; / of non-negative operands.  A region is {x, y, w, h, mode, param,
 * shape, colour} in luma samples of the visible coded picture (cfg.width x cfg.height: after scaling, geometry, orientation, stabilisation and warp; a letterbox
 * border is just samples here).
 *   1  even rectangle: x0 = x & ~1, x1 = (x + w + 1) & ~1, rows likewise (floors): W2 x H2 = (x1 - x0) x (y1 - y0), the region's own size.  Its intersection
 *      with the visible picture is the clipped rectangle C.  A region with an empty C contributes nothing and is no error
 *   2  membership, per 2 x 2 luma quad, so that luma and chroma agree.  Rectangle: every quad of C.  Ellipse: for the quad at region-local (qx, qy) let
 *      dx = 2 (2 qx + 1) - W2 and dy = 2 (2 qy + 1) - H2; the quad is inside iff dx^2 H2^2 + dy^2 W2^2 <= W2^2 H2^2, in 64 bits -- the unclipped size, so an ellipse
 *      half off the picture stays that ellipse
 *   3  sources: every region computes from the picture as it stood before any region was applied; a sample takes the value of the lowest-indexed region whose
 *      shape contains it; samples in no shape keep their bytes
 *   4  fill: the colour is 0xRRGGBB, converted with the output's matrix and range by the ten words c of mi355enc_csc_coefficients:
 *      Y = clip255((c0 R + c1 G + c2 B + (c9 << 16) + 32768) >> 16), Cb = clip255((c3 R + c4 G + c5 B + (128 << 16) + 32768) >> 16), Cr with c6 .. c8 (>> floors)
 *   5  pixelate: param is the cell size c, even, 4 .. 64.  Cells tile from (x0, y0) of the even rectangle, so the grid moves with the region.  A cell's luma
 *      value is (sum + n / 2) / n over its samples inside C, n that count (edge and clipped cells are smaller); chroma likewise, per component, over the cell's
 *      c / 2 chroma footprint inside C.  Means are taken over the rectangle's cell even under an ellipse: only membership is elliptical
 *   6  blur: param is the radius r, 1 .. 32.  On C a 1-D box mean runs horizontally, then vertically, then both again (H, V, H, V: a triangle response), rounded
 *      to 8 bits after every pass: out = (sum of 2r + 1 samples + r) / (2r + 1), neighbour positions clamped to C -- nothing outside the clipped rectangle is
 *      read, so a region's result depends only on its own contents.  Chroma: radius (r + 1) >> 1, per component, on C's chroma rectangle
 *   7  margins: where a region changes the last visible column, row or corner, the coded-size margin beside it is stored as the replica of the new values
 *      (chroma: last pair and row).  Margin samples are never read
 * Host only, no device: */
typedef struct {
    int x, y, w, h;  /* luma samples; may reach beyond the picture (clipped).  |x|, |y| <= 16384, 1 <= w, h <= 16384 */
    int mode;        /* 1 fill, 2 pixelate, 3 blur */
    int param;       /* fill: 0; pixelate: the cell size, even, 4 .. 64; blur: the radius 1 .. 32 */
    int shape;       /* 0 rectangle, 1 the ellipse inscribed in it */
    unsigned colour; /* fill: 0xRRGGBB (at most 0xFFFFFF in every mode) */
} mi355enc_mask_region_t;
typedef struct {
    int n;           /* 0 .. 8 */
    mi355enc_mask_region_t region[8];
} mi355enc_mask_t;
int mi355enc_mask_check(const mi355enc_mask_t *cfg); /* MI355ENC_ERR_ARG for any field outside its range */
/* the element's string form: regions "x,y,w,h,mode,param[,shape]" joined by ';', decimal integers, blanks around them allowed; an empty string: no region.
 * Every region takes `colour`.  MI355ENC_ERR_ARG (cfg untouched) for anything else, a ninth region or a value mi355enc_mask_check refuses */
int mi355enc_mask_parse(const char *text, unsigned colour, mi355enc_mask_t *cfg);
/* rules 1 .. 6, the scalar way, in place on planes of exactly the visible size w x h (even, 2 .. 16384; y: h rows of w, uv: h / 2 rows of w, interleaved);
 * coef: the ten words of mi355enc_csc_coefficients for rule 4.  MI355ENC_ERR_NOMEM where its own scratch cannot be had */
int mi355enc_mask_apply_host(const mi355enc_mask_t *cfg, const int32_t coef[10], int w, int h, uint8_t *y, uint8_t *uv);
/* parts of the rule on their own, for tests: rule 2 for the quad at region-local (qx, qy) of a W2 x H2 region (1 inside, 0 outside; MI355ENC_ERR_ARG for sizes
 * that are not even and 2 .. 32770 or a quad outside 0 .. W2 / 2 - 1, 0 .. H2 / 2 - 1); rule 6's rounded mean of `sum` over 2r + 1 samples as the kernels and
 * mi355enc_mask_apply_host compute it, by a reciprocal (MI355ENC_ERR_ARG for r outside 1 .. 32 or a sum outside 0 .. 255 (2r + 1)); rule 4 into ycc[3] */
int mi355enc_mask_ellipse(int W2, int H2, int qx, int qy);
int mi355enc_mask_mean(int sum, int r);
int mi355enc_mask_colour(unsigned colour, const int32_t coef[10], uint8_t ycc[3]);
/* On a handle.  set: at any time and from any thread, with pictures in flight, no GPU call; cfg NULL or n = 0: off.  The configuration is latched by every
 * picture submitted from then on -- with frame-rate conversion by every output picture, each masked afresh -- and pictures already submitted keep theirs.  A
 * refused configuration leaves the handle's as it was.  While a picture carries an active mask, mi355enc_submit_device never codes from the caller's memory */
int mi355enc_set_mask(mi355enc_t *h, const mi355enc_mask_t *cfg);
int mi355enc_get_mask(const mi355enc_t *h, int *on, mi355enc_mask_t *cfg); /* what was set last (either pointer may be NULL; cfg: n = 0 when off) */
/* of the last collected picture: the configuration it carried (n = 0: none) and the count of sets it belongs to (0: none); MI355ENC_ERR_STATE before the first collect */
int mi355enc_last_mask(mi355enc_t *h, mi355enc_mask_t *cfg, unsigned *generation);
size_t mi355enc_debug_mask_bytes(const mi355enc_t *h); /* device bytes the feature holds (a result surface and two ping-pong planes): 0 until the first masked picture */
/* parity tests: the launches of a masked picture, on a host picture of the coded size (y: 16 mbh rows of 16 mbw, uv: 8 mbh rows of 16 mbw interleaved, margins
 * as the caller made them) with the handle's output matrix and range, in place; the handle's own setting plays no part */
int mi355enc_mask_probe(mi355enc_t *h, const mi355enc_mask_t *cfg, uint8_t *y, uint8_t *uv);
/* like mi355enc_submit, from host memory in `fmt`; planes[]/strides[]: as many entries as the format has planes */
int mi355enc_submit_fmt(mi355enc_t *h, int fmt, const uint8_t *const planes[3], const int strides[3], int64_t pts, int force_idr);
/* conversion stage alone (tests): writes the coded-size NV12 surfaces (16*mbw x 16*mbh luma, then interleaved chroma) */
int mi355enc_stage_csc(mi355enc_t *h, int fmt, const uint8_t *const planes[3], const int strides[3], uint8_t *out_y, uint8_t *out_uv);
/* ... on planes that lie in this GPU's memory, into device memory (tests of unaligned planes, probes: no transfer, one launch): the planes as they are --
 * any address, any stride -- of the coded visible size, into coded-size surfaces of stride 16 * mb_width at 8-byte aligned addresses.  Every format but
 * NV12 (which has no conversion); ignores mi355enc_set_input_size.  Returns when the launch has completed. */
int mi355enc_stage_csc_device(mi355enc_t *h, int fmt, const void *const d_planes[3], const int strides[3], void *d_out_y, void *d_out_uv);
int mi355enc_submit_device(mi355enc_t *h, const void *d_y, int y_stride, const void *d_uv,
                           int uv_stride, int64_t pts, int force_idr);
/* Downscaling on the way in.  The pictures submitted from now on are in_w x in_h; the device scales them to the
 * coded size cfg.width x cfg.height with a separable Catmull-Rom filter (integer arithmetic, tables built once here), in the launch
 * that would otherwise copy or convert them.  Per axis cfg size <= in <= 8 * cfg size, even sizes (MI355ENC_ERR_ARG otherwise); the cfg
 * size itself returns to the unscaled path.  Valid only before the first submit (MI355ENC_ERR_STATE after it).  A scale that changes the
 * aspect ratio writes the sample aspect ratio into the SPS VUI (aspect_ratio_idc 255). */
int mi355enc_set_input_size(mi355enc_t *h, int in_w, int in_h);
/* scale stage alone (tests): planes of the input size in `fmt` (NV12: Y, UV) -> the coded-size NV12 surfaces, like mi355enc_stage_csc;
 * MI355ENC_ERR_STATE before mi355enc_set_input_size */
int mi355enc_stage_scale(mi355enc_t *h, int fmt, const uint8_t *const planes[3], const int strides[3], uint8_t *out_y, uint8_t *out_uv);
/* The scale tables (host only, no device needed).  kind: MI355ENC_SCALE_LUMA (either axis: `in` -> `out` samples), MI355ENC_SCALE_CHROMA_V
 * (4:2:0 chroma rows: in / 2 -> out / 2), MI355ENC_SCALE_CHROMA_H (chroma columns, cosited: in / 2 -> out / 2), MI355ENC_SCALE_CHROMA_V422
 * (4:2:2 chroma rows: in -> out / 2); in and out are luma sizes of the axis.  Entry i: first[i], the first source index of its taps (not
 * clamped), and coef[i * taps + k], k < *taps, 14-bit weights that sum to 16384.  Returns the number of entries (with first and coef NULL:
 * only that and *taps), MI355ENC_ERR_ARG for upscaling, a ratio above 8 or odd sizes. */
enum { MI355ENC_SCALE_LUMA = 0, MI355ENC_SCALE_CHROMA_V = 1, MI355ENC_SCALE_CHROMA_H = 2, MI355ENC_SCALE_CHROMA_V422 = 3 };
int mi355enc_scale_table(int in, int out, int kind, int *first, int16_t *coef, size_t coef_cap, int *taps);
/* ---- input geometry: crop, upscale, letterbox: what `videocrop ! videoscale add-borders=true ! videobox` do in front of an encoder ----
 * The crop rectangle (crop_*) of the submitted in_w x in_h picture is resampled into the destination rectangle (dst_*) of the pre-orientation target
 * (cfg.width x cfg.height, exchanged under a transposing orientation); everything else of the target takes the border colour.  The filter is section 10's,
 * with the unstretched kernel where an axis is scaled up; a tap outside the crop rectangle is clamped to the rectangle's edge, and nothing outside it is read.
 * Valid: all numbers even and >= 0, rectangle sizes >= 2, both rectangles inside their pictures, in_w, in_h <= 8192, per axis crop <= 8 dst and dst <= 8 crop,
 * border components 0 .. 255.  The SPS carries the exact sample aspect ratio (crop_w dst_h) : (crop_h dst_w) (exchanged under a transposing orientation, absent
 * when 1:1) -- or, with MI355ENC_GEOM_KEEP_SAR, none: the headers of an unscaled stream.
 * mi355enc_set_input_geometry: before the first submit only (MI355ENC_ERR_STATE after it); MI355ENC_ERR_ARG for a geometry that is not valid (the handle stays as
 * it was).  It replaces an earlier mi355enc_set_input_size and is replaced by a later one; either order with mi355enc_set_orientation gives the same handle.
 * mi355enc_set_crop: between submits, on a handle with a geometry (MI355ENC_ERR_STATE without): the crop of the pictures submitted from now on; input size,
 * destination and border stay.  Pictures in flight keep theirs.  Host work only: the tables are rebuilt and travel to the device with the next submit, in stream
 * order; nothing is allocated on the device, no stream is waited for.  MI355ENC_ERR_ARG for a crop outside the rule, and -- without MI355ENC_GEOM_KEEP_SAR -- for
 * one whose crop_w : crop_h differs from the geometry's (the SPS would have to change). */
enum { MI355ENC_GEOM_KEEP_SAR = 1 };
typedef struct {
    int in_w, in_h;                         /* the submitted pictures */
    int crop_x, crop_y, crop_w, crop_h;     /* inside them */
    int dst_x, dst_y, dst_w, dst_h;         /* inside the pre-orientation target */
    int border_y, border_cb, border_cr;     /* (16, 128, 128): black */
    unsigned flags;                         /* MI355ENC_GEOM_* */
} mi355enc_geometry_t;
int mi355enc_set_input_geometry(mi355enc_t *h, const mi355enc_geometry_t *g);
int mi355enc_get_input_geometry(const mi355enc_t *h, mi355enc_geometry_t *g); /* MI355ENC_ERR_STATE: the handle has none */
int mi355enc_set_crop(mi355enc_t *h, int crop_x, int crop_y, int crop_w, int crop_h);
/* host only: mi355enc_scale_table's counterpart with a crop offset and upscaling: `crop` luma samples from luma offset crop_off on -> `dst` luma samples
 * of the axis; first[] counts in the whole source plane (chroma kinds: in chroma samples / rows).  With crop_off 0 and crop >= dst it is
 * mi355enc_scale_table's table, entry for entry.  MI355ENC_ERR_ARG for odd or negative values, sizes below 2 and a ratio beyond 8 either way. */
int mi355enc_geometry_table(int crop_off, int crop, int dst, int kind, int *first, int16_t *coef, size_t coef_cap, int *taps);
/* host only: the largest rectangle of src_w : src_h inside tw x th (even), centred: the constrained axis is filled, the other one is 2 round(other / 2)
 * (half up; at least 2, at most the target's), dx = ((tw - dw) / 4) 2 and dy likewise */
int mi355enc_fit_rect(int src_w, int src_h, int tw, int th, int *dx, int *dy, int *dw, int *dh);
/* host only: the validity rule against a pre-orientation target tw x th (MI355ENC_OK or MI355ENC_ERR_ARG), and the sample aspect ratio a geometry puts into
 * the SPS (0:0: none), with its terms exchanged for a transposing orientation */
int mi355enc_geometry_check(const mi355enc_geometry_t *g, int tw, int th);
int mi355enc_geometry_sar(const mi355enc_geometry_t *g, int transposed, int *sar_w, int *sar_h);
/* the launch alone (tests), like mi355enc_stage_scale; MI355ENC_ERR_STATE before mi355enc_set_input_geometry */
int mi355enc_stage_geometry(mi355enc_t *h, int fmt, const uint8_t *const planes[3], const int strides[3], uint8_t *out_y, uint8_t *out_uv);
/* ---- MJPEG input ----------------------------------------------
 * A baseline JPEG picture goes straight in: the host parses the markers and runs the serial Huffman decode, the device does dequantisation,
 * the 8x8 inverse DCT (IJG's accurate integer one: what libjpeg's ISLOW produces), level shift, clamp and the step from 4:2:2 / 4:4:4 to
 * 4:2:0, into the coded NV12 surfaces.  Accepted: SOF0 / SOF1, 8 bit, Huffman coded, one interleaved scan; one component, or three with
 * chroma sampling 1x1 and luma sampling 2x2, 2x1 or 1x1; 8-bit quantisation tables; DRI / RSTn; APPn / COM skipped; a picture without DHT
 * uses the typical tables of T.81 Annex K.3.  Everything else, and every picture whose data does not decode, is MI355ENC_ERR_ARG. */
typedef struct { int width, height, components, hs, vs, restart_interval, has_dht; } mi355enc_jpeg_info_t;
/* host only: what the markers in front of the scan say (hs, vs: the luma sampling factors; 1, 1 for a single component) */
int mi355enc_jpeg_info(const uint8_t *data, size_t len, mi355enc_jpeg_info_t *info);
/* host only: the entropy decode.  coef (coef_cap int16 of room, MI355ENC_ERR_OVERFLOW when that is too little): per component, the blocks of
 * its MCU-padded plane in raster order, each 64 int16 in natural (row-major) order, quantisation not applied.  qt[c]: component c's
 * quantisation table in natural order.  info may be NULL. */
int mi355enc_jpeg_entropy_decode(const uint8_t *data, size_t len, int16_t *coef, size_t coef_cap, uint16_t qt[3][64], mi355enc_jpeg_info_t *info);
/* like mi355enc_submit_fmt, from a JPEG picture whose size is the handle's input size (even width and height).  The bytes are the caller's
 * again when the call returns.  A refused or corrupt picture (MI355ENC_ERR_ARG) leaves the handle exactly as it was: nothing is enqueued. */
int mi355enc_submit_jpeg(mi355enc_t *h, const uint8_t *data, size_t len, int64_t pts, int force_idr);
/* decode stage alone (tests): writes the coded-size NV12 surfaces, like mi355enc_stage_csc */
int mi355enc_stage_jpeg(mi355enc_t *h, const uint8_t *data, size_t len, uint8_t *out_y, uint8_t *out_uv);
/* ... and the kernel alone, on coefficients the caller made up: a picture of the handle's input size with luma sampling hs x vs and
 * `components` components, coef and qt laid out as mi355enc_jpeg_entropy_decode writes them */
int mi355enc_stage_jpeg_blocks(mi355enc_t *h, int hs, int vs, int components, const int16_t *coef, const uint16_t qt[3][64], uint8_t *out_y, uint8_t *out_uv);

/* ---- orientation of the input picture on the device: what `videoflip` does in front of an encoder ----
 * The eight methods of GstVideoOrientationMethod, as a permutation of samples: luma as a plane of bytes, chroma as a plane of (Cb, Cr) pairs of half the
 * size (a pair is never split; the half-sample shift in chroma siting that a rotation implies is ignored, as videoflip ignores it).
 * cfg.width x cfg.height stays the coded, visible size: that of the ORIENTED picture.  With a transposing method (90r, 90l, ul-lr, ur-ll) the pictures
 * submitted are cfg.height x cfg.width, or -- with mi355enc_set_input_size(in_w, in_h) -- in_w x in_h, scaled to cfg.height x cfg.width and then
 * oriented; the per-axis limits of mi355enc_set_input_size hold against that pre-orientation target, and the sample aspect ratio in the SPS is the
 * scaler's with its two terms exchanged.  A JPEG picture has the pre-orientation input size.  Orientation runs after decode / conversion / scaling and
 * before the text overlay (the text stays upright); the quality metrics measure against the oriented source.
 * mi355enc_set_orientation: before the first submit only (MI355ENC_ERR_STATE after it); MI355ENC_ERR_ARG outside 0 .. 7, and for a method whose
 * pre-orientation target the input size set before does not fit (the handle stays as it was).  It may be called before or after
 * mi355enc_set_input_size: the handle ends up the same.  Identity (the default) is today's input path, untouched. */
enum { MI355ENC_ORIENT_IDENTITY = 0, MI355ENC_ORIENT_90R, MI355ENC_ORIENT_180, MI355ENC_ORIENT_90L,
       MI355ENC_ORIENT_HORIZ, MI355ENC_ORIENT_VERT, MI355ENC_ORIENT_UL_LR, MI355ENC_ORIENT_UR_LL };
int mi355enc_set_orientation(mi355enc_t *h, int method);
int mi355enc_get_orientation(const mi355enc_t *h);
/* host only: size of the oriented picture, and for an output sample the input sample it comes from */
int mi355enc_orient_size(int method, int in_w, int in_h, int *out_w, int *out_h);
int mi355enc_orient_source(int method, int out_w, int out_h, int x, int y, int *sx, int *sy);
/* kernel alone (tests): NV12 host planes of the pre-orientation size (cfg.height x cfg.width for a transposing method, else cfg.width x cfg.height) at
 * the given strides -> coded-size surfaces, stride 16 * mb_width.  Methods 1 .. 7; ignores the handle's own method and input size. */
int mi355enc_stage_orient(mi355enc_t *h, int method, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride,
                          uint8_t *out_y, uint8_t *out_uv);
/* ... on planes in this GPU's memory, any address and stride, into device surfaces of stride 16 * mb_width; touches nothing of the encoder's.
 * Returns when the launch has completed. */
int mi355enc_stage_orient_device(mi355enc_t *h, int method, const void *d_y, int y_stride, const void *d_uv, int uv_stride,
                                 void *d_out_y, void *d_out_uv);
/* development: bytes of device memory the handle holds for pre-orientation pictures (0 until an oriented picture is submitted; always 0 with identity) */
size_t mi355enc_debug_orient_bytes(const mi355enc_t *h);
int mi355enc_pending(const mi355enc_t *h);
int mi355enc_collect(mi355enc_t *h, uint8_t *out, size_t out_cap, size_t *out_len, int *is_keyframe,
                     int64_t *pts, int *qp);

/* Fault injection (tests): behaves as if a kernel's bounded wait on the device had just run out with error word `code` (> 0): waits
 * for the device to drain, then sets the sticky word every waiting kernel reports through.  The pictures submitted next come back from
 * collect() through the recovery path: re-encoded in stream order, starting with an IDR picture; stats.recoveries counts it. */
int mi355enc_debug_trip_wait(mi355enc_t *h, unsigned code);

/* Long-run state (tests; DESIGN.md "State that outlives a picture"): the per-handle picture epoch, the four counts the kernels compare on the device
 * (macroblocks per row of all gated fused P stages; workgroups of all band-deblocking launches; intra macroblock rows of all fused launches; rows of
 * all QP_Y chains) and the two counts behind idr_pic_id and frame_num.  mi355enc_debug_set_counters puts a handle where a long run would have put
 * it: MI355ENC_ERR_STATE unless nothing is pending; it waits for every stream of the handle, then sets the host-side values AND the device-side words
 * they are compared with to the same numbers.  A field whose bit in `keep` is set (bit i: field i in the order below) is not touched.  The next picture
 * is stamped epoch + 1 (0 is skipped).  Everything tagged with an epoch -- the strips and progress words on the device, the band-done words and the
 * epoch the host remembers for each reconstruction buffer -- keeps what the last picture left: exactly a handle that has been running.
 * Contract: after the call the handle behaves like one whose pictures so far had brought each value to the given number. */
typedef struct { uint32_t epoch, pmb_rows_total, db_started_total, ip_done_total, qpc_total, idr_count, frames_since_idr, keep; } mi355enc_counters_t;
int mi355enc_debug_get_counters(mi355enc_t *h, mi355enc_counters_t *out); /* keep: 0 */
int mi355enc_debug_set_counters(mi355enc_t *h, const mi355enc_counters_t *in);

int mi355enc_get_stats(mi355enc_t *h, mi355enc_stats_t *st);
void mi355enc_reset_stats(mi355enc_t *h);

/* ---- quality metrics of the coded pictures, computed on the device ----
 * Source against deblocked reconstruction, both as the coding kernels see them: NV12 at the coded size, the source AFTER conversion, scaling
 * and padding (with mi355enc_set_input_size or a format other than NV12 the comparison is against the converted / scaled surface, not the
 * caller's picture).  Only the visible cfg.width x cfg.height samples count (chroma: width / 2 x height / 2 per component), never the margin
 * of the coded size.
 *   sse[c]        sum of (src - rec)^2 over the visible samples of Y, Cb, Cr: exact integers.
 *   SSIM of luma  x264's integer form: 4x4 blocks anchored at (0, 0), width / 4 x height / 4 of them (a remainder of two columns or rows is
 *                 left out); a window is a 2x2 group of blocks at every block position; per window, with s1 = sum src, s2 = sum rec,
 *                 ss = sum src^2 + sum rec^2, s12 = sum src rec over its 64 samples, C1 = 416, C2 = 235963:
 *                 q = rint((2 s1 s2 + C1)(2 (64 s12 - s1 s2) + C2) / ((s1^2 + s2^2 + C1)(64 ss - s1^2 - s2^2 + C2)) * 2^30), the integers
 *                 exact, the two products and the quotient one IEEE binary64 rounding each, round-half-even: bit-reproducible.
 *                 ssim_sum = sum of q, ssim_windows = their number.
 *   derived on the host: psnr[c] = 10 log10(255^2 samples[c] / sse[c]) (100.0 when sse[c] is 0), ssim = ssim_sum / (ssim_windows * 2^30). */
typedef struct {
    uint64_t sse[3];          /* Y, Cb, Cr over the visible samples */
    uint64_t samples[3];
    int64_t  ssim_sum;        /* sum of rint(ssim_window * 2^30)    */
    uint64_t ssim_windows;
    double   psnr[3], ssim;   /* derived on the host                */
    int64_t  pts;
    uint64_t pictures;        /* mi355enc_quality_totals only       */
} mi355enc_quality_t;
/* Off by default; valid only before the first submit (MI355ENC_ERR_STATE after it).  Off: nothing is allocated, launched or waited for.  On: one more
 * launch per picture behind its deblocking launch, and collect() of a picture returns only when that picture's metrics have landed.  The access
 * units are byte for byte the same either way.  A picture re-encoded by a recovery reports the metrics of the re-encode; all-skip pictures are
 * measured against the reference they repeat. */
int mi355enc_set_quality_metrics(mi355enc_t *h, int on);
/* the metrics of the last collected picture; MI355ENC_ERR_STATE with metrics off or before the first collect */
int mi355enc_last_quality(mi355enc_t *h, mi355enc_quality_t *q);
/* integer sums over all pictures collected since open or mi355enc_reset_stats (`pictures` of them; pts: the last one's); psnr[] and ssim are
 * derived from the summed integers (global PSNR, mean SSIM).  MI355ENC_ERR_STATE with metrics off. */
int mi355enc_quality_totals(mi355enc_t *h, mi355enc_quality_t *q);
/* The kernel alone (tests): host planes of the coded size, stride 16 * mb_width; the visible size is the handle's.  Works with metrics off.  Like
 * every single-stage call it overwrites the encoder's surfaces: the next picture submitted is coded as an IDR picture. */
int mi355enc_stage_quality(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, const uint8_t *rec_y, const uint8_t *rec_uv, mi355enc_quality_t *q);
/* ... on planes that already lie in this GPU's memory: any address; the source at any stride >= width (an address or stride that is not a multiple
 * of four takes the kernel's byte-wise path), the reconstruction at stride 16 * mb_width.  Touches nothing of the encoder's. */
int mi355enc_stage_quality_device(mi355enc_t *h, const void *d_src_y, const void *d_src_uv, int src_stride,
                                  const void *d_rec_y, const void *d_rec_uv, mi355enc_quality_t *q);

/* ---- text overlay ---------------------------------------------
 * A few lines of text (the reference's on-screen statistics line) drawn into every submitted picture on the GPU, in place of a `textoverlay`
 * element in front of the encoder: a built-in 8 x 16 monospace bitmap font (printable ASCII; any other byte but '\n' draws as '?'; '\n'
 * starts a new line; at most 255 bytes are used; no markup), white text with a black outline, optionally on a shaded box.  The text is drawn
 * into the NV12 picture of the coded visible size -- after conversion and scaling, before the padding to whole macroblocks -- so the stream is
 * byte for byte that of the same pictures with the text already in them.  Off (no text, or ""): nothing is allocated or launched. */
typedef struct { int halign, valign;      /* 0 left/top, 1 centre, 2 right/bottom */
                 int xpad, ypad;          /* luma samples, >= 0                    */
                 int scale;               /* 0 auto, 1..8                          */
                 int shaded_background; } mi355enc_overlay_style_t;
#define MI355ENC_OVERLAY_MAX_TEXT 255
void mi355enc_overlay_default_style(mi355enc_overlay_style_t *st);     /* right, top, 16, 16, auto, 0 */
int  mi355enc_set_overlay_style(mi355enc_t *h, const mi355enc_overlay_style_t *st); /* ERR_ARG out of range; any time, latched per picture */
int  mi355enc_set_overlay_text(mi355enc_t *h, const char *text);       /* NULL or "" : off; thread-safe; no GPU call */
int  mi355enc_last_overlay(mi355enc_t *h, char *buf, size_t cap);      /* text drawn into the last collected picture; returns its length, ERR_STATE before the first collect */
int  mi355enc_overlay_glyph(int ch, uint8_t rows[16]);                 /* host only: the font, MSB = left pixel; ERR_ARG outside 0x20..0x7E */
int  mi355enc_stage_overlay(mi355enc_t *h, const char *text, const mi355enc_overlay_style_t *st,
                            uint8_t *y, uint8_t *uv);                  /* kernel alone (tests): coded-size host planes, stride 16*mbw, in place */
/* (mi355enc_last_overlay: the text is cut to cap - 1 bytes and always terminated; the length returned is that of the whole text.
 * mi355enc_set_overlay_text and mi355enc_set_overlay_style may be called from any thread while another one submits: a picture carries exactly
 * one of the texts that were set.  With a text set, mi355enc_submit_device copies the caller's planes: they are never written.) */

/* ---- image layers ----------------------------------------------
 * Up to MI355ENC_IMAGE_LAYERS images with straight (not premultiplied) alpha -- a logo, a watermark, a scoreboard bitmap -- blended into every
 * submitted picture on the GPU, in place of a `gdkpixbufoverlay` in front of the encoder.  A layer is drawn 1:1 (never scaled) with its top-left
 * pixel at (x, y) of the coded visible picture, luma samples, any integer in -16384 .. 16384; what falls outside the picture is clipped.  Layers
 * are blended in index order, after conversion, scaling and orientation (the image stays upright) and before the text overlay (text is on top) and
 * the padding to whole macroblocks: the stream is byte for byte that of the same pictures with the images already in them.  fmt: one of the four
 * 4-byte orders, the byte they call X being A -- MI355ENC_FMT_BGRX = BGRA, RGBX = RGBA, XRGB = ARGB, XBGR = ABGR.  The colour is converted with the
 * matrix and range RGB input is converted with (the colorimetry setter's rule); a matrix code RGB input refuses makes the submit of a picture with an
 * active layer fail with MI355ENC_ERR_ARG.  opacity 0 .. 256 scales the image's alpha: a = (A * opacity + 128) >> 8.  With no layer ever set nothing
 * is allocated or launched. */
#define MI355ENC_IMAGE_LAYERS 4
#define MI355ENC_IMAGE_MAX_DIM 4096
typedef struct { int fmt; const uint8_t *pixels; int w, h, stride;   /* stride in bytes, >= 4 w */
                 int x, y, opacity; } mi355enc_image_layer_t;
typedef struct { int w, h, x, y, opacity; uint32_t serial; } mi355enc_image_info_t;
/* img NULL or pixels NULL: the layer is off.  Copies the pixels; thread-safe against a running submit; no GPU call; any time.  Every successful call
 * on a layer adds one to that layer's serial.  ERR_ARG (the handle stays as it was): no handle, a layer outside 0 .. 3, a fmt outside the four orders,
 * sizes outside 1 .. 4096, stride < 4 w, a place outside -16384 .. 16384, an opacity outside 0 .. 256. */
int mi355enc_set_image(mi355enc_t *h, int layer, const mi355enc_image_layer_t *img);
/* place and opacity of a layer's image: any time, latched per picture; ERR_STATE on a layer that is off */
int mi355enc_set_image_place(mi355enc_t *h, int layer, int x, int y, int opacity);
/* what was blended into the last collected picture for one layer; serial 0 and w = h = 0: nothing */
int mi355enc_last_image(mi355enc_t *h, int layer, mi355enc_image_info_t *info);
/* the kernels alone (tests): coded-size host planes, stride 16*mbw, in place; layers 0 .. n - 1, n <= 4 (an entry without pixels is skipped);
 * ERR_STATE with pictures pending */
int mi355enc_stage_image(mi355enc_t *h, const mi355enc_image_layer_t *layers, int n, uint8_t *y, uint8_t *uv);
size_t mi355enc_debug_image_bytes(const mi355enc_t *h); /* device memory held for images: 0 until a picture with an active layer is submitted */
/* host only: Y', Cb, Cr of one colour as the layers use it; ERR_ARG for a matrix outside 1, 5, 6, 9, a range outside 0, 1 or a component outside 0 .. 255 */
int mi355enc_image_pixel(int matrix, int full_range, int r, int g, int b, uint8_t ycbcr[3]);
/* host only: a Netpbm PAM (P7) file, TUPLTYPE RGB_ALPHA with DEPTH 4 or RGB with DEPTH 3 (alpha 255), MAXVAL 255, sizes 1 .. 4096, as RGBA into
 * rgba (cap bytes of room).  rgba NULL: only *w and *h.  ERR_OVERFLOW: cap is too small; ERR_ARG: anything else.  (PNG would need an inflate: out of scope.) */
int mi355enc_image_load_pam(const uint8_t *data, size_t len, int *w, int *h, uint8_t *rgba, size_t cap);
/* ---- JPEG stills of the running stream --------------------------
 * A still is a baseline JFIF JPEG (SOF0, 8 bit, Y 2x2 + Cb + Cr, one interleaved scan, the typical Huffman tables of T.81 Annex K.3, no restart markers) of
 * one picture of the stream, taken while the stream runs: one more launch in that picture's pipeline leaves the quantised levels in pinned host memory, and
 * the Huffman coding runs in the thread that takes the still.  The access units are byte for byte those of the stream without stills.
 *   what     0: the coded source -- what the coding kernels read for the picture, after conversion, scaling, geometry, orientation, image layers and text;
 *            1: the deblocked reconstruction -- what a decoder shows.  Only the visible width x height samples are used.
 *   reduce   s = 1, 2, 4 or 8: the still is ceil(width / s) x ceil(height / s); a sample is the rounded mean of its s x s source samples, coordinates clamped
 *            to the picture; chroma likewise from the width / 2 x height / 2 planes into ceil(ow / 2) x ceil(oh / 2).
 *   quality  1 .. 100, libjpeg's scale of the Annex K.1 tables.
 * The arithmetic is libjpeg's accurate integer path (jfdctint and its quantiser): a grey JPEG libjpeg writes of the same plane holds the same coefficients. */
typedef struct { int what, reduce, quality; } mi355enc_snapshot_req_t;
typedef struct { int64_t pts; uint64_t index; int width, height, what, quality; } mi355enc_snapshot_info_t; /* index: the picture's position in the stream */
/* Arms the NEXT submitted picture; a second request before that replaces the first.  Any thread, any time; no GPU call.  ERR_ARG for values out of range. */
int mi355enc_request_snapshot(mi355enc_t *h, const mi355enc_snapshot_req_t *req);
/* The still of the last armed picture that has been collected, coded here, in the caller's thread (any thread).  ERR_STATE while none is ready; ERR_OVERFLOW
 * with *len = the bytes needed (mi355enc_snapshot_max_bytes bounds them).  A still not taken is replaced by the next one; taking it twice yields the same
 * bytes.  info may be NULL. */
int mi355enc_take_snapshot(mi355enc_t *h, uint8_t *out, size_t cap, size_t *len, mi355enc_snapshot_info_t *info);
/* pinned host and device memory held for stills: 0 until the first armed picture is submitted (with no request nothing is allocated, launched or waited for) */
size_t mi355enc_debug_snapshot_bytes(const mi355enc_t *h);
/* host only: the two quantisation tables of a quality (0 luminance, 1 chrominance; natural order); the multiplier the device divides by 8 q with,
 * ceil(2^32 / (8 q)) (0 outside 1 .. 255); an upper bound of a still's size (0 for sizes outside 1 .. 65535) */
int mi355enc_snapshot_tables(int quality, uint16_t qt[2][64]);
uint32_t mi355enc_snapshot_reciprocal(int q);
size_t mi355enc_snapshot_max_bytes(int ow, int oh);
/* host only: the file of a still of ow x oh from its levels -- per component (Y, Cb, Cr) the blocks of its MCU-padded plane in raster order, 64 int16 each in
 * natural order: the layout mi355enc_jpeg_entropy_decode returns for a 4:2:0 picture of that size.  ERR_ARG for a level Huffman coding cannot express
 * (an AC level beyond +-1023, a DC difference beyond 11 bits); ERR_OVERFLOW with *len = the bytes needed. */
int mi355enc_snapshot_write(const int16_t *levels, const uint16_t qt[2][64], int ow, int oh, uint8_t *out, size_t cap, size_t *len);
/* the kernel alone (tests): NV12 host planes of w x h (even, 2 .. 16384; independent of the handle's size) -> the levels of the still reduced by `reduce`
 * (room for the blocks of a ceil(w / reduce) x ceil(h / reduce) picture) and the tables of `quality` */
int mi355enc_stage_snapshot_blocks(mi355enc_t *h, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride, int w, int ht, int reduce, int quality,
                                   int16_t *levels, uint16_t qt[2][64]);
/* ... on planes in this GPU's memory, any address and stride: no byte outside the visible w x ht is read */
int mi355enc_stage_snapshot_blocks_device(mi355enc_t *h, const void *d_y, int y_stride, const void *d_uv, int uv_stride, int w, int ht, int reduce, int quality,
                                          int16_t *levels, uint16_t qt[2][64]);
/* ... and the whole file */
int mi355enc_stage_snapshot(mi355enc_t *h, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride, int w, int ht, int reduce, int quality,
                            uint8_t *out, size_t cap, size_t *len);
/* ---- frame-rate conversion --------------------------------------
 * In place of a `videorate ! video/x-raw,framerate=...` in front of the encoder.  On, the pictures a handle codes lie on a regular grid of ticks at the
 * configured fps_num / fps_den: tick k at T0 + k D / N (D = pts_per_second * fps_den, N = fps_num), its pts T0 + floor(k D / N); the first picture submitted
 * sets T0 to its pts and is tick 0.  The pts of the submitted pictures decide which of them a tick shows:
 *   hold   an input at p makes the ticks up to floor((2 N (p - T0) + D) / (2 D)) due (no later than half a tick period after p).  No due tick: the input is
 *          dropped -- nothing of it is decoded, transferred or latched.  n due ticks: the first n - 1 repeat the previous output picture's source, the last
 *          one shows the input.  Nothing waits for a later input.
 *   blend  ticks up to floor((16 N (p - T0) + D) / (16 D)) are due (a sixteenth of a period of tolerance); a due tick is the mix of the previous input (at
 *          p0) and this one (at p1) with w = clamp(round-half-up(256 (T_k - p0) / (p1 - p0)), 0, 256) from the exact rational T_k, every sample
 *          (a (256 - w) + b w + 128) >> 8 after the colour step, luma and chroma alike (w = 0 and w = 256 give a and b exactly).  Every input is
 *          transferred and kept; one with no due tick yields no picture.
 * An input whose pts lies below the previous input's, or that would make more than max_fill + 1 ticks due, re-anchors: T0 = its pts, one picture, a resync.
 * max_fill is clamped to cfg.pipeline_depth: a submit that yields n pictures takes n slots.  With fewer free ones the submit returns MI355ENC_ERR_STATE and
 * has touched nothing -- collect, then submit again (in blend mode a submit that yields no picture still passes through one free slot).  Image layers and
 * text are drawn afresh into every output picture, repeats included; they are never mixed or kept.  force_idr goes to the first picture a submit yields; a
 * submit that yields none carries it to the next picture coded.  mi355enc_collect returns every picture with its tick's pts.  mi355enc_submit_device never
 * takes its in-place exit and mi355enc_encode returns MI355ENC_ERR_STATE with conversion on.  Off (the default): nothing is allocated or launched. */
typedef struct { int mode; int64_t pts_per_second; int max_fill; } mi355enc_rate_t;            /* mode 0 off, 1 hold, 2 blend */
typedef struct { uint64_t in, out, dropped, repeated, blended, resyncs; } mi355enc_rate_stats_t; /* blended: pictures with 0 < w < 256 */
#define MI355ENC_RATE_MAX_OUT 16 /* most pictures one step of a plan yields: max_fill is 0 .. 15 there */
/* the rule's state (host only): initialise with mi355enc_rate_plan_init, then treat as opaque */
typedef struct { int mode, fps_num, fps_den, max_fill, started; int64_t pps, t0, k_next, prev_pts; } mi355enc_rate_plan_t;
int mi355enc_rate_check(const mi355enc_rate_t *r);                           /* host only: ERR_ARG for no r, mode outside 0..2, pts_per_second <= 0, max_fill < 0 */
int mi355enc_set_rate_conversion(mi355enc_t *h, const mi355enc_rate_t *r);   /* before the first submit only (ERR_STATE after); ERR_ARG as above */
int mi355enc_rate_peek(const mi355enc_t *h, int64_t pts);                    /* pictures a submit with this pts would enqueue now: 0 .. max_fill + 1 (1 with conversion off); changes nothing */
int mi355enc_last_submit_count(const mi355enc_t *h);                         /* pictures the last successful submit enqueued */
int mi355enc_rate_stats(mi355enc_t *h, mi355enc_rate_stats_t *st);           /* ERR_STATE with conversion off */
size_t mi355enc_debug_rate_bytes(const mi355enc_t *h);                       /* device memory held for it: 0 when off, and in hold mode with max_fill 0 */
/* host only, no handle: the rule itself.  init: max_fill is clamped to 0 .. 15; k_next < 0 starts an empty plan (the first input anchors it), k_next >= 0 one
 * anchored at t0 whose ticks below k_next are out.  step: one input; *n pictures (0 .. max_fill + 1) with their pts and weights (hold: 0 a repeat, 256 the
 * input) in arrays of MI355ENC_RATE_MAX_OUT entries, *resync 1 when it re-anchored.  ERR_ARG for a missing pointer or a plan that was not initialised. */
void mi355enc_rate_plan_init(mi355enc_rate_plan_t *plan, int mode, int64_t pts_per_second, int fps_num, int fps_den, int max_fill, int64_t t0, int64_t k_next);
int mi355enc_rate_plan_step(mi355enc_rate_plan_t *plan, int64_t pts, int *n, int64_t out_pts[], int weight[], int *resync);
/* the launch alone (tests): out = mix of a and b with weight w256 (0 .. 256); host planes of the coded size, stride 16 * mb_width; works with conversion off;
 * ERR_STATE with pictures pending */
int mi355enc_stage_rate(mi355enc_t *h, int w256, const uint8_t *a_y, const uint8_t *a_uv, const uint8_t *b_y, const uint8_t *b_uv, uint8_t *out_y, uint8_t *out_uv);
size_t mi355enc_max_au_bytes(const mi355enc_t *h);
const char *mi355enc_strerror(int code);
int mi355enc_abi_version(void);

/* ---- inspection of the last collected picture (parity tests) ----------------------
 * Copies device state to host: coded-size planes (stride = 16*mb_width), the 16-byte
 * per-macroblock records and the 408 int16 levels per macroblock (layout: DESIGN.md).
 * MI355ENC_FETCH_MBINFO returns the records as they were handed to the entropy coder.  With adaptive quantisation (aq_mode 1) the `qp` byte of a macroblock that sends
 * no mb_qp_delta (P_Skip, or no coded block and not Intra_16x16) is NOT defined there: the deblocking launch's QP_Y chain rewrites it on the device (7.4.5: the QP_Y of the
 * macroblock before it) while the hand-over copies the records, and the entropy coder never reads it -- take `qp` only from macroblocks that send a delta. */
/* MI355ENC_FETCH_SCALE_TABLES: the device's copy of the scale tables (after mi355enc_set_input_size): the luma horizontal, luma vertical,
 * chroma horizontal, chroma vertical 4:2:0 and chroma vertical 4:2:2 tables in this order, each as int32 first[n] then int16 coef[n][taps]
 * (mi355enc_scale_table's), padded to a multiple of 16 bytes. */
/* MI355ENC_FETCH_SOURCE_Y / _UV: the coded source surfaces of the last collected picture as its kernels read them -- behind the colour step, picture controls,
 * frame-rate conversion, image layers and text.  They are its slot's: valid until the next submit (which may reuse the slot); MI355ENC_ERR_STATE before the
 * first collect and for a picture mi355enc_submit_device encoded in place. */
enum { MI355ENC_FETCH_RECON_Y = 0, MI355ENC_FETCH_RECON_UV = 1, MI355ENC_FETCH_PREFILTER_Y = 2,
       MI355ENC_FETCH_PREFILTER_UV = 3, MI355ENC_FETCH_MBINFO = 4, MI355ENC_FETCH_LEVELS = 5, MI355ENC_FETCH_SCALE_TABLES = 6,
       MI355ENC_FETCH_SOURCE_Y = 7, MI355ENC_FETCH_SOURCE_UV = 8 };
int mi355enc_fetch(mi355enc_t *h, int what, void *dst, size_t dst_bytes);
int mi355enc_mb_width(const mi355enc_t *h);
int mi355enc_mb_height(const mi355enc_t *h);

/* ---- single-stage entry points (parity tests; same kernels the encoder launches) ----
 * All planes are host pointers to coded-size (multiple-of-16) surfaces with stride 16*mbw;
 * mbinfo is mbw*mbh 16-byte records, levels mbw*mbh*408 int16. */
/* Whole-sample motion search: SAD surfaces (35 x 36 uint16 per macroblock: row dy+16, column dx+16; the 33 x 33 upper-left
 * part is the +-16 search range; surf_out may be NULL) and the first selection, 8 bytes per macroblock {i16 mvx, mvy
 * (quarter-sample units, multiples of 4); u16 sad, bits}. */
int mi355enc_stage_me(mi355enc_t *h, const uint8_t *cur_y, const uint8_t *ref_y, int qp, uint16_t *surf_out, void *imv_out);
/* One more selection over the surfaces, bits charged against the median of the neighbours' vectors in imv_in. */
int mi355enc_stage_me_select(mi355enc_t *h, const uint16_t *surf, const void *imv_in, int qp, void *imv_out);
/* the same iteration in the form the encoder's later passes use (macroblocks whose predictors are unchanged against imv_prev -- the field imv_in was selected from -- are copied) */
int mi355enc_stage_me_select_next(mi355enc_t *h, const uint16_t *surf, const void *imv_in, const void *imv_prev, int qp, void *imv_out);
/* Two-kernel form of the P stage (High-profile path): refine the vectors in mbinfo (mvx, mvy in quarter-sample units, cost) in place ... */
int mi355enc_stage_subpel(mi355enc_t *h, const uint8_t *cur_y, const uint8_t *ref_y, int qp, void *mbinfo_inout);
/* ... and prediction, residual (4x4 or 8x8 transform), reconstruction for the vectors in mbinfo */
int mi355enc_stage_inter(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, const uint8_t *ref_y,
                         const uint8_t *ref_uv, int qp, void *mbinfo_inout, uint8_t *rec_y, uint8_t *rec_uv,
                         int16_t *levels);
/* The fused P-macroblock stage the encoder runs, from the final whole-sample field `imv` and the surfaces: predictor estimates,
 * skip probe, sub-sample refinement (if `refine`), intra-or-inter against `idec` (32 bytes per macroblock as written by
 * mi355enc_stage_intra_analyse; NULL: inter only), residual with coefficient decimation; `drop`: 0 .. 12.  With run_intra_p the
 * macroblocks decided intra are reconstructed afterwards (intra_p_kernel); without, they only carry type and modes. */
int mi355enc_stage_pmb(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, const uint8_t *ref_y, const uint8_t *ref_uv,
                       int qp, int drop, int refine, const void *imv, const uint16_t *surf, const void *idec, int run_intra_p,
                       void *mbinfo_out, uint8_t *rec_y, uint8_t *rec_uv, int16_t *levels);
/* I picture: analysis + reconstruction wavefront; `drop`: rate control's ladder for I pictures, 0 off .. 12 (Intra_16x16 only, and a
 * macroblock's luma / chroma levels are not sent when their magnitudes sum to no more than the level's threshold) */
int mi355enc_stage_intra(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, int qp, int drop, void *mbinfo_out,
                         uint8_t *rec_y, uint8_t *rec_uv, int16_t *levels);
/* open-loop intra analysis only: 152 uint16 per macroblock {i16[4], chroma[4], i4[16][9]}, 0xFFFF = mode unavailable; and
 * (idec_out may be NULL) the decisions taken from them at `qp`: 32 bytes per macroblock {u8 modes4[16] by luma4x4BlkIdx;
 * u8 mode16, chroma mode, use_i4, 0; u32 cost (luma + chroma), cost_luma, 0} */
int mi355enc_stage_intra_analyse(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, int qp, uint16_t *isad_out, void *idec_out);
int mi355enc_stage_deblock(mi355enc_t *h, uint8_t *rec_y, uint8_t *rec_uv, const void *mbinfo);
/* Time `iters` back-to-back launches of one stage on the handle's stream with HIP events;
 * stage: 0 ME, 1 inter, 2 intra (whole wavefront), 3 deblock (whole wavefront), 4 sub-sample refinement,
 * 5 / 6 / 7 input conversion from I420 / YUY2 / UYVY, 8 one vector-selection iteration, 9 fused P stage, 10 intra macroblocks of a P picture,
 * 11 the quality-metrics launch (slot 0's source surfaces against reconstruction buffer 1),
 * 12 the JPEG launch for the handle's input size as 4:2:2, on whatever slot 0's coefficient buffer holds,
 * 13 the orientation launch at the handle's size (the handle's method; 90r on a handle without one), on whatever slot 0's raw staging buffer holds,
 * 14 the scale / geometry launch for an NV12 picture of the handle's input size (MI355ENC_ERR_STATE without mi355enc_set_input_size / _geometry), likewise,
 * 15 the blend launch of image layer 0 at its current place into slot 0's source surfaces (MI355ENC_ERR_STATE without an image on layer 0),
 * 16 the still launch on slot 0's source surfaces, with the reduction and quality of the last mi355enc_request_snapshot (1 and 75 without one),
 * 17 the colour step on slot 0's source surfaces (MI355ENC_ERR_STATE when the handle has no conversion),
 * 18 the frame-rate conversion's mix launch (w = 128) of the keep buffer and slot 0's source surfaces, in place (MI355ENC_ERR_STATE with conversion off),
 * 19 / 20 / 21 the tone-mapping conversion launch of a P010 / I420_10 / V210 picture in slot 0's raw staging buffer (whatever the last conversion left there;
 * MI355ENC_ERR_STATE without mi355enc_set_hdr_input), 22 the plain P010 conversion launch from the same buffer,
 * 23 / 24 the picture controls set last (mi355enc_set_adjust) in place on slot 0's source surfaces: 23 the pointwise form, 24 the stencil form with the hand-back
 * of its scratch plane (MI355ENC_ERR_STATE when the value set last is off or of the other form),
 * 25 / 26 the temporal noise filter set last (mi355enc_set_denoise) in place on slot 0's source surfaces and the handle's history: 25 filtering (the history
 * primed by the launch in front of the timed ones, if it was not valid), 26 priming (MI355ENC_ERR_STATE when the value set last is off).  Both leave the
 * history invalid: the next picture submitted primes.
 * 27 / 28 its motion-compensated form with the range set last (mi355enc_set_denoise_motion; MI355ENC_ERR_STATE when that is 0 or the filter is off): 27 the
 * search alone, 28 the search and the compensated filter.  They leave the history invalid likewise.
 * 29 / 30 the stabiliser's launches (mi355enc_set_stabilize; MI355ENC_ERR_STATE when it is off or the handle has no geometry): 29 the projection launch with
 * its clear at the handle's input size on slot 0's raw staging buffer, 30 the match launch on whatever the projection buffers hold.  Both leave the
 * trajectory unprimed: the next picture submitted primes.
 * 31 the warp set last (mi355enc_set_warp / mi355enc_set_warp_mesh; MI355ENC_ERR_STATE when it is off) on slot 0's source surfaces.
 * 32 / 33 / 34 the launches of automatic levels and white balance with the value set last (mi355enc_set_autolevel; MI355ENC_ERR_STATE when it is off) on slot
 * 0's source surfaces: 32 measure, 33 decide (on the slabs of a measure launch in front of the timed ones), 34 apply (with that decision's table and
 * offsets, so the surfaces change with every launch).  They leave the state unprimed: the next picture submitted primes.
 * 35 the 3D LUT set last (mi355enc_set_lut3d; MI355ENC_ERR_STATE when it is off) on slot 0's source surfaces, in the form mi355enc_lut3d_plan names.
 * 36 / 37 the spatial noise filter with the value set last (mi355enc_set_denoise_spatial) on slot 0's source surfaces: 36 the filter launches of a manual
 * setting (both planes with both strengths above 0), 37 measure + decide + the filter launches of an automatic one (with both bounds 0: measure + decide
 * alone); MI355ENC_ERR_STATE with a setting of the other kind or none.  37 leaves the state unprimed: the next picture submitted primes.
 * Uses whatever the handle's surfaces currently hold.  Returns average ms per launch. */
int mi355enc_time_stage(mi355enc_t *h, int stage, int iters, double *avg_ms);


/* ---- host-only stages (no device needed; what collect() runs once the packed hand-over has landed) ----
 * SPS+PPS, and one CAVLC slice NAL from macroblock records + levels.  *out_len = bytes. */
int mi355enc_host_write_headers(int width, int height, int fps_num, int fps_den, int transform8x8, uint8_t *out, size_t out_cap,
                                size_t *out_len);
/* ... with a sample aspect ratio (sar_w : sar_h; 0: none) and the colorimetry of mi355enc_set_colorimetry in the VUI; (0, 0, 0, 2, 2, 2) gives the bytes of
 * mi355enc_host_write_headers */
int mi355enc_host_write_headers_vui(int width, int height, int fps_num, int fps_den, int transform8x8, int sar_w, int sar_h, int full_range, int primaries,
                                    int transfer, int matrix, uint8_t *out, size_t out_cap, size_t *out_len);
int mi355enc_host_write_slice(int mb_width, int mb_height, int is_idr, int frame_num, int idr_pic_id, int slice_qp, int transform8x8,
                              const void *mbinfo, const int16_t *levels, uint8_t *out, size_t out_cap, size_t *out_len);
/* process-wide, for the two host stage functions below: I pictures are written as slices of `rows` macroblock rows (0, the default: one slice) */
void mi355enc_host_set_slice_rows(int rows);
/* ... P pictures as slices of `rows` rows (0: one slice), and the disable_deblocking_filter_idc every slice header (I and P) carries: 0 or 2 */
void mi355enc_host_set_p_slices(int rows, int dbf_idc);
/* the single-stage entry points of a handle work on one-slice pictures unless told otherwise (the encoder itself follows cfg.intra_slices) */
int mi355enc_stage_set_slice_rows(mi355enc_t *h, int rows);
int mi355enc_slice_rows(const mi355enc_t *h); /* rows per slice of this handle's I pictures (0: one slice) */
int mi355enc_p_slice_rows(const mi355enc_t *h); /* ... and of its P pictures */
int mi355enc_stage_set_slice_deblock(mi355enc_t *h, int idc); /* the single-stage entry points: disable_deblocking_filter_idc of the picture's slices, 0 (default) or 2 */
/* (with idc 2 every slice is a whole number of the deblocker's bands, four macroblock rows: a single-stage call made with idc 2 and slice rows
 * that are not a multiple of four returns MI355ENC_ERR_ARG, whichever of the two settings came first) */
/* the same slice through the packed hand-over format and `threads` row-parallel host threads (bit-identical result) */
int mi355enc_host_write_slice_packed(int mbw, int mbh, int is_idr, int frame_num, int idr_pic_id, int qp, int t8, int threads, const void *mbinfo,
                                     const int16_t *levels, uint8_t *out, size_t cap, size_t *out_len);
/* One CAVLC residual block (9.2) through the slice writer's block coder, for known-answer tests: coef in scan order, maxnum 16
 * (whole 4x4 block), 15 (AC of Intra16x16 / chroma) or 4 (chroma DC); nC as 9.2.1 derives it.  Bits MSB-first into out
 * (cap >= 64 bytes); returns the number of bits, negative on error. */
int mi355enc_host_cavlc_block(const int16_t *coef, int maxnum, int nC, uint8_t *out, size_t cap);
/* Rate-control model on its own: per picture one pick (QP and, below QP 51, the drop level: 0 .. 12, 255 = all-skip picture)
 * and -- possibly one picture later, as with pipeline_depth 1 -- one update with the bytes it produced, in the same order.
 * rc is an opaque block of MI355ENC_RC_BYTES bytes owned by the caller. */
#define MI355ENC_RC_BYTES 512
void mi355enc_rc_init(void *rc, double fps, int gop, uint32_t bps, int qp_min, int qp_max);
void mi355enc_rc_set_bitrate(void *rc, uint32_t bps);
void mi355enc_rc_pick(void *rc, int is_idr, int *qp, int *drop);
void mi355enc_rc_update(void *rc, int is_idr, int qp, int drop, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
