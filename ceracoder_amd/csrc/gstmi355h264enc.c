/*
 * gstmi355h264enc.c -- GStreamer element `mi355h264enc`: the drop-in for the `x264enc`
 * token of ceracoder's pipeline files
 * (/root/reference/pipeline/generic/x264_superfast_camlink:5:
 *      `x264enc speed-preset=2 key-int-max=60 name=venc_kbps`).
 *
 * Contract taken from the reference:
 *  - found by NAME, not type: `venc_bps` (value in bit/s) is tried first, then `venc_kbps`
 *    (value / 1000)                       /root/reference/src/gst/encoder_control.c:29-32
 *  - the property the binary writes is "bps"        .../encoder_control.c:53
 *    (README/docs call it "bitrate": /root/reference/README.md:256) -> both exist here and
 *    alias one target; "bitrate" is kbit/s with x264enc's default 2048
 *  - every x264 pipeline file of the reference says `name=venc_kbps`
 *    (pipeline/generic/x264_*:5-6, generic-builder.ts:54), for which encoder_control.c:53
 *    writes bitrate / 1000 into "bps": an element NAMED venc_kbps therefore reads and writes
 *    "bps" in kbit/s, so that such a file works with only the factory token changed
 *  - first write happens in state NULL, before PLAYING /root/reference/src/ceracoder.c:515-518
 *  - later writes come from the GLib main thread every <= 20 ms while the streaming thread
 *    encodes                                         /root/reference/src/ceracoder.c:266-295
 *  - upstream zeroes DTS and smooths PTS             /root/reference/src/ceracoder.c:371-423
 *    -> output DTS = PTS, no reordering
 *  - errors go to the bus; the app exits on ERROR    /root/reference/src/ceracoder.c:425-438
 * API level: GStreamer 1.14 (GstVideoEncoder).  Plain C; the device is reached only
 * through the C ABI in include/mi355enc.h.  There is no CPU path: without a HIP device the
 * element posts an ERROR when it leaves READY.
 */
#include <gst/gst.h>
#include <gst/video/gstvideoencoder.h>
#include <gst/video/video.h>
#include <errno.h>
#include <glib/gstdio.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/mi355enc.h"

#define PACKAGE "ceracoder-amd"
#define VERSION "0.1.0"

GST_DEBUG_CATEGORY_STATIC(mi355_debug);
#define GST_CAT_DEFAULT mi355_debug

typedef struct {
    GstVideoEncoder parent;
    /* properties (guarded by the object lock; bitrate is additionally forwarded atomically) */
    guint rate_raw;     /* the target as it was written: through "bps" in the unit the element's NAME implies, through "bitrate" in kbit/s */
    gboolean rate_is_bps; /* the last write came through "bps" */
    guint key_int_max;
    gint device_id, me_range, qp, pipeline_depth, speed_preset;
    gint open_depth;  /* pipeline-depth the encoder was opened with: a write to the property in mid-stream takes effect at the next (re)negotiation */
    gboolean stats;
    gint threads;
    gboolean scenecut, exclusive_gpu;
    guint vbv_ms;
    gboolean pinned_input;
    gboolean jpeg;    /* the sink caps are image/jpeg: buffers are JPEG pictures, decoded on the way in (mi355enc_submit_jpeg) */
    gint jpeg_refused; /* ... and how many of them in a row the encoder has refused */
    /* coding tools: -1 = not set on the element, i.e. what speed-preset selects (preset_tools); an explicit write wins */
    gint dct8x8, i8x8, aq_mode, intra_in_p, slices, slice_deblock;
    gint intra_slices;
    gboolean single_stream;
    gboolean dct8x8_adaptive; /* with dct8x8: the transform size is chosen per P macroblock (cfg.transform8x8 = 2) */
    gboolean quality_stats;   /* per-picture PSNR / SSIM computed on the device (mi355enc_set_quality_metrics); with stats=true the stream's figures are printed at close */
    gboolean intra_refresh;   /* periodic intra refresh instead of periodic IDR pictures (mi355enc_set_intra_refresh); key-int-max is the refresh period */
    /* text overlay drawn on the device (mi355enc_set_overlay_text / _style): written through the overlay-* properties or by the
     * custom event of an `mi355textoverlay` element upstream; stored here (object lock) and forwarded to the open encoder, which latches it per picture */
    gchar ov_text[MI355ENC_OVERLAY_MAX_TEXT + 1];
    mi355enc_overlay_style_t ov_style;
    /* image layer 0 blended in on the device (mi355enc_set_image / _set_image_place), in place of a gdkpixbufoverlay upstream: the file
     * image-location named last (a Netpbm PAM, read when the property is written), its RGBA pixels, and the place and alpha; stored here (object lock) and
     * forwarded to the open encoder, which latches them per picture.  img_rgba NULL: the layer is off */
    gchar *img_location;
    guint8 *img_rgba;
    gint img_w, img_h, img_x, img_y;
    gdouble img_alpha;
    /* orientation on the device (mi355enc_set_orientation): the video-direction property (GstVideoOrientationMethod, AUTO follows the
     * upstream image-orientation tag), what the last such tag said, and the method the open encoder was opened with (a change reopens it at the next picture) */
    gint direction, tag_direction, open_direction;
    gint out_w, out_h;        /* coded size (mpph265enc's width / height): 0 = the input's; smaller: scaled down on the device (mi355enc_set_input_size) */
    /* input geometry on the device (mi355enc_set_input_geometry / _set_crop): videocrop's crop-* (input samples; odd values count as the even
     * value below), videoscale's add-borders (the picture keeps its shape inside width x height), upscale (width / height may exceed the input), border-color
     * (0xYYCbCr).  All at their defaults: none of this is used.  open_geom: the open handle has a geometry, with the crop open_crop (left, right, top, bottom); a
     * crop that changes while playing is latched in front of the next picture (as the direction is) and goes through mi355enc_set_crop where that is enough */
    gint crop[4];
    gboolean add_borders, upscale;
    guint border_color;
    gboolean open_geom;
    gint open_crop[4];
    /* streaming state */
    mi355enc_t *enc;
    GstVideoCodecState *input_state;
    gsize max_au;
    guint8 *au_buf;     /* access units are coded here (worst-case size, allocated once per format) and copied into right-sized buffers */
    GstClockTime last_pts;
    /* where the streaming thread's time goes, per stage (microseconds, summed; printed with stats=true): what separates the element's rate from the C ABI's */
    gint64 us_map, us_submit, us_collect, us_output, us_push, us_frames;
    /* JPEG stills of the running stream (mi355enc_request_snapshot / _take_snapshot).  Properties (object lock): the file (empty: off), the
     * interval in ms of stream time, quality, reduction, source (0 the coded source, 1 the decoded picture).  The streaming thread arms a picture every interval and
     * wakes the helper for the collects that may have completed it; the helper -- never the streaming thread -- takes the still (the Huffman coding runs there),
     * writes location.tmp, renames it over location and posts `mi355-snapshot`.  snap_enc_mu: held by the helper while it uses the encoder and by whoever
     * closes or opens it (s->enc and snap_gen change under it, taken in front of the object lock).  snap_mu / snap_cv: the helper's wake-ups, and snap_count.
     * snap_next: object lock.  snap_gen counts the encoders opened: a new one resets what the helper remembers of the last still it wrote. */
    gchar *snap_location;
    /* frame-rate conversion: the properties (read at the next set_format), what the encoder was opened with, and per submitted frame that
     * yielded pictures their number -- a FIFO in submission order, so that collected access units meet their GstVideoCodecFrame: a frame's pictures but the last
     * are pushed as buffers of their own, the last one finishes the frame */
    gint rate_mode, out_fps_n, out_fps_d, max_fill;
    /* picture controls on the device (mi355enc_set_adjust): brightness, contrast, hue, saturation with videobalance's names, ranges and
     * defaults, gamma, sharpen, sharpen-threshold; stored in the library's integers (the doubles as thousandths, lround) under the object lock and forwarded like
     * the overlay's text -- any thread, at any time */
    mi355enc_adjust_t adj;
    /* temporal noise reduction on the device (mi355enc_set_denoise): denoise-luma, denoise-chroma; stored and forwarded like the picture controls */
    mi355enc_denoise_t dn;
    /* spatial noise reduction on the device (mi355enc_set_denoise_spatial): denoise-spatial-luma, denoise-spatial-chroma, denoise-auto (a
     * double 0 .. 8, stored as thousandths, lround; 0: manual), denoise-auto-percentile, denoise-auto-speed; stored and forwarded like the picture controls */
    mi355enc_denoise_spatial_t ds;
    /* automatic levels and white balance on the device (mi355enc_set_autolevel): auto-levels, auto-balance (doubles 0 .. 1, stored as
     * thousandths, lround), auto-speed, auto-clip (percent, both clips), auto-max-gain; stored under the object lock and forwarded like the picture controls */
    mi355enc_autolevel_t al;
    /* a 3D colour LUT on the device (mi355enc_set_lut3d): lut3d-location, the path of a .cube file, read and parsed in the setter (""
     * or NULL: off; lut_nodes: its lut_size^3 nodes, NULL: none), and lut3d-strength, a double 0 .. 1 stored as round(256 x); under the object lock */
    gchar *lut_location; guint32 *lut_nodes; gint lut_size, lut_strength;
    /* region-of-interest quantisation (mi355enc_set_roi): roi, the rectangles as "x,y,w,h,delta[,feather];..." (parsed in the setter; ""
     * or NULL: off; roi_text: the string as it was accepted), and roi-balance, the cap of the background offset; under the object lock.  The library latches
     * the map with the next frame submitted */
    gchar *roi_text; mi355enc_roi_t roi;
    /* privacy masks (mi355enc_set_mask): mask, the regions as "x,y,w,h,mode,param[,shape];..." (parsed in the setter; "" or NULL: off;
     * mask_text: the string as it was accepted), and mask-color, the fill colour 0xRRGGBB every region takes; under the object lock.  The library latches the
     * configuration with the next frame submitted */
    gchar *mask_text; mi355enc_mask_t mask; guint mask_color;
    /* stabilize (mi355enc_set_stabilize): the margin in input samples per side (0: off; odd values count as the even value below), added
     * to each of crop-* when the geometry is built -- so a change while playing is a crop change --, and the estimator's range and leak */
    gint stab, stab_range, stab_leak;
    /* lens, roll and keystone correction (mi355enc_set_warp): lens-k1, lens-k2, lens-zoom, roll (degrees), keystone-h, keystone-v as the
     * doubles they were set to, warp-filter (0 bilinear, 1 bicubic); all neutral: off.  Forwarded like the picture controls; the fill is border-color */
    gdouble warp_k1, warp_k2, warp_zoom, warp_roll, warp_kh, warp_kv;
    gint warp_filter;
    gint dn_motion; /* denoise-motion: the search range of its motion compensation (mi355enc_set_denoise_motion; section 25), 0: none */
    gint hdr_input, hdr_peak, hdr_target; /* hdr-input (0 off, 16 pq, 18 hlg), hdr-peak-nits, hdr-target-nits: read at the next set_format */
    gint open_rate;           /* 0: conversion off */
    GstClockTime tick;        /* duration of an output picture */
    guint8 rate_q[8]; guint rate_qh, rate_qn;
    gchar *out_colorimetry; /* output-colorimetry: what the coded samples are to mean (NULL or "": what the input's mean) */
    guint snap_interval;
    gint snap_quality, snap_reduce, snap_source;
    GstClockTime snap_next;   /* stream time of the next picture to arm (NONE: the next one) */
    gint snap_watch;          /* collects to come that may complete an armed picture */
    GMutex snap_mu, snap_enc_mu;
    GCond snap_cv;
    GThread *snap_thread;
    gint snap_wake;
    gboolean snap_stop;
    guint64 snap_count;
    guint snap_gen;
} GstMi355H264Enc;
typedef struct { GstVideoEncoderClass parent_class; } GstMi355H264EncClass;

#define GST_TYPE_MI355H264ENC (gst_mi355h264enc_get_type())
#define GST_MI355H264ENC(o) (G_TYPE_CHECK_INSTANCE_CAST((o), GST_TYPE_MI355H264ENC, GstMi355H264Enc))
G_DEFINE_TYPE_WITH_CODE(GstMi355H264Enc, gst_mi355h264enc, GST_TYPE_VIDEO_ENCODER, G_IMPLEMENT_INTERFACE(GST_TYPE_VIDEO_DIRECTION, NULL))

enum { PROP_0, PROP_BPS, PROP_BITRATE, PROP_KEY_INT_MAX, PROP_DEVICE_ID, PROP_ME_RANGE, PROP_QP, PROP_PIPELINE_DEPTH,
       PROP_SPEED_PRESET, PROP_STATS, PROP_DCT8X8, PROP_THREADS, PROP_SCENECUT, PROP_VBV, PROP_INTRA_IN_P, PROP_EXCLUSIVE, PROP_PINNED_INPUT, PROP_AQ_MODE, PROP_SINGLE_STREAM, PROP_INTRA_SLICES, PROP_I8X8, PROP_SLICES, PROP_SLICE_DEBLOCK, PROP_DCT8X8_ADAPTIVE, PROP_INTRA_REFRESH, PROP_WIDTH, PROP_HEIGHT, PROP_QUALITY_STATS,
       PROP_OV_TEXT, PROP_OV_HALIGN, PROP_OV_VALIGN, PROP_OV_XPAD, PROP_OV_YPAD, PROP_OV_SCALE, PROP_OV_SHADED, PROP_VIDEO_DIRECTION,
       PROP_CROP_LEFT, PROP_CROP_RIGHT, PROP_CROP_TOP, PROP_CROP_BOTTOM, PROP_ADD_BORDERS, PROP_UPSCALE, PROP_BORDER_COLOR,
       PROP_IMG_LOCATION, PROP_IMG_X, PROP_IMG_Y, PROP_IMG_ALPHA,
       PROP_SNAP_LOCATION, PROP_SNAP_INTERVAL, PROP_SNAP_QUALITY, PROP_SNAP_REDUCE, PROP_SNAP_SOURCE,
       PROP_OUTPUT_COLORIMETRY, PROP_RATE_CONVERSION, PROP_OUTPUT_FRAMERATE, PROP_MAX_FILL, PROP_HDR_INPUT, PROP_HDR_PEAK_NITS, PROP_HDR_TARGET_NITS,
       PROP_ADJ_BRIGHTNESS, PROP_ADJ_CONTRAST, PROP_ADJ_HUE, PROP_ADJ_SATURATION, PROP_ADJ_GAMMA, PROP_ADJ_SHARPEN, PROP_ADJ_SHARPEN_THRESHOLD,
       PROP_DENOISE_LUMA, PROP_DENOISE_CHROMA, PROP_DENOISE_MOTION, PROP_DS_LUMA, PROP_DS_CHROMA, PROP_DS_AUTO, PROP_DS_PERCENTILE, PROP_DS_SPEED, PROP_STABILIZE, PROP_STABILIZE_RANGE, PROP_STABILIZE_LEAK, PROP_AUTO_LEVELS, PROP_AUTO_BALANCE, PROP_AUTO_SPEED, PROP_AUTO_CLIP, PROP_AUTO_MAX_GAIN, PROP_LUT3D_LOCATION, PROP_LUT3D_STRENGTH, PROP_ROI, PROP_ROI_BALANCE, PROP_MASK, PROP_MASK_COLOR,
       PROP_LENS_K1, PROP_LENS_K2, PROP_LENS_ZOOM, PROP_ROLL, PROP_KEYSTONE_H, PROP_KEYSTONE_V, PROP_WARP_FILTER };

static GstStaticPadTemplate sink_tmpl = GST_STATIC_PAD_TEMPLATE("sink", GST_PAD_SINK, GST_PAD_ALWAYS,
    GST_STATIC_CAPS("video/x-raw, format=(string){ NV12, I420, YUY2, UYVY, Y42B, Y444, YV12, NV21, BGRx, RGBx, xRGB, xBGR, BGRA, RGBA, ARGB, ABGR, BGR, RGB, P010_10LE, I420_10LE, v210, GRAY8 }, width=(int)[16,8192], height=(int)[16,8192], framerate=(fraction)[0/1,MAX]; "
                    "image/jpeg, width=(int)[16,8192], height=(int)[16,8192], framerate=(fraction)[0/1,MAX]"));
static GstStaticPadTemplate src_tmpl = GST_STATIC_PAD_TEMPLATE("src", GST_PAD_SRC, GST_PAD_ALWAYS,
    GST_STATIC_CAPS("video/x-h264, stream-format=(string)byte-stream, alignment=(string)au, profile=(string){ constrained-baseline, high }, "
                    "width=(int)[16,8192], height=(int)[16,8192], framerate=(fraction)[0/1,MAX]"));

static GType rate_conversion_type(void) {
    static GType t = 0;
    static const GEnumValue v[] = {{0, "Off: every input picture is coded", "off"}, {1, "Drop or repeat pictures to the output ticks", "hold"},
                                   {2, "Blend neighbouring pictures at the output ticks' instants", "blend"}, {0, NULL, NULL}};
    if (!t) t = g_enum_register_static("GstMi355H264EncRateConversion", v);
    return t;
}
static GType warp_filter_type(void) {
    static GType t = 0;
    static const GEnumValue v[] = {{0, "Two taps per axis", "bilinear"}, {1, "Four taps per axis (Catmull-Rom)", "bicubic"}, {0, NULL, NULL}};
    if (!t) t = g_enum_register_static("GstMi355H264EncWarpFilter", v);
    return t;
}
static GType hdr_input_type(void) { /* (the values are the transfer's H.264 Table E-4 code points: what mi355enc_set_hdr_input takes) */
    static GType t = 0;
    static const GEnumValue v[] = {{0, "Off: 10-bit input is rounded to 8 bits", "off"}, {16, "PQ (SMPTE ST 2084), BT.2020: tone-mapped to SDR", "pq"},
                                   {18, "HLG (BT.2100), BT.2020: tone-mapped to SDR", "hlg"}, {0, NULL, NULL}};
    if (!t) t = g_enum_register_static("GstMi355H264EncHdrInput", v);
    return t;
}
static GType snapshot_source_type(void) {
    static GType t = 0;
    static const GEnumValue v[] = {{0, "The coded source", "source"}, {1, "The decoded picture", "decoded"}, {0, NULL, NULL}};
    if (!t) t = g_enum_register_static("GstMi355H264EncSnapshotSource", v);
    return t;
}

/* x264enc's speed-preset enum, accepted so that an x264enc line converts by changing only the factory name */
static GType speed_preset_type(void) {
    static GType t = 0;
    static const GEnumValue v[] = {{0, "No preset", "None"}, {1, "ultrafast", "ultrafast"}, {2, "superfast", "superfast"},
                                   {3, "veryfast", "veryfast"}, {4, "faster", "faster"}, {5, "fast", "fast"}, {6, "medium", "medium"},
                                   {7, "slow", "slow"}, {8, "slower", "slower"}, {9, "veryslow", "veryslow"}, {10, "placebo", "placebo"},
                                   {0, NULL, NULL}};
    if (!t) t = g_enum_register_static("GstMi355H264EncPreset", v);
    return t;
}

/* What x264enc's speed-preset selects, restated in the tools this encoder has.  The reference's pipeline files pass speed-preset=2 (superfast) and =3
 * (veryfast) (/root/reference/pipeline/generic/x264_superfast_camlink:5, x264_veryfast_camlink:5; generator bindings/typescript/src/pipeline/generic-builder.ts:43-55),
 * so the one-token swap has to land on a toolset and not on "ignored".  x264's own table: ultrafast = no 8x8 transform, no adaptive quantisation, no partitions;
 * superfast and slower keep the 8x8 transform with Intra_8x8 and aq-mode 1 (partitions i8x8,i4x4); veryfast and slower analyse inter partitions and
 * Intra_4x4 in P pictures.  Here: 0 (none) / 1: Constrained Baseline, one QP per picture -- the library's defaults; 2 (superfast) and above: dct8x8 + i8x8 +
 * aq-mode 1 (High profile).  What the slower presets would add -- Intra_4x4 in P pictures (intra-in-p=2), inter partitions (4x4 transform only) -- measured
 * rate-distortion neutral here and, with adaptive quantisation, Intra_4x4 in P puts a picture's stages in stream order: they stay explicit
 * switches.  Slices follow the library's default (mi355enc_default_cfg) unless `slices` / `slice-deblock` are set. */
typedef struct { gint dct8x8, i8x8, aq_mode, partitions, intra_in_p, slices, slice_deblock; } toolset_t;
static void preset_tools(gint preset, toolset_t *t) {
    t->dct8x8 = t->i8x8 = t->aq_mode = preset >= 2; t->partitions = 0; /* (inter partitions: no property -- the search the fused stage can afford is rate-distortion neutral; cfg.partitions remains in the C ABI) */ t->intra_in_p = 1;
    t->slices = -1; t->slice_deblock = -1; /* the library's defaults (mi355enc_default_cfg) */
}
/* the element's effective tools: explicit properties over the preset's (object lock held) */
static void effective_tools(GstMi355H264Enc *s, toolset_t *t) {
    preset_tools(s->speed_preset, t);
    if (s->dct8x8 >= 0) t->dct8x8 = s->dct8x8;
    if (s->i8x8 >= 0) t->i8x8 = s->i8x8;
    if (s->aq_mode >= 0) t->aq_mode = s->aq_mode;
    if (s->intra_in_p >= 0) t->intra_in_p = s->intra_in_p;
    if (s->slices >= 0) t->slices = s->slices;
    if (s->slice_deblock >= 0) t->slice_deblock = s->slice_deblock;
    if (!t->dct8x8) t->i8x8 = 0; /* Intra_8x8 needs the 8x8 transform (High profile) */
}

/* The unit of "bps" follows the reference's naming rule (encoder_control.c:29-32,53): an element named venc_kbps is sent
 * bitrate / 1000.  Called with the object lock held (the name is guarded by it). */
static guint bps_unit(GstMi355H264Enc *s) {
    const gchar *n = GST_OBJECT_NAME(s);
    return (n && strcmp(n, "venc_kbps") == 0) ? 1000u : 1u;
}
static guint clamp_bps(guint64 v) { return v < 1000 ? 1000u : v > 1000000000u ? 1000000000u : (guint)v; }
/* The target in bit/s, resolved where it is consumed (object lock held): `mi355h264enc bps=6000 name=venc_kbps` sets the property before
 * the element has its name, and g_object_set followed by gst_object_set_name does the same -- a unit applied at write time would be wrong. */
static guint target_bps(GstMi355H264Enc *s) { return clamp_bps((guint64)s->rate_raw * (s->rate_is_bps ? bps_unit(s) : 1000u)); }

/* textoverlay's alignment words; the values are those of mi355enc_overlay_style_t ("baseline" is taken as bottom).  Shared with gstmi355textoverlay.c */
GType gst_mi355_overlay_halign_type(void) {
    static GType t = 0;
    static const GEnumValue v[] = {{0, "left", "left"}, {1, "center", "center"}, {2, "right", "right"}, {0, NULL, NULL}};
    if (!t) t = g_enum_register_static("GstMi355OverlayHAlign", v);
    return t;
}
GType gst_mi355_overlay_valign_type(void) {
    static GType t = 0;
    static const GEnumValue v[] = {{0, "top", "top"}, {1, "center", "center"}, {2, "bottom", "bottom"}, {3, "baseline", "baseline"}, {0, NULL, NULL}};
    if (!t) t = g_enum_register_static("GstMi355OverlayVAlign", v);
    return t;
}
/* stored text / style -> the encoder, if one is open (object lock held; the library only stores: no GPU call, any thread) */
static void overlay_forward(GstMi355H264Enc *s) {
    if (!s->enc) return;
    /* (the property ranges and the event's checks keep the style inside what the library takes: a refusal would leave element and encoder apart, so it is said) */
    if (mi355enc_set_overlay_style(s->enc, &s->ov_style) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the overlay style: it keeps its previous one");
    if (mi355enc_set_overlay_text(s->enc, s->ov_text) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the overlay text");
}
/* stored picture controls -> the encoder, if one is open (object lock held; the library builds two small tables and stores: no GPU call, any thread) */
static void adjust_forward(GstMi355H264Enc *s) {
    if (s->enc && mi355enc_set_adjust(s->enc, &s->adj) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the picture controls: it keeps its previous ones");
}
/* stored automatic levels and white balance -> the encoder, if one is open (object lock held; the library only stores: no GPU call, any thread) */
static void autolevel_forward(GstMi355H264Enc *s) {
    if (s->enc && mi355enc_set_autolevel(s->enc, &s->al) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the automatic levels: it keeps its previous setting");
}
/* stored noise filter strengths -> the encoder, if one is open (object lock held; the library builds three small tables and stores: no GPU call, any thread) */
/* what the crop rectangle is built from: crop-* (even), each with the stabiliser's margin on top.  Called with the object lock held */
static void effective_crop(const GstMi355H264Enc *s, int crop[4]) {
    for (int i = 0; i < 4; i++) crop[i] = (s->crop[i] & ~1) + (s->stab & ~1);
}
/* the stabiliser's setting to the encoder (object lock held): on with a margin; the margin itself is part of the crop and follows on the crop's path */
static void stabilize_forward(GstMi355H264Enc *s) {
    const int m = s->stab & ~1;
    const mi355enc_stabilize_t st = {m ? s->stab_range : 0, s->stab_leak, m, m};
    if (s->enc && mi355enc_set_stabilize(s->enc, &st) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the stabiliser's setting: it keeps its previous one");
}
/* the warp's properties to the encoder (object lock held; the library builds a mesh of a few thousand nodes and stores: no GPU call, any thread): doubles to
 * Q16 by lround, the roll through libm, the fill from border-color; all neutral: off.  Every forward that turns it on is a new mesh in front of the next picture */
static void warp_forward(GstMi355H264Enc *s) {
    if (!s->enc) return;
    const double a = s->warp_roll * G_PI / 180.0;
    const mi355enc_warp_params_t p = {(int)lround(s->warp_k1 * 65536.0), (int)lround(s->warp_k2 * 65536.0), (int)lround(s->warp_zoom * 65536.0),
                                      (int)lround(cos(a) * 65536.0), (int)lround(sin(a) * 65536.0), (int)lround(s->warp_kh * 65536.0), (int)lround(s->warp_kv * 65536.0)};
    const mi355enc_warp_t w = {s->warp_filter, {(uint8_t)(s->border_color >> 16), (uint8_t)(s->border_color >> 8), (uint8_t)s->border_color}};
    const gboolean neutral = !p.k1 && !p.k2 && p.zoom == 65536 && p.cos == 65536 && !p.sin && !p.kh && !p.kv;
    if (mi355enc_set_warp(s->enc, neutral ? NULL : &w, neutral ? NULL : &p) != MI355ENC_OK)
        GST_WARNING_OBJECT(s, "the encoder refused the lens / roll / keystone values (the picture would leave the mesh's range): it keeps its previous ones");
}
/* stored spatial noise filter -> the encoder, if one is open (object lock held; the library only stores: no GPU call, any thread) */
static void dspatial_forward(GstMi355H264Enc *s) {
    if (s->enc && mi355enc_set_denoise_spatial(s->enc, &s->ds) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the spatial noise filter: it keeps its previous setting");
}
static void denoise_forward(GstMi355H264Enc *s) {
    if (s->enc && mi355enc_set_denoise(s->enc, &s->dn) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the noise filter's strengths: it keeps its previous ones");
    if (s->enc && mi355enc_set_denoise_motion(s->enc, s->dn_motion) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the noise filter's search range: it keeps its previous one");
}
static void overlay_store_text(GstMi355H264Enc *s, const gchar *t) { g_strlcpy(s->ov_text, t ? t : "", sizeof s->ov_text); }

/* stored image, place and alpha -> layer 0 of the encoder, if one is open (object lock held; the library only copies and stores: no GPU call, any thread).
 * pixels: the image itself has changed (or the encoder is new); otherwise only place and opacity travel */
static int image_opacity(const GstMi355H264Enc *s) { return (int)rint(256.0 * s->img_alpha); }
static void image_forward(GstMi355H264Enc *s, gboolean pixels) {
    if (!s->enc) return;
    if (!s->img_rgba) { if (pixels) mi355enc_set_image(s->enc, 0, NULL); return; }
    if (pixels) {
        const mi355enc_image_layer_t im = {MI355ENC_FMT_RGBX, s->img_rgba, s->img_w, s->img_h, 4 * s->img_w, s->img_x, s->img_y, image_opacity(s)};
        if (mi355enc_set_image(s->enc, 0, &im) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the image: it keeps its previous one");
    } else if (mi355enc_set_image_place(s->enc, 0, s->img_x, s->img_y, image_opacity(s)) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the image's place");
}
/* image-location: the file is read here, in the setter, outside the object lock (the warning goes to the bus).  "" or NULL: off.  A file that cannot be read or
 * that the PAM reader refuses leaves the layer as it was */
static void image_set_location(GstMi355H264Enc *s, const gchar *path) {
    guint8 *rgba = NULL;
    gint w = 0, h = 0;
    if (path && *path) {
        gchar *data = NULL;
        gsize len = 0;
        GError *err = NULL;
        if (!g_file_get_contents(path, &data, &len, &err)) {
            GST_ELEMENT_WARNING(s, RESOURCE, OPEN_READ, ("mi355h264enc: cannot read image-location \"%s\": the image layer stays as it was", path), ("%s", err ? err->message : "?"));
            g_clear_error(&err);
            return;
        }
        int r = mi355enc_image_load_pam((const guint8 *)data, len, &w, &h, NULL, 0);
        if (r == MI355ENC_OK) {
            rgba = g_malloc((gsize)w * h * 4);
            r = mi355enc_image_load_pam((const guint8 *)data, len, &w, &h, rgba, (gsize)w * h * 4);
        }
        g_free(data);
        if (r != MI355ENC_OK) {
            g_free(rgba);
            GST_ELEMENT_WARNING(s, STREAM, FORMAT, ("mi355h264enc: image-location \"%s\" is not a PAM file this element takes (P7, RGB_ALPHA or RGB, MAXVAL 255, at most 4096 x 4096): "
                                                    "the image layer stays as it was", path), ("mi355enc_image_load_pam returned %d", r));
            return;
        }
    }
    GST_OBJECT_LOCK(s);
    g_free(s->img_location); s->img_location = g_strdup(path ? path : "");
    g_free(s->img_rgba); s->img_rgba = rgba; s->img_w = w; s->img_h = h;
    image_forward(s, TRUE);
    GST_OBJECT_UNLOCK(s);
}

/* stored table and strength -> the encoder, if one is open (object lock held; the library checks, copies and stores: no GPU call, any thread) */
static void lut3d_forward(GstMi355H264Enc *s) {
    if (!s->enc) return;
    const mi355enc_lut3d_t set = {s->lut_size, s->lut_strength};
    if (mi355enc_set_lut3d(s->enc, s->lut_nodes ? &set : NULL, s->lut_nodes) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the 3D LUT: it keeps its previous one");
}
/* lut3d-location: the file is read and parsed here, in the setter, outside the object lock (the warning goes to the bus).  "" or NULL: off.  A file that cannot
 * be read or that the parser refuses leaves the step as it was */
static void lut3d_set_location(GstMi355H264Enc *s, const gchar *path) {
    guint32 *nodes = NULL;
    int n = 0;
    if (path && *path) {
        gchar *data = NULL;
        gsize len = 0;
        GError *err = NULL;
        if (!g_file_get_contents(path, &data, &len, &err)) {
            GST_ELEMENT_WARNING(s, RESOURCE, OPEN_READ, ("mi355h264enc: cannot read lut3d-location \"%s\": the 3D LUT stays as it was", path), ("%s", err ? err->message : "?"));
            g_clear_error(&err);
            return;
        }
        const gsize cap = 65 * 65 * 65;
        nodes = g_malloc(cap * sizeof *nodes);
        const int r = mi355enc_lut3d_parse_cube(data, len, nodes, cap, &n);
        g_free(data);
        if (r != MI355ENC_OK) {
            g_free(nodes);
            GST_ELEMENT_WARNING(s, STREAM, FORMAT, ("mi355h264enc: lut3d-location \"%s\" is not a .cube file this element takes (LUT_3D_SIZE 2 .. 65, unit input range): "
                                                    "the 3D LUT stays as it was", path), ("mi355enc_lut3d_parse_cube returned %d", r));
            return;
        }
    }
    GST_OBJECT_LOCK(s);
    g_free(s->lut_location); s->lut_location = g_strdup(path ? path : "");
    g_free(s->lut_nodes); s->lut_nodes = nodes; s->lut_size = n;
    lut3d_forward(s);
    GST_OBJECT_UNLOCK(s);
}

/* stored rectangles and balance -> the encoder, if one is open (object lock held; the library computes the map and stores it: no GPU call, any thread) */
static void roi_forward(GstMi355H264Enc *s) {
    if (!s->enc) return;
    if (mi355enc_set_roi(s->enc, s->roi.n_rects > 0 ? &s->roi : NULL, NULL) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the region of interest: it keeps its previous one");
}
/* roi: parsed here, in the setter, outside the object lock (the warning goes to the bus).  "" or NULL: off.  A string the parser refuses leaves the map as it was */
static void roi_set_text(GstMi355H264Enc *s, const gchar *text) {
    mi355enc_roi_t c;
    mi355enc_roi_default(&c);
    if (mi355enc_roi_parse(text ? text : "", &c) != MI355ENC_OK) {
        GST_ELEMENT_WARNING(s, LIBRARY, SETTINGS, ("mi355h264enc: roi \"%s\" is not a list of at most 8 rectangles x,y,w,h,delta[,feather] joined by ';' (delta -12 .. 12 and not 0, "
                                                   "feather 0 .. 8): the region of interest stays as it was", text), (NULL));
        return;
    }
    GST_OBJECT_LOCK(s);
    c.balance = s->roi.balance;
    s->roi = c;
    g_free(s->roi_text); s->roi_text = g_strdup(text ? text : "");
    roi_forward(s);
    GST_OBJECT_UNLOCK(s);
}

/* stored regions -> the encoder, if one is open (object lock held; the library checks and stores them: no GPU call, any thread) */
static void mask_forward(GstMi355H264Enc *s) {
    if (!s->enc) return;
    for (int k = 0; k < s->mask.n; k++) s->mask.region[k].colour = s->mask_color;
    if (mi355enc_set_mask(s->enc, s->mask.n > 0 ? &s->mask : NULL) != MI355ENC_OK) GST_WARNING_OBJECT(s, "the encoder refused the privacy masks: it keeps its previous ones");
}
/* mask: parsed here, in the setter, outside the object lock (the warning goes to the bus).  "" or NULL: off.  A string the parser refuses leaves the masks as they were */
static void mask_set_text(GstMi355H264Enc *s, const gchar *text) {
    mi355enc_mask_t c;
    if (mi355enc_mask_parse(text ? text : "", 0, &c) != MI355ENC_OK) {
        GST_ELEMENT_WARNING(s, LIBRARY, SETTINGS, ("mi355h264enc: mask \"%s\" is not a list of at most 8 regions x,y,w,h,mode,param[,shape] joined by ';' (mode 1 fill with param 0, "
                                                   "2 pixelate with an even cell 4 .. 64, 3 blur with a radius 1 .. 32; shape 0 or 1): the masks stay as they were", text), (NULL));
        return;
    }
    GST_OBJECT_LOCK(s);
    s->mask = c;
    g_free(s->mask_text); s->mask_text = g_strdup(text ? text : "");
    mask_forward(s);
    GST_OBJECT_UNLOCK(s);
}

static void set_property(GObject *obj, guint id, const GValue *val, GParamSpec *ps) {
    GstMi355H264Enc *s = GST_MI355H264ENC(obj);
    if (id == PROP_MASK) { mask_set_text(s, g_value_get_string(val)); return; }
    if (id == PROP_ROI) { roi_set_text(s, g_value_get_string(val)); return; }
    if (id == PROP_IMG_LOCATION) { image_set_location(s, g_value_get_string(val)); return; }
    if (id == PROP_LUT3D_LOCATION) { lut3d_set_location(s, g_value_get_string(val)); return; }
    GST_OBJECT_LOCK(s);
    switch (id) {
    case PROP_SNAP_LOCATION: g_free(s->snap_location); s->snap_location = g_value_dup_string(val); s->snap_next = GST_CLOCK_TIME_NONE; break;
    case PROP_SNAP_INTERVAL: s->snap_interval = g_value_get_uint(val); break;
    case PROP_SNAP_QUALITY: s->snap_quality = g_value_get_int(val); break;
    case PROP_SNAP_REDUCE: { const gint r = g_value_get_int(val); if (r == 1 || r == 2 || r == 4 || r == 8) s->snap_reduce = r; else GST_WARNING_OBJECT(s, "snapshot-reduce %d: not 1, 2, 4 or 8; stays %d", r, s->snap_reduce); break; }
    case PROP_SNAP_SOURCE: s->snap_source = g_value_get_enum(val); break;
    case PROP_RATE_CONVERSION: s->rate_mode = g_value_get_enum(val); break; /* (these three are read at the next set_format) */
    case PROP_OUTPUT_FRAMERATE: s->out_fps_n = gst_value_get_fraction_numerator(val); s->out_fps_d = gst_value_get_fraction_denominator(val); break;
    case PROP_MAX_FILL: s->max_fill = g_value_get_int(val); break;
    case PROP_HDR_INPUT: s->hdr_input = g_value_get_enum(val); break; /* (these three are read at the next set_format) */
    case PROP_HDR_PEAK_NITS: s->hdr_peak = g_value_get_int(val); break;
    case PROP_HDR_TARGET_NITS: s->hdr_target = g_value_get_int(val); break;
    case PROP_ADJ_BRIGHTNESS: s->adj.brightness = (int)lround(1000.0 * g_value_get_double(val)); adjust_forward(s); break;
    case PROP_ADJ_CONTRAST: s->adj.contrast = (int)lround(1000.0 * g_value_get_double(val)); adjust_forward(s); break;
    case PROP_ADJ_HUE: s->adj.hue = (int)lround(1000.0 * g_value_get_double(val)); adjust_forward(s); break;
    case PROP_ADJ_SATURATION: s->adj.saturation = (int)lround(1000.0 * g_value_get_double(val)); adjust_forward(s); break;
    case PROP_ADJ_GAMMA: s->adj.gamma = (int)lround(1000.0 * g_value_get_double(val)); adjust_forward(s); break;
    case PROP_ADJ_SHARPEN: s->adj.sharpen = g_value_get_int(val); adjust_forward(s); break;
    case PROP_ADJ_SHARPEN_THRESHOLD: s->adj.sharpen_threshold = g_value_get_int(val); adjust_forward(s); break;
    case PROP_AUTO_LEVELS: s->al.levels = (int)lround(1000.0 * g_value_get_double(val)); autolevel_forward(s); break;
    case PROP_AUTO_BALANCE: s->al.balance = (int)lround(1000.0 * g_value_get_double(val)); autolevel_forward(s); break;
    case PROP_AUTO_SPEED: s->al.speed = g_value_get_int(val); autolevel_forward(s); break;
    case PROP_AUTO_CLIP: s->al.clip_low = s->al.clip_high = (int)lround(100.0 * g_value_get_double(val)); autolevel_forward(s); break;
    case PROP_AUTO_MAX_GAIN: s->al.max_gain = (int)lround(1000.0 * g_value_get_double(val)); autolevel_forward(s); break;
    case PROP_LUT3D_STRENGTH: s->lut_strength = (int)lround(256.0 * g_value_get_double(val)); lut3d_forward(s); break;
    case PROP_ROI_BALANCE: s->roi.balance = g_value_get_int(val); roi_forward(s); break;
    case PROP_MASK_COLOR: s->mask_color = g_value_get_uint(val); mask_forward(s); break;
    case PROP_DENOISE_LUMA: s->dn.luma = g_value_get_int(val); denoise_forward(s); break;
    case PROP_DENOISE_CHROMA: s->dn.chroma = g_value_get_int(val); denoise_forward(s); break;
    case PROP_DENOISE_MOTION: s->dn_motion = g_value_get_int(val); denoise_forward(s); break;
    case PROP_DS_LUMA: s->ds.luma = g_value_get_int(val); dspatial_forward(s); break;
    case PROP_DS_CHROMA: s->ds.chroma = g_value_get_int(val); dspatial_forward(s); break;
    case PROP_DS_AUTO: s->ds.auto_gain = (int)lround(1000.0 * g_value_get_double(val)); dspatial_forward(s); break;
    case PROP_DS_PERCENTILE: s->ds.percentile = g_value_get_int(val); dspatial_forward(s); break;
    case PROP_DS_SPEED: s->ds.speed = g_value_get_int(val); dspatial_forward(s); break;
    case PROP_STABILIZE: s->stab = g_value_get_int(val); break; /* (a crop change: latched in front of the next picture, the setting with it) */
    case PROP_STABILIZE_RANGE: s->stab_range = g_value_get_int(val); stabilize_forward(s); break;
    case PROP_STABILIZE_LEAK: s->stab_leak = g_value_get_int(val); stabilize_forward(s); break;
    case PROP_LENS_K1: s->warp_k1 = g_value_get_double(val); warp_forward(s); break;
    case PROP_LENS_K2: s->warp_k2 = g_value_get_double(val); warp_forward(s); break;
    case PROP_LENS_ZOOM: s->warp_zoom = g_value_get_double(val); warp_forward(s); break;
    case PROP_ROLL: s->warp_roll = g_value_get_double(val); warp_forward(s); break;
    case PROP_KEYSTONE_H: s->warp_kh = g_value_get_double(val); warp_forward(s); break;
    case PROP_KEYSTONE_V: s->warp_kv = g_value_get_double(val); warp_forward(s); break;
    case PROP_WARP_FILTER: s->warp_filter = g_value_get_enum(val); warp_forward(s); break;
    case PROP_OUTPUT_COLORIMETRY: g_free(s->out_colorimetry); s->out_colorimetry = g_value_dup_string(val); break; /* (read at the next set_format) */
    case PROP_IMG_X: s->img_x = g_value_get_int(val); image_forward(s, FALSE); break;
    case PROP_IMG_Y: s->img_y = g_value_get_int(val); image_forward(s, FALSE); break;
    case PROP_IMG_ALPHA: s->img_alpha = g_value_get_double(val); image_forward(s, FALSE); break;
    case PROP_OV_TEXT: overlay_store_text(s, g_value_get_string(val)); overlay_forward(s); break;
    case PROP_OV_HALIGN: s->ov_style.halign = g_value_get_enum(val); overlay_forward(s); break;
    case PROP_OV_VALIGN: s->ov_style.valign = g_value_get_enum(val) > 2 ? 2 : g_value_get_enum(val); overlay_forward(s); break;
    case PROP_OV_XPAD: s->ov_style.xpad = g_value_get_int(val); overlay_forward(s); break;
    case PROP_OV_YPAD: s->ov_style.ypad = g_value_get_int(val); overlay_forward(s); break;
    case PROP_OV_SCALE: s->ov_style.scale = g_value_get_int(val); overlay_forward(s); break;
    case PROP_OV_SHADED: s->ov_style.shaded_background = g_value_get_boolean(val) ? 1 : 0; overlay_forward(s); break;
    case PROP_BPS: s->rate_raw = g_value_get_uint(val); s->rate_is_bps = TRUE; if (s->enc) mi355enc_set_bitrate(s->enc, target_bps(s)); break;
    case PROP_BITRATE: s->rate_raw = g_value_get_uint(val); s->rate_is_bps = FALSE; if (s->enc) mi355enc_set_bitrate(s->enc, target_bps(s)); break;
    case PROP_KEY_INT_MAX: s->key_int_max = g_value_get_uint(val); break;
    case PROP_DEVICE_ID: s->device_id = g_value_get_int(val); break;
    case PROP_ME_RANGE: s->me_range = g_value_get_int(val); break;
    case PROP_QP: s->qp = g_value_get_int(val); if (s->enc) mi355enc_set_fixed_qp(s->enc, s->qp); break;
    case PROP_PIPELINE_DEPTH: s->pipeline_depth = g_value_get_int(val); break;
    case PROP_SPEED_PRESET: s->speed_preset = g_value_get_enum(val); break;
    case PROP_STATS: s->stats = g_value_get_boolean(val); break;
    case PROP_DCT8X8: s->dct8x8 = g_value_get_boolean(val) ? 1 : 0; break;
    case PROP_DCT8X8_ADAPTIVE: s->dct8x8_adaptive = g_value_get_boolean(val); break;
    case PROP_INTRA_REFRESH: s->intra_refresh = g_value_get_boolean(val); break;
    case PROP_QUALITY_STATS: s->quality_stats = g_value_get_boolean(val); break;
    case PROP_VIDEO_DIRECTION: { const gint d = g_value_get_enum(val); s->direction = d >= 0 && d <= GST_VIDEO_ORIENTATION_AUTO ? d : 0; break; } /* (CUSTOM: nothing here to be custom about) */
    case PROP_WIDTH: s->out_w = g_value_get_int(val); break;
    case PROP_CROP_LEFT: case PROP_CROP_RIGHT: case PROP_CROP_TOP: case PROP_CROP_BOTTOM: s->crop[id - PROP_CROP_LEFT] = g_value_get_int(val); break;
    case PROP_ADD_BORDERS: s->add_borders = g_value_get_boolean(val); break;
    case PROP_UPSCALE: s->upscale = g_value_get_boolean(val); break;
    case PROP_BORDER_COLOR: s->border_color = g_value_get_uint(val); break;
    case PROP_HEIGHT: s->out_h = g_value_get_int(val); break;
    case PROP_THREADS: s->threads = g_value_get_int(val); break;
    case PROP_SCENECUT: s->scenecut = g_value_get_boolean(val); break;
    case PROP_EXCLUSIVE: s->exclusive_gpu = g_value_get_boolean(val); break;
    case PROP_VBV: s->vbv_ms = g_value_get_uint(val); break;
    case PROP_INTRA_IN_P: s->intra_in_p = g_value_get_int(val); break;
    case PROP_PINNED_INPUT: s->pinned_input = g_value_get_boolean(val); break;
    case PROP_AQ_MODE: s->aq_mode = g_value_get_int(val); break;
    case PROP_INTRA_SLICES: s->intra_slices = g_value_get_int(val); break;
    case PROP_SLICES: s->slices = g_value_get_int(val); break;
    case PROP_SLICE_DEBLOCK: s->slice_deblock = g_value_get_boolean(val) ? 1 : 0; break;
    case PROP_I8X8: s->i8x8 = g_value_get_boolean(val) ? 1 : 0; break;
    case PROP_SINGLE_STREAM: s->single_stream = g_value_get_boolean(val); break;
    default: G_OBJECT_WARN_INVALID_PROPERTY_ID(obj, id, ps); break;
    }
    GST_OBJECT_UNLOCK(s);
}
static void get_property(GObject *obj, guint id, GValue *val, GParamSpec *ps) {
    GstMi355H264Enc *s = GST_MI355H264ENC(obj);
    toolset_t t;
    GST_OBJECT_LOCK(s);
    effective_tools(s, &t); /* a tool property reads as what the encoder will use: the explicit value, or the preset's */
    switch (id) {
    case PROP_IMG_LOCATION: g_value_set_string(val, s->img_location ? s->img_location : ""); break;
    case PROP_SNAP_LOCATION: g_value_set_string(val, s->snap_location ? s->snap_location : ""); break;
    case PROP_SNAP_INTERVAL: g_value_set_uint(val, s->snap_interval); break;
    case PROP_SNAP_QUALITY: g_value_set_int(val, s->snap_quality); break;
    case PROP_SNAP_REDUCE: g_value_set_int(val, s->snap_reduce); break;
    case PROP_SNAP_SOURCE: g_value_set_enum(val, s->snap_source); break;
    case PROP_RATE_CONVERSION: g_value_set_enum(val, s->rate_mode); break;
    case PROP_OUTPUT_FRAMERATE: gst_value_set_fraction(val, s->out_fps_n, s->out_fps_d > 0 ? s->out_fps_d : 1); break;
    case PROP_MAX_FILL: g_value_set_int(val, s->max_fill); break;
    case PROP_HDR_INPUT: g_value_set_enum(val, s->hdr_input); break;
    case PROP_HDR_PEAK_NITS: g_value_set_int(val, s->hdr_peak); break;
    case PROP_HDR_TARGET_NITS: g_value_set_int(val, s->hdr_target); break;
    case PROP_ADJ_BRIGHTNESS: g_value_set_double(val, s->adj.brightness / 1000.0); break;
    case PROP_ADJ_CONTRAST: g_value_set_double(val, s->adj.contrast / 1000.0); break;
    case PROP_ADJ_HUE: g_value_set_double(val, s->adj.hue / 1000.0); break;
    case PROP_ADJ_SATURATION: g_value_set_double(val, s->adj.saturation / 1000.0); break;
    case PROP_ADJ_GAMMA: g_value_set_double(val, s->adj.gamma / 1000.0); break;
    case PROP_ADJ_SHARPEN: g_value_set_int(val, s->adj.sharpen); break;
    case PROP_ADJ_SHARPEN_THRESHOLD: g_value_set_int(val, s->adj.sharpen_threshold); break;
    case PROP_AUTO_LEVELS: g_value_set_double(val, s->al.levels / 1000.0); break;
    case PROP_AUTO_BALANCE: g_value_set_double(val, s->al.balance / 1000.0); break;
    case PROP_AUTO_SPEED: g_value_set_int(val, s->al.speed); break;
    case PROP_AUTO_CLIP: g_value_set_double(val, s->al.clip_low / 100.0); break;
    case PROP_AUTO_MAX_GAIN: g_value_set_double(val, s->al.max_gain / 1000.0); break;
    case PROP_LUT3D_LOCATION: g_value_set_string(val, s->lut_location ? s->lut_location : ""); break;
    case PROP_LUT3D_STRENGTH: g_value_set_double(val, s->lut_strength / 256.0); break;
    case PROP_ROI: g_value_set_string(val, s->roi_text ? s->roi_text : ""); break;
    case PROP_ROI_BALANCE: g_value_set_int(val, s->roi.balance); break;
    case PROP_MASK: g_value_set_string(val, s->mask_text ? s->mask_text : ""); break;
    case PROP_MASK_COLOR: g_value_set_uint(val, s->mask_color); break;
    case PROP_DENOISE_LUMA: g_value_set_int(val, s->dn.luma); break;
    case PROP_DENOISE_CHROMA: g_value_set_int(val, s->dn.chroma); break;
    case PROP_DENOISE_MOTION: g_value_set_int(val, s->dn_motion); break;
    case PROP_DS_LUMA: g_value_set_int(val, s->ds.luma); break;
    case PROP_DS_CHROMA: g_value_set_int(val, s->ds.chroma); break;
    case PROP_DS_AUTO: g_value_set_double(val, s->ds.auto_gain / 1000.0); break;
    case PROP_DS_PERCENTILE: g_value_set_int(val, s->ds.percentile); break;
    case PROP_DS_SPEED: g_value_set_int(val, s->ds.speed); break;
    case PROP_STABILIZE: g_value_set_int(val, s->stab); break;
    case PROP_STABILIZE_RANGE: g_value_set_int(val, s->stab_range); break;
    case PROP_STABILIZE_LEAK: g_value_set_int(val, s->stab_leak); break;
    case PROP_LENS_K1: g_value_set_double(val, s->warp_k1); break;
    case PROP_LENS_K2: g_value_set_double(val, s->warp_k2); break;
    case PROP_LENS_ZOOM: g_value_set_double(val, s->warp_zoom); break;
    case PROP_ROLL: g_value_set_double(val, s->warp_roll); break;
    case PROP_KEYSTONE_H: g_value_set_double(val, s->warp_kh); break;
    case PROP_KEYSTONE_V: g_value_set_double(val, s->warp_kv); break;
    case PROP_WARP_FILTER: g_value_set_enum(val, s->warp_filter); break;
    case PROP_OUTPUT_COLORIMETRY: g_value_set_string(val, s->out_colorimetry ? s->out_colorimetry : ""); break;
    case PROP_IMG_X: g_value_set_int(val, s->img_x); break;
    case PROP_IMG_Y: g_value_set_int(val, s->img_y); break;
    case PROP_IMG_ALPHA: g_value_set_double(val, s->img_alpha); break;
    case PROP_OV_TEXT: g_value_set_string(val, s->ov_text); break;
    case PROP_OV_HALIGN: g_value_set_enum(val, s->ov_style.halign); break;
    case PROP_OV_VALIGN: g_value_set_enum(val, s->ov_style.valign); break;
    case PROP_OV_XPAD: g_value_set_int(val, s->ov_style.xpad); break;
    case PROP_OV_YPAD: g_value_set_int(val, s->ov_style.ypad); break;
    case PROP_OV_SCALE: g_value_set_int(val, s->ov_style.scale); break;
    case PROP_OV_SHADED: g_value_set_boolean(val, s->ov_style.shaded_background != 0); break;
    case PROP_BPS: g_value_set_uint(val, s->rate_is_bps ? s->rate_raw : target_bps(s) / bps_unit(s)); break;
    case PROP_BITRATE: g_value_set_uint(val, target_bps(s) / 1000u); break;
    case PROP_KEY_INT_MAX: g_value_set_uint(val, s->key_int_max); break;
    case PROP_DEVICE_ID: g_value_set_int(val, s->device_id); break;
    case PROP_ME_RANGE: g_value_set_int(val, s->me_range); break;
    case PROP_QP: g_value_set_int(val, s->qp); break;
    case PROP_PIPELINE_DEPTH: g_value_set_int(val, s->pipeline_depth); break;
    case PROP_SPEED_PRESET: g_value_set_enum(val, s->speed_preset); break;
    case PROP_STATS: g_value_set_boolean(val, s->stats); break;
    case PROP_DCT8X8: g_value_set_boolean(val, t.dct8x8 != 0); break;
    case PROP_DCT8X8_ADAPTIVE: g_value_set_boolean(val, s->dct8x8_adaptive); break;
    case PROP_INTRA_REFRESH: g_value_set_boolean(val, s->intra_refresh); break;
    case PROP_QUALITY_STATS: g_value_set_boolean(val, s->quality_stats); break;
    case PROP_VIDEO_DIRECTION: g_value_set_enum(val, s->direction); break;
    case PROP_WIDTH: g_value_set_int(val, s->out_w); break;
    case PROP_CROP_LEFT: case PROP_CROP_RIGHT: case PROP_CROP_TOP: case PROP_CROP_BOTTOM: g_value_set_int(val, s->crop[id - PROP_CROP_LEFT]); break;
    case PROP_ADD_BORDERS: g_value_set_boolean(val, s->add_borders); break;
    case PROP_UPSCALE: g_value_set_boolean(val, s->upscale); break;
    case PROP_BORDER_COLOR: g_value_set_uint(val, s->border_color); break;
    case PROP_HEIGHT: g_value_set_int(val, s->out_h); break;
    case PROP_THREADS: g_value_set_int(val, s->threads); break;
    case PROP_SCENECUT: g_value_set_boolean(val, s->scenecut); break;
    case PROP_EXCLUSIVE: g_value_set_boolean(val, s->exclusive_gpu); break;
    case PROP_VBV: g_value_set_uint(val, s->vbv_ms); break;
    case PROP_INTRA_IN_P: g_value_set_int(val, t.intra_in_p); break;
    case PROP_PINNED_INPUT: g_value_set_boolean(val, s->pinned_input); break;
    case PROP_AQ_MODE: g_value_set_int(val, t.aq_mode); break;
    case PROP_INTRA_SLICES: g_value_set_int(val, s->intra_slices); break;
    case PROP_SLICES: g_value_set_int(val, t.slices < 0 ? 0 : t.slices); break;
    case PROP_SLICE_DEBLOCK: g_value_set_boolean(val, t.slice_deblock != 0); break; /* (unset: the library's default, on) */
    case PROP_I8X8: g_value_set_boolean(val, t.i8x8 != 0); break;
    case PROP_SINGLE_STREAM: g_value_set_boolean(val, s->single_stream); break;
    default: G_OBJECT_WARN_INVALID_PROPERTY_ID(obj, id, ps); break;
    }
    GST_OBJECT_UNLOCK(s);
}

static void close_encoder(GstMi355H264Enc *s) {
    mi355enc_t *e;
    g_mutex_lock(&s->snap_enc_mu); /* (the stills' helper is not inside the encoder from here on) */
    GST_OBJECT_LOCK(s);
    e = s->enc; s->enc = NULL;
    GST_OBJECT_UNLOCK(s);
    g_mutex_unlock(&s->snap_enc_mu);
    if (e) {
        if (s->stats) {
            mi355enc_stats_t st;
            if (mi355enc_get_stats(e, &st) == 0)
                g_printerr("{\"element\":\"mi355h264enc\",\"frames\":%" G_GUINT64_FORMAT ",\"idr\":%" G_GUINT64_FORMAT ",\"bytes\":%" G_GUINT64_FORMAT
                           ",\"ms_entropy\":%.3f,\"ms_wait\":%.3f,\"last_qp\":%u,\"open_ms\":%.1f,\"target_bps\":%u"
                           ",\"streaming_thread_us_per_frame\":{\"map_input\":%.1f,\"submit\":%.1f,\"collect\":%.1f,\"output_buffer\":%.1f,\"push_downstream\":%.1f}}\n", st.frames, st.idr_frames, st.bytes,
                           st.ms_entropy, st.ms_wait, st.last_qp, st.ms_open, st.target_bps, (double)s->us_map / (double)(s->us_frames ? s->us_frames : 1),
                           (double)s->us_submit / (double)(s->us_frames ? s->us_frames : 1), (double)s->us_collect / (double)(s->us_frames ? s->us_frames : 1),
                           (double)s->us_output / (double)(s->us_frames ? s->us_frames : 1), (double)s->us_push / (double)(s->us_frames ? s->us_frames : 1));
            mi355enc_quality_t q; /* (MI355ENC_ERR_STATE unless quality-stats=true) */
            if (mi355enc_quality_totals(e, &q) == 0 && q.pictures)
                g_printerr("{\"element\":\"mi355h264enc\",\"quality\":{\"pictures\":%" G_GUINT64_FORMAT ",\"psnr_y\":%.3f,\"psnr_cb\":%.3f,\"psnr_cr\":%.3f,\"ssim\":%.5f}}\n",
                           q.pictures, q.psnr[0], q.psnr[1], q.psnr[2], q.ssim);
            g_mutex_lock(&s->snap_mu);
            const guint64 n_stills = s->snap_count;
            g_mutex_unlock(&s->snap_mu);
            if (n_stills) g_printerr("{\"element\":\"mi355h264enc\",\"snapshots\":%" G_GUINT64_FORMAT "}\n", n_stills);
        }
        mi355enc_close(e);
    }
}
/* ---- JPEG stills: the helper thread */
static void snapshot_write_file(GstMi355H264Enc *s, const guint8 *data, gsize len, const mi355enc_snapshot_info_t *info) {
    GST_OBJECT_LOCK(s);
    gchar *loc = g_strdup(s->snap_location ? s->snap_location : "");
    GST_OBJECT_UNLOCK(s);
    if (*loc) {
        gchar *tmp = g_strconcat(loc, ".tmp", NULL);
        int why = 0; /* errno of the step that failed first */
        FILE *f = fopen(tmp, "wb");
        gboolean ok = f != NULL;
        if (!ok) why = errno;
        if (ok && fwrite(data, 1, len, f) != len) { ok = FALSE; why = errno; }
        if (f && fclose(f) != 0 && ok) { ok = FALSE; why = errno; }
        if (ok && g_rename(tmp, loc) != 0) { ok = FALSE; why = errno; }
        if (ok) {
            g_mutex_lock(&s->snap_mu);
            s->snap_count++;
            g_mutex_unlock(&s->snap_mu);
            gst_element_post_message(GST_ELEMENT(s), gst_message_new_element(GST_OBJECT(s), gst_structure_new("mi355-snapshot", "location", G_TYPE_STRING, loc,
                "width", G_TYPE_INT, info->width, "height", G_TYPE_INT, info->height, "pts", G_TYPE_UINT64, (guint64)info->pts, "bytes", G_TYPE_UINT64, (guint64)len, NULL)));
        } else GST_ELEMENT_WARNING(s, RESOURCE, WRITE, ("mi355h264enc: cannot write the still %s", loc), ("%s", g_strerror(why))); /* a warning, never an error: the stream goes on */
        g_free(tmp);
    }
    g_free(loc);
}
static gpointer snapshot_helper(gpointer u) {
    GstMi355H264Enc *s = (GstMi355H264Enc *)u;
    guint8 *buf = NULL;
    gsize cap = 0;
    gboolean have_last = FALSE;
    guint64 last_index = 0;
    gint64 last_pts = 0;
    guint gen = 0;
    for (;;) {
        g_mutex_lock(&s->snap_mu);
        while (!s->snap_wake && !s->snap_stop) g_cond_wait(&s->snap_cv, &s->snap_mu);
        const gboolean stop = s->snap_stop;
        s->snap_wake = 0;
        g_mutex_unlock(&s->snap_mu);
        if (stop) break;
        mi355enc_snapshot_info_t info;
        size_t len = 0;
        int r = MI355ENC_ERR_STATE;
        g_mutex_lock(&s->snap_enc_mu);
        if (s->snap_gen != gen) { gen = s->snap_gen; have_last = FALSE; } /* another encoder: its pictures count from 0 again */
        if (s->enc) {
            r = mi355enc_take_snapshot(s->enc, buf, cap, &len, &info);
            if (r == MI355ENC_ERR_OVERFLOW && !(have_last && info.index == last_index && info.pts == last_pts)) { /* a new still that needs more room */
                g_free(buf); cap = len + len / 4; buf = (guint8 *)g_malloc(cap);
                r = mi355enc_take_snapshot(s->enc, buf, cap, &len, &info);
            }
        }
        g_mutex_unlock(&s->snap_enc_mu);
        if (r != MI355ENC_OK || (have_last && info.index == last_index && info.pts == last_pts)) continue; /* nothing ready, or the still already written */
        have_last = TRUE; last_index = info.index; last_pts = info.pts;
        snapshot_write_file(s, buf, len, &info);
    }
    g_free(buf);
    return NULL;
}
static void snapshot_wake(GstMi355H264Enc *s) {
    g_mutex_lock(&s->snap_mu);
    if (!s->snap_thread) { s->snap_stop = FALSE; s->snap_thread = g_thread_new("mi355-snapshot", snapshot_helper, s); }
    s->snap_wake = 1;
    g_cond_signal(&s->snap_cv);
    g_mutex_unlock(&s->snap_mu);
}
static void snapshot_stop(GstMi355H264Enc *s) {
    g_mutex_lock(&s->snap_mu);
    GThread *t = s->snap_thread;
    s->snap_thread = NULL; s->snap_stop = TRUE;
    g_cond_signal(&s->snap_cv);
    g_mutex_unlock(&s->snap_mu);
    if (t) g_thread_join(t);
}
/* streaming thread, in front of a picture's submit: every snapshot-interval of stream time one picture is armed */
static void snapshot_maybe_arm(GstMi355H264Enc *s, GstVideoCodecFrame *frame) {
    GST_OBJECT_LOCK(s);
    const gboolean on = s->snap_location && *s->snap_location;
    const mi355enc_snapshot_req_t req = {s->snap_source, s->snap_reduce, s->snap_quality};
    const GstClockTime step = (GstClockTime)s->snap_interval * GST_MSECOND, pts = frame->pts;
    const gboolean due = !(GST_CLOCK_TIME_IS_VALID(s->snap_next) && GST_CLOCK_TIME_IS_VALID(pts) && pts < s->snap_next);
    if (on && due) s->snap_next = GST_CLOCK_TIME_IS_VALID(pts) ? pts + step : GST_CLOCK_TIME_NONE;
    GST_OBJECT_UNLOCK(s);
    if (!on || !due) return;
    if (mi355enc_request_snapshot(s->enc, &req) != MI355ENC_OK) return;
    s->snap_watch = s->open_depth + 2;
}
static gboolean enc_stop(GstVideoEncoder *ve) {
    GstMi355H264Enc *s = GST_MI355H264ENC(ve);
    snapshot_stop(s);
    close_encoder(s);
    if (s->input_state) { gst_video_codec_state_unref(s->input_state); s->input_state = NULL; }
    g_free(s->au_buf); s->au_buf = NULL;
    return TRUE;
}
static GstFlowReturn drain(GstMi355H264Enc *s, gboolean push);
static gboolean enc_start(GstVideoEncoder *ve) {
    (void)ve;
    return TRUE; /* geometry is unknown until set_format; the device is opened there, still before data flows */
}

/* the formats of mi355enc.h beyond the first four; -1: none of them.  An alpha byte is ignored like a padding byte */
static int rgb_or_planar_fmt(GstVideoFormat f) {
    switch (f) {
    case GST_VIDEO_FORMAT_Y42B: return MI355ENC_FMT_Y42B;
    case GST_VIDEO_FORMAT_Y444: return MI355ENC_FMT_Y444;
    case GST_VIDEO_FORMAT_YV12: return MI355ENC_FMT_YV12;
    case GST_VIDEO_FORMAT_NV21: return MI355ENC_FMT_NV21;
    case GST_VIDEO_FORMAT_BGRx: case GST_VIDEO_FORMAT_BGRA: return MI355ENC_FMT_BGRX;
    case GST_VIDEO_FORMAT_RGBx: case GST_VIDEO_FORMAT_RGBA: return MI355ENC_FMT_RGBX;
    case GST_VIDEO_FORMAT_xRGB: case GST_VIDEO_FORMAT_ARGB: return MI355ENC_FMT_XRGB;
    case GST_VIDEO_FORMAT_xBGR: case GST_VIDEO_FORMAT_ABGR: return MI355ENC_FMT_XBGR;
    case GST_VIDEO_FORMAT_BGR: return MI355ENC_FMT_BGR;
    case GST_VIDEO_FORMAT_RGB: return MI355ENC_FMT_RGB;
    case GST_VIDEO_FORMAT_P010_10LE: return MI355ENC_FMT_P010; /* 10-bit and grey */
    case GST_VIDEO_FORMAT_I420_10LE: return MI355ENC_FMT_I420_10;
    case GST_VIDEO_FORMAT_v210: return MI355ENC_FMT_V210;
    case GST_VIDEO_FORMAT_GRAY8: return MI355ENC_FMT_GRAY8;
    default: return -1;
    }
}
/* GstVideoColorimetry -> the code points of H.264 Tables E-3 / E-4 / E-5 (GStreamer 1.14 has no gst_video_color_*_to_iso); what has no code point: 2,
 * unspecified.  The transfer function of BT.709 beside the BT.601 matrix is written as 6 (SMPTE 170M: the same curve under its standard-definition
 * name, what later GStreamer versions call GST_VIDEO_TRANSFER_BT601), so that `colorimetry=bt601` reads 6 / 6 / 6. */
static void colorimetry_codes(const GstVideoColorimetry *c, int *full, int *prim, int *trc, int *mat) {
    *full = c->range == GST_VIDEO_COLOR_RANGE_0_255;
    switch (c->primaries) {
    case GST_VIDEO_COLOR_PRIMARIES_BT709: *prim = 1; break;
    case GST_VIDEO_COLOR_PRIMARIES_BT470M: *prim = 4; break;
    case GST_VIDEO_COLOR_PRIMARIES_BT470BG: *prim = 5; break;
    case GST_VIDEO_COLOR_PRIMARIES_SMPTE170M: *prim = 6; break;
    case GST_VIDEO_COLOR_PRIMARIES_SMPTE240M: *prim = 7; break;
    case GST_VIDEO_COLOR_PRIMARIES_FILM: *prim = 8; break;
    case GST_VIDEO_COLOR_PRIMARIES_BT2020: *prim = 9; break;
    default: *prim = 2; break;
    }
    switch (c->matrix) {
    case GST_VIDEO_COLOR_MATRIX_RGB: *mat = 0; break;
    case GST_VIDEO_COLOR_MATRIX_FCC: *mat = 4; break;
    case GST_VIDEO_COLOR_MATRIX_BT709: *mat = 1; break;
    case GST_VIDEO_COLOR_MATRIX_BT601: *mat = 6; break;
    case GST_VIDEO_COLOR_MATRIX_SMPTE240M: *mat = 7; break;
    case GST_VIDEO_COLOR_MATRIX_BT2020: *mat = 9; break;
    default: *mat = 2; break;
    }
    switch (c->transfer) {
    case GST_VIDEO_TRANSFER_GAMMA10: *trc = 8; break;
    case GST_VIDEO_TRANSFER_GAMMA22: *trc = 4; break;
    case GST_VIDEO_TRANSFER_GAMMA28: *trc = 5; break;
    case GST_VIDEO_TRANSFER_BT709: *trc = c->matrix == GST_VIDEO_COLOR_MATRIX_BT601 ? 6 : 1; break;
    case GST_VIDEO_TRANSFER_SMPTE240M: *trc = 7; break;
    case GST_VIDEO_TRANSFER_SRGB: *trc = 13; break;
    case GST_VIDEO_TRANSFER_LOG100: *trc = 9; break;
    case GST_VIDEO_TRANSFER_LOG316: *trc = 10; break;
    case GST_VIDEO_TRANSFER_BT2020_12: *trc = 15; break;
    default: *trc = 2; break;
    }
}

/* video-direction: the method in force (object lock held) -- the property, or with AUTO what the last image-orientation tag said */
static int effective_direction(GstMi355H264Enc *s) { return s->direction == GST_VIDEO_ORIENTATION_AUTO ? s->tag_direction : s->direction; }
static gboolean direction_transposes(int d) { return d == GST_VIDEO_ORIENTATION_90R || d == GST_VIDEO_ORIENTATION_90L || d == GST_VIDEO_ORIENTATION_UL_LR || d == GST_VIDEO_ORIENTATION_UR_LL; }
/* image-orientation tag -> direction (the table of gst_video_orientation_from_tag, which GStreamer has from 1.20 on); FALSE: no such tag, or a value outside the table */
static gboolean direction_from_tag(GstTagList *tl, int *dir) {
#if GST_CHECK_VERSION(1, 20, 0)
    GstVideoOrientationMethod m;
    if (!gst_video_orientation_from_tag(tl, &m)) return FALSE;
    *dir = (int)m;
    return TRUE;
#else
    static const struct { const char *tag; int dir; } tab[] = {{"rotate-0", GST_VIDEO_ORIENTATION_IDENTITY}, {"rotate-90", GST_VIDEO_ORIENTATION_90R}, {"rotate-180", GST_VIDEO_ORIENTATION_180},
        {"rotate-270", GST_VIDEO_ORIENTATION_90L}, {"flip-rotate-0", GST_VIDEO_ORIENTATION_HORIZ}, {"flip-rotate-90", GST_VIDEO_ORIENTATION_UR_LL},
        {"flip-rotate-180", GST_VIDEO_ORIENTATION_VERT}, {"flip-rotate-270", GST_VIDEO_ORIENTATION_UL_LR}};
    gchar *v = NULL;
    gboolean ok = FALSE;
    if (!gst_tag_list_get_string(tl, GST_TAG_IMAGE_ORIENTATION, &v) || !v) return FALSE;
    for (guint i = 0; i < G_N_ELEMENTS(tab); i++) if (!g_ascii_strcasecmp(v, tab[i].tag)) { *dir = tab[i].dir; ok = TRUE; }
    g_free(v);
    return ok;
#endif
}

static gboolean enc_set_format(GstVideoEncoder *ve, GstVideoCodecState *state) {
    GstMi355H264Enc *s = GST_MI355H264ENC(ve);
    GstVideoInfo *vi = &state->info;
    mi355enc_cfg_t cfg;
    mi355enc_t *e = NULL;
    int fn = GST_VIDEO_INFO_FPS_N(vi), fd = GST_VIDEO_INFO_FPS_D(vi);
    if (fn <= 0 || fd <= 0) { fn = 30; fd = 1; } /* variable framerate: rate control assumes 30 */
    if (s->enc) drain(s, TRUE); /* renegotiation in mid-stream: the picture still on the device belongs to the old format (x264enc flushes here too) */
    close_encoder(s);
    const int in_w = GST_VIDEO_INFO_WIDTH(vi), in_h = GST_VIDEO_INFO_HEIGHT(vi);
    /* MJPEG input: size and framerate come from the caps, the pictures are decoded on the way in */
    const GstStructure *cs = state->caps ? gst_caps_get_structure(state->caps, 0) : NULL;
    const gboolean jpeg = cs && gst_structure_has_name(cs, "image/jpeg");
    if (jpeg && (in_w < 16 || in_h < 16)) {
        GST_ELEMENT_ERROR(s, CORE, NEGOTIATION, ("mi355h264enc: image/jpeg caps need width and height"), ("caps without a size"));
        return FALSE;
    }
    /* output-colorimetry: the coded samples' meaning where it is not to be the input's */
    GstVideoColorimetry out_col;
    GST_OBJECT_LOCK(s);
    gchar *out_str = s->out_colorimetry && *s->out_colorimetry ? g_strdup(s->out_colorimetry) : NULL;
    GST_OBJECT_UNLOCK(s);
    const gboolean convert = out_str != NULL;
    if (out_str && !gst_video_colorimetry_from_string(&out_col, out_str)) {
        GST_ELEMENT_ERROR(s, LIBRARY, SETTINGS, ("mi355h264enc: output-colorimetry=%s is not a colorimetry", out_str), ("gst_video_colorimetry_from_string failed"));
        g_free(out_str);
        return FALSE;
    }
    g_free(out_str);
    GST_OBJECT_LOCK(s);
    const int dir = effective_direction(s);
    const gboolean tr = direction_transposes(dir);
    /* the crop rectangle (section 16): all four at 0 is the whole input */
    int crop[4];
    effective_crop(s, crop); /* (with the stabiliser's margin: the crop leaves that much room around it) */
    const int crop_w = in_w - crop[0] - crop[1], crop_h = in_h - crop[2] - crop[3];
    const gboolean add_borders = s->add_borders, upscale = s->upscale;
    const guint border = s->border_color;
    /* width / height mean the coded, i.e. oriented, size; 0: the oriented (cropped) input's.  What the input is scaled to is that size turned back */
    const int out_w = s->out_w > 0 ? s->out_w : (tr ? crop_h : crop_w), out_h = s->out_h > 0 ? s->out_h : (tr ? crop_w : crop_h);
    GST_OBJECT_UNLOCK(s);
    const int pre_w = tr ? out_h : out_w, pre_h = tr ? out_w : out_h;
    /* a geometry only where today's path cannot do it: a crop, borders, or a size above the input's that `upscale` allows */
    const gboolean geom = crop[0] || crop[1] || crop[2] || crop[3] || add_borders || (upscale && (pre_w > in_w || pre_h > in_h));
    mi355enc_geometry_t gm;
    memset(&gm, 0, sizeof gm);
    if (geom) {
        if (crop_w < 2 || crop_h < 2 || out_w < 16 || out_h < 16) {
            GST_ELEMENT_ERROR(s, CORE, NEGOTIATION, ("mi355h264enc: the crop leaves no picture"), ("crop %d/%d/%d/%d of %dx%d", crop[0], crop[1], crop[2], crop[3], in_w, in_h));
            return FALSE;
        }
        gm.in_w = in_w; gm.in_h = in_h;
        gm.crop_x = crop[0]; gm.crop_y = crop[2]; gm.crop_w = crop_w; gm.crop_h = crop_h;
        gm.dst_w = pre_w; gm.dst_h = pre_h;
        if (add_borders) { /* the picture keeps its shape; the rounding to even sizes is not an aspect ratio anybody meant: nothing from it in the SPS */
            mi355enc_fit_rect(crop_w, crop_h, pre_w, pre_h, &gm.dst_x, &gm.dst_y, &gm.dst_w, &gm.dst_h);
            gm.flags = MI355ENC_GEOM_KEEP_SAR;
        }
        gm.border_y = (border >> 16) & 255; gm.border_cb = (border >> 8) & 255; gm.border_cr = border & 255;
        if (!upscale && (gm.dst_w > crop_w || gm.dst_h > crop_h)) {
            GST_ELEMENT_ERROR(s, CORE, NEGOTIATION, ("mi355h264enc: width / height above the input's need upscale=true"), ("%dx%d from %dx%d", gm.dst_w, gm.dst_h, crop_w, crop_h));
            return FALSE;
        }
    }
    mi355enc_default_cfg(&cfg, out_w, out_h, fn, fd);
    GST_OBJECT_LOCK(s);
    cfg.gop = s->key_int_max ? (int)s->key_int_max : 250;
    cfg.me_range = s->me_range; cfg.bitrate_bps = target_bps(s); cfg.device_id = s->device_id; cfg.fixed_qp = s->qp;
    cfg.pipeline_depth = s->pipeline_depth; cfg.cavlc_threads = s->threads > 0 ? s->threads : 0; cfg.scenecut = s->scenecut ? 1 : 0; cfg.exclusive_device = s->exclusive_gpu ? 1 : 0; cfg.vbv_ms = (int)s->vbv_ms;
    cfg.single_stream = s->single_stream ? 1 : 0; cfg.intra_slices = s->intra_slices;
    {
        toolset_t t;
        effective_tools(s, &t);
        cfg.transform8x8 = t.dct8x8 ? (s->dct8x8_adaptive ? 2 : 1) : 0; cfg.i8x8 = t.i8x8; cfg.aq_mode = t.aq_mode; cfg.partitions = t.partitions; cfg.intra_in_p = t.intra_in_p;
        if (t.slices >= 0) cfg.slices = t.slices;               /* (-1: mi355enc_default_cfg's) */
        if (t.slice_deblock >= 0) cfg.slice_deblock = t.slice_deblock;
    }
    const gboolean intra_refresh = s->intra_refresh, quality_stats = s->quality_stats;
    const int rate_mode = s->rate_mode, max_fill = s->max_fill;
    const int hdr_input = s->hdr_input, hdr_peak = s->hdr_peak, hdr_target = s->hdr_target;
    if (rate_mode && s->out_fps_n > 0 && s->out_fps_d > 0) { cfg.fps_num = fn = s->out_fps_n; cfg.fps_den = fd = s->out_fps_d; } /* the encoder runs at the output rate: rate control and the VUI follow the ticks */
    if (intra_refresh) { cfg.partitions = 0; if (!cfg.intra_in_p) cfg.intra_in_p = 1; } /* (the refresh columns are intra macroblocks of P pictures; no partitions) */
    GST_OBJECT_UNLOCK(s);
    /* hdr-input: GStreamer 1.14's caps cannot say PQ or HLG, so the property does; only the three 10-bit formats can be HDR here */
    if (hdr_input) {
        const GstVideoFormat f = jpeg ? GST_VIDEO_FORMAT_UNKNOWN : GST_VIDEO_INFO_FORMAT(vi);
        if (f != GST_VIDEO_FORMAT_P010_10LE && f != GST_VIDEO_FORMAT_I420_10LE && f != GST_VIDEO_FORMAT_v210) {
            GST_ELEMENT_ERROR(s, CORE, NEGOTIATION, ("mi355h264enc: hdr-input needs P010_10LE, I420_10LE or v210 input"), ("caps %s", jpeg ? "image/jpeg" : gst_video_format_to_string(f)));
            return FALSE;
        }
    }
    int r = mi355enc_open(&cfg, &e);
    if (r == MI355ENC_OK && intra_refresh) r = mi355enc_set_intra_refresh(e, 1); /* (refused with key-int-max < 2) */
    if (r == MI355ENC_OK) { /* what the samples mean goes into the SPS (x264enc copies its input caps' colorimetry likewise); YUV input is only labelled */
        int full, prim, trc, mat;
        colorimetry_codes(&vi->colorimetry, &full, &prim, &trc, &mat);
        if (jpeg && !gst_structure_has_field(cs, "colorimetry")) { full = 1; mat = 6; prim = trc = 2; } /* JFIF: what the caps of a `jpegdec` in front would have said */
        if (GST_VIDEO_INFO_IS_RGB(vi) && mat != 1 && mat != 6 && mat != 9) {
            /* RGB is converted here: with what `videoconvert` would have negotiated for the encoder's input -- BT.709 for HD, BT.601 below, limited range */
            prim = trc = mat = (out_w > 1024 || out_h > 576) ? 1 : 6;
            full = 0;
        } else if (GST_VIDEO_INFO_IS_RGB(vi)) full = 0;
        if (hdr_input) { /* tone-mapped to SDR: the caps give the input's range only; the SPS says output-colorimetry, else BT.709 limited -- never the caps' bt2020 label */
            const int in_full = full;
            full = 0; prim = trc = mat = 1;
            if (convert) {
                colorimetry_codes(&out_col, &full, &prim, &trc, &mat);
                if (mat != 1 && mat != 2 && mat != 5 && mat != 6) r = MI355ENC_ERR_ARG; /* (the library would refuse the first picture) */
            }
            if (r == MI355ENC_OK) r = mi355enc_set_hdr_input(e, hdr_input, in_full, hdr_peak, hdr_target); /* (refused: a peak or target outside the setter's range) */
        } else if (convert) { /* the SPS carries the output's codes; YUV input is converted to them on the device from what the caps say it is, RGB straight to them */
            const int in_full = full, in_mat = mat;
            colorimetry_codes(&out_col, &full, &prim, &trc, &mat);
            if (mat != 1 && mat != 2 && mat != 5 && mat != 6 && mat != 9) r = MI355ENC_ERR_ARG; /* (the library would refuse the first picture) */
            if (r == MI355ENC_OK && !GST_VIDEO_INFO_IS_RGB(vi)) r = mi355enc_set_input_colorimetry(e, in_full, in_mat); /* (refused: an input matrix outside 1, 5, 6, 9, 2) */
        }
        if (r == MI355ENC_OK) r = mi355enc_set_colorimetry(e, full, prim, trc, mat);
    }
    if (r == MI355ENC_OK && dir != 0) r = mi355enc_set_orientation(e, dir); /* (first: the input size is then checked against the pre-orientation target) */
    if (r == MI355ENC_OK && geom) r = mi355enc_set_input_geometry(e, &gm); /* (refused: a ratio above 8 either way, odd sizes) */
    else if (r == MI355ENC_OK && (in_w != pre_w || in_h != pre_h)) r = mi355enc_set_input_size(e, in_w, in_h); /* (refused: upscaling, a ratio above 8, odd sizes) */
    if (r == MI355ENC_OK && quality_stats) r = mi355enc_set_quality_metrics(e, 1);
    if (r == MI355ENC_OK && rate_mode) { const mi355enc_rate_t rt = {rate_mode, GST_SECOND, max_fill}; r = mi355enc_set_rate_conversion(e, &rt); }
    if (r != MI355ENC_OK) {
        if (e) mi355enc_close(e);
        GST_ELEMENT_ERROR(s, LIBRARY, INIT, ("mi355h264enc: cannot open the MI355X encoder: %s", mi355enc_strerror(r)),
                          ("mi355enc_open(%dx%d from %dx%d input, device-id=%d) returned %d", cfg.width, cfg.height, in_w, in_h, cfg.device_id, r));
        return FALSE;
    }
    g_mutex_lock(&s->snap_enc_mu); /* (the stills' helper sees the encoder change under this one; same order as close_encoder) */
    GST_OBJECT_LOCK(s);
    s->enc = e;
    s->snap_gen++; s->snap_next = GST_CLOCK_TIME_NONE; s->snap_watch = 0; /* stills start over with the new encoder */
    s->open_depth = cfg.pipeline_depth;
    s->open_rate = rate_mode; s->tick = gst_util_uint64_scale(GST_SECOND, (guint64)fd, (guint64)fn); s->rate_qh = s->rate_qn = 0;
    s->open_direction = dir;
    s->open_geom = geom;
    memcpy(s->open_crop, crop, sizeof crop);
    s->jpeg = jpeg; s->jpeg_refused = 0;
    mi355enc_set_bitrate(e, target_bps(s)); /* a write that raced with open() must not be lost */
    overlay_forward(s);                     /* ... nor the overlay's text and style, set before the device was opened */
    image_forward(s, TRUE);                 /* ... nor the image layer */
    adjust_forward(s);                      /* ... nor the picture controls */
    autolevel_forward(s);                   /* ... nor the automatic levels and white balance */
    lut3d_forward(s);                       /* ... nor the 3D LUT */
    roi_forward(s);                         /* ... nor the region of interest */
    mask_forward(s);                        /* ... nor the privacy masks */
    denoise_forward(s);                     /* ... nor the noise filter */
    dspatial_forward(s);                    /* ... nor the spatial noise filter */
    stabilize_forward(s);                   /* ... nor the stabiliser */
    warp_forward(s);                        /* ... nor the warp */
    GST_OBJECT_UNLOCK(s);
    g_mutex_unlock(&s->snap_enc_mu);
    s->max_au = mi355enc_max_au_bytes(e);
    g_free(s->au_buf);
    s->au_buf = g_malloc(s->max_au);
    s->last_pts = GST_CLOCK_TIME_NONE;
    {
        mi355enc_stats_t st;
        if (mi355enc_get_stats(e, &st) == 0)
            GST_INFO_OBJECT(s, "opened %dx%d @%d/%d on device %d in %.1f ms, target %u bit/s, gop %d", cfg.width, cfg.height, fn, fd, cfg.device_id, st.ms_open, cfg.bitrate_bps, cfg.gop);
    }
    if (s->input_state) gst_video_codec_state_unref(s->input_state);
    s->input_state = gst_video_codec_state_ref(state);
    GstCaps *caps = gst_caps_new_simple("video/x-h264", "stream-format", G_TYPE_STRING, "byte-stream", "alignment", G_TYPE_STRING, "au",
                                        "profile", G_TYPE_STRING, cfg.transform8x8 ? "high" : "constrained-baseline", NULL);
    GstVideoCodecState *out = gst_video_encoder_set_output_state(ve, caps, state);
    if (in_w != out_w || in_h != out_h || tr) { /* the coded size; a scale that changes the aspect ratio changes the samples' (the SPS VUI carries the same), and a
                                                   transposing direction exchanges the size and the two terms of the pixel-aspect-ratio */
        out->info.width = out_w; out->info.height = out_h;
        gint pn = 1, pd = 1;
        if (geom && add_borders) { pn = GST_VIDEO_INFO_PAR_N(vi); pd = GST_VIDEO_INFO_PAR_D(vi); } /* (the picture keeps its shape, so the samples keep theirs) */
        else if (geom) gst_util_fraction_multiply(GST_VIDEO_INFO_PAR_N(vi), GST_VIDEO_INFO_PAR_D(vi), crop_w * pre_h, crop_h * pre_w, &pn, &pd);
        else gst_util_fraction_multiply(GST_VIDEO_INFO_PAR_N(vi), GST_VIDEO_INFO_PAR_D(vi), in_w * pre_h, in_h * pre_w, &pn, &pd);
        out->info.par_n = tr ? pd : pn; out->info.par_d = tr ? pn : pd;
    }
    if (rate_mode) { out->info.fps_n = fn; out->info.fps_d = fd; } /* the source caps carry the output rate */
    gst_video_codec_state_unref(out);
    if (cfg.pipeline_depth > 0) {
        GstClockTime d = gst_util_uint64_scale(GST_SECOND, (guint64)fd * cfg.pipeline_depth, fn);
        gst_video_encoder_set_latency(ve, d, d);
    }
    return gst_video_encoder_negotiate(ve);
}

/* entropy-code the oldest submitted picture and push it in a buffer of exactly its size (the worst case, max_au, is
 * 12 MB at 1080p: buffers of that capacity would sit in the downstream queues of the reference's pipelines, which hold up
 * to 1000 of them -- pipeline/generic/x264_superfast_camlink:7) */
static GstFlowReturn collect_into(GstMi355H264Enc *s, GstVideoCodecFrame *frame) {
    GstVideoEncoder *ve = GST_VIDEO_ENCODER(s);
    size_t len = 0;
    int key = 0, qp = 0;
    const gint64 t0 = g_get_monotonic_time();
    int64_t tick_pts = 0;
    int r = mi355enc_collect(s->enc, s->au_buf, s->max_au, &len, &key, &tick_pts, &qp);
    const gint64 t1 = g_get_monotonic_time();
    s->us_collect += t1 - t0;
    if (r != MI355ENC_OK) {
        GST_ELEMENT_ERROR(s, STREAM, ENCODE, ("mi355h264enc: encode failed: %s", mi355enc_strerror(r)), ("mi355enc_collect returned %d", r));
        gst_video_encoder_finish_frame(ve, frame);
        return GST_FLOW_ERROR;
    }
    if (s->snap_watch > 0) { s->snap_watch--; snapshot_wake(s); } /* an armed picture may just have been collected: the helper looks */
    if (s->open_rate && s->rate_qn && s->rate_q[s->rate_qh] > 1) {
        /* frame-rate conversion: a picture in front of the frame's own (a repeat, or an earlier mix of the same pair) leaves as a buffer of its own, with its
         * tick's PTS; the frame stays the oldest one */
        s->rate_q[s->rate_qh]--;
        GstBuffer *b = gst_buffer_new_allocate(NULL, len, NULL);
        if (!b) { gst_video_codec_frame_unref(frame); return GST_FLOW_ERROR; }
        gst_buffer_fill(b, 0, s->au_buf, len);
        GstClockTime t = (GstClockTime)tick_pts;
        if (GST_CLOCK_TIME_IS_VALID(s->last_pts) && t < s->last_pts) t = s->last_pts;
        s->last_pts = t;
        GST_BUFFER_PTS(b) = GST_BUFFER_DTS(b) = t;
        GST_BUFFER_DURATION(b) = s->tick;
        if (!key) GST_BUFFER_FLAG_SET(b, GST_BUFFER_FLAG_DELTA_UNIT);
        gst_video_codec_frame_unref(frame); /* (get_oldest_frame's reference) */
        return gst_pad_push(GST_VIDEO_ENCODER_SRC_PAD(ve), b);
    }
    if (s->open_rate) { /* the frame's own picture: it carries its tick's PTS, not the input's */
        if (s->rate_qn) { s->rate_qh = (s->rate_qh + 1) % G_N_ELEMENTS(s->rate_q); s->rate_qn--; }
        frame->pts = (GstClockTime)tick_pts; frame->duration = s->tick;
    }
    GstFlowReturn fr = gst_video_encoder_allocate_output_frame(ve, frame, len);
    if (fr != GST_FLOW_OK) { gst_video_encoder_finish_frame(ve, frame); return fr; }
    gst_buffer_fill(frame->output_buffer, 0, s->au_buf, len);
    if (key) GST_VIDEO_CODEC_FRAME_SET_SYNC_POINT(frame);
    else GST_VIDEO_CODEC_FRAME_UNSET_SYNC_POINT(frame);
    /* No reordering: DTS = PTS.  Upstream (`identity name=ptsfixup`, ceracoder.c:371-423) rewrites PTS onto a fixed grid and
     * zeroes DTS; whatever arrives, the PTS sequence leaving here never runs backwards (mpegtsmux and SRT receivers reject
     * that), so a picture stamped at or before its predecessor takes the predecessor's stamp. */
    if (GST_CLOCK_TIME_IS_VALID(frame->pts) && GST_CLOCK_TIME_IS_VALID(s->last_pts) && frame->pts < s->last_pts) frame->pts = s->last_pts;
    if (GST_CLOCK_TIME_IS_VALID(frame->pts)) s->last_pts = frame->pts;
    frame->dts = frame->pts;
    GST_LOG_OBJECT(s, "access unit %" G_GSIZE_FORMAT " bytes, %s, qp %d, pts %" GST_TIME_FORMAT, len, key ? "sync point" : "P", qp, GST_TIME_ARGS(frame->pts));
    const gint64 t2 = g_get_monotonic_time();
    s->us_output += t2 - t1;
    fr = gst_video_encoder_finish_frame(ve, frame); /* the base class's bookkeeping and the push into whatever follows (a queue in the reference's pipelines) */
    s->us_push += g_get_monotonic_time() - t2; s->us_frames++;
    return fr;
}

/* frame-rate conversion, in front of a submit: the pictures it will yield need as many free slots (blend: at least one) -- collected here */
static GstFlowReturn rate_make_room(GstMi355H264Enc *s, GstClockTime pts) {
    GstVideoEncoder *ve = GST_VIDEO_ENCODER(s);
    int need = mi355enc_rate_peek(s->enc, (int64_t)pts);
    if (need < 1 && s->open_rate == 2) need = 1;
    GstFlowReturn fr = GST_FLOW_OK;
    while (fr == GST_FLOW_OK && mi355enc_pending(s->enc) + need > s->open_depth + 1) {
        GstVideoCodecFrame *old = gst_video_encoder_get_oldest_frame(ve);
        if (!old) break;
        fr = collect_into(s, old);
    }
    return fr;
}
/* ... and behind it: the frame's count goes into the FIFO; a frame that yields no picture is finished without a buffer (TRUE: done) */
static gboolean rate_submitted(GstMi355H264Enc *s, GstVideoCodecFrame *frame, GstFlowReturn *fr) {
    const int n = mi355enc_last_submit_count(s->enc);
    if (n <= 0) { *fr = gst_video_encoder_finish_frame(GST_VIDEO_ENCODER(s), frame); return TRUE; }
    s->rate_q[(s->rate_qh + s->rate_qn++) % G_N_ELEMENTS(s->rate_q)] = (guint8)n;
    return FALSE;
}
/* after a submit: as many collects as keep no more than pipeline-depth pictures in flight (one, without conversion) */
static GstFlowReturn collect_down(GstMi355H264Enc *s) {
    GstVideoEncoder *ve = GST_VIDEO_ENCODER(s);
    GstFlowReturn fr = GST_FLOW_OK;
    while (fr == GST_FLOW_OK && mi355enc_pending(s->enc) > s->open_depth) {
        GstVideoCodecFrame *old = gst_video_encoder_get_oldest_frame(ve);
        if (!old) break;
        fr = collect_into(s, old); /* finish_frame() consumes the reference */
        if (!s->open_rate) break;
    }
    return fr;
}
static GstFlowReturn enc_handle_frame(GstVideoEncoder *ve, GstVideoCodecFrame *frame) {
    GstMi355H264Enc *s = GST_MI355H264ENC(ve);
    GstVideoFrame vf;
    if (!s->enc || !s->input_state) { gst_video_encoder_finish_frame(ve, frame); return GST_FLOW_NOT_NEGOTIATED; }
    GST_OBJECT_LOCK(s);
    gboolean turn = effective_direction(s) != s->open_direction;
    int crop[4];
    effective_crop(s, crop);
    const gboolean recrop = memcmp(crop, s->open_crop, sizeof crop) != 0;
    const gboolean same_size = s->out_w > 0 && s->out_h > 0; /* (width / height at 0 follow the crop: the coded size changes with it) */
    GST_OBJECT_UNLOCK(s);
    if (recrop && !turn) { /* the crop changed while playing: latched here, in front of the next picture.  Where the handle can take it -- same coded size, and without
                              add-borders the same aspect ratio -- it is mi355enc_set_crop and nothing else changes; otherwise what a caps change does */
        const int in_w = GST_VIDEO_INFO_WIDTH(&s->input_state->info), in_h = GST_VIDEO_INFO_HEIGHT(&s->input_state->info);
        if (s->open_geom && same_size && mi355enc_set_crop(s->enc, crop[0], crop[2], in_w - crop[0] - crop[1], in_h - crop[2] - crop[3]) == MI355ENC_OK) {
            GST_OBJECT_LOCK(s);
            memcpy(s->open_crop, crop, sizeof crop);
            stabilize_forward(s); /* (a margin that changed with the crop) */
            GST_OBJECT_UNLOCK(s);
        } else turn = TRUE;
    }
    if (turn) { /* the direction changed while running (property or tag): exactly what a caps change does -- drain, reopen (this picture is an IDR picture), renegotiate the source caps */
        GstVideoCodecState *st = gst_video_codec_state_ref(s->input_state);
        const gboolean ok = enc_set_format(ve, st);
        gst_video_codec_state_unref(st);
        if (!ok) { gst_video_encoder_finish_frame(ve, frame); return GST_FLOW_NOT_NEGOTIATED; }
    }
    if (GST_BUFFER_FLAG_IS_SET(frame->input_buffer, GST_BUFFER_FLAG_DROPPABLE)) {
        /* what `identity name=ptsfixup` does to a picture that arrived too early to get a slot on its PTS grid (ceracoder.c:414-419:
         * "dropping an input buffer"): it keeps its raw, non-monotone PTS.  Not coded, no output buffer. */
        GST_DEBUG_OBJECT(s, "input picture flagged DROPPABLE (pts %" GST_TIME_FORMAT "): not coded", GST_TIME_ARGS(frame->pts));
        return gst_video_encoder_finish_frame(ve, frame);
    }
    snapshot_maybe_arm(s, frame);
    if (s->open_rate) { const GstFlowReturn fr = rate_make_room(s, frame->pts); if (fr != GST_FLOW_OK) { gst_video_encoder_finish_frame(ve, frame); return fr; } }
    const gint64 t0 = g_get_monotonic_time();
    if (s->jpeg) { /* a picture the encoder refuses (not baseline, another size, corrupt data) is dropped; ten in a row: this is not a stream it can take */
        GstMapInfo mi;
        if (!gst_buffer_map(frame->input_buffer, &mi, GST_MAP_READ)) { gst_video_encoder_finish_frame(ve, frame); return GST_FLOW_ERROR; }
        const gint64 t1 = g_get_monotonic_time();
        const int r = mi355enc_submit_jpeg(s->enc, mi.data, mi.size, (int64_t)frame->pts, GST_VIDEO_CODEC_FRAME_IS_FORCE_KEYFRAME(frame) ? 1 : 0);
        s->us_map += t1 - t0; s->us_submit += g_get_monotonic_time() - t1;
        gst_buffer_unmap(frame->input_buffer, &mi); /* (the coefficients are in the encoder's own memory) */
        if (r == MI355ENC_ERR_ARG) {
            GST_WARNING_OBJECT(s, "JPEG picture refused (pts %" GST_TIME_FORMAT "): dropped", GST_TIME_ARGS(frame->pts));
            if (++s->jpeg_refused >= 10) {
                GST_ELEMENT_ERROR(s, STREAM, DECODE, ("mi355h264enc: ten JPEG pictures in a row refused"), ("baseline JPEG of %dx%d expected",
                                  GST_VIDEO_INFO_WIDTH(&s->input_state->info), GST_VIDEO_INFO_HEIGHT(&s->input_state->info)));
                gst_video_encoder_finish_frame(ve, frame);
                return GST_FLOW_ERROR;
            }
            return gst_video_encoder_finish_frame(ve, frame); /* no output buffer: dropped */
        }
        if (r != MI355ENC_OK) {
            GST_ELEMENT_ERROR(s, STREAM, ENCODE, ("mi355h264enc: submit failed: %s", mi355enc_strerror(r)), ("mi355enc_submit_jpeg returned %d", r));
            gst_video_encoder_finish_frame(ve, frame);
            return GST_FLOW_ERROR;
        }
        s->jpeg_refused = 0;
        GstFlowReturn fr = GST_FLOW_OK;
        if (s->open_rate && rate_submitted(s, frame, &fr)) return fr;
        fr = collect_down(s);
        gst_video_codec_frame_unref(frame);
        return fr;
    }
    if (!gst_video_frame_map(&vf, &s->input_state->info, frame->input_buffer, GST_MAP_READ)) {
        gst_video_encoder_finish_frame(ve, frame);
        return GST_FLOW_ERROR;
    }
    /* NV12 goes in as is; I420 (x264enc's native format), packed and planar 4:2:2, 4:4:4 and RGB are converted on the device, so the
     * `videoconvert` in front of the encoder (pipeline/generic/x264_superfast_camlink:4) degenerates to a pass-through */
    int fmt = MI355ENC_FMT_NV12;
    switch (GST_VIDEO_INFO_FORMAT(&s->input_state->info)) {
    case GST_VIDEO_FORMAT_I420: fmt = MI355ENC_FMT_I420; break;
    case GST_VIDEO_FORMAT_YUY2: fmt = MI355ENC_FMT_YUY2; break;
    case GST_VIDEO_FORMAT_UYVY: fmt = MI355ENC_FMT_UYVY; break;
    default: { const int f = rgb_or_planar_fmt(GST_VIDEO_INFO_FORMAT(&s->input_state->info)); if (f >= 0) fmt = f; break; } /* converted on the device as well */
    }
    const uint8_t *planes[3] = {NULL, NULL, NULL};
    int strides[3] = {0, 0, 0};
    for (guint i = 0; i < GST_VIDEO_FRAME_N_PLANES(&vf) && i < 3; i++) {
        planes[i] = GST_VIDEO_FRAME_PLANE_DATA(&vf, i);
        strides[i] = GST_VIDEO_FRAME_PLANE_STRIDE(&vf, i);
    }
    const gint64 t1 = g_get_monotonic_time();
    int r = mi355enc_submit_fmt(s->enc, fmt, planes, strides, (int64_t)frame->pts, GST_VIDEO_CODEC_FRAME_IS_FORCE_KEYFRAME(frame) ? 1 : 0);
    s->us_map += t1 - t0; s->us_submit += g_get_monotonic_time() - t1;
    gst_video_frame_unmap(&vf); /* pageable memory: submit() has copied the picture out; pinned memory of our pool: the transfer is in flight and the
                                   codec frame keeps the buffer until the picture is collected */
    if (r != MI355ENC_OK) {
        GST_ELEMENT_ERROR(s, STREAM, ENCODE, ("mi355h264enc: submit failed: %s", mi355enc_strerror(r)), ("mi355enc_submit returned %d", r));
        gst_video_encoder_finish_frame(ve, frame);
        return GST_FLOW_ERROR;
    }
    GstFlowReturn fr = GST_FLOW_OK;
    if (s->open_rate && rate_submitted(s, frame, &fr)) return fr;
    fr = collect_down(s);
    gst_video_codec_frame_unref(frame);
    return fr;
}
static GstFlowReturn drain(GstMi355H264Enc *s, gboolean push) {
    GstVideoEncoder *ve = GST_VIDEO_ENCODER(s);
    GstFlowReturn fr = GST_FLOW_OK;
    while (s->enc && mi355enc_pending(s->enc) > 0) {
        GstVideoCodecFrame *old = gst_video_encoder_get_oldest_frame(ve);
        if (!old) break;
        if (push) fr = collect_into(s, old);
        else {
            size_t n = 0;
            mi355enc_collect(s->enc, s->au_buf, s->max_au, &n, NULL, NULL, NULL);
            if (s->open_rate && s->rate_qn && s->rate_q[s->rate_qh] > 1) { s->rate_q[s->rate_qh]--; gst_video_codec_frame_unref(old); continue; } /* (not the frame's last picture yet) */
            if (s->open_rate && s->rate_qn) { s->rate_qh = (s->rate_qh + 1) % G_N_ELEMENTS(s->rate_q); s->rate_qn--; }
            gst_video_encoder_finish_frame(ve, old); /* no output buffer: dropped */
        }
        if (fr != GST_FLOW_OK) break;
    }
    return fr;
}
static GstFlowReturn enc_finish(GstVideoEncoder *ve) { return drain(GST_MI355H264ENC(ve), TRUE); }
static gboolean enc_flush(GstVideoEncoder *ve) { drain(GST_MI355H264ENC(ve), FALSE); return TRUE; }
/* ---- pinned input memory for the upstream element.  The ALLOCATION query is answered with a buffer pool whose memory comes from
 * mi355enc_host_alloc(): a source that takes the offer (videotestsrc, v4l2src in its copying modes, decoders, videoconvert) writes its
 * pictures straight into pinned memory and mi355enc_submit() transfers them from there asynchronously -- no staging pass over the picture
 * on the streaming thread.  A source that declines (its own pool, mmap'ed capture buffers) is staged by submit() as before. */
typedef struct { GstAllocator parent; } GstMi355PinAllocator;
typedef struct { GstAllocatorClass parent_class; } GstMi355PinAllocatorClass;
G_DEFINE_TYPE(GstMi355PinAllocator, gst_mi355_pin_allocator, GST_TYPE_ALLOCATOR)
static GstMemory *pin_alloc(GstAllocator *a, gsize size, GstAllocationParams *params) {
    (void)a;
    const gsize align = params->align | 63u, maxsize = size + params->prefix + params->padding + align;
    guint8 *data = (guint8 *)mi355enc_host_alloc(maxsize);
    if (!data) return NULL; /* GStreamer falls back to the default allocator */
    const gsize off = ((gsize)(-(gintptr)(data + params->prefix)) & align) + params->prefix; /* data + off is aligned */
    return gst_memory_new_wrapped((GstMemoryFlags)0, data, maxsize, off, size, data, (GDestroyNotify)mi355enc_host_free); /* sysmem semantics; freed through the notify */
}
static void pin_free(GstAllocator *a, GstMemory *m) { (void)a; (void)m; } /* never reached: wrapped memory belongs to the system allocator */
static void gst_mi355_pin_allocator_class_init(GstMi355PinAllocatorClass *k) { GST_ALLOCATOR_CLASS(k)->alloc = pin_alloc; GST_ALLOCATOR_CLASS(k)->free = pin_free; }
static void gst_mi355_pin_allocator_init(GstMi355PinAllocator *a) { GST_OBJECT_FLAG_SET(a, GST_ALLOCATOR_FLAG_CUSTOM_ALLOC); }

/* With a coded size of its own (width / height) the element decouples the sizes of its two pads: what downstream accepts (video/x-h264 at the
 * coded size) says nothing about the input's size, so downstream's caps are not proxied upstream as the base class does by default. */
static GstCaps *enc_getcaps(GstVideoEncoder *ve, GstCaps *filter) {
    GstMi355H264Enc *s = GST_MI355H264ENC(ve);
    GST_OBJECT_LOCK(s);
    const gboolean scaled = s->out_w > 0 || s->out_h > 0 || s->direction != GST_VIDEO_ORIENTATION_IDENTITY || /* (a direction may exchange the size: the pads' sizes are decoupled as well) */
                            s->rate_mode != 0; /* (frame-rate conversion: the pads' frame rates are decoupled likewise) */
    GST_OBJECT_UNLOCK(s);
    if (!scaled) return gst_video_encoder_proxy_getcaps(ve, NULL, filter);
    GstCaps *t = gst_pad_get_pad_template_caps(GST_VIDEO_ENCODER_SINK_PAD(ve));
    if (filter) { GstCaps *i = gst_caps_intersect_full(filter, t, GST_CAPS_INTERSECT_FIRST); gst_caps_unref(t); t = i; }
    return t;
}
static gboolean enc_propose_allocation(GstVideoEncoder *ve, GstQuery *q) {
    GstMi355H264Enc *s = GST_MI355H264ENC(ve);
    GstCaps *caps = NULL;
    gboolean need_pool = FALSE;
    GstVideoInfo vi;
    gst_query_parse_allocation(q, &caps, &need_pool);
    if (s->pinned_input && caps && gst_video_info_from_caps(&vi, caps) && GST_VIDEO_INFO_FORMAT(&vi) != GST_VIDEO_FORMAT_ENCODED) { /* (raw caps only: a JPEG source keeps its own buffers) */
        GstAllocator *alloc = (GstAllocator *)g_object_new(gst_mi355_pin_allocator_get_type(), NULL);
        GstAllocationParams params;
        gst_allocation_params_init(&params);
        params.align = 63;
        gst_query_add_allocation_param(q, alloc, &params);
        const guint min = (guint)s->pipeline_depth + 2; /* pictures in flight hold their buffers until collect() */
        GstBufferPool *pool = gst_video_buffer_pool_new();
        GstStructure *cfg = gst_buffer_pool_get_config(pool);
        gst_buffer_pool_config_set_params(cfg, caps, (guint)GST_VIDEO_INFO_SIZE(&vi), min, 0);
        gst_buffer_pool_config_set_allocator(cfg, alloc, &params);
        gst_buffer_pool_config_add_option(cfg, GST_BUFFER_POOL_OPTION_VIDEO_META);
        if (gst_buffer_pool_set_config(pool, cfg)) gst_query_add_allocation_pool(q, pool, (guint)GST_VIDEO_INFO_SIZE(&vi), min, 0);
        gst_object_unref(pool);
        gst_object_unref(alloc);
    }
    gst_query_add_allocation_meta(q, GST_VIDEO_META_API_TYPE, NULL);
    return GST_VIDEO_ENCODER_CLASS(gst_mi355h264enc_parent_class)->propose_allocation(ve, q);
}
/* The custom downstream event of `mi355textoverlay` (gstmi355textoverlay.c): serialized, so it arrives on the streaming thread in front of the picture it
 * was sent before -- through `queue` and `videoconvert` as well.  Fields that are present replace the element's own; the event ends here. */
static gboolean enc_sink_event(GstVideoEncoder *ve, GstEvent *ev) {
    GstMi355H264Enc *s = GST_MI355H264ENC(ve);
    if (GST_EVENT_TYPE(ev) == GST_EVENT_CUSTOM_DOWNSTREAM && gst_event_has_name(ev, "mi355-overlay")) {
        const GstStructure *st = gst_event_get_structure(ev);
        gint v; gboolean b;
        GST_OBJECT_LOCK(s);
        if (gst_structure_has_field(st, "text")) overlay_store_text(s, gst_structure_get_string(st, "text"));
        if (gst_structure_get_int(st, "halign", &v) && v >= 0 && v <= 2) s->ov_style.halign = v;
        if (gst_structure_get_int(st, "valign", &v) && v >= 0 && v <= 2) s->ov_style.valign = v;
        if (gst_structure_get_int(st, "xpad", &v) && v >= 0 && v <= 8192) s->ov_style.xpad = v;
        if (gst_structure_get_int(st, "ypad", &v) && v >= 0 && v <= 8192) s->ov_style.ypad = v;
        if (gst_structure_get_boolean(st, "shaded-background", &b)) s->ov_style.shaded_background = b ? 1 : 0;
        overlay_forward(s);
        GST_OBJECT_UNLOCK(s);
        gst_event_unref(ev);
        return TRUE;
    }
    if (GST_EVENT_TYPE(ev) == GST_EVENT_TAG) { /* video-direction=auto follows the upstream image-orientation tag; the picture leaves upright, so the tag ends here */
        GstTagList *tl = NULL;
        int dir = 0;
        gst_event_parse_tag(ev, &tl);
        if (tl && direction_from_tag(tl, &dir)) {
            GST_OBJECT_LOCK(s);
            s->tag_direction = dir;
            const gboolean follow = s->direction == GST_VIDEO_ORIENTATION_AUTO;
            GST_OBJECT_UNLOCK(s);
            if (follow) {
                GstTagList *rest = gst_tag_list_copy(tl);
                gst_tag_list_remove_tag(rest, GST_TAG_IMAGE_ORIENTATION);
                gst_event_unref(ev);
                if (gst_tag_list_is_empty(rest)) { gst_tag_list_unref(rest); return TRUE; }
                ev = gst_event_new_tag(rest);
            }
        }
    }
    return GST_VIDEO_ENCODER_CLASS(gst_mi355h264enc_parent_class)->sink_event(ve, ev);
}
static void finalize(GObject *obj) {
    enc_stop(GST_VIDEO_ENCODER(obj));
    g_free(GST_MI355H264ENC(obj)->img_location);
    g_free(GST_MI355H264ENC(obj)->img_rgba);
    g_free(GST_MI355H264ENC(obj)->snap_location);
    g_free(GST_MI355H264ENC(obj)->lut_location);
    g_free(GST_MI355H264ENC(obj)->roi_text);
    g_free(GST_MI355H264ENC(obj)->mask_text);
    g_free(GST_MI355H264ENC(obj)->lut_nodes);
    g_free(GST_MI355H264ENC(obj)->out_colorimetry);
    g_mutex_clear(&GST_MI355H264ENC(obj)->snap_mu); g_mutex_clear(&GST_MI355H264ENC(obj)->snap_enc_mu); g_cond_clear(&GST_MI355H264ENC(obj)->snap_cv);
    G_OBJECT_CLASS(gst_mi355h264enc_parent_class)->finalize(obj);
}

static void gst_mi355h264enc_class_init(GstMi355H264EncClass *k) {
    GObjectClass *g = G_OBJECT_CLASS(k);
    GstElementClass *e = GST_ELEMENT_CLASS(k);
    GstVideoEncoderClass *v = GST_VIDEO_ENCODER_CLASS(k);
    const GParamFlags F = (GParamFlags)(G_PARAM_READWRITE | G_PARAM_STATIC_STRINGS | GST_PARAM_MUTABLE_PLAYING);
    g->set_property = set_property; g->get_property = get_property; g->finalize = finalize;
    g_object_class_install_property(g, PROP_BPS, g_param_spec_uint("bps", "Bitrate (bit/s)",
        "Target bitrate; the property ceracoder's encoder_control writes.  In bit/s -- except on an element named venc_kbps, which the reference sends kbit/s (encoder_control.c:29-32,53)", 1, 1000000000, 2048000, F));
    g_object_class_install_property(g, PROP_BITRATE, g_param_spec_uint("bitrate", "Bitrate (kbit/s)",
        "Target bitrate in kbit/s (x264enc-compatible alias of bps)", 1, 1000000, 2048, F));
    g_object_class_install_property(g, PROP_KEY_INT_MAX, g_param_spec_uint("key-int-max", "Key-frame interval",
        "Maximal distance between two IDR pictures (0 = 250)", 0, 100000, 60, F));
    g_object_class_install_property(g, PROP_DEVICE_ID, g_param_spec_int("device-id", "HIP device", "GPU ordinal (one stream per GPU)", 0, 63, 0, F));
    g_object_class_install_property(g, PROP_ME_RANGE, g_param_spec_int("me-range", "Motion search range", "Full-search radius, integer pels", 1, 16, 16, F));
    g_object_class_install_property(g, PROP_QP, g_param_spec_int("qp", "Constant QP", "-1: rate control on; 0..51: constant quantiser", -1, 51, -1, F));
    g_object_class_install_property(g, PROP_PIPELINE_DEPTH, g_param_spec_int("pipeline-depth", "Pipeline depth",
        "0: output each picture before taking the next; 1: overlap host entropy coding with the next picture (+1 frame latency); 2: three pictures in flight (+2 frames)", 0, 2, 0, F));
    g_object_class_install_property(g, PROP_SPEED_PRESET, g_param_spec_enum("speed-preset", "Speed preset",
        "x264enc's presets mapped onto this encoder's tools: None / ultrafast = Constrained Baseline, one quantiser per picture; superfast = dct8x8 + i8x8 + aq-mode=1 "
        "(High profile), and so do the slower ones.  A tool property set explicitly wins over the preset", speed_preset_type(), 0, F));
    g_object_class_install_property(g, PROP_THREADS, g_param_spec_int("threads", "Entropy-coding threads",
        "Host threads that code one slice row-parallel (bit-identical output); like x264enc's property of the same name, 0 = automatic (a quarter of the CPUs, at most 8), 1 = streaming thread only", 0, 64, 0, F));
    g_object_class_install_property(g, PROP_VBV, g_param_spec_uint("vbv-buf-capacity", "VBV buffer (ms)",
        "Rate control's buffer model in milliseconds of stream at the setpoint (x264enc's property of the same name and default)", 100, 10000, 600, F));
    g_object_class_install_property(g, PROP_INTRA_IN_P, g_param_spec_int("intra-in-p", "Intra macroblocks in P pictures",
        "Macroblocks of P pictures may be coded intra (uncovered regions, partial scene changes): 0 never, 1 Intra_16x16, 2 Intra_4x4 as well", 0, 2, 1, F));
    g_object_class_install_property(g, PROP_EXCLUSIVE, g_param_spec_boolean("exclusive-gpu", "This stream has the GPU to itself",
        "One stream per GPU: kernels may wait on the device for other kernels' progress (a P picture's motion-compensation stage beside the previous picture's deblocking, the deblocker beside the intra macroblocks: about 10 % more frames/s); leave false when other processes encode on the same GPU", FALSE, F));
    g_object_class_install_property(g, PROP_AQ_MODE, g_param_spec_int("aq-mode", "Adaptive quantisation",
        "0: one quantiser per picture; 1: a QP offset per macroblock from the variance of its source samples (x264enc's aq-mode 1 in spirit), coded with mb_qp_delta", 0, 1, 0, F));
    g_object_class_install_property(g, PROP_INTRA_SLICES, g_param_spec_int("intra-slices", "Slices per I picture",
        "Slices per IDR picture, one NAL unit each (0: about 17 macroblock rows per slice, 4 at 1080p): the slices are reconstructed side by side", 0, 64, 0, F));
    g_object_class_install_property(g, PROP_SLICES, g_param_spec_int("slices", "Slices per P picture",
        "Slices per P picture, one NAL unit each (0: automatic, like intra-slices -- about 17 macroblock rows per slice, 4 at 1080p; 1: one slice): vector and intra prediction stop at a "
        "slice's first row; with slice-deblock the slices are independent dependency chains for the deblocking launch, which sets the picture period (x264enc: what threads / "
        "sliced-threads do to a picture).  Costs 2-4 % bitrate on panning content", 0, 64, 0, F));
    g_object_class_install_property(g, PROP_SLICE_DEBLOCK, g_param_spec_boolean("slice-deblock", "Slice-local deblocking",
        "The deblocking filter stops at slice boundaries (disable_deblocking_filter_idc 2) in I and P pictures; slice heights become multiples of four macroblock rows", TRUE, F));
    g_object_class_install_property(g, PROP_I8X8, g_param_spec_boolean("i8x8", "Intra 8x8",
        "With dct8x8: the macroblocks of I pictures may be Intra_8x8 (x264enc: part of dct8x8; here a switch of its own: IDR pictures 1.4 - 3.9 % smaller, a key-int 60 stream 1 - 3 % slower)", FALSE, F));
    g_object_class_install_property(g, PROP_SINGLE_STREAM, g_param_spec_boolean("single-stream", "One HIP stream",
        "Run every stage of this encoder in order on one HIP stream (one hardware queue): for many encoders sharing a GPU", FALSE, F));
    g_object_class_install_property(g, PROP_PINNED_INPUT, g_param_spec_boolean("pinned-input", "Offer pinned input buffers",
        "Answer the upstream ALLOCATION query with a buffer pool in pinned host memory: a source that takes it writes pictures the GPU can fetch without a staging copy", TRUE, F));
    g_object_class_install_property(g, PROP_SCENECUT, g_param_spec_boolean("scenecut", "Scene-cut recovery",
        "Code an IDR picture two pictures after a scene cut (detected from the summed motion cost; x264 decides inside its lookahead instead)", TRUE, F));
    g_object_class_install_property(g, PROP_DCT8X8, g_param_spec_boolean("dct8x8", "8x8 transform",
        "Adaptive spatial transform size as in x264enc: High-profile stream, P macroblocks use the 8x8 transform", FALSE, F));
    g_object_class_install_property(g, PROP_DCT8X8_ADAPTIVE, g_param_spec_boolean("dct8x8-adaptive", "Per-macroblock transform size",
        "With dct8x8: every coded P macroblock chooses between the 4x4 and the 8x8 transform (SA8D against SATD of its prediction residual), as x264enc's dct8x8 does; "
        "without dct8x8 ignored. speed-preset does not set it", FALSE, F));
    g_object_class_install_property(g, PROP_INTRA_REFRESH, g_param_spec_boolean("intra-refresh", "Intra refresh",
        "Use periodic intra refresh instead of IDR frames, as in x264enc: a column of intra macroblocks sweeps the picture once every key-int-max frames "
        "(2 .. 256; opening fails otherwise), which start with SPS, PPS and a recovery point SEI and are marked as sync points; IDR frames only for the first frame, forced key units and "
        "scene cuts. Implies intra macroblocks in P frames and no partitions", FALSE, F));
    g_object_class_install_property(g, PROP_WIDTH, g_param_spec_int("width", "Coded width",
        "Width of the coded picture; 0: the input's.  Smaller than the input: the picture is scaled down on the GPU (up to 8:1 per axis, even sizes)", 0, 8192, 0, F));
    g_object_class_install_property(g, PROP_HEIGHT, g_param_spec_int("height", "Coded height",
        "Height of the coded picture; 0: the input's.  Smaller than the input: the picture is scaled down on the GPU (up to 8:1 per axis, even sizes)", 0, 8192, 0, F));
    g_object_class_install_property(g, PROP_CROP_LEFT, g_param_spec_int("crop-left", "Crop left", "Input samples to crop at the left, on the GPU (as videocrop; odd values count as the even value below; may change while playing)", 0, 8192, 0, F));
    g_object_class_install_property(g, PROP_CROP_RIGHT, g_param_spec_int("crop-right", "Crop right", "Input samples to crop at the right", 0, 8192, 0, F));
    g_object_class_install_property(g, PROP_CROP_TOP, g_param_spec_int("crop-top", "Crop top", "Input samples to crop at the top", 0, 8192, 0, F));
    g_object_class_install_property(g, PROP_CROP_BOTTOM, g_param_spec_int("crop-bottom", "Crop bottom", "Input samples to crop at the bottom", 0, 8192, 0, F));
    g_object_class_install_property(g, PROP_ADD_BORDERS, g_param_spec_boolean("add-borders", "Add borders",
        "Keep the picture's shape inside width x height and fill the rest with border-color (as videoscale add-borders=true), on the GPU", FALSE, F));
    g_object_class_install_property(g, PROP_UPSCALE, g_param_spec_boolean("upscale", "Allow upscaling", "Let width / height exceed the input's (up to 8:1 per axis)", FALSE, F));
    g_object_class_install_property(g, PROP_BORDER_COLOR, g_param_spec_uint("border-color", "Border colour", "Packed 0xYYCbCr", 0, 0xFFFFFF, 0x108080, F));
    g_object_class_install_property(g, PROP_QUALITY_STATS, g_param_spec_boolean("quality-stats", "Quality metrics",
        "Measure every coded picture on the GPU (PSNR of Y, Cb, Cr and SSIM of the luma, source against reconstruction); with stats=true the stream's figures are printed when the encoder closes. Read when the encoder opens", FALSE,
        (GParamFlags)(G_PARAM_READWRITE | G_PARAM_STATIC_STRINGS | GST_PARAM_MUTABLE_READY)));
    g_object_class_install_property(g, PROP_OV_TEXT, g_param_spec_string("overlay-text", "Overlay text",
        "Text drawn into every picture on the GPU (built-in 8x16 bitmap font, printable ASCII, newline starts a line, at most 255 bytes, no markup); empty: off. "
        "Settable while playing: the write only stores, the next picture carries it. An mi355textoverlay element upstream writes it through an event", "", F));
    g_object_class_install_property(g, PROP_OV_HALIGN, g_param_spec_enum("overlay-halignment", "Overlay horizontal alignment", "Where the text box sits, and how its lines are aligned inside it", gst_mi355_overlay_halign_type(), 2, F));
    g_object_class_install_property(g, PROP_OV_VALIGN, g_param_spec_enum("overlay-valignment", "Overlay vertical alignment", "Where the text box sits (baseline: bottom)", gst_mi355_overlay_valign_type(), 0, F));
    g_object_class_install_property(g, PROP_OV_XPAD, g_param_spec_int("overlay-xpad", "Overlay horizontal padding", "Luma samples between the text box and the left / right picture edge", 0, 8192, 16, F));
    g_object_class_install_property(g, PROP_OV_YPAD, g_param_spec_int("overlay-ypad", "Overlay vertical padding", "Luma samples between the text box and the top / bottom picture edge", 0, 8192, 16, F));
    g_object_class_install_property(g, PROP_OV_SCALE, g_param_spec_int("overlay-scale", "Overlay scale", "Luma samples per font pixel, 1..8; 0: height / 540, at least 1 (720p 1, 1080p 2, 2160p 4)", 0, 8, 0, F));
    g_object_class_install_property(g, PROP_OV_SHADED, g_param_spec_boolean("overlay-shaded-background", "Overlay shaded background", "Darken the text box", FALSE, F));
    g_object_class_install_property(g, PROP_IMG_LOCATION, g_param_spec_string("image-location", "Image location",
        "A Netpbm PAM file (P7; RGB_ALPHA or RGB, MAXVAL 255, at most 4096 x 4096) blended into every picture on the GPU, 1:1, under the overlay text (as gdkpixbufoverlay's location; "
        "PNG is not read: convert with `pngtopam -alphapam`). Read when the property is written, also while playing; a file that cannot be taken posts a warning and changes nothing; empty: off", "", F));
    g_object_class_install_property(g, PROP_IMG_X, g_param_spec_int("image-offset-x", "Image X offset", "Luma samples from the picture's left edge to the image's (negative: the image starts outside)", -16384, 16384, 0, F));
    g_object_class_install_property(g, PROP_IMG_Y, g_param_spec_int("image-offset-y", "Image Y offset", "Luma samples from the picture's top edge to the image's", -16384, 16384, 0, F));
    g_object_class_install_property(g, PROP_IMG_ALPHA, g_param_spec_double("image-alpha", "Image alpha", "Global alpha of the image, multiplied onto its own (as gdkpixbufoverlay's alpha)", 0.0, 1.0, 1.0, F));
    g_object_class_install_property(g, PROP_SNAP_LOCATION, g_param_spec_string("snapshot-location", "Still location",
        "File a JPEG still of the running stream is written to every snapshot-interval (through location.tmp and a rename; an element message mi355-snapshot follows each); empty: off. The still is transformed on the GPU and Huffman coded on a helper thread; the stream's bytes do not change", "", F));
    g_object_class_install_property(g, PROP_SNAP_INTERVAL, g_param_spec_uint("snapshot-interval", "Still interval (ms)", "Stream time between two stills", 0, G_MAXUINT, 1000, F));
    g_object_class_install_property(g, PROP_SNAP_QUALITY, g_param_spec_int("snapshot-quality", "Still quality", "libjpeg's quality scale", 1, 100, 75, F));
    g_object_class_install_property(g, PROP_SNAP_REDUCE, g_param_spec_int("snapshot-reduce", "Still reduction", "1, 2, 4 or 8: the still is the picture's size divided by it (rounded up)", 1, 8, 4, F));
    g_object_class_install_property(g, PROP_SNAP_SOURCE, g_param_spec_enum("snapshot-source", "Still source", "source: the picture that is coded, with scaling, orientation, image and text in it; decoded: what a decoder shows", snapshot_source_type(), 0, F));
    g_object_class_install_property(g, PROP_OUTPUT_COLORIMETRY, g_param_spec_string("output-colorimetry", "Output colorimetry", "what the coded samples are to mean, e.g. bt709 or bt601 (a GstVideoColorimetry string): the SPS says this, and YUV input is converted on the GPU from the range and matrix its caps give; empty: label the stream as the input, convert nothing", "", F));
    g_object_class_install_property(g, PROP_RATE_CONVERSION, g_param_spec_enum("rate-conversion", "Frame-rate conversion", "convert the frame rate on the GPU in place of a videorate in front: hold drops or repeats pictures to the output ticks, blend mixes neighbouring pictures at the ticks' instants", rate_conversion_type(), 0, F));
    g_object_class_install_property(g, PROP_OUTPUT_FRAMERATE, gst_param_spec_fraction("output-framerate", "Output frame rate", "with rate-conversion: the frame rate of the stream and of the source caps; 0/1: the sink caps' rate", 0, 1, G_MAXINT, 1, 0, 1, F));
    g_object_class_install_property(g, PROP_MAX_FILL, g_param_spec_int("max-fill", "Most repeats", "with rate-conversion: the most pictures one input may be preceded by (a longer hole in the timestamps re-anchors the ticks); at most pipeline-depth take effect", 0, 15, 2, F));
    g_object_class_install_property(g, PROP_HDR_INPUT, g_param_spec_enum("hdr-input", "HDR input", "the 10-bit input (P010_10LE, I420_10LE, v210) is PQ or HLG with BT.2020 primaries and matrix: tone-mapped on the GPU to SDR BT.709 (or to output-colorimetry) in the conversion launch; the caps give the range; other caps are an error", hdr_input_type(), 0, F));
    g_object_class_install_property(g, PROP_HDR_PEAK_NITS, g_param_spec_int("hdr-peak-nits", "HDR source peak", "with hdr-input: the source's peak luminance in cd/m^2 (HLG: the nominal peak Lw), 400 .. 10000 (hlg: .. 2000); 0: 1000", 0, 10000, 0, F));
    g_object_class_install_property(g, PROP_HDR_TARGET_NITS, g_param_spec_int("hdr-target-nits", "SDR target peak", "with hdr-input: the luminance the SDR peak stands for in cd/m^2, 100 .. 400; 0: 203 (BT.2408's reference white)", 0, 400, 0, F));
    g_object_class_install_property(g, PROP_ADJ_BRIGHTNESS, g_param_spec_double("brightness", "Brightness", "picture controls on the GPU (videobalance's property): added to the luma, in units of the luma scale", -1.0, 1.0, 0.0, F));
    g_object_class_install_property(g, PROP_ADJ_CONTRAST, g_param_spec_double("contrast", "Contrast", "picture controls on the GPU (videobalance's property): luma gain about black", 0.0, 2.0, 1.0, F));
    g_object_class_install_property(g, PROP_ADJ_HUE, g_param_spec_double("hue", "Hue", "picture controls on the GPU (videobalance's property): chroma rotation in units of pi", -1.0, 1.0, 0.0, F));
    g_object_class_install_property(g, PROP_ADJ_SATURATION, g_param_spec_double("saturation", "Saturation", "picture controls on the GPU (videobalance's property): chroma gain", 0.0, 2.0, 1.0, F));
    g_object_class_install_property(g, PROP_ADJ_GAMMA, g_param_spec_double("gamma", "Gamma", "picture controls on the GPU (the gamma element's property): t -> t^(1 / gamma) on the luma between black and white", 0.1, 10.0, 1.0, F));
    g_object_class_install_property(g, PROP_ADJ_SHARPEN, g_param_spec_int("sharpen", "Sharpen", "picture controls on the GPU: 3 x 3 unsharp mask on the luma in sixteenths of its amount (16: original + detail); negative softens (-16: the binomial blur); 0: off", -16, 64, 0, F));
    g_object_class_install_property(g, PROP_ADJ_SHARPEN_THRESHOLD, g_param_spec_int("sharpen-threshold", "Sharpen threshold", "with sharpen > 0: detail of at most this many codes is left alone (coring)", 0, 32, 0, F));
    g_object_class_install_property(g, PROP_AUTO_LEVELS, g_param_spec_double("auto-levels", "Automatic levels", "automatic levels on the GPU, measured per picture behind the noise filter and in front of the picture controls: how much of the stretch of the measured black and white point to the range's ends is applied; 0: off", 0.0, 1.0, 0.0, F));
    g_object_class_install_property(g, PROP_AUTO_BALANCE, g_param_spec_double("auto-balance", "Automatic white balance", "automatic white balance on the GPU (grey world, a constant chroma offset): how much of the measured cast is taken out; 0: off", 0.0, 1.0, 0.0, F));
    g_object_class_install_property(g, PROP_AUTO_SPEED, g_param_spec_int("auto-speed", "Automatic speed", "how fast the automatic levels and white balance follow the measurement, in 1/256 per picture; 256: at once (a knob, not a tuned value)", 1, 256, 16, F));
    g_object_class_install_property(g, PROP_AUTO_CLIP, g_param_spec_double("auto-clip", "Automatic clip", "the percentage of the samples that may fall below the black point, and likewise above the white point", 0.0, 20.0, 0.5, F));
    g_object_class_install_property(g, PROP_AUTO_MAX_GAIN, g_param_spec_double("auto-max-gain", "Automatic maximum gain", "the largest contrast gain the automatic levels apply", 1.0, 8.0, 2.0, F));
    g_object_class_install_property(g, PROP_LUT3D_LOCATION, g_param_spec_string("lut3d-location", "3D LUT location",
        "a 3D colour LUT on the GPU, behind the noise filter and in front of automatic levels and the picture controls: the path of a .cube file (LUT_3D_SIZE 2 .. 65, tetrahedral interpolation), read when the property is set, at any time; empty: off.  A file that cannot be read or parsed posts a warning and leaves the step as it was", "", F));
    g_object_class_install_property(g, PROP_LUT3D_STRENGTH, g_param_spec_double("lut3d-strength", "3D LUT strength", "how much of the 3D LUT's grade is applied, per sample between the input and the graded value; 0: off", 0.0, 1.0, 1.0, F));
    g_object_class_install_property(g, PROP_ROI, g_param_spec_string("roi", "Regions of interest",
        "Up to 8 rectangles \"x,y,w,h,delta[,feather]\" joined by ';': luma samples of the coded picture, a QP offset -12 .. 12 (negative: finer, not 0) inside and the macroblocks "
        "0 .. 8 over which it ramps to 0 outside; takes effect with the next frame; empty: off", "", F));
    g_object_class_install_property(g, PROP_MASK, g_param_spec_string("mask", "Privacy masks",
        "Up to 8 regions \"x,y,w,h,mode,param[,shape]\" joined by ';', made unreadable on the GPU under logos and text: luma samples of the coded picture; mode 1 fill (param 0, "
        "in mask-color), 2 pixelate (param: the even cell size 4 .. 64), 3 blur (param: the radius 1 .. 32); shape 0 rectangle, 1 ellipse; takes effect with the next frame; empty: off", "", F));
    g_object_class_install_property(g, PROP_MASK_COLOR, g_param_spec_uint("mask-color", "Mask colour", "The colour of filled mask regions, packed 0xRRGGBB", 0, 0xFFFFFF, 0, F));
    g_object_class_install_property(g, PROP_ROI_BALANCE, g_param_spec_int("roi-balance", "Region-of-interest balance",
        "The bits the regions of interest take are taken from the rest of the picture: the cap of the QP offset the macroblocks outside every region get; 0: off", 0, 12, 0, F));
    g_object_class_install_property(g, PROP_DS_LUMA, g_param_spec_int("denoise-spatial-luma", "Spatial denoise luma", "spatial noise reduction on the GPU, edge-preserving, in front of the temporal filter: the luma noise amplitude in codes that is filtered fully -- with denoise-auto above 0 the upper bound of the measured strength; 0: off", 0, MI355ENC_DENOISE_SPATIAL_MAX, 0, F));
    g_object_class_install_property(g, PROP_DS_CHROMA, g_param_spec_int("denoise-spatial-chroma", "Spatial denoise chroma", "spatial noise reduction on the GPU: the chroma noise amplitude in codes that is filtered fully -- with denoise-auto above 0 the upper bound of the measured strength; 0: off", 0, MI355ENC_DENOISE_SPATIAL_MAX, 0, F));
    g_object_class_install_property(g, PROP_DS_AUTO, g_param_spec_double("denoise-auto", "Automatic denoise strength", "the spatial filter's strength as this multiple of the noise sigma measured per picture on the GPU (0.25 .. 8; a knob, not a tuned value); with both bounds 0 the noise is measured and reported and nothing is filtered; 0: manual", 0.0, 8.0, 0.0, F));
    g_object_class_install_property(g, PROP_DS_PERCENTILE, g_param_spec_int("denoise-auto-percentile", "Automatic denoise percentile", "the percentile of the 8 x 8 blocks' noise estimates that is taken as the picture's noise level", 1, 50, 25, F));
    g_object_class_install_property(g, PROP_DS_SPEED, g_param_spec_int("denoise-auto-speed", "Automatic denoise speed", "how fast the measured noise level follows the pictures, in 1/256 per picture; 256: at once", 1, 256, 32, F));
    g_object_class_install_property(g, PROP_DENOISE_LUMA, g_param_spec_int("denoise-luma", "Denoise luma", "temporal noise reduction on the GPU, motion-adaptive, in front of the picture controls: the luma noise amplitude in codes that is filtered fully; 0: off", 0, MI355ENC_DENOISE_MAX, 0, F));
    g_object_class_install_property(g, PROP_DENOISE_CHROMA, g_param_spec_int("denoise-chroma", "Denoise chroma", "temporal noise reduction on the GPU: the chroma noise amplitude in codes that is filtered fully; 0: off", 0, MI355ENC_DENOISE_MAX, 0, F));
    g_object_class_install_property(g, PROP_STABILIZE, g_param_spec_int("stabilize", "Stabilize", "electronic image stabilisation on the GPU: the margin in input samples per side that the crop may move by to follow the camera's shake (added to each of crop-*; odd values count as the even value below); 0: off", 0, MI355ENC_STABILIZE_MARGIN_MAX, 0, F));
    g_object_class_install_property(g, PROP_STABILIZE_RANGE, g_param_spec_int("stabilize-range", "Stabilize range", "the largest motion between two pictures the stabiliser measures, in input luma samples (the input must be at least four times that in both directions)", 1, MI355ENC_STABILIZE_RANGE_MAX, 16, F));
    g_object_class_install_property(g, PROP_LENS_K1, g_param_spec_double("lens-k1", "Lens k1", "lens correction on the GPU (DESIGN.md section 27): the radial term in r^2, r = 1 at the picture's corner; negative straightens a barrel", -1.0, 1.0, 0.0, F));
    g_object_class_install_property(g, PROP_LENS_K2, g_param_spec_double("lens-k2", "Lens k2", "lens correction on the GPU: the radial term in r^4", -1.0, 1.0, 0.0, F));
    g_object_class_install_property(g, PROP_LENS_ZOOM, g_param_spec_double("lens-zoom", "Lens zoom", "how far out the corrected picture reads its source: below 1 magnifies (and hides the fill), above 1 shrinks", 0.25, 4.0, 1.0, F));
    g_object_class_install_property(g, PROP_ROLL, g_param_spec_double("roll", "Roll", "rotation about the picture's centre in degrees, on the GPU (a horizon that is off)", -180.0, 180.0, 0.0, F));
    g_object_class_install_property(g, PROP_KEYSTONE_H, g_param_spec_double("keystone-h", "Keystone horizontal", "perspective correction on the GPU: how much the picture's scale changes from its left to its right edge", -0.5, 0.5, 0.0, F));
    g_object_class_install_property(g, PROP_KEYSTONE_V, g_param_spec_double("keystone-v", "Keystone vertical", "perspective correction on the GPU: converging verticals", -0.5, 0.5, 0.0, F));
    g_object_class_install_property(g, PROP_WARP_FILTER, g_param_spec_enum("warp-filter", "Warp filter", "the resampling filter of lens-*, roll and keystone-*; samples whose source lies outside the picture take border-color", warp_filter_type(), 1, F));
    g_object_class_install_property(g, PROP_STABILIZE_LEAK, g_param_spec_int("stabilize-leak", "Stabilize leak", "how fast the stabilised crop returns to its place, in 1/256 per picture; 0: never (a knob, not a tuned value)", 0, 255, 16, F));
    g_object_class_install_property(g, PROP_DENOISE_MOTION, g_param_spec_int("denoise-motion", "Denoise motion", "motion compensation of the temporal noise reduction: per 8 x 8 block the history is searched within this many luma samples; 0: none (the filter lets go where the picture moves)", 0, MI355ENC_DENOISE_MOTION_MAX, 0, F));
    g_object_class_override_property(g, PROP_VIDEO_DIRECTION, "video-direction"); /* GstVideoDirection: identity, 90r, 180, 90l, horiz, vert, ul-lr, ur-ll, auto -- as on videoflip */
    g_object_class_install_property(g, PROP_STATS, g_param_spec_boolean("stats", "Print stats", "Print a JSON line with counters when the encoder closes", FALSE, F));
    gst_element_class_add_static_pad_template(e, &sink_tmpl);
    gst_element_class_add_static_pad_template(e, &src_tmpl);
    gst_element_class_set_static_metadata(e, "MI355X H.264 encoder", "Codec/Encoder/Video/Hardware",
        "H.264 (Constrained Baseline) encoder on AMD Instinct MI355X via hand-written HIP kernels", "ceracoder-amd");
    v->start = enc_start; v->stop = enc_stop; v->set_format = enc_set_format; v->handle_frame = enc_handle_frame; v->getcaps = enc_getcaps;
    v->finish = enc_finish; v->flush = enc_flush; v->propose_allocation = enc_propose_allocation; v->sink_event = enc_sink_event;
}
static void gst_mi355h264enc_init(GstMi355H264Enc *s) {
    s->rate_raw = 2048; s->rate_is_bps = FALSE; s->key_int_max = 60; s->device_id = 0; s->me_range = 16; s->qp = -1; s->pipeline_depth = 0; s->speed_preset = 0;
    s->stats = FALSE; s->dct8x8 = -1; s->threads = 0; s->scenecut = TRUE; s->exclusive_gpu = FALSE; s->vbv_ms = 600; s->intra_in_p = -1; s->pinned_input = TRUE; s->aq_mode = -1; s->slices = -1; s->slice_deblock = -1; s->intra_slices = 0; s->i8x8 = -1; s->single_stream = FALSE; s->dct8x8_adaptive = FALSE; s->intra_refresh = FALSE; s->quality_stats = FALSE; s->enc = NULL; s->input_state = NULL; s->max_au = 0; s->au_buf = NULL; s->last_pts = GST_CLOCK_TIME_NONE;
    s->us_map = s->us_submit = s->us_collect = s->us_output = s->us_push = s->us_frames = 0;
    s->ov_text[0] = 0; mi355enc_overlay_default_style(&s->ov_style);
    s->img_location = NULL; s->img_rgba = NULL; s->img_w = s->img_h = s->img_x = s->img_y = 0; s->img_alpha = 1.0;
    s->direction = s->tag_direction = s->open_direction = GST_VIDEO_ORIENTATION_IDENTITY;
    s->border_color = 0x108080;
    s->out_colorimetry = NULL;
    s->hdr_input = 0; s->hdr_peak = 0; s->hdr_target = 0;
    mi355enc_adjust_default(&s->adj);
    mi355enc_denoise_default(&s->dn);
    mi355enc_denoise_spatial_default(&s->ds);
    mi355enc_autolevel_default(&s->al);
    s->lut_location = NULL; s->lut_nodes = NULL; s->lut_size = 0; s->lut_strength = 256;
    s->roi_text = NULL; mi355enc_roi_default(&s->roi);
    s->mask_text = NULL; memset(&s->mask, 0, sizeof s->mask); s->mask_color = 0;
    s->dn_motion = 0;
    s->stab = 0; s->stab_range = 16; s->stab_leak = 16;
    s->warp_k1 = s->warp_k2 = s->warp_roll = s->warp_kh = s->warp_kv = 0.0; s->warp_zoom = 1.0; s->warp_filter = 1;
    s->rate_mode = 0; s->out_fps_n = 0; s->out_fps_d = 1; s->max_fill = 2; s->open_rate = 0; s->tick = GST_CLOCK_TIME_NONE; s->rate_qh = s->rate_qn = 0;
    s->snap_location = NULL; s->snap_interval = 1000; s->snap_quality = 75; s->snap_reduce = 4; s->snap_source = 0; s->snap_next = GST_CLOCK_TIME_NONE; s->snap_watch = 0;
    g_mutex_init(&s->snap_mu); g_mutex_init(&s->snap_enc_mu); g_cond_init(&s->snap_cv);
    s->snap_thread = NULL; s->snap_wake = 0; s->snap_stop = FALSE; s->snap_count = 0; s->snap_gen = 0;
}

GType gst_mi355tsmux_get_type(void); /* gstmi355tsmux.c */
GType gst_mi355textoverlay_get_type(void); /* gstmi355textoverlay.c */
static gboolean plugin_init(GstPlugin *p) {
    GST_DEBUG_CATEGORY_INIT(mi355_debug, "mi355h264enc", 0, "MI355X H.264 encoder");
    return gst_element_register(p, "mi355h264enc", GST_RANK_NONE, GST_TYPE_MI355H264ENC) &&
           gst_element_register(p, "mi355tsmux", GST_RANK_NONE, gst_mi355tsmux_get_type()) &&
           gst_element_register(p, "mi355textoverlay", GST_RANK_NONE, gst_mi355textoverlay_get_type());
}
GST_PLUGIN_DEFINE(GST_VERSION_MAJOR, GST_VERSION_MINOR, mi355h264enc, "MI355X-native H.264 encoder for ceracoder", plugin_init, VERSION,
                  "LGPL", PACKAGE, "https://github.com/CERALIVE/ceracoder")
