"""ctypes mirror of include/mi355enc.h -- plumbing only: every call below is one C-ABI call.

The library is the product; there is no Python or CPU fallback.  If libmi355enc.so is
missing or no HIP device is usable, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355ENC_LIB") or os.path.join(_HERE, "libmi355enc.so")  # (MI355ENC_LIB: development builds, tools/build_variant.sh)

LEVELS_PER_MB = 408
MBINFO_DTYPE = np.dtype(
    [("mvx", "<i2"), ("mvy", "<i2"), ("mb_type", "u1"), ("i16_mode", "u1"), ("chroma_mode", "u1"),
     ("qp", "u1"), ("nzmask", "<u4"), ("cost", "<u4")]
)

FETCH_RECON_Y, FETCH_RECON_UV, FETCH_PREFILTER_Y, FETCH_PREFILTER_UV, FETCH_MBINFO, FETCH_LEVELS = range(6)
FETCH_SCALE_TABLES = 6  # the device's copy of the scale tables (Encoder.scale_tables_device())
FETCH_SOURCE_Y, FETCH_SOURCE_UV = 7, 8  # the last collected picture's coded source surfaces, valid until the next submit
FETCH_BAND_CUTS, FETCH_ERROR_WORD, FETCH_SYNC_WORDS = 102, 103, 104  # development: Encoder.band_cuts(), Encoder.error_word(), Encoder.sync_words()
BAND_ROWS = 4  # MI355_BAND_ROWS: macroblock rows per band of the band deblocker
ERR_ARG, ERR_STATE = -1, -6
ERR_OVERFLOW = -5
FMT_NV12, FMT_I420, FMT_YUY2, FMT_UYVY = range(4)
FMT_Y42B, FMT_Y444, FMT_YV12, FMT_NV21, FMT_BGRX, FMT_RGBX, FMT_XRGB, FMT_XBGR, FMT_BGR, FMT_RGB = range(4, 14)  # converted by k_csc.hip
FMT_P010, FMT_I420_10, FMT_V210, FMT_GRAY8 = range(14, 18)  # 10-bit and grey input
SCALE_LUMA, SCALE_CHROMA_V, SCALE_CHROMA_H, SCALE_CHROMA_V422 = range(4)  # kinds of scale_table()
IDEC = np.dtype([("modes4", "u1", (16,)), ("mode16", "u1"), ("cmode", "u1"), ("use_i4", "u1"), ("pad", "u1"), ("cost", "<u4"), ("cost_luma", "<u4"), ("rsv", "<u4")])
IMV_DTYPE = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("sad", "<u2"), ("bits", "<u2")])
SURF_ROWS, SURF_COLS = 35, 36
DROP_MAX, DROP_SKIP = 12, 255
STAGE_ME, STAGE_INTER, STAGE_INTRA, STAGE_DEBLOCK, STAGE_SUBPEL, STAGE_CSC_I420, STAGE_CSC_YUY2, STAGE_CSC_UYVY, STAGE_ME_SELECT, STAGE_PMB, STAGE_INTRA_P, STAGE_QUALITY, STAGE_JPEG, STAGE_ORIENT, STAGE_SCALE, STAGE_IMAGE, STAGE_SNAPSHOT, STAGE_YUV_CONVERT, STAGE_RATE = range(19)
STAGE_ADJUST_POINT, STAGE_ADJUST_SHARPEN = 23, 24  # the picture controls set last on slot 0's surfaces: pointwise form, stencil form
STAGE_DENOISE_SEARCH, STAGE_DENOISE_MC = 27, 28  # ... with motion compensation: the search alone, the search and the compensated filter
DENOISE_MOTION_MAX = 16
STAGE_STABILIZE_PROJECT, STAGE_STABILIZE_MATCH = 29, 30  # the stabiliser's launches: clear + projection at the input size, match
STABILIZE_RANGE_MAX, STABILIZE_MARGIN_MAX = 32, 1024
STAGE_WARP = 31  # the warp set last on slot 0's surfaces
STAGE_AUTOLEVEL_MEASURE, STAGE_AUTOLEVEL_DECIDE, STAGE_AUTOLEVEL_APPLY = 32, 33, 34  # the launches of automatic levels and white balance
WARP_BILINEAR, WARP_BICUBIC = 0, 1
STAGE_MASK_CELLS, STAGE_MASK_BLUR = 38, 39  # the privacy masks set last on slot 0's surfaces: the pixelate and commit launches (the fill is the commit's) / the blur launches
STAGE_DENOISE_SPATIAL, STAGE_DENOISE_SPATIAL_AUTO = 36, 37  # the spatial noise filter set last on slot 0's surfaces: manual / automatic, both planes
DENOISE_SPATIAL_MAX = 32
STAGE_LUT3D = 35  # the 3D colour LUT set last on slot 0's surfaces
LUT3D_N_MIN, LUT3D_N_MAX = 2, 65
LUT3D_DIRECT, LUT3D_STAGED = 0, 1  # the launch forms (lut3d_plan, lut3d_probe)
WARP_NODE_MIN, WARP_NODE_MAX = -2048 * 256, 10240 * 256
STAGE_DENOISE, STAGE_DENOISE_PRIME = 25, 26  # the temporal noise filter set last on slot 0's surfaces and the handle's history: filtering, priming
STAGE_HDR_P010, STAGE_HDR_I420_10, STAGE_HDR_V210, STAGE_DEEP_P010 = 19, 20, 21, 22  # the tone-mapping launch per format, and the plain P010 launch beside it
HDR_PQ, HDR_HLG = 16, 18  # mi355enc_set_hdr_input: the transfer's H.264 Table E-4 code point
# mi355enc_set_orientation: GstVideoOrientationMethod's numbers
ORIENT_IDENTITY, ORIENT_90R, ORIENT_180, ORIENT_90L, ORIENT_HORIZ, ORIENT_VERT, ORIENT_UL_LR, ORIENT_UR_LL = range(8)
ORIENT_NAMES = ("identity", "90r", "180", "90l", "horiz", "vert", "ul-lr", "ur-ll")

EXPORTS = [
    "mi355enc_abi_version", "mi355enc_strerror", "mi355enc_default_cfg", "mi355enc_open", "mi355enc_close",
    "mi355enc_set_bitrate", "mi355enc_get_bitrate", "mi355enc_set_fixed_qp", "mi355enc_set_fixed_drop", "mi355enc_set_intra_refresh", "mi355enc_stage_me_select", "mi355enc_stage_me_select_next", "mi355enc_encode", "mi355enc_submit",
    "mi355enc_submit_device", "mi355enc_pending", "mi355enc_collect", "mi355enc_get_stats", "mi355enc_reset_stats",
    "mi355enc_max_au_bytes", "mi355enc_fetch", "mi355enc_mb_width", "mi355enc_mb_height", "mi355enc_stage_me",
    "mi355enc_stage_subpel", "mi355enc_stage_inter", "mi355enc_stage_pmb", "mi355enc_stage_intra", "mi355enc_stage_intra_analyse", "mi355enc_stage_csc", "mi355enc_submit_fmt", "mi355enc_host_write_slice_packed", "mi355enc_stage_deblock", "mi355enc_time_stage",
    "mi355enc_host_write_headers", "mi355enc_host_write_slice", "mi355enc_host_set_slice_rows", "mi355enc_host_set_p_slices", "mi355enc_stage_set_slice_rows", "mi355enc_slice_rows", "mi355enc_p_slice_rows", "mi355enc_stage_set_slice_deblock", "mi355enc_rc_init", "mi355enc_rc_set_bitrate",
    "mi355enc_rc_pick", "mi355enc_rc_update", "mi355enc_host_cavlc_block", "mi355enc_debug_trip_wait", "mi355enc_debug_get_counters", "mi355enc_debug_set_counters", "mi355enc_host_alloc", "mi355enc_host_free",
    "mi355enc_set_input_size", "mi355enc_stage_scale", "mi355enc_scale_table",
    "mi355enc_set_colorimetry", "mi355enc_csc_coefficients", "mi355enc_host_write_headers_vui", "mi355enc_stage_csc_device",
    "mi355enc_set_input_colorimetry", "mi355enc_yuv_coefficients", "mi355enc_stage_yuv_convert",
    "mi355enc_set_quality_metrics", "mi355enc_last_quality", "mi355enc_quality_totals", "mi355enc_stage_quality", "mi355enc_stage_quality_device",
    "mi355enc_overlay_default_style", "mi355enc_set_overlay_style", "mi355enc_set_overlay_text", "mi355enc_last_overlay", "mi355enc_overlay_glyph", "mi355enc_stage_overlay",
    "mi355enc_set_image", "mi355enc_set_image_place", "mi355enc_last_image", "mi355enc_stage_image", "mi355enc_debug_image_bytes", "mi355enc_image_pixel", "mi355enc_image_load_pam",
    "mi355enc_jpeg_info", "mi355enc_jpeg_entropy_decode", "mi355enc_submit_jpeg", "mi355enc_stage_jpeg", "mi355enc_stage_jpeg_blocks",
    "mi355enc_set_orientation", "mi355enc_get_orientation", "mi355enc_orient_size", "mi355enc_orient_source", "mi355enc_stage_orient", "mi355enc_stage_orient_device",
    "mi355enc_debug_orient_bytes",
    "mi355enc_set_input_geometry", "mi355enc_get_input_geometry", "mi355enc_set_crop", "mi355enc_geometry_table", "mi355enc_fit_rect", "mi355enc_stage_geometry",
    "mi355enc_geometry_check", "mi355enc_geometry_sar",
    "mi355enc_request_snapshot", "mi355enc_take_snapshot", "mi355enc_debug_snapshot_bytes", "mi355enc_snapshot_tables", "mi355enc_snapshot_reciprocal",
    "mi355enc_snapshot_max_bytes", "mi355enc_snapshot_write", "mi355enc_stage_snapshot_blocks", "mi355enc_stage_snapshot_blocks_device", "mi355enc_stage_snapshot",
    "mi355enc_rate_check", "mi355enc_set_rate_conversion", "mi355enc_rate_peek", "mi355enc_last_submit_count", "mi355enc_rate_stats", "mi355enc_debug_rate_bytes",
    "mi355enc_rate_plan_init", "mi355enc_rate_plan_step", "mi355enc_stage_rate",
    "mi355enc_set_hdr_input", "mi355enc_hdr_tables",
    "mi355enc_adjust_default", "mi355enc_adjust_check", "mi355enc_adjust_tables", "mi355enc_set_adjust", "mi355enc_get_adjust", "mi355enc_last_adjust", "mi355enc_stage_adjust",
    "mi355enc_debug_adjust_bytes",
    "mi355enc_denoise_default", "mi355enc_denoise_check", "mi355enc_denoise_tables", "mi355enc_set_denoise", "mi355enc_get_denoise", "mi355enc_last_denoise", "mi355enc_stage_denoise",
    "mi355enc_debug_denoise_bytes",
    "mi355enc_set_denoise_motion", "mi355enc_get_denoise_motion", "mi355enc_last_denoise_motion", "mi355enc_denoise_motion_key", "mi355enc_stage_denoise_search", "mi355enc_stage_denoise_mc",
    "mi355enc_stabilize_default", "mi355enc_stabilize_check", "mi355enc_set_stabilize", "mi355enc_get_stabilize", "mi355enc_last_stabilize", "mi355enc_debug_stabilize_bytes",
    "mi355enc_stabilize_project", "mi355enc_stabilize_vote", "mi355enc_stabilize_motion", "mi355enc_stabilize_step", "mi355enc_stabilize_probe_project", "mi355enc_stabilize_probe_match",
    "mi355enc_autolevel_default", "mi355enc_autolevel_check", "mi355enc_autolevel_decide", "mi355enc_set_autolevel", "mi355enc_get_autolevel", "mi355enc_last_autolevel",
    "mi355enc_debug_autolevel_bytes", "mi355enc_autolevel_probe_stage", "mi355enc_autolevel_probe_measure", "mi355enc_autolevel_probe_decide",
    "mi355enc_warp_params_default", "mi355enc_warp_coeff", "mi355enc_warp_mesh_size", "mi355enc_warp_mesh_check", "mi355enc_warp_build", "mi355enc_warp_apply_host",
    "mi355enc_set_warp", "mi355enc_set_warp_mesh", "mi355enc_get_warp", "mi355enc_last_warp", "mi355enc_debug_warp_bytes", "mi355enc_warp_probe", "mi355enc_warp_plan", "mi355enc_debug_warp_staging",
    "mi355enc_denoise_spatial_default", "mi355enc_denoise_spatial_check", "mi355enc_denoise_spatial_tables", "mi355enc_denoise_spatial_apply_host",
    "mi355enc_denoise_spatial_measure_host", "mi355enc_denoise_spatial_decide", "mi355enc_set_denoise_spatial", "mi355enc_get_denoise_spatial",
    "mi355enc_last_denoise_spatial", "mi355enc_debug_denoise_spatial_bytes", "mi355enc_denoise_spatial_probe_stage", "mi355enc_denoise_spatial_probe_measure",
    "mi355enc_denoise_spatial_probe_decide",
    "mi355enc_lut3d_coefficients", "mi355enc_lut3d_check", "mi355enc_lut3d_identity", "mi355enc_lut3d_parse_cube", "mi355enc_lut3d_apply_host", "mi355enc_lut3d_plan",
    "mi355enc_set_lut3d", "mi355enc_get_lut3d", "mi355enc_last_lut3d", "mi355enc_debug_lut3d_bytes", "mi355enc_lut3d_probe", "mi355enc_debug_lut3d_form",
    "mi355enc_roi_default", "mi355enc_roi_check", "mi355enc_roi_map", "mi355enc_roi_parse", "mi355enc_set_roi", "mi355enc_get_roi", "mi355enc_last_roi",
    "mi355enc_debug_roi_bytes", "mi355enc_roi_probe_set_map", "mi355enc_roi_probe_offsets",
    "mi355enc_mask_check", "mi355enc_mask_parse", "mi355enc_mask_apply_host", "mi355enc_mask_ellipse", "mi355enc_mask_mean", "mi355enc_mask_colour",
    "mi355enc_set_mask", "mi355enc_get_mask", "mi355enc_last_mask", "mi355enc_debug_mask_bytes", "mi355enc_mask_probe",
]


class Cfg(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fps_num", C.c_int), ("fps_den", C.c_int), ("gop", C.c_int),
                ("me_range", C.c_int), ("bitrate_bps", C.c_uint32), ("device_id", C.c_int), ("fixed_qp", C.c_int),
                ("qp_min", C.c_int), ("qp_max", C.c_int), ("pipeline_depth", C.c_int), ("profile_events", C.c_int),
                ("use_graphs", C.c_int), ("keep_prefilter", C.c_int), ("transform8x8", C.c_int), ("i4x4", C.c_int), ("subpel", C.c_int), ("deblock_mode", C.c_int), ("intra_in_p", C.c_int), ("cavlc_threads", C.c_int), ("intra_mode", C.c_int), ("vbv_ms", C.c_int), ("scenecut", C.c_int), ("exclusive_device", C.c_int), ("aq_mode", C.c_int), ("single_stream", C.c_int), ("intra_slices", C.c_int), ("partitions", C.c_int), ("profile_overlap", C.c_int), ("i8x8", C.c_int), ("slices", C.c_int), ("slice_deblock", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("idr_frames", C.c_uint64), ("bytes", C.c_uint64), ("last_qp", C.c_uint32),
                ("last_bytes", C.c_uint32), ("target_bps", C.c_uint32), ("ms_me", C.c_double), ("ms_inter", C.c_double),
                ("ms_intra", C.c_double), ("ms_deblock", C.c_double), ("ms_total_gpu", C.c_double), ("ms_subpel", C.c_double), ("n_me", C.c_uint64),
                ("n_inter", C.c_uint64), ("n_intra", C.c_uint64), ("n_deblock", C.c_uint64), ("ms_entropy", C.c_double),
                ("ms_wait", C.c_double), ("n_total_gpu", C.c_uint64), ("ms_deblock_idr", C.c_double), ("n_deblock_idr", C.c_uint64), ("cavlc_threads", C.c_uint32), ("last_drop", C.c_uint32), ("ms_select", C.c_double), ("ms_analyse_p", C.c_double), ("ms_intra_p", C.c_double), ("skip_pictures", C.c_uint64), ("ms_open", C.c_double),
                ("recoveries", C.c_uint32), ("last_error_word", C.c_uint32), ("safe_level", C.c_uint32), ("pinned_inputs", C.c_uint64)]


class Counters(C.Structure):
    """mi355enc_counters_t: the picture epoch, the four counts the kernels compare on the device, the counts behind idr_pic_id and frame_num; keep: bit i set =
    mi355enc_debug_set_counters leaves field i alone"""
    _fields_ = [("epoch", C.c_uint32), ("pmb_rows_total", C.c_uint32), ("db_started_total", C.c_uint32), ("ip_done_total", C.c_uint32),
                ("qpc_total", C.c_uint32), ("idr_count", C.c_uint32), ("frames_since_idr", C.c_uint32), ("keep", C.c_uint32)]
    NAMES = ("epoch", "pmb_rows_total", "db_started_total", "ip_done_total", "qpc_total", "idr_count", "frames_since_idr")


class Quality(C.Structure):
    """mi355enc_quality_t: sse / samples of Y, Cb, Cr, the fixed-point SSIM sum and its window count, and what the host derives from them"""
    _fields_ = [("sse", C.c_uint64 * 3), ("samples", C.c_uint64 * 3), ("ssim_sum", C.c_int64), ("ssim_windows", C.c_uint64),
                ("psnr", C.c_double * 3), ("ssim", C.c_double), ("pts", C.c_int64), ("pictures", C.c_uint64)]

    def ints(self):
        """the integers the device computed: (sse_y, sse_cb, sse_cr, ssim_sum, ssim_windows)"""
        return (int(self.sse[0]), int(self.sse[1]), int(self.sse[2]), int(self.ssim_sum), int(self.ssim_windows))


class JpegInfo(C.Structure):
    """mi355enc_jpeg_info_t: what the markers in front of a JPEG picture's scan say (hs, vs: luma sampling factors)"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("components", C.c_int), ("hs", C.c_int), ("vs", C.c_int), ("restart_interval", C.c_int), ("has_dht", C.c_int)]


class OverlayStyle(C.Structure):
    """mi355enc_overlay_style_t: halign / valign 0 left / top, 1 centre, 2 right / bottom; pads in luma samples; scale 0 = auto, 1 .. 8"""
    _fields_ = [("halign", C.c_int), ("valign", C.c_int), ("xpad", C.c_int), ("ypad", C.c_int), ("scale", C.c_int), ("shaded_background", C.c_int)]


class Adjust(C.Structure):
    """mi355enc_adjust_t: picture controls in integers -- brightness, contrast, saturation, hue, gamma in thousandths, sharpen in sixteenths, the coring threshold"""
    _fields_ = [("brightness", C.c_int), ("contrast", C.c_int), ("saturation", C.c_int), ("hue", C.c_int), ("gamma", C.c_int), ("sharpen", C.c_int), ("sharpen_threshold", C.c_int)]
    NAMES = ("brightness", "contrast", "saturation", "hue", "gamma", "sharpen", "sharpen_threshold")

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in self.NAMES}


class Denoise(C.Structure):
    """mi355enc_denoise_t: the temporal noise filter's strengths, 0 .. 32 codes each, 0: that plane is not filtered"""
    _fields_ = [("luma", C.c_int), ("chroma", C.c_int)]

    def as_dict(self):
        return dict(luma=int(self.luma), chroma=int(self.chroma))


class Stabilize(C.Structure):
    """mi355enc_stabilize_t: search range 0 .. 32 input luma samples (0: off), leak 0 .. 255, how far the crop may move per side (even, 0 .. 1024)"""
    _fields_ = [("range", C.c_int), ("leak", C.c_int), ("margin_x", C.c_int), ("margin_y", C.c_int)]

    def as_dict(self):
        return dict(range=int(self.range), leak=int(self.leak), margin_x=int(self.margin_x), margin_y=int(self.margin_y))


class StabilizeInfo(C.Structure):
    """mi355enc_stabilize_info_t: a picture's record -- measured motion, valid votes per axis, the crop's displacement, the trajectory's state (1/256 sample)"""
    _fields_ = [(n, C.c_int) for n in ("mx", "my", "votes_x", "votes_y", "ox", "oy", "sx", "sy")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Autolevel(C.Structure):
    """mi355enc_autolevel_t: levels / balance in thousandths (both 0: off), speed 1 .. 256, the clips in ten-thousandths, max_gain in thousandths, the vote's reach"""
    NAMES = ("levels", "balance", "speed", "clip_low", "clip_high", "max_gain", "reach")
    _fields_ = [(n, C.c_int) for n in NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in self.NAMES}


class AutolevelMeas(C.Structure):
    """mi355enc_autolevel_meas_t: the luma histogram, the chroma voters, the visible chroma samples, the voters' sums of Cb and Cr"""
    _fields_ = [("hist", C.c_uint32 * 256), ("voters", C.c_uint32), ("chroma", C.c_uint32), ("su", C.c_uint64), ("sv", C.c_uint64)]

    def as_dict(self):
        return dict(hist=np.array(self.hist, np.int64), voters=int(self.voters), chroma=int(self.chroma), su=int(self.su), sv=int(self.sv))


class AutolevelInfo(C.Structure):
    """mi355enc_autolevel_info_t: a picture's record -- its measurement, the state behind it (1/256 code), the chroma offsets, whether the chroma vote was valid"""
    _fields_ = [(n, C.c_int) for n in ("lo", "hi", "voters", "du", "dv", "s_lo", "s_hi", "s_du", "s_dv", "off_u", "off_v", "valid")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class DenoiseSpatial(C.Structure):
    """mi355enc_denoise_spatial_t: luma / chroma 0 .. 32 (strengths, or with auto_gain their upper bounds), auto_gain 0 (manual) or 250 .. 8000 (thousandths of
    the measured sigma), percentile 1 .. 50, speed 1 .. 256"""
    NAMES = ("luma", "chroma", "auto_gain", "percentile", "speed")
    _fields_ = [(n, C.c_int) for n in NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in self.NAMES}


class DenoiseSpatialMeas(C.Structure):
    """mi355enc_denoise_spatial_meas_t: the voting blocks' histogram over the noise bins, the candidate blocks, the voters"""
    _fields_ = [("hist", C.c_uint32 * 256), ("candidates", C.c_uint32), ("voters", C.c_uint32)]

    def as_dict(self):
        return dict(hist=np.array(self.hist, np.int64), candidates=int(self.candidates), voters=int(self.voters))


class DenoiseSpatialInfo(C.Structure):
    """mi355enc_denoise_spatial_info_t: a picture's record -- its measurement, the state behind it (1/256 bin), the strengths it was filtered with"""
    NAMES = ("candidates", "voters", "v", "valid", "x", "s_luma", "s_chroma")
    _fields_ = [(n, C.c_int) for n in NAMES + ("reserved",)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in self.NAMES}


class Lut3d(C.Structure):
    """mi355enc_lut3d_t: the nodes per axis and the strength 0 .. 256"""
    _fields_ = [("size", C.c_int), ("strength", C.c_int)]

    def as_dict(self):
        return dict(size=int(self.size), strength=int(self.strength))


class RoiRect(C.Structure):
    """mi355enc_roi_rect_t: a rectangle in luma samples, its QP offset -12 .. +12 (not 0) and its feather 0 .. 8 in macroblocks"""
    _fields_ = [(n, C.c_int) for n in ("x", "y", "w", "h", "delta", "feather")]


class Roi(C.Structure):
    """mi355enc_roi_t: up to eight rectangles and the cap 0 .. 12 of the background offset"""
    _fields_ = [("n_rects", C.c_int), ("rect", RoiRect * 8), ("balance", C.c_int)]

    def as_dict(self):
        n = max(0, min(8, int(self.n_rects)))
        return dict(rects=[tuple(int(getattr(self.rect[k], f)) for f, _ in RoiRect._fields_) for k in range(n)], balance=int(self.balance))


class MaskRegion(C.Structure):
    """mi355enc_mask_region_t: a rectangle in luma samples, mode 1 fill / 2 pixelate / 3 blur, param (0 / the cell size / the radius), shape 0 rectangle / 1
    ellipse, and the fill colour 0xRRGGBB"""
    _fields_ = [(n, C.c_int) for n in ("x", "y", "w", "h", "mode", "param", "shape")] + [("colour", C.c_uint)]


class Mask(C.Structure):
    """mi355enc_mask_t: up to eight regions"""
    _fields_ = [("n", C.c_int), ("region", MaskRegion * 8)]

    def as_list(self):
        n = max(0, min(8, int(self.n)))
        return [tuple(int(getattr(self.region[k], f)) for f, _ in MaskRegion._fields_) for k in range(n)]


class Warp(C.Structure):
    """mi355enc_warp_t: the filter (0 bilinear, 1 bicubic) and the Y, Cb, Cr of the samples whose source lies outside the picture"""
    _fields_ = [("kind", C.c_int), ("fill", C.c_uint8 * 3)]

    def as_dict(self):
        return dict(kind=int(self.kind), fill=tuple(int(v) for v in self.fill))


class WarpParams(C.Structure):
    """mi355enc_warp_params_t, Q16: radial terms, zoom, the roll's cos / sin, keystone"""
    _fields_ = [(n, C.c_int) for n in ("k1", "k2", "zoom", "cos", "sin", "kh", "kv")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ImageLayer(C.Structure):
    """mi355enc_image_layer_t: 4-byte pixels with straight alpha in byte order fmt (FMT_BGRX = BGRA, FMT_RGBX = RGBA, FMT_XRGB = ARGB, FMT_XBGR = ABGR), rows `stride`
    bytes apart, the top-left pixel at (x, y) of the coded visible picture, opacity 0 .. 256"""
    _fields_ = [("fmt", C.c_int), ("pixels", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("stride", C.c_int), ("x", C.c_int), ("y", C.c_int), ("opacity", C.c_int)]


class ImageInfo(C.Structure):
    """mi355enc_image_info_t: what a layer put into a picture (serial 0, w = h = 0: nothing)"""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("x", C.c_int), ("y", C.c_int), ("opacity", C.c_int), ("serial", C.c_uint32)]

    def as_tuple(self):
        return (self.w, self.h, self.x, self.y, self.opacity, int(self.serial))


class Geometry(C.Structure):
    """mi355enc_geometry_t: the submitted size, the crop rectangle inside it, the destination rectangle inside the pre-orientation target, the border colour, flags"""
    _fields_ = [("in_w", C.c_int), ("in_h", C.c_int), ("crop_x", C.c_int), ("crop_y", C.c_int), ("crop_w", C.c_int), ("crop_h", C.c_int),
                ("dst_x", C.c_int), ("dst_y", C.c_int), ("dst_w", C.c_int), ("dst_h", C.c_int),
                ("border_y", C.c_int), ("border_cb", C.c_int), ("border_cr", C.c_int), ("flags", C.c_uint)]


class SnapshotReq(C.Structure):
    """mi355enc_snapshot_req_t: what 0 the coded source / 1 the deblocked reconstruction; reduce 1, 2, 4 or 8; quality 1 .. 100"""
    _fields_ = [("what", C.c_int), ("reduce", C.c_int), ("quality", C.c_int)]


class SnapshotInfo(C.Structure):
    """mi355enc_snapshot_info_t: the picture a still was taken of (index: its position in the stream) and the still's size"""
    _fields_ = [("pts", C.c_int64), ("index", C.c_uint64), ("width", C.c_int), ("height", C.c_int), ("what", C.c_int), ("quality", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class Rate(C.Structure):
    """mi355enc_rate_t: mode 0 off / 1 hold / 2 blend; the pts units per second; the most repeats one submit may yield"""
    _fields_ = [("mode", C.c_int), ("pts_per_second", C.c_int64), ("max_fill", C.c_int)]


class RateStats(C.Structure):
    """mi355enc_rate_stats_t"""
    _fields_ = [("in_", C.c_uint64), ("out", C.c_uint64), ("dropped", C.c_uint64), ("repeated", C.c_uint64), ("blended", C.c_uint64), ("resyncs", C.c_uint64)]

    def as_dict(self):
        return {k.rstrip("_"): int(getattr(self, k)) for k, _ in self._fields_}


class RatePlanState(C.Structure):
    """mi355enc_rate_plan_t"""
    _fields_ = [("mode", C.c_int), ("fps_num", C.c_int), ("fps_den", C.c_int), ("max_fill", C.c_int), ("started", C.c_int),
                ("pps", C.c_int64), ("t0", C.c_int64), ("k_next", C.c_int64), ("prev_pts", C.c_int64)]


RATE_OFF, RATE_HOLD, RATE_BLEND = 0, 1, 2
RATE_MAX_OUT = 16
SNAP_SOURCE, SNAP_DECODED = 0, 1
IMAGE_LAYERS, IMAGE_MAX_DIM = 4, 4096
GEOM_KEEP_SAR = 1  # mi355enc_geometry_t.flags: no aspect ratio from the geometry in the SPS
OVERLAY_MAX_TEXT = 255
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libmi355enc.so not built (run `python -c 'import __graft_entry__ as g; g.build()'`)")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.mi355enc_strerror.restype = C.c_char_p
        L.mi355enc_strerror.argtypes = [C.c_int]
        L.mi355enc_default_cfg.restype = None
        L.mi355enc_default_cfg.argtypes = [C.POINTER(Cfg), C.c_int, C.c_int, C.c_int, C.c_int]
        L.mi355enc_open.argtypes = [C.POINTER(Cfg), C.POINTER(vp)]
        L.mi355enc_close.restype = None
        L.mi355enc_close.argtypes = [vp]
        L.mi355enc_set_bitrate.argtypes = [vp, C.c_uint32]
        L.mi355enc_get_bitrate.restype = C.c_uint32
        L.mi355enc_get_bitrate.argtypes = [vp]
        L.mi355enc_set_fixed_qp.argtypes = [vp, C.c_int]
        L.mi355enc_set_fixed_drop.argtypes = [vp, C.c_int]
        L.mi355enc_set_intra_refresh.argtypes = [vp, C.c_int]
        L.mi355enc_encode.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, vp, C.c_size_t,
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.mi355enc_submit.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int]
        L.mi355enc_submit_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int]
        L.mi355enc_pending.argtypes = [vp]
        L.mi355enc_collect.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.mi355enc_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.mi355enc_reset_stats.restype = None
        L.mi355enc_reset_stats.argtypes = [vp]
        L.mi355enc_max_au_bytes.restype = C.c_size_t
        L.mi355enc_max_au_bytes.argtypes = [vp]
        L.mi355enc_fetch.argtypes = [vp, C.c_int, vp, C.c_size_t]
        L.mi355enc_mb_width.argtypes = [vp]
        L.mi355enc_mb_height.argtypes = [vp]
        L.mi355enc_stage_me.argtypes = [vp, vp, vp, C.c_int, vp, vp]
        L.mi355enc_stage_me_select.argtypes = [vp, vp, vp, C.c_int, vp]
        L.mi355enc_stage_subpel.argtypes = [vp, vp, vp, C.c_int, vp]
        L.mi355enc_stage_inter.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
        L.mi355enc_stage_pmb.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp]
        L.mi355enc_stage_intra.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
        L.mi355enc_stage_intra_analyse.argtypes = [vp, vp, vp, C.c_int, vp, vp]
        L.mi355enc_stage_deblock.argtypes = [vp, vp, vp, vp]
        L.mi355enc_submit_fmt.argtypes = [vp, C.c_int, vp, vp, C.c_int64, C.c_int]
        L.mi355enc_stage_csc.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.mi355enc_debug_trip_wait.argtypes = [vp, C.c_uint]
        L.mi355enc_debug_get_counters.argtypes = [vp, C.POINTER(Counters)]
        L.mi355enc_debug_set_counters.argtypes = [vp, C.POINTER(Counters)]
        L.mi355enc_set_input_size.argtypes = [vp, C.c_int, C.c_int]
        L.mi355enc_stage_scale.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.mi355enc_scale_table.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, C.c_size_t, C.POINTER(C.c_int)]
        L.mi355enc_set_colorimetry.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.mi355enc_csc_coefficients.argtypes = [C.c_int, C.c_int, vp]
        L.mi355enc_host_write_headers_vui.argtypes = [C.c_int] * 11 + [vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.mi355enc_stage_csc_device.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.mi355enc_set_input_colorimetry.argtypes = [vp, C.c_int, C.c_int]
        L.mi355enc_yuv_coefficients.argtypes = [C.c_int] * 4 + [vp]
        L.mi355enc_set_hdr_input.argtypes = [vp] + [C.c_int] * 4
        L.mi355enc_hdr_tables.argtypes = [C.c_int] * 6 + [vp, C.c_size_t, vp]
        L.mi355enc_stage_yuv_convert.argtypes = [vp, vp, vp]
        L.mi355enc_adjust_default.restype = None
        L.mi355enc_adjust_default.argtypes = [C.POINTER(Adjust)]
        L.mi355enc_adjust_check.argtypes = [C.POINTER(Adjust)]
        L.mi355enc_adjust_tables.argtypes = [C.POINTER(Adjust), C.c_int, vp, vp]
        L.mi355enc_set_adjust.argtypes = [vp, C.POINTER(Adjust)]
        L.mi355enc_get_adjust.argtypes = [vp, C.POINTER(Adjust)]
        L.mi355enc_last_adjust.argtypes = [vp, C.POINTER(Adjust)]
        L.mi355enc_stage_adjust.argtypes = [vp, C.POINTER(Adjust), vp, vp]
        L.mi355enc_debug_adjust_bytes.restype = C.c_size_t
        L.mi355enc_debug_adjust_bytes.argtypes = [vp]
        L.mi355enc_denoise_default.restype = None
        L.mi355enc_denoise_default.argtypes = [C.POINTER(Denoise)]
        L.mi355enc_denoise_check.argtypes = [C.POINTER(Denoise)]
        L.mi355enc_denoise_tables.argtypes = [C.POINTER(Denoise), vp, vp, vp]
        L.mi355enc_set_denoise.argtypes = [vp, C.POINTER(Denoise)]
        L.mi355enc_get_denoise.argtypes = [vp, C.POINTER(Denoise)]
        L.mi355enc_last_denoise.argtypes = [vp, C.POINTER(Denoise)]
        L.mi355enc_stage_denoise.argtypes = [vp, C.POINTER(Denoise)] + [vp] * 6
        L.mi355enc_debug_denoise_bytes.restype = C.c_size_t
        L.mi355enc_debug_denoise_bytes.argtypes = [vp]
        L.mi355enc_set_denoise_motion.argtypes = [vp, C.c_int]
        L.mi355enc_get_denoise_motion.argtypes = [vp, C.POINTER(C.c_int)]
        L.mi355enc_last_denoise_motion.argtypes = [vp, C.POINTER(C.c_int)]
        L.mi355enc_denoise_motion_key.restype = C.c_uint32
        L.mi355enc_denoise_motion_key.argtypes = [C.c_int] * 4
        L.mi355enc_stage_denoise_search.argtypes = [vp, C.POINTER(Denoise), C.c_int, vp, vp, vp]
        L.mi355enc_stage_denoise_mc.argtypes = [vp, C.POINTER(Denoise), C.c_int] + [vp] * 7
        L.mi355enc_autolevel_default.restype = None
        L.mi355enc_autolevel_default.argtypes = [C.POINTER(Autolevel)]
        L.mi355enc_autolevel_check.argtypes = [C.POINTER(Autolevel)]
        L.mi355enc_autolevel_decide.argtypes = [C.POINTER(AutolevelMeas), C.POINTER(Autolevel), C.c_int, C.c_int, C.POINTER(C.c_int32 * 4), C.POINTER(AutolevelInfo), vp]
        L.mi355enc_set_autolevel.argtypes = [vp, C.POINTER(Autolevel)]
        L.mi355enc_get_autolevel.argtypes = [vp, C.POINTER(Autolevel)]
        L.mi355enc_last_autolevel.argtypes = [vp, C.POINTER(Autolevel), C.POINTER(AutolevelInfo), vp]
        L.mi355enc_debug_autolevel_bytes.restype = C.c_size_t
        L.mi355enc_debug_autolevel_bytes.argtypes = [vp]
        L.mi355enc_autolevel_probe_stage.argtypes = [vp, C.POINTER(Autolevel), vp, vp, C.POINTER(AutolevelInfo), vp]
        L.mi355enc_autolevel_probe_measure.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(C.c_int * 4), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(AutolevelMeas)]
        L.mi355enc_autolevel_probe_decide.argtypes = [vp, C.POINTER(AutolevelMeas), C.POINTER(Autolevel), C.c_int, C.c_int, C.POINTER(C.c_int32 * 4), C.POINTER(AutolevelInfo), vp]
        L.mi355enc_stabilize_default.restype = None
        L.mi355enc_stabilize_default.argtypes = [C.POINTER(Stabilize)]
        L.mi355enc_stabilize_check.argtypes = [C.POINTER(Stabilize)]
        L.mi355enc_set_stabilize.argtypes = [vp, C.POINTER(Stabilize)]
        L.mi355enc_get_stabilize.argtypes = [vp, C.POINTER(Stabilize)]
        L.mi355enc_last_stabilize.argtypes = [vp, C.POINTER(Stabilize), C.POINTER(StabilizeInfo)]
        L.mi355enc_debug_stabilize_bytes.restype = C.c_size_t
        L.mi355enc_debug_stabilize_bytes.argtypes = [vp]
        L.mi355enc_stabilize_project.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.mi355enc_stabilize_vote.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.mi355enc_stabilize_motion.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
        L.mi355enc_stabilize_step.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)] * 2
        L.mi355enc_stabilize_probe_project.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.mi355enc_stabilize_probe_match.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(Stabilize), C.POINTER(C.c_int * 4), C.POINTER(C.c_int * 2), C.c_int, C.POINTER(StabilizeInfo)]
        L.mi355enc_warp_params_default.restype = None
        L.mi355enc_warp_params_default.argtypes = [C.POINTER(WarpParams)]
        L.mi355enc_warp_coeff.argtypes = [C.c_int, C.c_int, vp]
        L.mi355enc_warp_mesh_size.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355enc_warp_mesh_check.argtypes = [vp, C.c_int, C.c_int]
        L.mi355enc_warp_build.argtypes = [C.POINTER(WarpParams), C.c_int, C.c_int, vp, C.c_size_t]
        L.mi355enc_warp_apply_host.argtypes = [C.POINTER(Warp), vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int]
        L.mi355enc_set_warp.argtypes = [vp, C.POINTER(Warp), C.POINTER(WarpParams)]
        L.mi355enc_set_warp_mesh.argtypes = [vp, C.POINTER(Warp), vp, C.c_int, C.c_int]
        L.mi355enc_get_warp.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(Warp)]
        L.mi355enc_last_warp.argtypes = [vp, C.POINTER(C.c_uint)]
        L.mi355enc_debug_warp_bytes.restype = C.c_size_t
        L.mi355enc_debug_warp_bytes.argtypes = [vp]
        L.mi355enc_warp_probe.argtypes = [vp, C.POINTER(Warp), vp, vp, vp]
        L.mi355enc_warp_plan.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355enc_debug_warp_staging.argtypes = [vp, C.c_int]
        L.mi355enc_denoise_spatial_default.restype = None
        L.mi355enc_denoise_spatial_default.argtypes = [C.POINTER(DenoiseSpatial)]
        L.mi355enc_denoise_spatial_check.argtypes = [C.POINTER(DenoiseSpatial)]
        L.mi355enc_denoise_spatial_tables.argtypes = [C.c_int, vp, vp]
        L.mi355enc_denoise_spatial_apply_host.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_int * 4), C.c_int, C.c_int, C.c_int, C.c_int]
        L.mi355enc_denoise_spatial_measure_host.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int * 4), C.c_int, C.c_int, C.c_int, C.POINTER(DenoiseSpatialMeas)]
        L.mi355enc_denoise_spatial_decide.argtypes = [C.POINTER(DenoiseSpatialMeas), C.POINTER(DenoiseSpatial), C.c_int, C.POINTER(C.c_int32), C.POINTER(DenoiseSpatialInfo)]
        L.mi355enc_set_denoise_spatial.argtypes = [vp, C.POINTER(DenoiseSpatial)]
        L.mi355enc_get_denoise_spatial.argtypes = [vp, C.POINTER(DenoiseSpatial)]
        L.mi355enc_last_denoise_spatial.argtypes = [vp, C.POINTER(DenoiseSpatial), C.POINTER(DenoiseSpatialInfo)]
        L.mi355enc_debug_denoise_spatial_bytes.restype = C.c_size_t
        L.mi355enc_debug_denoise_spatial_bytes.argtypes = [vp]
        L.mi355enc_denoise_spatial_probe_stage.argtypes = [vp, C.POINTER(DenoiseSpatial), vp, vp, C.POINTER(DenoiseSpatialInfo)]
        L.mi355enc_denoise_spatial_probe_measure.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_int * 4), C.c_int, C.c_int, C.c_int, C.POINTER(DenoiseSpatialMeas)]
        L.mi355enc_denoise_spatial_probe_decide.argtypes = [vp, C.POINTER(DenoiseSpatialMeas), C.POINTER(DenoiseSpatial), C.c_int, C.POINTER(C.c_int32), C.POINTER(DenoiseSpatialInfo)]
        L.mi355enc_lut3d_coefficients.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32 * 19)]
        L.mi355enc_lut3d_check.argtypes = [vp, C.c_int]
        L.mi355enc_lut3d_identity.argtypes = [C.c_int, vp]
        L.mi355enc_lut3d_parse_cube.argtypes = [C.c_char_p, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_int)]
        L.mi355enc_lut3d_apply_host.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.POINTER(C.c_int * 4)]
        L.mi355enc_lut3d_plan.argtypes = [C.c_int]
        L.mi355enc_set_lut3d.argtypes = [vp, C.POINTER(Lut3d), vp]
        L.mi355enc_get_lut3d.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(Lut3d)]
        L.mi355enc_last_lut3d.argtypes = [vp, C.POINTER(Lut3d), C.POINTER(C.c_uint)]
        L.mi355enc_debug_lut3d_bytes.restype = C.c_size_t
        L.mi355enc_debug_lut3d_bytes.argtypes = [vp]
        L.mi355enc_lut3d_probe.argtypes = [vp, C.POINTER(Lut3d), vp, vp, vp, C.c_int]
        L.mi355enc_debug_lut3d_form.argtypes = [vp, C.c_int]
        L.mi355enc_roi_default.argtypes = [C.POINTER(Roi)]
        L.mi355enc_roi_default.restype = None
        L.mi355enc_roi_check.argtypes = [C.POINTER(Roi)]
        L.mi355enc_roi_map.argtypes = [C.POINTER(Roi), vp, C.c_int, C.c_int, vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355enc_roi_parse.argtypes = [C.c_char_p, C.POINTER(Roi)]
        L.mi355enc_set_roi.argtypes = [vp, C.POINTER(Roi), vp]
        L.mi355enc_get_roi.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(Roi)]
        L.mi355enc_last_roi.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355enc_debug_roi_bytes.restype = C.c_size_t
        L.mi355enc_debug_roi_bytes.argtypes = [vp]
        L.mi355enc_roi_probe_set_map.argtypes = [vp, vp]
        L.mi355enc_roi_probe_offsets.argtypes = [vp, vp, vp]
        L.mi355enc_mask_check.argtypes = [C.POINTER(Mask)]
        L.mi355enc_mask_parse.argtypes = [C.c_char_p, C.c_uint, C.POINTER(Mask)]
        L.mi355enc_mask_apply_host.argtypes = [C.POINTER(Mask), vp, C.c_int, C.c_int, vp, vp]
        L.mi355enc_mask_ellipse.argtypes = [C.c_int] * 4
        L.mi355enc_mask_mean.argtypes = [C.c_int] * 2
        L.mi355enc_mask_colour.argtypes = [C.c_uint, vp, vp]
        L.mi355enc_set_mask.argtypes = [vp, C.POINTER(Mask)]
        L.mi355enc_get_mask.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(Mask)]
        L.mi355enc_last_mask.argtypes = [vp, C.POINTER(Mask), C.POINTER(C.c_uint)]
        L.mi355enc_debug_mask_bytes.restype = C.c_size_t
        L.mi355enc_debug_mask_bytes.argtypes = [vp]
        L.mi355enc_mask_probe.argtypes = [vp, C.POINTER(Mask), vp, vp]
        L.mi355enc_set_quality_metrics.argtypes = [vp, C.c_int]
        L.mi355enc_last_quality.argtypes = [vp, C.POINTER(Quality)]
        L.mi355enc_quality_totals.argtypes = [vp, C.POINTER(Quality)]
        L.mi355enc_stage_quality.argtypes = [vp, vp, vp, vp, vp, C.POINTER(Quality)]
        L.mi355enc_stage_quality_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.POINTER(Quality)]
        L.mi355enc_overlay_default_style.restype = None
        L.mi355enc_overlay_default_style.argtypes = [C.POINTER(OverlayStyle)]
        L.mi355enc_set_overlay_style.argtypes = [vp, C.POINTER(OverlayStyle)]
        L.mi355enc_set_overlay_text.argtypes = [vp, C.c_char_p]
        L.mi355enc_last_overlay.argtypes = [vp, vp, C.c_size_t]
        L.mi355enc_overlay_glyph.argtypes = [C.c_int, vp]
        L.mi355enc_stage_overlay.argtypes = [vp, C.c_char_p, C.POINTER(OverlayStyle), vp, vp]
        L.mi355enc_set_image.argtypes = [vp, C.c_int, C.POINTER(ImageLayer)]
        L.mi355enc_set_image_place.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.mi355enc_last_image.argtypes = [vp, C.c_int, C.POINTER(ImageInfo)]
        L.mi355enc_stage_image.argtypes = [vp, C.POINTER(ImageLayer), C.c_int, vp, vp]
        L.mi355enc_debug_image_bytes.restype = C.c_size_t
        L.mi355enc_debug_image_bytes.argtypes = [vp]
        L.mi355enc_image_pixel.argtypes = [C.c_int] * 5 + [vp]
        L.mi355enc_image_load_pam.argtypes = [vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), vp, C.c_size_t]
        L.mi355enc_jpeg_info.argtypes = [vp, C.c_size_t, C.POINTER(JpegInfo)]
        L.mi355enc_jpeg_entropy_decode.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(JpegInfo)]
        L.mi355enc_submit_jpeg.argtypes = [vp, vp, C.c_size_t, C.c_int64, C.c_int]
        L.mi355enc_stage_jpeg.argtypes = [vp, vp, C.c_size_t, vp, vp]
        L.mi355enc_stage_jpeg_blocks.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
        L.mi355enc_set_orientation.argtypes = [vp, C.c_int]
        L.mi355enc_get_orientation.argtypes = [vp]
        L.mi355enc_orient_size.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355enc_orient_source.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355enc_stage_orient.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp]
        L.mi355enc_stage_orient_device.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp]
        L.mi355enc_debug_orient_bytes.restype = C.c_size_t
        L.mi355enc_debug_orient_bytes.argtypes = [vp]
        L.mi355enc_set_input_geometry.argtypes = [vp, C.POINTER(Geometry)]
        L.mi355enc_get_input_geometry.argtypes = [vp, C.POINTER(Geometry)]
        L.mi355enc_set_crop.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.mi355enc_geometry_table.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_size_t, C.POINTER(C.c_int)]
        L.mi355enc_fit_rect.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)] * 4
        L.mi355enc_stage_geometry.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.mi355enc_geometry_check.argtypes = [C.POINTER(Geometry), C.c_int, C.c_int]
        L.mi355enc_geometry_sar.argtypes = [C.POINTER(Geometry), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355enc_request_snapshot.argtypes = [vp, C.POINTER(SnapshotReq)]
        L.mi355enc_take_snapshot.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(SnapshotInfo)]
        L.mi355enc_debug_snapshot_bytes.restype = C.c_size_t
        L.mi355enc_debug_snapshot_bytes.argtypes = [vp]
        L.mi355enc_snapshot_tables.argtypes = [C.c_int, vp]
        L.mi355enc_snapshot_reciprocal.restype = C.c_uint32
        L.mi355enc_snapshot_reciprocal.argtypes = [C.c_int]
        L.mi355enc_snapshot_max_bytes.restype = C.c_size_t
        L.mi355enc_snapshot_max_bytes.argtypes = [C.c_int, C.c_int]
        L.mi355enc_snapshot_write.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.mi355enc_stage_snapshot_blocks.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
        L.mi355enc_stage_snapshot_blocks_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
        L.mi355enc_stage_snapshot.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.mi355enc_rate_check.argtypes = [C.POINTER(Rate)]
        L.mi355enc_set_rate_conversion.argtypes = [vp, C.POINTER(Rate)]
        L.mi355enc_rate_peek.argtypes = [vp, C.c_int64]
        L.mi355enc_last_submit_count.argtypes = [vp]
        L.mi355enc_rate_stats.argtypes = [vp, C.POINTER(RateStats)]
        L.mi355enc_debug_rate_bytes.restype = C.c_size_t
        L.mi355enc_debug_rate_bytes.argtypes = [vp]
        L.mi355enc_rate_plan_init.restype = None
        L.mi355enc_rate_plan_init.argtypes = [C.POINTER(RatePlanState), C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64]
        L.mi355enc_rate_plan_step.argtypes = [C.POINTER(RatePlanState), C.c_int64, C.POINTER(C.c_int), vp, vp, C.POINTER(C.c_int)]
        L.mi355enc_stage_rate.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
        L.mi355enc_host_alloc.restype = vp
        L.mi355enc_host_alloc.argtypes = [C.c_size_t]
        L.mi355enc_host_free.restype = None
        L.mi355enc_host_free.argtypes = [vp]
        L.mi355enc_time_stage.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.mi355enc_host_write_headers.argtypes = [C.c_int] * 5 + [vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.mi355enc_host_set_slice_rows.argtypes = [C.c_int]
        L.mi355enc_host_set_slice_rows.restype = None
        L.mi355enc_host_set_p_slices.argtypes = [C.c_int, C.c_int]
        L.mi355enc_host_set_p_slices.restype = None
        L.mi355enc_stage_set_slice_rows.argtypes = [vp, C.c_int]
        L.mi355enc_slice_rows.argtypes = [vp]
        L.mi355enc_p_slice_rows.argtypes = [vp]
        L.mi355enc_stage_set_slice_deblock.argtypes = [vp, C.c_int]
        L.mi355enc_host_write_slice.argtypes = [C.c_int] * 7 + [vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.mi355enc_host_write_slice_packed.argtypes = [C.c_int] * 8 + [vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.mi355enc_host_cavlc_block.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
        L.mi355enc_rc_init.restype = None
        L.mi355enc_rc_init.argtypes = [vp, C.c_double, C.c_int, C.c_uint32, C.c_int, C.c_int]
        L.mi355enc_rc_set_bitrate.restype = None
        L.mi355enc_rc_set_bitrate.argtypes = [vp, C.c_uint32]
        L.mi355enc_rc_pick.restype = None
        L.mi355enc_rc_pick.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355enc_rc_update.restype = None
        L.mi355enc_rc_update.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_size_t]
        _lib = L
    return _lib


def host_cavlc_block(coef, maxnum, nC):
    """One residual block through the product's CAVLC block coder; returns the bits as a '0'/'1' string."""
    L = load()
    c = np.ascontiguousarray(coef, np.int16)
    assert c.size == maxnum
    out = np.zeros(64, np.uint8)
    n = L.mi355enc_host_cavlc_block(c.ctypes.data_as(C.c_void_p), maxnum, nC, out.ctypes.data_as(C.c_void_p), out.size)
    if n < 0:
        raise RuntimeError("mi355enc_host_cavlc_block: %d" % n)
    return "".join("{:08b}".format(b) for b in out)[:n]


def host_write_headers(width, height, fps_num, fps_den=1, transform8x8=False, colorimetry=None, sar=None):
    """SPS + PPS.  colorimetry: (full_range, primaries, transfer, matrix) for the VUI (Encoder.set_colorimetry); sar: (w, h) sample aspect ratio."""
    L = load()
    out, n = np.empty(256, np.uint8), C.c_size_t(0)
    if colorimetry is None and sar is None:
        r = L.mi355enc_host_write_headers(width, height, fps_num, fps_den, int(transform8x8), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
    else:
        fr, p, t, m = colorimetry if colorimetry is not None else (0, 2, 2, 2)
        sw, sh = sar if sar is not None else (0, 0)
        r = L.mi355enc_host_write_headers_vui(width, height, fps_num, fps_den, int(transform8x8), int(sw), int(sh), int(fr), int(p), int(t), int(m),
                                              out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
    if r:
        raise RuntimeError("mi355enc_host_write_headers: %d" % r)
    return bytes(out[: n.value])


def yuv_coefficients(in_matrix, in_full, out_matrix, out_full):
    """The library's integer YUV -> YUV table (host only): int32 (9,) = cyy, cyb, cyr, cbb, cbr, crb, crr in 2^-16 units, the input's and the output's luma offset."""
    c = np.zeros(9, np.int32)
    r = load().mi355enc_yuv_coefficients(int(in_matrix), int(in_full), int(out_matrix), int(out_full), c.ctypes.data_as(C.c_void_p))
    if r:
        raise EncoderError("mi355enc_yuv_coefficients(%d, %d, %d, %d): %d" % (in_matrix, in_full, out_matrix, out_full, r))
    return c


def adjust(a=None, **kw):
    """An Adjust: the neutral values (mi355enc_adjust_default), then a's (an Adjust or a dict) and the keywords' on top.  Not checked here."""
    st = Adjust()
    load().mi355enc_adjust_default(C.byref(st))
    src = a.as_dict() if isinstance(a, Adjust) else dict(a or {})
    src.update(kw)
    for k, v in src.items():
        if k not in Adjust.NAMES:
            raise TypeError("adjust: no parameter %r" % (k,))
        setattr(st, k, int(v))
    return st


def adjust_check(a=None, **kw):
    """mi355enc_adjust_check (host only): 0, or the error code for a value outside its range"""
    return load().mi355enc_adjust_check(C.byref(adjust(a, **kw)))


def adjust_tables(a, full_range=0):
    """The picture controls' luma table and chroma rotation for an output range (host only): (uint8 (256,), int32 (2,) = cu, su)."""
    st = adjust(a)
    luma, chroma = np.zeros(256, np.uint8), np.zeros(2, np.int32)
    r = load().mi355enc_adjust_tables(C.byref(st), int(full_range), luma.ctypes.data_as(C.c_void_p), chroma.ctypes.data_as(C.c_void_p))
    if r:
        raise EncoderError("mi355enc_adjust_tables(%r, %d): %d" % (st.as_dict(), full_range, r))
    return luma, chroma


def denoise(d=None, **kw):
    """A Denoise: off, then d's (a Denoise or a dict) and the keywords' luma / chroma on top.  Not checked here."""
    src = d.as_dict() if isinstance(d, Denoise) else dict(d or {})
    src.update(kw)
    if set(src) - {"luma", "chroma"}:
        raise TypeError("denoise: no parameter %r" % (sorted(set(src) - {"luma", "chroma"}),))
    return Denoise(int(src.get("luma", 0)), int(src.get("chroma", 0)))


def stabilize(s=None, **kw):
    """A Stabilize: off with leak 16, then s's (a Stabilize or a dict) and the keywords' range / leak / margin_x / margin_y on top; margin=m or margin=(mx, my) sets
    both margins.  stabilize(range=16, margin=32) is the usual way to turn it on.  Not checked here."""
    src = s.as_dict() if isinstance(s, Stabilize) else dict(s or {})
    src.update(kw)
    if "margin" in src:
        m = src.pop("margin")
        src["margin_x"], src["margin_y"] = (m, m) if np.isscalar(m) else m
    if set(src) - {"range", "leak", "margin_x", "margin_y"}:
        raise TypeError("stabilize: no parameter %r" % (sorted(set(src) - {"range", "leak", "margin_x", "margin_y"}),))
    return Stabilize(int(src.get("range", 0)), int(src.get("leak", 16)), int(src.get("margin_x", 0)), int(src.get("margin_y", 0)))


def stabilize_check(s=None, **kw):
    """mi355enc_stabilize_check (host only): 0, or the error code"""
    return load().mi355enc_stabilize_check(C.byref(stabilize(s, **kw)))


def _luma_view(luma, step):
    """(address, stride, w, h) of a 2-D uint8 view whose samples lie `step` bytes apart in their rows"""
    if luma.dtype != np.uint8 or luma.ndim != 2 or luma.strides[1] != step:
        raise ValueError("a 2-D uint8 view with samples %d bytes apart" % step)
    return luma.ctypes.data, int(luma.strides[0]), int(luma.shape[1]), int(luma.shape[0])


def stabilize_project(luma):
    """mi355enc_stabilize_project (host only): the band sums of a luma plane -- a 2-D uint8 view, samples 1 or 2 bytes apart, any row stride -> (C (4, w), R (4, h)) uint32"""
    step = int(luma.strides[1])
    addr, stride, w, h = _luma_view(luma, step)
    sums = np.zeros(4 * (w + h), np.uint32)
    r = load().mi355enc_stabilize_project(addr, stride, step, w, h, _p(sums))
    if r:
        raise EncoderError("mi355enc_stabilize_project: %d" % r)
    return sums[:4 * w].reshape(4, w), sums[4 * w:].reshape(4, h)


def stabilize_vote(p, q, rng):
    """mi355enc_stabilize_vote (host only): (valid, d) of projection p against the previous picture's q"""
    p, q = np.ascontiguousarray(p, np.uint32), np.ascontiguousarray(q, np.uint32)
    d = C.c_int(0)
    r = load().mi355enc_stabilize_vote(_p(p), _p(q), int(p.size), int(rng), C.byref(d))
    if r < 0 or p.size != q.size:
        raise EncoderError("mi355enc_stabilize_vote: %d" % r)
    return bool(r), int(d.value)


def stabilize_motion(votes):
    """mi355enc_stabilize_motion (host only): the lower median of the valid votes, 0 with none"""
    v = (C.c_int * max(1, len(votes)))(*[int(x) for x in votes])
    m = C.c_int(0)
    r = load().mi355enc_stabilize_motion(v, len(votes), C.byref(m))
    if r:
        raise EncoderError("mi355enc_stabilize_motion: %d" % r)
    return int(m.value)


def stabilize_step(S, m, leak, lo, hi):
    """mi355enc_stabilize_step (host only): one trajectory step of an axis -> (S, o)"""
    s_out, o = C.c_int(0), C.c_int(0)
    r = load().mi355enc_stabilize_step(int(S), int(m), int(leak), int(lo), int(hi), C.byref(s_out), C.byref(o))
    if r:
        raise EncoderError("mi355enc_stabilize_step(%d, %d, %d, %d, %d): %d" % (S, m, leak, lo, hi, r))
    return int(s_out.value), int(o.value)


def autolevel(a=None, **kw):
    """An Autolevel: the defaults (off: mi355enc_autolevel_default), then a's (an Autolevel or a dict) and the keywords' on top; clip=c sets both clips.
    autolevel(levels=1000, balance=1000) is the usual way to turn it on.  Not checked here."""
    st = Autolevel()
    load().mi355enc_autolevel_default(C.byref(st))
    src = a.as_dict() if isinstance(a, Autolevel) else dict(a or {})
    src.update(kw)
    if "clip" in src:
        src["clip_low"] = src["clip_high"] = src.pop("clip")
    for k, v in src.items():
        if k not in Autolevel.NAMES:
            raise TypeError("autolevel: no parameter %r" % (k,))
        setattr(st, k, int(v))
    return st


def autolevel_check(a=None, **kw):
    """mi355enc_autolevel_check (host only): 0, or the error code for a value outside its range"""
    return load().mi355enc_autolevel_check(C.byref(autolevel(a, **kw)))


def autolevel_meas(hist, voters, su, sv, chroma):
    """An AutolevelMeas from the histogram (256 counts), n, su, sv and NC"""
    m = AutolevelMeas()
    m.hist[:] = [int(v) for v in hist]
    m.voters, m.chroma, m.su, m.sv = int(voters), int(chroma), int(su), int(sv)
    return m


def _autolevel_decide(fn, what, m, a, full_range, state, prime):
    st = (C.c_int32 * 4)(*[int(v) for v in (state if state is not None else (0, 0, 0, 0))])
    info, table = AutolevelInfo(), np.zeros(256, np.uint8)
    m = m if isinstance(m, AutolevelMeas) else autolevel_meas(**m)
    r = fn(C.byref(m), C.byref(autolevel(a)), int(full_range), int(bool(prime)), C.byref(st), C.byref(info), _p(table))
    if r:
        raise EncoderError("%s: failed (%d)" % (what, r))
    return info.as_dict(), table, tuple(int(v) for v in st)


def autolevel_decide(m, a, full_range=0, state=None, prime=False):
    """mi355enc_autolevel_decide (host only): a picture's decision from its measurement (an AutolevelMeas or dict(hist=, voters=, su=, sv=, chroma=)), a
    setting, the output range and the state {Lo, Hi, Du, Dv} going in -> (record, table, state coming out)"""
    return _autolevel_decide(load().mi355enc_autolevel_decide, "autolevel_decide", m, a, full_range, state, prime)


def denoise_spatial(a=None, **kw):
    """A DenoiseSpatial: the defaults (off: mi355enc_denoise_spatial_default), then a's (a DenoiseSpatial or a dict) and the keywords' on top.  Not checked here."""
    st = DenoiseSpatial()
    load().mi355enc_denoise_spatial_default(C.byref(st))
    src = a.as_dict() if isinstance(a, DenoiseSpatial) else dict(a or {})
    src.update(kw)
    for k, v in src.items():
        if k not in DenoiseSpatial.NAMES:
            raise TypeError("denoise_spatial: no parameter %r" % (k,))
        setattr(st, k, int(v))
    return st


def denoise_spatial_check(a=None, **kw):
    """mi355enc_denoise_spatial_check (host only): 0, or the error code for a value outside its range"""
    return load().mi355enc_denoise_spatial_check(C.byref(denoise_spatial(a, **kw)))


def denoise_spatial_tables(s):
    """mi355enc_denoise_spatial_tables (host only): (R_s, F_s) of a strength 0 .. 32"""
    weight, filt = np.zeros(256, np.uint8), np.zeros(256, np.uint16)
    r = load().mi355enc_denoise_spatial_tables(int(s), _p(weight), _p(filt))
    if r:
        raise EncoderError("denoise_spatial_tables: failed (%d)" % r)
    return weight, filt


def _surface_args(y, rect, visible):
    H, W = y.shape
    rect = rect if rect is not None else (0, W, 0, H)
    vw, vh = visible if visible is not None else (W, H)
    return W, H, C.byref((C.c_int * 4)(*[int(v) for v in rect])), int(vw), int(vh)


def denoise_spatial_apply_host(y, uv, s_luma, s_chroma, rect=None, visible=None):
    """mi355enc_denoise_spatial_apply_host (host only): the filter on NV12 surfaces y (H x W) / uv (H / 2 x W) inside rect (x0, x1, y0, y1; all of it without)
    with the visible size (vw, vh); a strength of -1 leaves its plane alone -> new (y, uv)"""
    y, uv = np.ascontiguousarray(y, np.uint8).copy(), np.ascontiguousarray(uv, np.uint8).copy()
    r = load().mi355enc_denoise_spatial_apply_host(_p(y), _p(uv), *_surface_args(y, rect, visible), int(s_luma), int(s_chroma))
    if r:
        raise EncoderError("denoise_spatial_apply_host: failed (%d)" % r)
    return y, uv


def denoise_spatial_measure_host(y, rect=None, visible=None, full_range=0):
    """mi355enc_denoise_spatial_measure_host (host only): dict(hist=, candidates=, voters=) of a luma surface"""
    y, m = np.ascontiguousarray(y, np.uint8), DenoiseSpatialMeas()
    r = load().mi355enc_denoise_spatial_measure_host(_p(y), *_surface_args(y, rect, visible), int(full_range), C.byref(m))
    if r:
        raise EncoderError("denoise_spatial_measure_host: failed (%d)" % r)
    return m.as_dict()


def denoise_spatial_meas(hist, candidates, voters):
    m = DenoiseSpatialMeas()
    m.hist[:] = [int(v) for v in hist]
    m.candidates, m.voters = int(candidates), int(voters)
    return m


def _denoise_spatial_decide(fn, what, m, a, x, prime):
    st, info = C.c_int32(int(x) if x is not None else 0), DenoiseSpatialInfo()
    m = m if isinstance(m, DenoiseSpatialMeas) else denoise_spatial_meas(**m)
    r = fn(C.byref(m), C.byref(denoise_spatial(a)), int(bool(prime)), C.byref(st), C.byref(info))
    if r:
        raise EncoderError("%s: failed (%d)" % (what, r))
    return info.as_dict(), int(st.value)


def denoise_spatial_decide(m, a, x=None, prime=False):
    """mi355enc_denoise_spatial_decide (host only): a picture's decision from its measurement (a DenoiseSpatialMeas or dict(hist=, candidates=, voters=)), an
    automatic setting and the state X going in -> (record, X coming out)"""
    return _denoise_spatial_decide(load().mi355enc_denoise_spatial_decide, "denoise_spatial_decide", m, a, x, prime)


def roi(rects=(), balance=0):
    """A Roi from rects = [(x, y, w, h, delta[, feather]), ...] and the balance cap (or a Roi, or a dict of both, as it is); nothing is checked here"""
    if isinstance(rects, Roi):
        return rects
    if isinstance(rects, dict):
        rects, balance = rects.get("rects", ()), rects.get("balance", 0)
    rects = list(rects)
    if len(rects) > 8:
        raise EncoderError("roi: more than 8 rectangles")
    c = Roi()
    c.n_rects, c.balance = len(rects), int(balance)
    for k, r in enumerate(rects):
        r = tuple(int(v) for v in r) + ((0,) if len(r) == 5 else ())
        c.rect[k] = RoiRect(*r)
    return c


def roi_check(cfg):
    """mi355enc_roi_check (host only): 0, or the error code for a field outside its range"""
    return load().mi355enc_roi_check(C.byref(roi(cfg)))


def roi_map(cfg, user, mbw, mbh):
    """mi355enc_roi_map (host only): the map of cfg (None: no rectangle) and the caller's int8 map `user` (None: none) for mbw x mbh macroblocks ->
    (t as int8 (mbh, mbw), active, background); EncoderError where it is refused"""
    out, act, bg = np.zeros((int(mbh), int(mbw)), np.int8), C.c_int(-1), C.c_int(-1)
    u = None if user is None else np.ascontiguousarray(user, np.int8).reshape(-1)
    if u is not None and u.size != int(mbw) * int(mbh):
        raise EncoderError("roi_map: the caller's map has %d values for %d macroblocks" % (u.size, int(mbw) * int(mbh)))
    r = load().mi355enc_roi_map(None if cfg is None else C.byref(roi(cfg)), None if u is None else _p(u), int(mbw), int(mbh), _p(out), C.byref(act), C.byref(bg))
    if r:
        raise EncoderError("roi_map: refused (%d)" % r)
    return out, bool(act.value), int(bg.value)


def roi_parse(text, balance=0):
    """mi355enc_roi_parse (host only): the element's string form "x,y,w,h,delta[,feather];..." -> a Roi with that balance; EncoderError where it is refused"""
    c = Roi()
    c.balance = int(balance)
    r = load().mi355enc_roi_parse(text.encode() if isinstance(text, str) else text, C.byref(c))
    if r:
        raise EncoderError("roi_parse: refused (%d)" % r)
    return c


def mask(regions=()):
    """A Mask from regions = [(x, y, w, h, mode, param[, shape[, colour]]), ...] (or a Mask as it is; None: none); nothing is checked here"""
    if isinstance(regions, Mask):
        return regions
    regions = list(regions or ())
    if len(regions) > 8:
        raise EncoderError("mask: more than 8 regions")
    c = Mask()
    c.n = len(regions)
    for k, r in enumerate(regions):
        r = tuple(int(v) for v in r)
        c.region[k] = MaskRegion(*(r + (0,) * (8 - len(r))))
    return c


def mask_check(cfg):
    """mi355enc_mask_check (host only): 0, or the error code for a field outside its range"""
    return load().mi355enc_mask_check(C.byref(mask(cfg)))


def mask_parse(text, colour=0):
    """mi355enc_mask_parse (host only): the element's string form "x,y,w,h,mode,param[,shape];..." -> a Mask whose regions take `colour`; EncoderError where refused"""
    c = Mask()
    r = load().mi355enc_mask_parse(text.encode() if isinstance(text, str) else text, int(colour), C.byref(c))
    if r:
        raise EncoderError("mask_parse: refused (%d)" % r)
    return c


def mask_apply_host(cfg, y, uv, coef):
    """mi355enc_mask_apply_host (host only): the scalar rule on planes of the visible size, y (h, w) and uv (h / 2, w), with the ten words `coef` of
    csc_coefficients -> new (y, uv)"""
    y, uv = np.array(y, np.uint8, order="C"), np.array(uv, np.uint8, order="C")
    h, w = y.shape
    assert uv.shape == (h // 2, w)
    k = np.ascontiguousarray(coef, np.int32)
    r = load().mi355enc_mask_apply_host(C.byref(mask(cfg)), _p(k), w, h, _p(y), _p(uv))
    if r:
        raise EncoderError("mask_apply_host: refused (%d)" % r)
    return y, uv


def mask_ellipse(W2, H2, qx, qy):
    """mi355enc_mask_ellipse (host only): rule 2 for the quad at region-local (qx, qy) of a W2 x H2 region: 1 inside, 0 outside, negative: refused"""
    return load().mi355enc_mask_ellipse(int(W2), int(H2), int(qx), int(qy))


def mask_mean(total, r):
    """mi355enc_mask_mean (host only): rule 6's rounded mean of `total` over 2r + 1 samples, by the reciprocal the kernels use; negative: refused"""
    return load().mi355enc_mask_mean(int(total), int(r))


def mask_colour(colour, coef):
    """mi355enc_mask_colour (host only): rule 4, 0xRRGGBB -> (Y, Cb, Cr) with the ten words of csc_coefficients"""
    out, k = np.zeros(3, np.uint8), np.ascontiguousarray(coef, np.int32)
    r = load().mi355enc_mask_colour(int(colour), _p(k), _p(out))
    if r:
        raise EncoderError("mask_colour: refused (%d)" % r)
    return tuple(int(v) for v in out)


def _lut3d_nodes(nodes):
    """(nodes as a contiguous uint32 array, N); ValueError unless their number is a cube"""
    n = np.ascontiguousarray(nodes, np.uint32).reshape(-1)
    N = int(round(n.size ** (1.0 / 3.0)))
    if N ** 3 != n.size:
        raise ValueError("lut3d: %d nodes are no cube" % n.size)
    return n, N


def lut3d_coefficients(matrix, full_range):
    """mi355enc_lut3d_coefficients (host only): the 19 words -- Minv, Mf, yoff -- of a matrix code (1, 5, 6, 9) and a range"""
    out = (C.c_int32 * 19)()
    r = load().mi355enc_lut3d_coefficients(int(matrix), int(full_range), C.byref(out))
    if r:
        raise EncoderError("lut3d_coefficients: failed (%d)" % r)
    return [int(v) for v in out]


def lut3d_check(nodes, N):
    """mi355enc_lut3d_check (host only): 0, or the error code for N outside 2 .. 65 or a node with a top bit set"""
    return load().mi355enc_lut3d_check(_p(np.ascontiguousarray(nodes, np.uint32)), int(N))


def lut3d_identity(N):
    """mi355enc_lut3d_identity (host only): the identity table of N nodes per axis"""
    if not LUT3D_N_MIN <= N <= LUT3D_N_MAX:
        raise EncoderError("lut3d_identity: N outside %d .. %d" % (LUT3D_N_MIN, LUT3D_N_MAX))
    nodes = np.zeros(N ** 3, np.uint32)
    r = load().mi355enc_lut3d_identity(int(N), _p(nodes))
    if r:
        raise EncoderError("lut3d_identity: failed (%d)" % r)
    return nodes


def parse_cube(text, cap=LUT3D_N_MAX ** 3):
    """mi355enc_lut3d_parse_cube (host only, no locale): a .cube text (str or bytes) -> (nodes, N); EncoderError where the file is refused"""
    data = text.encode("latin-1", "replace") if isinstance(text, str) else bytes(text)
    nodes, N = np.zeros(max(int(cap), 1), np.uint32), C.c_int(0)
    r = load().mi355enc_lut3d_parse_cube(data, len(data), _p(nodes), int(cap), C.byref(N))
    if r:
        raise EncoderError("parse_cube: refused (%d)" % r)
    return nodes[:N.value ** 3].copy(), int(N.value)


def lut3d_apply_host(nodes, strength, matrix, full_range, y, uv, rect=None):
    """mi355enc_lut3d_apply_host (host only): the rule on NV12 planes y (H x W) / uv (H / 2 x W) inside rect (x0, x1, y0, y1; all of it without) -> new (y, uv)"""
    n, N = _lut3d_nodes(nodes)
    y, uv = np.array(y, np.uint8, order="C"), np.array(uv, np.uint8, order="C")
    H, W = y.shape
    assert uv.shape == (H // 2, W)
    r4 = (C.c_int * 4)(*[int(v) for v in (rect if rect is not None else (0, W, 0, H))])
    r = load().mi355enc_lut3d_apply_host(_p(n), N, int(strength), int(matrix), int(full_range), _p(y), _p(uv), W, H, C.byref(r4))
    if r:
        raise EncoderError("lut3d_apply_host: failed (%d)" % r)
    return y, uv


def lut3d_plan(N):
    """mi355enc_lut3d_plan (host only): LUT3D_DIRECT or LUT3D_STAGED, the launch form that serves N"""
    r = load().mi355enc_lut3d_plan(int(N))
    if r < 0:
        raise EncoderError("lut3d_plan: failed (%d)" % r)
    return r


def warp(s=None, **kw):
    """A Warp: bicubic with a black fill (16, 128, 128), then s's (a Warp or a dict) and the keywords' kind / fill on top.  Not checked here."""
    src = s.as_dict() if isinstance(s, Warp) else dict(s or {})
    src.update(kw)
    if set(src) - {"kind", "fill"}:
        raise TypeError("warp: no parameter %r" % (sorted(set(src) - {"kind", "fill"}),))
    return Warp(int(src.get("kind", WARP_BICUBIC)), (C.c_uint8 * 3)(*[int(v) for v in src.get("fill", (16, 128, 128))]))


def warp_params(p=None, **kw):
    """A WarpParams: the neutral values, then p's (a WarpParams or a dict) and the keywords' on top, all Q16 integers.  Not checked here."""
    src = p.as_dict() if isinstance(p, WarpParams) else dict(p or {})
    src.update(kw)
    names = [n for n, _ in WarpParams._fields_]
    if set(src) - set(names):
        raise TypeError("warp_params: no parameter %r" % (sorted(set(src) - set(names)),))
    d = WarpParams()
    load().mi355enc_warp_params_default(C.byref(d))
    for n in names:
        setattr(d, n, int(src.get(n, getattr(d, n))))
    return d


def warp_mesh_size(w, h):
    """mi355enc_warp_mesh_size: (nx, ny) of a w x h picture"""
    nx, ny = C.c_int(0), C.c_int(0)
    r = load().mi355enc_warp_mesh_size(int(w), int(h), C.byref(nx), C.byref(ny))
    if r:
        raise EncoderError("mi355enc_warp_mesh_size(%d, %d): %d" % (w, h, r))
    return int(nx.value), int(ny.value)


def warp_coeff(kind, f):
    """mi355enc_warp_coeff (host only): the four taps of fraction f"""
    c = np.zeros(4, np.int16)
    r = load().mi355enc_warp_coeff(int(kind), int(f), _p(c))
    if r:
        raise EncoderError("mi355enc_warp_coeff(%d, %d): %d" % (kind, f, r))
    return [int(v) for v in c]


def warp_build(w, h, p=None, **kw):
    """mi355enc_warp_build (host only): the mesh of a parameter set for a w x h picture, int32 (ny, nx, 2) holding {sx, sy}; EncoderError where it is refused"""
    nx, ny = warp_mesh_size(w, h)
    mesh = np.zeros((ny, nx, 2), np.int32)
    r = load().mi355enc_warp_build(C.byref(warp_params(p, **kw)), int(w), int(h), _p(mesh), mesh.size)
    if r:
        raise EncoderError("mi355enc_warp_build: %d" % r)
    return mesh


def _mesh(mesh, w, h):
    nx, ny = warp_mesh_size(w, h)
    m = np.ascontiguousarray(mesh, np.int32)
    if m.shape != (ny, nx, 2):
        raise ValueError("a mesh of shape (%d, %d, 2)" % (ny, nx))
    return m, nx, ny


def warp_plan(mesh, w, h):
    """mi355enc_warp_plan (host only): (staged, direct) -- how many of the launch's 32 x 32 tiles take which of the kernel's two forms"""
    m, nx, ny = _mesh(mesh, w, h)
    st, di = C.c_int(0), C.c_int(0)
    r = load().mi355enc_warp_plan(_p(m), nx, ny, int(w), int(h), C.byref(st), C.byref(di))
    if r:
        raise EncoderError("mi355enc_warp_plan: %d" % r)
    return int(st.value), int(di.value)


def warp_apply_host(s, mesh, y, uv):
    """mi355enc_warp_apply_host (host only): NV12 planes of the visible size (h, w) and (h / 2, w) warped through the mesh; returns the new planes"""
    y, uv = np.ascontiguousarray(y, np.uint8), np.ascontiguousarray(uv, np.uint8)
    h, w = y.shape
    if uv.shape != (h // 2, w):
        raise ValueError("NV12 planes of one picture")
    m, _, _ = _mesh(mesh, w, h)
    oy, ouv = np.empty_like(y), np.empty_like(uv)
    r = load().mi355enc_warp_apply_host(C.byref(warp(s)), _p(m), w, h, _p(y), w, _p(uv), w, _p(oy), w, _p(ouv), w)
    if r:
        raise EncoderError("mi355enc_warp_apply_host: %d" % r)
    return oy, ouv


def denoise_check(d=None, **kw):
    """mi355enc_denoise_check (host only): 0, or the error code for a strength outside 0 .. 32"""
    return load().mi355enc_denoise_check(C.byref(denoise(d, **kw)))


def denoise_tables(d=None, **kw):
    """The temporal noise filter's tables (host only): (B, the luma's P, the chroma's P), uint8 (256,) each."""
    st = denoise(d, **kw)
    t = [np.zeros(256, np.uint8) for _ in range(3)]
    r = load().mi355enc_denoise_tables(C.byref(st), *[a.ctypes.data_as(C.c_void_p) for a in t])
    if r:
        raise EncoderError("mi355enc_denoise_tables(%r): %d" % (st.as_dict(), r))
    return tuple(t)


def denoise_motion_key(cost, dx, dy, s):
    """mi355enc_denoise_motion_key (host only): the word the motion search ranks a candidate by; 0xFFFFFFFF for arguments outside its ranges"""
    return int(load().mi355enc_denoise_motion_key(int(cost), int(dx), int(dy), int(s)))


def _denoise_vectors(words):
    """the search's words per block -> (vec (.., 2) int8 as (dx, dy), M uint16)"""
    return np.stack([(words & 255).astype(np.uint8).view(np.int8), ((words >> 8) & 255).astype(np.uint8).view(np.int8)], axis=-1), (words >> 16).astype(np.uint16)


def hdr_tables(transfer, full_range=0, peak_nits=0, target_nits=0, out_matrix=1, out_full=0):
    """The parameter block of the HDR tone map in the device's integer arithmetic (host only; include/mi355enc.h has the layout): int32 (7726,)."""
    L, n = load(), C.c_size_t(0)
    args = [int(v) for v in (transfer, full_range, peak_nits, target_nits, out_matrix, out_full)]
    r = L.mi355enc_hdr_tables(*args, None, 0, C.byref(n))
    if r:
        raise EncoderError("mi355enc_hdr_tables%r: %d" % (tuple(args), r))
    out = np.zeros(n.value, np.int32)
    r = L.mi355enc_hdr_tables(*args, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
    if r:
        raise EncoderError("mi355enc_hdr_tables%r: %d" % (tuple(args), r))
    return out


def csc_coefficients(matrix, full_range):
    """The library's integer RGB -> Y'CbCr matrix (host only): int32 (10,) = yr, yg, yb, br, bg, bb, rr, rg, rb in 2^-16 units and the luma offset."""
    c = np.zeros(10, np.int32)
    r = load().mi355enc_csc_coefficients(int(matrix), int(full_range), c.ctypes.data_as(C.c_void_p))
    if r:
        raise EncoderError("mi355enc_csc_coefficients(%d, %d): %d" % (matrix, full_range, r))
    return c


def host_set_slice_rows(rows):
    """The host stage functions write I pictures as slices of `rows` macroblock rows from now on (0: one slice)."""
    load().mi355enc_host_set_slice_rows(int(rows))


def host_set_p_slices(rows, dbf_idc=0):
    """... and P pictures as slices of `rows` rows (0: one slice); dbf_idc: the disable_deblocking_filter_idc of every slice header (0 or 2)."""
    load().mi355enc_host_set_p_slices(int(rows), int(dbf_idc))


def host_write_slice(mbw, mbh, is_idr, frame_num, idr_pic_id, qp, mbinfo, levels, transform8x8=False):
    L = load()
    out, n = np.empty(mbw * mbh * 1536 + 4096, np.uint8), C.c_size_t(0)
    mbinfo, levels = np.ascontiguousarray(mbinfo), np.ascontiguousarray(levels, np.int16)
    r = L.mi355enc_host_write_slice(mbw, mbh, int(is_idr), frame_num, idr_pic_id, qp, int(transform8x8), mbinfo.ctypes.data_as(C.c_void_p),
                                    levels.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
    if r:
        raise RuntimeError("mi355enc_host_write_slice: %d" % r)
    return bytes(out[: n.value])


def host_write_slice_packed(mbw, mbh, is_idr, frame_num, idr_pic_id, qp, mbinfo, levels, threads=1, transform8x8=False):
    L = load()
    out, n = np.empty(mbw * mbh * 1536 + 4096, np.uint8), C.c_size_t(0)
    mbinfo, levels = np.ascontiguousarray(mbinfo), np.ascontiguousarray(levels, np.int16)
    r = L.mi355enc_host_write_slice_packed(mbw, mbh, int(is_idr), frame_num, idr_pic_id, qp, int(transform8x8), int(threads), mbinfo.ctypes.data_as(C.c_void_p),
                                           levels.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
    if r:
        raise RuntimeError("mi355enc_host_write_slice_packed: %d" % r)
    return bytes(out[: n.value])


def scale_table(n_in, n_out, kind):
    """The library's downscaling table (host only): `kind` one of SCALE_*; n_in / n_out luma samples of the axis.
    -> (first: int32 (n,), the first source index of every entry's taps; coef: int16 (n, taps), 14-bit weights)."""
    L = load()
    taps = C.c_int(0)
    n = L.mi355enc_scale_table(int(n_in), int(n_out), int(kind), None, None, 0, C.byref(taps))
    if n < 0:
        raise EncoderError("mi355enc_scale_table(%d, %d, %d): %s (%d)" % (n_in, n_out, kind, L.mi355enc_strerror(n).decode(), n))
    first, coef = np.zeros(n, np.int32), np.zeros((n, taps.value), np.int16)
    r = L.mi355enc_scale_table(int(n_in), int(n_out), int(kind), _p(first), _p(coef), coef.size, C.byref(taps))
    if r != n:
        raise EncoderError("mi355enc_scale_table: %d" % r)
    return first, coef


def geometry_table(crop_off, crop, dst, kind):
    """scale_table's counterpart with a crop offset and upscaling (host only): `crop` luma samples from luma offset crop_off on -> `dst` luma samples;
    first counts in the whole source plane.  -> (first, coef) as scale_table."""
    L = load()
    taps = C.c_int(0)
    n = L.mi355enc_geometry_table(int(crop_off), int(crop), int(dst), int(kind), None, None, 0, C.byref(taps))
    if n < 0:
        raise EncoderError("mi355enc_geometry_table(%d, %d, %d, %d): %s (%d)" % (crop_off, crop, dst, kind, L.mi355enc_strerror(n).decode(), n))
    first, coef = np.zeros(n, np.int32), np.zeros((n, taps.value), np.int16)
    r = L.mi355enc_geometry_table(int(crop_off), int(crop), int(dst), int(kind), _p(first), _p(coef), coef.size, C.byref(taps))
    if r != n:
        raise EncoderError("mi355enc_geometry_table: %d" % r)
    return first, coef


def fit_rect(src_w, src_h, tw, th):
    """(dx, dy, dw, dh): the largest even rectangle of src_w : src_h inside tw x th, centred at even offsets (host only)"""
    v = [C.c_int(0) for _ in range(4)]
    r = load().mi355enc_fit_rect(int(src_w), int(src_h), int(tw), int(th), *[C.byref(x) for x in v])
    if r:
        raise EncoderError("mi355enc_fit_rect: %d" % r)
    return tuple(x.value for x in v)


def geometry(in_size, crop=None, dst=None, target=None, border=(16, 128, 128), keep_sar=False):
    """A Geometry: in_size (w, h); crop (x, y, w, h), default the whole input; dst (x, y, w, h), default the whole `target` (w, h)"""
    iw, ih = in_size
    cx, cy, cw, ch = crop if crop is not None else (0, 0, iw, ih)
    dx, dy, dw, dh = dst if dst is not None else (0, 0, target[0], target[1])
    return Geometry(int(iw), int(ih), int(cx), int(cy), int(cw), int(ch), int(dx), int(dy), int(dw), int(dh),
                    int(border[0]), int(border[1]), int(border[2]), GEOM_KEEP_SAR if keep_sar else 0)


def geometry_valid(g, tw, th):
    """does Geometry g pass the validity rule against a pre-orientation target of tw x th? (host only)"""
    return load().mi355enc_geometry_check(C.byref(g), int(tw), int(th)) == 0


def geometry_sar(g, transposed=False):
    """(sar_w, sar_h) Geometry g puts into the SPS, None for none (host only)"""
    a, b = C.c_int(0), C.c_int(0)
    r = load().mi355enc_geometry_sar(C.byref(g), int(bool(transposed)), C.byref(a), C.byref(b))
    if r:
        raise EncoderError("mi355enc_geometry_sar: %d" % r)
    return (a.value, b.value) if a.value and b.value else None


def orient_method(m):
    """a method as its number: 0 .. 7, or one of ORIENT_NAMES"""
    return ORIENT_NAMES.index(m) if isinstance(m, str) else int(m)


def orient_size(method, in_w, in_h):
    """(w, h) of a picture of in_w x in_h after orientation (host only)"""
    w, h = C.c_int(0), C.c_int(0)
    r = load().mi355enc_orient_size(orient_method(method), int(in_w), int(in_h), C.byref(w), C.byref(h))
    if r != 0:
        raise EncoderError("mi355enc_orient_size: %d" % r)
    return w.value, h.value


def orient_source(method, out_w, out_h, x, y):
    """(sx, sy): the input sample that output sample (x, y) of an oriented out_w x out_h picture comes from (host only)"""
    sx, sy = C.c_int(0), C.c_int(0)
    r = load().mi355enc_orient_source(orient_method(method), int(out_w), int(out_h), int(x), int(y), C.byref(sx), C.byref(sy))
    if r != 0:
        raise EncoderError("mi355enc_orient_source: %d" % r)
    return sx.value, sy.value


def jpeg_info(data):
    """The header of a JPEG picture (host only): a JpegInfo; EncoderError for a stream the encoder does not take."""
    info = JpegInfo()
    buf = np.frombuffer(bytes(data), np.uint8)
    r = load().mi355enc_jpeg_info(_p(buf) if buf.size else None, buf.size, C.byref(info))
    if r != 0:
        raise EncoderError("mi355enc_jpeg_info: %s (%d)" % (load().mi355enc_strerror(r).decode(), r))
    return info


def jpeg_layout(info):
    """[(blocks per row, block rows)] of each component's MCU-padded plane"""
    mcux, mcuy = -(-info.width // (8 * info.hs)), -(-info.height // (8 * info.vs))
    return [(mcux * (1 if c else info.hs), mcuy * (1 if c else info.vs)) for c in range(info.components)]


def jpeg_entropy_decode(data, coef_cap=None):
    """The host's entropy decode of a JPEG picture (no device): (info, [per component an int16 array (block rows, blocks per row, 8, 8)], uint16 qt[3][8][8]).
    coef_cap: the room offered, in int16 (default: what the picture needs)."""
    info = jpeg_info(data)
    lay = jpeg_layout(info)
    need = sum(bw * bh for bw, bh in lay) * 64
    coef = np.zeros(max(need if coef_cap is None else int(coef_cap), 1), np.int16)
    qt = np.zeros((3, 64), np.uint16)
    buf = np.frombuffer(bytes(data), np.uint8)
    r = load().mi355enc_jpeg_entropy_decode(_p(buf), buf.size, _p(coef), coef.size if coef_cap is None else int(coef_cap), _p(qt), C.byref(info))
    if r != 0:
        raise EncoderError("mi355enc_jpeg_entropy_decode: %s (%d)" % (load().mi355enc_strerror(r).decode(), r))
    out, o = [], 0
    for bw, bh in lay:
        out.append(coef[o:o + bw * bh * 64].reshape(bh, bw, 8, 8))
        o += bw * bh * 64
    return info, out, qt.reshape(3, 8, 8)


def snapshot_size(w, h, reduce=1):
    """(ow, oh) of a still of a w x h picture"""
    return -(-w // reduce), -(-h // reduce)


def snapshot_layout(ow, oh):
    """[(blocks per row, block rows)] of Y, Cb, Cr of a still of ow x oh: the layout jpeg_entropy_decode returns for a 4:2:0 picture of that size"""
    mcux, mcuy = -(-ow // 16), -(-oh // 16)
    return [(2 * mcux, 2 * mcuy), (mcux, mcuy), (mcux, mcuy)]


def _snapshot_split(flat, ow, oh):
    out, o = [], 0
    for bw, bh in snapshot_layout(ow, oh):
        out.append(flat[o:o + bw * bh * 64].reshape(bh, bw, 8, 8))
        o += bw * bh * 64
    return out


def snapshot_tables(quality):
    """The two quantisation tables of a quality (host only): uint16 (2, 64), natural order."""
    qt = np.zeros((2, 64), np.uint16)
    r = load().mi355enc_snapshot_tables(int(quality), _p(qt))
    if r != 0:
        raise EncoderError("mi355enc_snapshot_tables: %s (%d)" % (load().mi355enc_strerror(r).decode(), r))
    return qt


def snapshot_reciprocal(q):
    """The multiplier the device divides by 8 q with (host only)."""
    return int(load().mi355enc_snapshot_reciprocal(int(q)))


def snapshot_max_bytes(ow, oh):
    return int(load().mi355enc_snapshot_max_bytes(int(ow), int(oh)))


def snapshot_write(levels, qt, ow, oh, cap=None, want_len=False):
    """The file of a still from its levels (host only): levels a list of per-component int16 arrays (block rows, blocks per row, 8, 8) or one flat array,
    qt uint16 (2, 64).  cap: the room offered (default: snapshot_max_bytes).  want_len: (return code, length) instead of the bytes."""
    flat = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int16).ravel() for c in levels]) if isinstance(levels, (list, tuple)) else levels, np.int16)
    q = np.ascontiguousarray(np.asarray(qt, np.uint16).reshape(2, 64))
    cap = snapshot_max_bytes(ow, oh) if cap is None else int(cap)
    out, n = np.empty(max(cap, 1), np.uint8), C.c_size_t(0)
    r = load().mi355enc_snapshot_write(_p(flat), _p(q), int(ow), int(oh), _p(out), cap, C.byref(n))
    if want_len:
        return r, int(n.value)
    if r != 0:
        raise EncoderError("mi355enc_snapshot_write: %s (%d)" % (load().mi355enc_strerror(r).decode(), r))
    return bytes(out[:n.value])


def overlay_style(**kw):
    """The library's default style (right, top, pads 16, auto scale, no shading) with the given fields replaced."""
    st = OverlayStyle()
    load().mi355enc_overlay_default_style(C.byref(st))
    for k, v in kw.items():
        if k not in dict(OverlayStyle._fields_):
            raise TypeError("no such overlay style field: %s" % k)
        setattr(st, k, int(v))
    return st


def overlay_glyph(ch):
    """The built-in font (host only): the 16 rows of the 8 x 16 cell of character code `ch`, MSB = left pixel."""
    rows = np.zeros(16, np.uint8)
    r = load().mi355enc_overlay_glyph(int(ch), rows.ctypes.data_as(C.c_void_p))
    if r:
        raise EncoderError("mi355enc_overlay_glyph(%d): %d" % (ch, r))
    return rows


def image_layer(pixels, x=0, y=0, opacity=256, fmt=FMT_RGBX):
    """An ImageLayer for pixels (h, w, 4) uint8 in byte order fmt; None: a layer without an image (off).  The array it points into is kept alive as `.keep`."""
    im = ImageLayer()
    im.fmt, im.x, im.y, im.opacity = int(fmt), int(x), int(y), int(opacity)
    if pixels is not None:
        a = np.asarray(pixels)
        if not (a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 4 and a.strides[2] == 1 and a.strides[1] == 4 and a.strides[0] >= 4 * a.shape[1]):
            a = np.ascontiguousarray(a, np.uint8)
        assert a.ndim == 3 and a.shape[2] == 4, "pixels: (h, w, 4)"
        im.keep = a
        im.pixels, im.w, im.h, im.stride = a.ctypes.data, a.shape[1], a.shape[0], a.strides[0]
    return im


def image_pixel(matrix, full_range, r, g, b):
    """(Y', Cb, Cr) of one colour as the image layers use it (host only)"""
    out = np.zeros(3, np.uint8)
    rc = load().mi355enc_image_pixel(int(matrix), int(full_range), int(r), int(g), int(b), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise EncoderError("mi355enc_image_pixel: %s (%d)" % (load().mi355enc_strerror(rc).decode(), rc))
    return int(out[0]), int(out[1]), int(out[2])


def load_pam(data, size_only=False):
    """A Netpbm PAM (P7) file as bytes -> RGBA pixels (h, w, 4) uint8, or (w, h) with size_only (host only)"""
    buf = np.frombuffer(bytes(data), np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    L = load()
    rc = L.mi355enc_image_load_pam(_p(buf) if buf.size else None, buf.size, C.byref(w), C.byref(h), None, 0)
    if rc:
        raise EncoderError("mi355enc_image_load_pam: %s (%d)" % (L.mi355enc_strerror(rc).decode(), rc))
    if size_only:
        return w.value, h.value
    out = np.empty((h.value, w.value, 4), np.uint8)
    rc = L.mi355enc_image_load_pam(_p(buf), buf.size, C.byref(w), C.byref(h), _p(out), out.nbytes)
    if rc:
        raise EncoderError("mi355enc_image_load_pam: %s (%d)" % (L.mi355enc_strerror(rc).decode(), rc))
    return out


def _text_bytes(text):
    return text.encode("latin-1") if isinstance(text, str) else (bytes(text) if text is not None else None)


def rate_check(mode, pts_per_second, max_fill):
    """mi355enc_rate_check: True when mi355enc_set_rate_conversion would take the three values (host only)"""
    return load().mi355enc_rate_check(C.byref(Rate(int(mode), int(pts_per_second), int(max_fill)))) == 0


class RatePlan:
    """The rule of the frame-rate conversion by itself (host logic; no device): which output pictures an input's pts yields."""

    def __init__(self, mode, pts_per_second, fps_num, fps_den=1, max_fill=2, t0=0, k_next=-1):
        self.L = load()
        self.st = RatePlanState()
        self.L.mi355enc_rate_plan_init(C.byref(self.st), int(mode), int(pts_per_second), int(fps_num), int(fps_den), int(max_fill), int(t0), int(k_next))

    def step(self, pts):
        """-> (out_pts list, weights list, resync): one entry per picture the input yields (hold: weight 0 a repeat, 256 the input)"""
        n, rs = C.c_int(0), C.c_int(0)
        t, w = (C.c_int64 * RATE_MAX_OUT)(), (C.c_int * RATE_MAX_OUT)()
        r = self.L.mi355enc_rate_plan_step(C.byref(self.st), int(pts), C.byref(n), t, w, C.byref(rs))
        if r:
            raise EncoderError("mi355enc_rate_plan_step: %d" % r)
        return [int(t[i]) for i in range(n.value)], [int(w[i]) for i in range(n.value)], bool(rs.value)


RC_BYTES = 512  # include/mi355enc.h MI355ENC_RC_BYTES


class RateControl:
    """The encoder's rate-control model by itself (host logic; no device)."""

    def __init__(self, fps, gop, bps, qp_min=10, qp_max=51):
        self.L = load()
        self.buf = (C.c_uint8 * RC_BYTES)()
        self.L.mi355enc_rc_init(self.buf, float(fps), gop, bps, qp_min, qp_max)

    def set_bitrate(self, bps):
        self.L.mi355enc_rc_set_bitrate(self.buf, int(bps))

    def pick(self, is_idr):
        """-> (qp, drop): drop 0 .. DROP_MAX is the ladder below QP 51, DROP_SKIP an all-skip picture"""
        qp, drop = C.c_int(0), C.c_int(0)
        self.L.mi355enc_rc_pick(self.buf, int(is_idr), C.byref(qp), C.byref(drop))
        return qp.value, drop.value

    def update(self, is_idr, qp, drop, nbytes):
        self.L.mi355enc_rc_update(self.buf, int(is_idr), qp, drop, nbytes)


class PinnedBuffer:
    """nbytes of pinned host memory from mi355enc_host_alloc(), viewed as a numpy uint8 array (`.array`); pictures submitted from it
    are DMA'd in place."""

    def __init__(self, nbytes):
        self.L = load()
        self.ptr = self.L.mi355enc_host_alloc(nbytes)
        if not self.ptr:
            raise EncoderError("mi355enc_host_alloc(%d) failed" % nbytes)
        self.array = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(self.ptr))

    def free(self):
        if getattr(self, "ptr", None):
            self.array = None
            self.L.mi355enc_host_free(self.ptr)
            self.ptr = None

    __del__ = free


class EncoderError(RuntimeError):
    pass


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _rows(a):
    """A picture plane as the library takes it.  A uint8 array of rows of adjacent samples is taken where it lies, at the
    row stride it has (a view into a wider or taller array, a plane inside a PinnedBuffer); anything else is made
    contiguous first."""
    if isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 2 and a.strides[-1] == 1 and a.strides[0] >= a.shape[1]:
        return a
    return np.ascontiguousarray(a, np.uint8)


class Encoder:
    """One H.264 stream on one GPU.  Arguments mirror the element's properties
    (bitrate in bits/s as written through `bps`, key-int-max -> gop)."""

    def __init__(self, width, height, fps=60, gop=60, bitrate_bps=6_000_000, device_id=0, fixed_qp=-1, me_range=16,
                 pipeline_depth=0, profile_events=False, use_graphs=True, keep_prefilter=False, fps_den=1, deblock_mode=0, subpel=True, i4x4=True, transform8x8=False, intra_in_p=True, cavlc_threads=0, intra_mode=0, scenecut=True, exclusive=False, aq=False, single_stream=False, intra_slices=0, profile_overlap=False, partitions=False, i8x8=False, slices="mirror", slice_deblock="mirror", intra_refresh=False, input_size=None, colorimetry=None, orientation=None, geometry=None, input_colorimetry=None, rate=None, hdr_input=None, adjust=None, denoise=None, stabilize=None, autolevel=None, denoise_spatial=None):
        self.L = load()
        cfg = Cfg()
        self.L.mi355enc_default_cfg(C.byref(cfg), width, height, fps, fps_den)
        cfg.gop, cfg.bitrate_bps, cfg.device_id, cfg.fixed_qp, cfg.me_range = gop, bitrate_bps, device_id, fixed_qp, me_range
        cfg.pipeline_depth, cfg.profile_events, cfg.use_graphs, cfg.keep_prefilter = (
            pipeline_depth, int(profile_events), int(use_graphs), int(keep_prefilter))
        cfg.deblock_mode = deblock_mode
        cfg.intra_in_p = int(intra_in_p)  # True / 1: Intra_16x16 (the default); 2: Intra_4x4 as well
        cfg.cavlc_threads = int(cavlc_threads)
        cfg.scenecut = int(scenecut)
        cfg.exclusive_device = int(exclusive)  # this encoder has the GPU to itself: kernels may wait on the device for each other (include/mi355enc.h)
        cfg.intra_mode = int(intra_mode)
        cfg.aq_mode = int(aq)
        cfg.single_stream = int(single_stream)
        cfg.profile_overlap = int(profile_overlap)  # sampled P pictures keep the free-running schedule (timers include device-side waits)
        cfg.i8x8 = int(i8x8)  # with transform8x8: Intra_8x8 macroblocks in I pictures (intra_mode 0)
        cfg.partitions = int(partitions)  # P macroblocks may be split into 16x8 / 8x16 / 8x8 partitions
        cfg.intra_slices = int(intra_slices)  # 0: about 17 macroblock rows per slice (1080p: 4 slices per I picture)
        # slices / slice_deblock: this mirror defaults to the one-slice P pictures and the filter across slice boundaries of rounds 1-3 (what the stage-by-stage parity
        # suite was written against); None = the library's own default (mi355enc_default_cfg: P pictures sliced like I pictures, slice-local deblocking)
        # (dev tools: MI355ENC_MIRROR_DEFAULTS=library makes the mirror's default the library's)
        lib_defaults = os.environ.get("MI355ENC_MIRROR_DEFAULTS") == "library"
        if isinstance(slices, str):
            slices = None if lib_defaults else 1
        if isinstance(slice_deblock, str):
            slice_deblock = None if lib_defaults else False
        if slices is not None:
            cfg.slices = int(slices)  # slices per P picture (0: automatic, 1: one)
        if slice_deblock is not None:
            cfg.slice_deblock = int(slice_deblock)  # the deblocking filter stops at slice boundaries (disable_deblocking_filter_idc 2)
        cfg.subpel = int(subpel)
        cfg.i4x4 = int(i4x4)
        cfg.transform8x8 = int(transform8x8)  # 0 / False: Constrained Baseline; 1 / True: High, 8x8 transform for every coded inter macroblock; 2: High, 4x4 or 8x8 per macroblock
        self.h = C.c_void_p()
        self._chk(self.L.mi355enc_open(C.byref(cfg), C.byref(self.h)), "open", close_on_fail=True)
        self.width, self.height = width, height
        self.mbw, self.mbh = self.L.mi355enc_mb_width(self.h), self.L.mi355enc_mb_height(self.h)
        self._out = np.empty(self.L.mi355enc_max_au_bytes(self.h), np.uint8)
        if intra_refresh:  # periodic intra refresh instead of periodic IDR pictures (refresh period: gop)
            self._chk(self.L.mi355enc_set_intra_refresh(self.h, 1), "set_intra_refresh", close_on_fail=True)
        if colorimetry is not None:  # (full_range, primaries, transfer, matrix): the VUI of every SPS, and the matrix RGB input is converted with
            self._chk(self.L.mi355enc_set_colorimetry(self.h, *[int(v) for v in colorimetry]), "set_colorimetry", close_on_fail=True)
        if input_colorimetry is not None:  # (full_range, matrix): what submitted YUV samples mean; converted on the device to `colorimetry` where the two differ
            self._chk(self.L.mi355enc_set_input_colorimetry(self.h, *[int(v) for v in input_colorimetry]), "set_input_colorimetry", close_on_fail=True)
        if hdr_input is not None:  # (transfer, full_range, peak_nits, target_nits): the 10-bit pictures submitted are PQ / HLG BT.2020 and are tone-mapped on the device to SDR in `colorimetry`
            self._chk(self.L.mi355enc_set_hdr_input(self.h, *[int(v) for v in hdr_input]), "set_hdr_input", close_on_fail=True)
        if adjust is not None:  # a dict of picture controls (brightness=..., sharpen=...): applied on the device to every picture from the first one on
            try:
                self.set_adjust(adjust)
            except EncoderError:
                self.close()
                raise
        if denoise is not None:  # dict(luma=, chroma=, motion=): the temporal noise filter's strengths and its search range (default 0: no motion compensation), from the first picture on
            try:
                denoise = denoise.as_dict() if isinstance(denoise, Denoise) else dict(denoise)
                self.set_denoise_motion(denoise.pop("motion", 0))
                self.set_denoise(denoise)
            except EncoderError:
                self.close()
                raise
        if stabilize is not None:  # dict(range=, leak=, margin=) or a Stabilize: the crop of `geometry` follows the camera's shake from the first picture on
            try:
                self.set_stabilize(stabilize)
            except EncoderError:
                self.close()
                raise
        if autolevel is not None:  # dict(levels=, balance=, ...) or an Autolevel: automatic levels and white balance from the first picture on
            try:
                self.set_autolevel(autolevel)
            except EncoderError:
                self.close()
                raise
        if denoise_spatial is not None:  # dict(luma=, chroma=, auto_gain=, ...) or a DenoiseSpatial: the spatial noise filter from the first picture on
            try:
                self.set_denoise_spatial(denoise_spatial)
            except EncoderError:
                self.close()
                raise
        self.rate_on = False
        if rate is not None:  # (mode, pts_per_second, max_fill): frame-rate conversion to fps / fps_den; every submit*() then returns the pictures it enqueued
            self._chk(self.L.mi355enc_set_rate_conversion(self.h, C.byref(Rate(*[int(v) for v in rate]))), "set_rate_conversion", close_on_fail=True)
            self.rate_on = int(rate[0]) != 0
        self.input_size = (width, height)
        self.orientation, self._in_set = ORIENT_IDENTITY, False
        if orientation is not None:  # 0 .. 7 or a name of ORIENT_NAMES: the pictures submitted are turned / mirrored on the device; width x height is the oriented size
            try:
                self.set_orientation(orientation)
            except EncoderError:
                self.close()
                raise
        if input_size is not None:  # (w, h) of the submitted pictures: scaled down on the device to width x height
            self._chk(self.L.mi355enc_set_input_size(self.h, int(input_size[0]), int(input_size[1])), "set_input_size", close_on_fail=True)
            self.input_size, self._in_set = (int(input_size[0]), int(input_size[1])), True
        if geometry is not None:  # a Geometry (geometry()): crop -> destination rectangle of the pre-orientation target, border around it
            try:
                self.set_input_geometry(geometry)
            except EncoderError:
                self.close()
                raise

    def _chk(self, r, what, close_on_fail=False):
        if r != 0:
            msg = self.L.mi355enc_strerror(r).decode()
            if close_on_fail and self.h:
                self.L.mi355enc_close(self.h)
                self.h = None
            raise EncoderError("mi355enc_%s: %s (%d)" % (what, msg, r))

    def close(self):
        if getattr(self, "h", None):
            self.L.mi355enc_close(self.h)
            self.h = None

    __del__ = close

    def set_bitrate(self, bps):
        self._chk(self.L.mi355enc_set_bitrate(self.h, int(bps)), "set_bitrate")

    def set_fixed_qp(self, qp):
        self._chk(self.L.mi355enc_set_fixed_qp(self.h, int(qp)), "set_fixed_qp")

    def set_fixed_drop(self, drop):
        self._chk(self.L.mi355enc_set_fixed_drop(self.h, int(drop)), "set_fixed_drop")

    def set_intra_refresh(self, on):
        self._chk(self.L.mi355enc_set_intra_refresh(self.h, int(bool(on))), "set_intra_refresh")

    def set_colorimetry(self, full_range, primaries, transfer, matrix):
        """H.264 Table E-3 / E-4 / E-5 code points for the VUI of every SPS from now on (before the first submit); RGB input is converted with them"""
        self._chk(self.L.mi355enc_set_colorimetry(self.h, int(full_range), int(primaries), int(transfer), int(matrix)), "set_colorimetry")

    def set_input_colorimetry(self, full_range, matrix):
        """what the submitted YUV samples mean (before the first submit): converted on the device to set_colorimetry's range and matrix where they differ"""
        self._chk(self.L.mi355enc_set_input_colorimetry(self.h, int(full_range), int(matrix)), "set_input_colorimetry")

    def set_hdr_input(self, transfer, full_range=0, peak_nits=0, target_nits=0):
        """the submitted 10-bit pictures (FMT_P010, FMT_I420_10, FMT_V210) are HDR (transfer HDR_PQ / HDR_HLG, BT.2020): tone-mapped to SDR BT.709 in their conversion
        launch (before the first submit; not beside set_input_colorimetry); every other input is refused from then on"""
        self._chk(self.L.mi355enc_set_hdr_input(self.h, int(transfer), int(full_range), int(peak_nits), int(target_nits)), "set_hdr_input")

    def set_adjust(self, a=None, **kw):
        """picture controls from the next submitted picture on (any time, any thread): brightness, contrast, saturation, hue, gamma in thousandths, sharpen in
        sixteenths, sharpen_threshold; unnamed ones are neutral, none at all (or all neutral) switches the step off"""
        self._chk(self.L.mi355enc_set_adjust(self.h, C.byref(adjust(a, **kw))), "set_adjust")

    def get_adjust(self):
        st = Adjust()
        self._chk(self.L.mi355enc_get_adjust(self.h, C.byref(st)), "get_adjust")
        return st.as_dict()

    def last_adjust(self):
        """the picture controls the last collected picture was submitted under (a dict); EncoderError before the first collect"""
        st = Adjust()
        self._chk(self.L.mi355enc_last_adjust(self.h, C.byref(st)), "last_adjust")
        return st.as_dict()

    def stage_adjust(self, a, y, uv):
        """The picture controls alone on host planes of the coded size, with the handle's geometry, orientation and output range; returns the adjusted copies."""
        y, uv = np.ascontiguousarray(y, np.uint8).copy(), np.ascontiguousarray(uv, np.uint8).copy()
        assert y.shape == (self.mbh * 16, self.mbw * 16) and uv.shape == (self.mbh * 8, self.mbw * 16)
        self._chk(self.L.mi355enc_stage_adjust(self.h, C.byref(adjust(a)), _p(y), _p(uv)), "stage_adjust")
        return y, uv

    def debug_adjust_bytes(self):
        return int(self.L.mi355enc_debug_adjust_bytes(self.h))

    def set_denoise(self, d=None, **kw):
        """the temporal noise filter from the next submitted picture on (any time, any thread): luma, chroma = 0 .. 32 codes; none (or both 0) switches it off"""
        self._chk(self.L.mi355enc_set_denoise(self.h, C.byref(denoise(d, **kw))), "set_denoise")

    def get_denoise(self):
        st = Denoise()
        self._chk(self.L.mi355enc_get_denoise(self.h, C.byref(st)), "get_denoise")
        return st.as_dict()

    def last_denoise(self):
        """the strengths the last collected picture was submitted under (a dict); EncoderError before the first collect"""
        st = Denoise()
        self._chk(self.L.mi355enc_last_denoise(self.h, C.byref(st)), "last_denoise")
        return st.as_dict()

    def stage_denoise(self, d, y, uv, hist_y=None, hist_uv=None):
        """The temporal noise filter alone on host planes of the coded size and their histories (uint16, the planes' shapes; None: that plane primes), with the
        handle's visible size.  Returns (y, uv, hist_y, hist_uv): the filtered copies and the new histories (None for a plane that keeps none)."""
        st = denoise(d)
        y, uv = np.ascontiguousarray(y, np.uint8).copy(), np.ascontiguousarray(uv, np.uint8).copy()
        assert y.shape == (self.mbh * 16, self.mbw * 16) and uv.shape == (self.mbh * 8, self.mbw * 16)
        hin = [None if a is None else np.ascontiguousarray(a, np.uint16) for a in (hist_y, hist_uv)]
        assert all(a is None or a.shape == p.shape for a, p in zip(hin, (y, uv)))
        hy = np.zeros(y.shape, np.uint16) if st.luma or st.chroma else None
        huv = np.zeros(uv.shape, np.uint16) if st.chroma else None
        ptr = lambda a: None if a is None else _p(a)
        self._chk(self.L.mi355enc_stage_denoise(self.h, C.byref(st), ptr(hin[0]), ptr(hin[1]), _p(y), _p(uv), ptr(hy), ptr(huv)), "stage_denoise")
        return y, uv, hy, huv

    def set_autolevel(self, a=None, **kw):
        """Automatic levels and white balance from the next picture submitted on (any time, any thread, no GPU call); None or both strengths 0: off."""
        self._chk(self.L.mi355enc_set_autolevel(self.h, C.byref(autolevel(a, **kw))), "set_autolevel")

    def get_autolevel(self):
        st = Autolevel()
        self._chk(self.L.mi355enc_get_autolevel(self.h, C.byref(st)), "get_autolevel")
        return st.as_dict()

    def last_autolevel(self):
        """(the setting, the record, the table) of the last collected picture; zeros for a picture the step did not run on"""
        st, info, table = Autolevel(), AutolevelInfo(), np.zeros(256, np.uint8)
        self._chk(self.L.mi355enc_last_autolevel(self.h, C.byref(st), C.byref(info), _p(table)), "last_autolevel")
        return st.as_dict(), info.as_dict(), table

    def debug_autolevel_bytes(self):
        return int(self.L.mi355enc_debug_autolevel_bytes(self.h))

    def stage_autolevel(self, a, y, uv):
        """The three launches alone on host planes of the coded size, primed by that picture -> (y, uv, record, table)."""
        y, uv = np.array(y, np.uint8, order="C"), np.array(uv, np.uint8, order="C")
        assert y.shape == (16 * self.mbh, 16 * self.mbw) and uv.shape == (8 * self.mbh, 16 * self.mbw)
        info, table = AutolevelInfo(), np.zeros(256, np.uint8)
        self._chk(self.L.mi355enc_autolevel_probe_stage(self.h, C.byref(autolevel(a)), _p(y), _p(uv), C.byref(info), _p(table)), "stage_autolevel")
        return y, uv, info.as_dict(), table

    def autolevel_probe_measure(self, y, uv, rect, visible, full_range=0, reach=48):
        """The measure launch alone: NV12 surfaces y (H x W) / uv (H / 2 x W), rect (x0, x1, y0, y1), visible (w, h) -> dict(hist, voters, chroma, su, sv)"""
        y, uv = np.ascontiguousarray(y, np.uint8), np.ascontiguousarray(uv, np.uint8)
        H, W = y.shape
        assert uv.shape == (H // 2, W)
        m = AutolevelMeas()
        self._chk(self.L.mi355enc_autolevel_probe_measure(self.h, _p(y), _p(uv), W, H, C.byref((C.c_int * 4)(*[int(v) for v in rect])), int(visible[0]), int(visible[1]),
                                                          int(full_range), int(reach), C.byref(m)), "autolevel_probe_measure")
        return m.as_dict()

    def autolevel_probe_decide(self, m, a, full_range=0, state=None, prime=False):
        """The decide launch alone: autolevel_decide's arguments and answer"""
        def fn(*args):
            return self.L.mi355enc_autolevel_probe_decide(self.h, *args)
        return _autolevel_decide(fn, "autolevel_probe_decide", m, a, full_range, state, prime)

    def set_stabilize(self, s=None, **kw):
        """electronic image stabilisation from the next submitted picture on (None: off); callable at any time from any thread"""
        self._chk(self.L.mi355enc_set_stabilize(self.h, C.byref(stabilize(s, **kw))), "set_stabilize")

    def get_stabilize(self):
        st = Stabilize()
        self._chk(self.L.mi355enc_get_stabilize(self.h, C.byref(st)), "get_stabilize")
        return st.as_dict()

    def last_stabilize(self):
        """(setting, record) of the last collected picture, as dicts; an unstabilised picture's record is zeros"""
        st, info = Stabilize(), StabilizeInfo()
        self._chk(self.L.mi355enc_last_stabilize(self.h, C.byref(st), C.byref(info)), "last_stabilize")
        return st.as_dict(), info.as_dict()

    def debug_stabilize_bytes(self):
        return int(self.L.mi355enc_debug_stabilize_bytes(self.h))

    def stabilize_probe_project(self, luma):
        """the projection launch alone on a host luma plane (a 2-D uint8 view, samples 1 or 2 bytes apart, any address and row stride) -> (C (4, w), R (4, h))"""
        step = int(luma.strides[1])
        addr, stride, w, h = _luma_view(luma, step)
        sums = np.zeros(4 * (w + h), np.uint32)
        self._chk(self.L.mi355enc_stabilize_probe_project(self.h, addr, stride, step, w, h, _p(sums)), "stabilize_probe_project")
        return sums[:4 * w].reshape(4, w), sums[4 * w:].reshape(4, h)

    def stabilize_probe_match(self, prev, cur, s, bounds, state=(0, 0), prime=False):
        """the match launch alone: prev, cur = (C (4, w), R (4, h)) of the previous and the current picture, s the setting, bounds (lo_x, hi_x, lo_y, hi_y),
        state (Sx, Sy) going in -> the record as a dict"""
        w, h = int(cur[0].shape[1]), int(cur[1].shape[1])
        flat = [np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint32).ravel(), np.asarray(r, np.uint32).ravel()])) for c, r in (prev, cur)]
        if flat[0].size != 4 * (w + h) or flat[1].size != 4 * (w + h):
            raise ValueError("sums of one size")
        info = StabilizeInfo()
        self._chk(self.L.mi355enc_stabilize_probe_match(self.h, _p(flat[0]), _p(flat[1]), w, h, C.byref(stabilize(s)), C.byref((C.c_int * 4)(*[int(v) for v in bounds])),
                                                        C.byref((C.c_int * 2)(*[int(v) for v in state])), int(bool(prime)), C.byref(info)), "stabilize_probe_match")
        return info.as_dict()

    def set_warp(self, s=None, p=None, **kw):
        """lens, roll and keystone correction from the next submitted picture on (any time, any thread): s the filter and fill (a Warp or a dict; None: off), p and
        the keywords the Q16 parameters of warp_params()"""
        if s is None and p is None and not kw:
            self._chk(self.L.mi355enc_set_warp(self.h, None, None), "set_warp")
        else:
            self._chk(self.L.mi355enc_set_warp(self.h, C.byref(warp(s)), C.byref(warp_params(p, **kw))), "set_warp")

    def set_denoise_spatial(self, a=None, **kw):
        """mi355enc_set_denoise_spatial: from the next picture submitted on; nothing that filters or measures (or no argument): off"""
        self._chk(self.L.mi355enc_set_denoise_spatial(self.h, C.byref(denoise_spatial(a, **kw))), "set_denoise_spatial")

    def get_denoise_spatial(self):
        st = DenoiseSpatial()
        self._chk(self.L.mi355enc_get_denoise_spatial(self.h, C.byref(st)), "get_denoise_spatial")
        return st.as_dict()

    def last_denoise_spatial(self):
        """-> (setting, record) of the last collected picture"""
        st, info = DenoiseSpatial(), DenoiseSpatialInfo()
        self._chk(self.L.mi355enc_last_denoise_spatial(self.h, C.byref(st), C.byref(info)), "last_denoise_spatial")
        return st.as_dict(), info.as_dict()

    def debug_denoise_spatial_bytes(self):
        return int(self.L.mi355enc_debug_denoise_spatial_bytes(self.h))

    def stage_denoise_spatial(self, a, y, uv):
        """The step alone on host planes of the coded size (an automatic setting is primed by the picture) -> (y', uv', record)"""
        y, uv = np.ascontiguousarray(y, np.uint8).copy(), np.ascontiguousarray(uv, np.uint8).copy()
        info = DenoiseSpatialInfo()
        self._chk(self.L.mi355enc_denoise_spatial_probe_stage(self.h, C.byref(denoise_spatial(a)), _p(y), _p(uv), C.byref(info)), "stage_denoise_spatial")
        return y, uv, info.as_dict()

    def denoise_spatial_probe_measure(self, y, rect=None, visible=None, full_range=0):
        """The measure launch alone on a host luma surface -> dict(hist=, candidates=, voters=)"""
        y, m = np.ascontiguousarray(y, np.uint8), DenoiseSpatialMeas()
        self._chk(self.L.mi355enc_denoise_spatial_probe_measure(self.h, _p(y), *_surface_args(y, rect, visible), int(full_range), C.byref(m)), "denoise_spatial_probe_measure")
        return m.as_dict()

    def denoise_spatial_probe_decide(self, m, a, x=None, prime=False):
        """The decide launch alone: denoise_spatial_decide's arguments and answer"""
        def fn(*args):
            return self.L.mi355enc_denoise_spatial_probe_decide(self.h, *args)
        return _denoise_spatial_decide(fn, "denoise_spatial_probe_decide", m, a, x, prime)

    def set_lut3d(self, nodes_or_cube_text=None, strength=256):
        """A 3D colour LUT from the next picture submitted on (any time, any thread, no GPU call): N^3 packed nodes, or the text of a .cube file (str or
        bytes), with a strength 0 .. 256; None: off.  The size may change while the stream runs; pictures in flight keep the table they were submitted with."""
        if nodes_or_cube_text is None:
            self._chk(self.L.mi355enc_set_lut3d(self.h, None, None), "set_lut3d")
            return
        if isinstance(nodes_or_cube_text, (str, bytes)):
            n, N = parse_cube(nodes_or_cube_text)
        else:
            n, N = _lut3d_nodes(nodes_or_cube_text)
        self._chk(self.L.mi355enc_set_lut3d(self.h, C.byref(Lut3d(N, int(strength))), _p(n)), "set_lut3d")

    def get_lut3d(self):
        """the setting set last as a dict(size=, strength=), None when off"""
        on, st = C.c_int(0), Lut3d()
        self._chk(self.L.mi355enc_get_lut3d(self.h, C.byref(on), C.byref(st)), "get_lut3d")
        return st.as_dict() if on.value else None

    def last_lut3d(self):
        """(the setting, the generation of the table) the last collected picture was graded with; zeros for an ungraded one"""
        st, g = Lut3d(), C.c_uint(0)
        self._chk(self.L.mi355enc_last_lut3d(self.h, C.byref(st), C.byref(g)), "last_lut3d")
        return st.as_dict(), int(g.value)

    def debug_lut3d_bytes(self):
        return int(self.L.mi355enc_debug_lut3d_bytes(self.h))

    def debug_lut3d_form(self, form):
        """measurements: the launch form of the handle's own LUT launches -- -1 the plan's, LUT3D_DIRECT, LUT3D_STAGED (the picture is the same)"""
        self._chk(self.L.mi355enc_debug_lut3d_form(self.h, int(form)), "debug_lut3d_form")

    def lut3d_probe(self, nodes, y, uv, strength=256, form=-1):
        """The LUT launch alone on host planes of the coded size; form -1: the plan's, LUT3D_DIRECT / LUT3D_STAGED: that one.  Returns the graded copies."""
        n, N = _lut3d_nodes(nodes)
        y, uv = np.ascontiguousarray(y, np.uint8).copy(), np.ascontiguousarray(uv, np.uint8).copy()
        assert y.shape == (self.mbh * 16, self.mbw * 16) and uv.shape == (self.mbh * 8, self.mbw * 16)
        self._chk(self.L.mi355enc_lut3d_probe(self.h, C.byref(Lut3d(N, int(strength))), _p(n), _p(y), _p(uv), int(form)), "lut3d_probe")
        return y, uv

    def set_roi(self, cfg=None, user_map=None):
        """Region-of-interest quantisation from the next picture submitted on (any time, any thread, no GPU call): a roi() / Roi / dict of rectangles and
        balance, and / or the caller's own int8 map of one offset -12 .. +12 per macroblock; both None: off.  Pictures in flight keep their map."""
        u = None if user_map is None else np.ascontiguousarray(user_map, np.int8).reshape(-1)
        if u is not None and u.size != self.mbw * self.mbh:
            raise EncoderError("set_roi: the map has %d values for %d macroblocks" % (u.size, self.mbw * self.mbh))
        self._chk(self.L.mi355enc_set_roi(self.h, None if cfg is None else C.byref(roi(cfg)), None if u is None else _p(u)), "set_roi")

    def get_roi(self):
        """the configuration set last as a dict(rects=, balance=), None when off"""
        on, c = C.c_int(0), Roi()
        self._chk(self.L.mi355enc_get_roi(self.h, C.byref(on), C.byref(c)), "get_roi")
        return c.as_dict() if on.value else None

    def last_roi(self):
        """(active, background, sum) of the last collected picture's map; (False, 0, 0) for a picture without"""
        a, b, s = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.mi355enc_last_roi(self.h, C.byref(a), C.byref(b), C.byref(s)), "last_roi")
        return bool(a.value), int(b.value), int(s.value)

    def debug_roi_bytes(self):
        return int(self.L.mi355enc_debug_roi_bytes(self.h))

    def roi_probe_set_map(self, t=None):
        """The single-stage entry points quantise with this int8 map of one offset per macroblock from now on (None: one QP per picture again); no device work"""
        u = None if t is None else np.ascontiguousarray(t, np.int8).reshape(-1)
        if u is not None and u.size != self.mbw * self.mbh:
            raise EncoderError("roi_probe_set_map: the map has %d values for %d macroblocks" % (u.size, self.mbw * self.mbh))
        self._chk(self.L.mi355enc_roi_probe_set_map(self.h, None if u is None else _p(u)), "roi_probe_set_map")

    def roi_probe_offsets(self, y):
        """The offsets a picture with the coded-size luma y would be coded with under the map set last: aq_kernel (aq on) and the compose launch -> int8 (mbh, mbw)"""
        y, out = np.ascontiguousarray(y, np.uint8), np.zeros((self.mbh, self.mbw), np.int8)
        assert y.shape == (self.mbh * 16, self.mbw * 16)
        self._chk(self.L.mi355enc_roi_probe_offsets(self.h, _p(y), _p(out)), "roi_probe_offsets")
        return out

    def set_mask(self, cfg=None):
        """Privacy masks from the next picture submitted on (any time, any thread, no GPU call): a mask() / Mask / list of regions; None or empty: off.
        Pictures in flight keep theirs."""
        self._chk(self.L.mi355enc_set_mask(self.h, None if cfg is None else C.byref(mask(cfg))), "set_mask")

    def get_mask(self):
        """the regions set last as a list of tuples, None when off"""
        on, c = C.c_int(0), Mask()
        self._chk(self.L.mi355enc_get_mask(self.h, C.byref(on), C.byref(c)), "get_mask")
        return c.as_list() if on.value else None

    def last_mask(self):
        """(regions, generation) of the last collected picture; ([], 0) for a picture without"""
        c, g = Mask(), C.c_uint(0)
        self._chk(self.L.mi355enc_last_mask(self.h, C.byref(c), C.byref(g)), "last_mask")
        return c.as_list(), int(g.value)

    def debug_mask_bytes(self):
        return int(self.L.mi355enc_debug_mask_bytes(self.h))

    def mask_probe(self, cfg, y, uv):
        """The launches of a masked picture on a host picture of the coded size (margins as given) -> new (y, uv); the handle's own setting plays no part"""
        y, uv = np.array(y, np.uint8, order="C"), np.array(uv, np.uint8, order="C")
        assert y.shape == (self.mbh * 16, self.mbw * 16) and uv.shape == (self.mbh * 8, self.mbw * 16)
        self._chk(self.L.mi355enc_mask_probe(self.h, C.byref(mask(cfg)), _p(y), _p(uv)), "mask_probe")
        return y, uv

    def set_warp_mesh(self, s, mesh):
        """... through the caller's own mesh, int32 (ny, nx, 2) for the coded visible size (s None: off)"""
        if s is None:
            self._chk(self.L.mi355enc_set_warp_mesh(self.h, None, None, 0, 0), "set_warp_mesh")
            return
        m, nx, ny = _mesh(mesh, self.width, self.height)
        self._chk(self.L.mi355enc_set_warp_mesh(self.h, C.byref(warp(s)), _p(m), nx, ny), "set_warp_mesh")

    def get_warp(self):
        """the setting set last as a dict, None when off"""
        on, st = C.c_int(0), Warp()
        self._chk(self.L.mi355enc_get_warp(self.h, C.byref(on), C.byref(st)), "get_warp")
        return st.as_dict() if on.value else None

    def last_warp(self):
        """the generation (count of successful sets) whose mesh the last collected picture was warped with, 0 for an unwarped one"""
        g = C.c_uint(0)
        self._chk(self.L.mi355enc_last_warp(self.h, C.byref(g)), "last_warp")
        return int(g.value)

    def debug_warp_bytes(self):
        return int(self.L.mi355enc_debug_warp_bytes(self.h))

    def debug_warp_staging(self, on):
        """measurements: False -- every tile of the warp launch takes the direct form (the picture is the same)"""
        self._chk(self.L.mi355enc_debug_warp_staging(self.h, int(bool(on))), "debug_warp_staging")

    def stage_warp(self, s, mesh, y, uv):
        """The warp launch alone on host planes of the coded size through `mesh` (of the coded visible size); returns the warped copies, margin included."""
        y, uv = np.ascontiguousarray(y, np.uint8).copy(), np.ascontiguousarray(uv, np.uint8).copy()
        assert y.shape == (self.mbh * 16, self.mbw * 16) and uv.shape == (self.mbh * 8, self.mbw * 16)
        m, _, _ = _mesh(mesh, self.width, self.height)
        self._chk(self.L.mi355enc_warp_probe(self.h, C.byref(warp(s)), _p(m), _p(y), _p(uv)), "stage_warp")
        return y, uv

    def debug_denoise_bytes(self):
        return int(self.L.mi355enc_debug_denoise_bytes(self.h))

    def set_denoise_motion(self, rng):
        """the noise filter's motion compensation from the next submitted picture on (any time, any thread): the search range, 0 .. 16 luma samples; 0: none"""
        self._chk(self.L.mi355enc_set_denoise_motion(self.h, int(rng)), "set_denoise_motion")

    def get_denoise_motion(self):
        v = C.c_int(0)
        self._chk(self.L.mi355enc_get_denoise_motion(self.h, C.byref(v)), "get_denoise_motion")
        return v.value

    def last_denoise_motion(self):
        """the range the last collected picture was submitted under; EncoderError before the first collect"""
        v = C.c_int(0)
        self._chk(self.L.mi355enc_last_denoise_motion(self.h, C.byref(v)), "last_denoise_motion")
        return v.value

    def stage_denoise_search(self, d, rng, y, hist_y):
        """The motion search alone: a luma plane of the coded size against a luma history (uint16, its shape), with the handle's visible size.  Returns (vec, M):
        per 8 x 8 block (dx, dy) as int8 (rows, columns, 2) and the vector's cost (uint16); zeros for a block without a visible sample."""
        st = denoise(d)
        y, hist_y = np.ascontiguousarray(y, np.uint8), np.ascontiguousarray(hist_y, np.uint16)
        assert y.shape == (self.mbh * 16, self.mbw * 16) and hist_y.shape == y.shape
        words = np.zeros((self.mbh * 2, self.mbw * 2), np.uint32)
        self._chk(self.L.mi355enc_stage_denoise_search(self.h, C.byref(st), int(rng), _p(y), _p(hist_y), _p(words)), "stage_denoise_search")
        return _denoise_vectors(words)

    def stage_denoise_mc(self, d, rng, y, uv, hist_y=None, hist_uv=None):
        """stage_denoise with a search range (0: that call itself).  Returns (y, uv, hist_y, hist_uv, vec, M): behind stage_denoise's four the search's result as
        stage_denoise_search returns it (zeros where no search ran)."""
        st = denoise(d)
        y, uv = np.ascontiguousarray(y, np.uint8).copy(), np.ascontiguousarray(uv, np.uint8).copy()
        assert y.shape == (self.mbh * 16, self.mbw * 16) and uv.shape == (self.mbh * 8, self.mbw * 16)
        hin = [None if a is None else np.ascontiguousarray(a, np.uint16) for a in (hist_y, hist_uv)]
        assert all(a is None or a.shape == p.shape for a, p in zip(hin, (y, uv)))
        hy = np.zeros(y.shape, np.uint16) if st.luma or st.chroma else None
        huv = np.zeros(uv.shape, np.uint16) if st.chroma else None
        words = np.zeros((self.mbh * 2, self.mbw * 2), np.uint32)
        ptr = lambda a: None if a is None else _p(a)
        self._chk(self.L.mi355enc_stage_denoise_mc(self.h, C.byref(st), int(rng), ptr(hin[0]), ptr(hin[1]), _p(y), _p(uv), ptr(hy), ptr(huv), _p(words)), "stage_denoise_mc")
        return (y, uv, hy, huv) + _denoise_vectors(words)

    def stage_yuv_convert(self, y, uv):
        """The colour step alone on host planes of the coded size, with the handle's geometry, orientation and colorimetries; returns the converted copies."""
        y, uv = np.ascontiguousarray(y, np.uint8).copy(), np.ascontiguousarray(uv, np.uint8).copy()
        assert y.shape == (self.mbh * 16, self.mbw * 16) and uv.shape == (self.mbh * 8, self.mbw * 16)
        self._chk(self.L.mi355enc_stage_yuv_convert(self.h, _p(y), _p(uv)), "stage_yuv_convert")
        return y, uv

    def encode(self, y, uv, pts=0, force_idr=False):
        y, uv = _rows(y), _rows(uv)
        n, key = C.c_size_t(0), C.c_int(0)
        self._chk(self.L.mi355enc_encode(self.h, _p(y), y.strides[0], _p(uv), uv.strides[0], pts, int(force_idr),
                                         _p(self._out), self._out.size, C.byref(n), C.byref(key)), "encode")
        return bytes(self._out[: n.value]), bool(key.value)

    def submit(self, y, uv, pts=0, force_idr=False):
        y, uv = _rows(y), _rows(uv)
        self._chk(self.L.mi355enc_submit(self.h, _p(y), y.strides[0], _p(uv), uv.strides[0], pts, int(force_idr)), "submit")
        return self._count()

    def _planes(self, planes):
        arrs = [np.ascontiguousarray(a) for a in planes]  # uint8, or the 16-bit / 32-bit words of FMT_P010 / FMT_I420_10 / FMT_V210 as their bytes
        arrs = [a if a.dtype == np.uint8 else a.view(np.uint8) if a.dtype.itemsize > 1 and a.dtype.kind == "u" else a.astype(np.uint8) for a in arrs]
        pp = (C.c_void_p * 3)(*([a.ctypes.data for a in arrs] + [None] * (3 - len(arrs))))
        ss = (C.c_int * 3)(*([a.strides[0] for a in arrs] + [0] * (3 - len(arrs))))
        return arrs, pp, ss

    def submit_fmt(self, fmt, planes, pts=0, force_idr=False):
        """fmt: FMT_I420 / FMT_YV12 / FMT_Y42B / FMT_Y444 (three planes), FMT_YUY2 / FMT_UYVY (one packed plane, 2 bytes per pixel), FMT_NV12 / FMT_NV21
        (Y and interleaved chroma), FMT_BGRX .. FMT_XBGR (one plane, 4 bytes per pixel), FMT_BGR / FMT_RGB (3 bytes per pixel), FMT_P010 (two planes of '<u2'), FMT_I420_10 (three of '<u2'), FMT_V210 (one plane of '<u4' words or of bytes), FMT_GRAY8
        (one plane).  A contiguous plane is taken where
        it lies (so one inside a PinnedBuffer is transferred in place)."""
        arrs, pp, ss = self._planes(planes)
        self._chk(self.L.mi355enc_submit_fmt(self.h, fmt, pp, ss, pts, int(force_idr)), "submit_fmt")
        return self._count()

    def stage_csc(self, fmt, planes):
        arrs, pp, ss = self._planes(planes)
        oy = np.empty((self.mbh * 16, self.mbw * 16), np.uint8)
        ouv = np.empty((self.mbh * 8, self.mbw * 16), np.uint8)
        self._chk(self.L.mi355enc_stage_csc(self.h, fmt, pp, ss, _p(oy), _p(ouv)), "stage_csc")
        return oy, ouv

    def submit_jpeg(self, data, pts=0, force_idr=False):
        """A baseline JPEG picture of the input size (bytes): entropy decode on the host, everything else on the device.  EncoderError (MI355ENC_ERR_ARG)
        for a picture that is refused or does not decode; nothing is enqueued then."""
        buf = np.frombuffer(bytes(data), np.uint8)
        self._chk(self.L.mi355enc_submit_jpeg(self.h, _p(buf) if buf.size else None, buf.size, pts, int(force_idr)), "submit_jpeg")
        return self._count()

    def _surfaces(self):
        return np.empty((self.mbh * 16, self.mbw * 16), np.uint8), np.empty((self.mbh * 8, self.mbw * 16), np.uint8)

    def stage_jpeg(self, data):
        """The JPEG path alone: the coded-size NV12 surfaces of a picture, like stage_csc."""
        buf = np.frombuffer(bytes(data), np.uint8)
        oy, ouv = self._surfaces()
        self._chk(self.L.mi355enc_stage_jpeg(self.h, _p(buf) if buf.size else None, buf.size, _p(oy), _p(ouv)), "stage_jpeg")
        return oy, ouv

    def stage_jpeg_blocks(self, hs, vs, components, coef, qt):
        """The JPEG kernel alone on made-up coefficients: coef a list of per-component int16 arrays (block rows, blocks per row, 8, 8) or one flat array, qt uint16 (3, 64)."""
        flat = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int16).ravel() for c in coef]) if isinstance(coef, (list, tuple)) else coef, np.int16)
        q = np.ascontiguousarray(np.asarray(qt, np.uint16).reshape(3, 64))
        oy, ouv = self._surfaces()
        self._chk(self.L.mi355enc_stage_jpeg_blocks(self.h, hs, vs, components, _p(flat), _p(q), _p(oy), _p(ouv)), "stage_jpeg_blocks")
        return oy, ouv

    def stage_csc_device(self, fmt, plane_ptrs, strides, out_y_ptr, out_uv_ptr):
        """The conversion launch alone on device-resident planes (addresses as ints, any alignment and stride) into device surfaces of the coded size."""
        pp = (C.c_void_p * 3)(*(list(plane_ptrs) + [None] * (3 - len(plane_ptrs))))
        ss = (C.c_int * 3)(*(list(strides) + [0] * (3 - len(strides))))
        self._chk(self.L.mi355enc_stage_csc_device(self.h, fmt, pp, ss, out_y_ptr, out_uv_ptr), "stage_csc_device")

    def set_input_size(self, w, h):
        """pictures submitted from now on are w x h (before the first submit; the coded size returns to the unscaled path)"""
        self._chk(self.L.mi355enc_set_input_size(self.h, int(w), int(h)), "set_input_size")
        self.input_size, self._in_set = (int(w), int(h)), True

    def set_input_geometry(self, g):
        """crop / scale / letterbox of the pictures submitted from now on (before the first submit): a Geometry; replaces set_input_size"""
        self._chk(self.L.mi355enc_set_input_geometry(self.h, C.byref(g)), "set_input_geometry")
        self.input_size, self._in_set = (g.in_w, g.in_h), True

    def get_input_geometry(self):
        g = Geometry()
        self._chk(self.L.mi355enc_get_input_geometry(self.h, C.byref(g)), "get_input_geometry")
        return g

    def set_crop(self, x, y, w, h):
        """the crop rectangle of the pictures submitted from now on (between submits, on an encoder with a geometry); pictures in flight keep theirs"""
        self._chk(self.L.mi355enc_set_crop(self.h, int(x), int(y), int(w), int(h)), "set_crop")

    def stage_geometry(self, fmt, planes):
        """The geometry launch alone: planes of the input size (row strides as the arrays have them) -> the coded-size NV12 surfaces."""
        return self.stage_scale(fmt, planes, entry="stage_geometry")

    def set_orientation(self, method):
        """orientation of the pictures submitted from now on (before the first submit): 0 .. 7 or "identity", "90r", "180", "90l", "horiz", "vert", "ul-lr",
        "ur-ll".  With a transposing method and no input size of its own the pictures submitted are height x width."""
        m = orient_method(method)
        self._chk(self.L.mi355enc_set_orientation(self.h, m), "set_orientation")
        self.orientation = m
        if not self._in_set:  # (it follows the method unless set_input_size gave one)
            self.input_size = self.pre_size()

    def pre_size(self):
        """(w, h) before orientation: what decode / conversion / scaling produce, and what is submitted unless set_input_size says otherwise"""
        return (self.height, self.width) if self.orientation in (ORIENT_90R, ORIENT_90L, ORIENT_UL_LR, ORIENT_UR_LL) else (self.width, self.height)

    def get_orientation(self):
        return self.L.mi355enc_get_orientation(self.h)

    def orient_bytes(self):
        """development: device memory held for pre-orientation pictures (0 with identity)"""
        return int(self.L.mi355enc_debug_orient_bytes(self.h))

    def stage_orient(self, method, y, uv):
        """The orientation kernel alone: NV12 host planes of the pre-orientation size (row strides as the arrays have them) -> the coded-size surfaces."""
        y, uv = _rows(y), _rows(uv)
        oy, ouv = self._surfaces()
        self._chk(self.L.mi355enc_stage_orient(self.h, orient_method(method), _p(y), y.strides[0], _p(uv), uv.strides[0], _p(oy), _p(ouv)), "stage_orient")
        return oy, ouv

    def stage_orient_device(self, method, y_ptr, y_stride, uv_ptr, uv_stride, out_y_ptr, out_uv_ptr):
        """... on device-resident planes (addresses as ints, any alignment and stride) into device surfaces of the coded size, stride 16 mbw."""
        self._chk(self.L.mi355enc_stage_orient_device(self.h, orient_method(method), y_ptr, int(y_stride), uv_ptr, int(uv_stride), out_y_ptr, out_uv_ptr), "stage_orient_device")

    def stage_scale(self, fmt, planes, entry="stage_scale"):
        """The scale kernel alone: planes of the input size (row strides as the arrays have them) -> the coded-size NV12 surfaces."""
        arrs = [a if a.dtype == np.uint8 and a.strides[-1] == 1 else np.ascontiguousarray(a, np.uint8) for a in planes]
        pp = (C.c_void_p * 3)(*([a.ctypes.data for a in arrs] + [None] * (3 - len(arrs))))
        ss = (C.c_int * 3)(*([a.strides[0] for a in arrs] + [0] * (3 - len(arrs))))
        oy = np.empty((self.mbh * 16, self.mbw * 16), np.uint8)
        ouv = np.empty((self.mbh * 8, self.mbw * 16), np.uint8)
        self._chk(getattr(self.L, "mi355enc_" + entry)(self.h, fmt, pp, ss, _p(oy), _p(ouv)), entry)
        return oy, ouv

    def scale_tables_device(self):
        """The device's copy of the scale tables: [(first, coef)] for luma horizontal, luma vertical, chroma horizontal, chroma vertical
        from 4:2:0 and from 4:2:2 (include/mi355enc.h MI355ENC_FETCH_SCALE_TABLES)."""
        (iw, ih), (ow, oh) = self.input_size, self.pre_size()
        spec = [(iw, ow, SCALE_LUMA), (ih, oh, SCALE_LUMA), (iw, ow, SCALE_CHROMA_H), (ih, oh, SCALE_CHROMA_V), (ih, oh, SCALE_CHROMA_V422)]
        shapes = [scale_table(*a)[1].shape for a in spec]
        sizes = [(n * 4 + n * t * 2 + 15) // 16 * 16 for n, t in shapes]
        blob = np.zeros(sum(sizes), np.uint8)
        self._chk(self.L.mi355enc_fetch(self.h, FETCH_SCALE_TABLES, _p(blob), blob.nbytes), "fetch")
        out, o = [], 0
        for (n, t), sz in zip(shapes, sizes):
            first = blob[o:o + 4 * n].view(np.int32).copy()
            coef = blob[o + 4 * n:o + 4 * n + 2 * n * t].view(np.int16).reshape(n, t).copy()
            out.append((first, coef))
            o += sz
        return out

    def set_quality_metrics(self, on=True):
        """per-picture PSNR / SSIM computed on the device from now on (before the first submit); last_quality() after every collect()"""
        self._chk(self.L.mi355enc_set_quality_metrics(self.h, int(bool(on))), "set_quality_metrics")

    def last_quality(self):
        """Quality of the last collected picture (EncoderError with metrics off or nothing collected)"""
        q = Quality()
        self._chk(self.L.mi355enc_last_quality(self.h, C.byref(q)), "last_quality")
        return q

    def quality_totals(self):
        """Quality summed over the pictures collected since open / reset_stats(): global PSNR, mean SSIM"""
        q = Quality()
        self._chk(self.L.mi355enc_quality_totals(self.h, C.byref(q)), "quality_totals")
        return q

    def stage_quality(self, src_y, src_uv, rec_y, rec_uv):
        """The metrics kernel alone on host planes of the coded size (16 mbh x 16 mbw luma, 8 mbh x 16 mbw interleaved chroma)."""
        a = [np.ascontiguousarray(p, np.uint8) for p in (src_y, src_uv, rec_y, rec_uv)]
        assert a[0].shape == a[2].shape == (self.mbh * 16, self.mbw * 16) and a[1].shape == a[3].shape == (self.mbh * 8, self.mbw * 16)
        q = Quality()
        self._chk(self.L.mi355enc_stage_quality(self.h, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), C.byref(q)), "stage_quality")
        return q

    def stage_quality_device(self, src_y_ptr, src_uv_ptr, src_stride, rec_y_ptr, rec_uv_ptr):
        """... on device-resident planes (addresses as ints): the source at any address and stride, the reconstruction at stride 16 mbw."""
        q = Quality()
        self._chk(self.L.mi355enc_stage_quality_device(self.h, src_y_ptr, src_uv_ptr, int(src_stride), rec_y_ptr, rec_uv_ptr, C.byref(q)), "stage_quality_device")
        return q

    def request_snapshot(self, what=SNAP_SOURCE, reduce=1, quality=75):
        """Arms the next submitted picture: a JPEG still of its coded source (what 0) or of its deblocked reconstruction (1), reduced by 1, 2, 4 or 8."""
        req = SnapshotReq(int(what), int(reduce), int(quality))
        self._chk(self.L.mi355enc_request_snapshot(self.h, C.byref(req)), "request_snapshot")

    def take_snapshot(self, cap=None):
        """(bytes, info dict) of the still of the last armed picture that has been collected -- Huffman coded here, in this thread -- or None while none is ready.
        cap: the room offered (default: what the still needs, asked for first); too little raises EncoderError with .need = the bytes needed."""
        n, info = C.c_size_t(0), SnapshotInfo()
        if cap is None:  # ask first: a capacity of 0 yields the bytes needed (coding the still twice costs less than a buffer for the worst case of the full size)
            r = self.L.mi355enc_take_snapshot(self.h, None, 0, C.byref(n), C.byref(info))
            if r == -6:
                return None
            if r != -5:
                self._chk(r, "take_snapshot")
            cap = int(n.value)
        out = np.empty(max(int(cap), 1), np.uint8)
        r = self.L.mi355enc_take_snapshot(self.h, _p(out), int(cap), C.byref(n), C.byref(info))
        if r == -6:
            return None
        if r == -5:
            e = EncoderError("mi355enc_take_snapshot: output buffer too small (-5)")
            e.need = int(n.value)
            raise e
        self._chk(r, "take_snapshot")
        return bytes(out[:n.value]), info.as_dict()

    def snapshot_bytes(self):
        """memory held for stills (0 until the first armed picture is submitted)"""
        return int(self.L.mi355enc_debug_snapshot_bytes(self.h))

    def stage_snapshot_blocks(self, y, uv, reduce=1, quality=75):
        """The still kernel alone: NV12 planes (h, w) and (h / 2, w) of any even size -> ([int16 (block rows, blocks per row, 8, 8)] of Y, Cb, Cr, qt uint16 (2, 64))."""
        y, uv = _rows(y), _rows(uv)
        h, w = y.shape
        ow, oh = snapshot_size(w, h, reduce)
        flat = np.zeros(sum(bw * bh for bw, bh in snapshot_layout(ow, oh)) * 64, np.int16)
        qt = np.zeros((2, 64), np.uint16)
        self._chk(self.L.mi355enc_stage_snapshot_blocks(self.h, _p(y), y.strides[0], _p(uv), uv.strides[0], w, h, int(reduce), int(quality), _p(flat), _p(qt)), "stage_snapshot_blocks")
        return _snapshot_split(flat, ow, oh), qt

    def stage_snapshot_blocks_device(self, y_ptr, y_stride, uv_ptr, uv_stride, w, h, reduce=1, quality=75):
        """... on planes in this GPU's memory (addresses as ints, any alignment and stride)"""
        ow, oh = snapshot_size(w, h, reduce)
        flat = np.zeros(sum(bw * bh for bw, bh in snapshot_layout(ow, oh)) * 64, np.int16)
        qt = np.zeros((2, 64), np.uint16)
        self._chk(self.L.mi355enc_stage_snapshot_blocks_device(self.h, y_ptr, y_stride, uv_ptr, uv_stride, w, h, int(reduce), int(quality), _p(flat), _p(qt)), "stage_snapshot_blocks_device")
        return _snapshot_split(flat, ow, oh), qt

    def stage_snapshot(self, y, uv, reduce=1, quality=75):
        """... and the whole file (bytes)"""
        y, uv = _rows(y), _rows(uv)
        h, w = y.shape
        ow, oh = snapshot_size(w, h, reduce)
        out, n = np.empty(snapshot_max_bytes(ow, oh), np.uint8), C.c_size_t(0)
        self._chk(self.L.mi355enc_stage_snapshot(self.h, _p(y), y.strides[0], _p(uv), uv.strides[0], w, h, int(reduce), int(quality), _p(out), out.size, C.byref(n)), "stage_snapshot")
        return bytes(out[:n.value])

    def set_overlay_text(self, text):
        """The text drawn into every picture submitted from now on (str or bytes; None or "": off).  Thread-safe, no GPU call."""
        self._chk(self.L.mi355enc_set_overlay_text(self.h, _text_bytes(text)), "set_overlay_text")

    def set_overlay_style(self, style=None, **kw):
        """An OverlayStyle, or the default style with fields replaced (halign=, valign=, xpad=, ypad=, scale=, shaded_background=)"""
        st = style if style is not None else overlay_style(**kw)
        self._chk(self.L.mi355enc_set_overlay_style(self.h, C.byref(st)), "set_overlay_style")

    def last_overlay(self):
        """The text drawn into the last collected picture, as bytes (b"": none)"""
        buf = C.create_string_buffer(OVERLAY_MAX_TEXT + 1)
        n = self.L.mi355enc_last_overlay(self.h, buf, len(buf))
        if n < 0:
            self._chk(n, "last_overlay")
        return buf.raw[:n]

    def stage_overlay(self, text, y, uv, style=None, **kw):
        """The overlay kernel alone on host planes of the coded size; returns the drawn copies."""
        st = style if style is not None else overlay_style(**kw)
        y, uv = np.ascontiguousarray(y, np.uint8).copy(), np.ascontiguousarray(uv, np.uint8).copy()
        assert y.shape == (self.mbh * 16, self.mbw * 16) and uv.shape == (self.mbh * 8, self.mbw * 16)
        self._chk(self.L.mi355enc_stage_overlay(self.h, _text_bytes(text), C.byref(st), _p(y), _p(uv)), "stage_overlay")
        return y, uv

    def set_image(self, layer, pixels, x=0, y=0, opacity=256, fmt=FMT_RGBX):
        """The image blended into every picture submitted from now on as layer 0 .. 3: pixels (h, w, 4) uint8 with straight alpha in byte order fmt, its
        top-left pixel at (x, y) of the coded visible picture, opacity 0 .. 256 (None: the layer is off).  The pixels are copied.  Thread-safe, no GPU call."""
        im = image_layer(pixels, x, y, opacity, fmt)
        self._chk(self.L.mi355enc_set_image(self.h, int(layer), C.byref(im) if pixels is not None else None), "set_image")

    def set_image_place(self, layer, x, y, opacity=256):
        """place and opacity of a layer's image from the next submitted picture on (EncoderError on a layer that is off)"""
        self._chk(self.L.mi355enc_set_image_place(self.h, int(layer), int(x), int(y), int(opacity)), "set_image_place")

    def last_image(self, layer=0):
        """(w, h, x, y, opacity, serial) of what layer `layer` put into the last collected picture; all 0: nothing"""
        info = ImageInfo()
        self._chk(self.L.mi355enc_last_image(self.h, int(layer), C.byref(info)), "last_image")
        return info.as_tuple()

    def image_bytes(self):
        """development: device memory held for images (0 until a picture with an active layer is submitted)"""
        return int(self.L.mi355enc_debug_image_bytes(self.h))

    def stage_image(self, layers, y, uv):
        """The image kernels alone on host planes of the coded size: layers a list of up to four ImageLayer (image_layer()), blended in order; returns the blended copies."""
        y, uv = np.ascontiguousarray(y, np.uint8).copy(), np.ascontiguousarray(uv, np.uint8).copy()
        assert y.shape == (self.mbh * 16, self.mbw * 16) and uv.shape == (self.mbh * 8, self.mbw * 16)
        arr = (ImageLayer * max(len(layers), 1))(*layers)
        self._chk(self.L.mi355enc_stage_image(self.h, arr, len(layers), _p(y), _p(uv)), "stage_image")
        return y, uv

    def submit_device(self, y_ptr, y_stride, uv_ptr, uv_stride, pts=0, force_idr=False):
        self._chk(self.L.mi355enc_submit_device(self.h, y_ptr, y_stride, uv_ptr, uv_stride, pts, int(force_idr)), "submit_device")
        return self._count()

    def _count(self):
        """what a submit*() returns: with frame-rate conversion the pictures it enqueued (0 .. max_fill + 1), otherwise None as ever"""
        return int(self.L.mi355enc_last_submit_count(self.h)) if getattr(self, "rate_on", False) else None

    def rate_peek(self, pts):
        """pictures a submit with this pts would enqueue now; changes nothing"""
        return int(self.L.mi355enc_rate_peek(self.h, int(pts)))

    def rate_stats(self):
        """dict of in / out / dropped / repeated / blended / resyncs; EncoderError with conversion off"""
        st = RateStats()
        self._chk(self.L.mi355enc_rate_stats(self.h, C.byref(st)), "rate_stats")
        return st.as_dict()

    def rate_bytes(self):
        """development: device memory held for the frame-rate conversion (0 when off, and in hold mode with max_fill 0)"""
        return int(self.L.mi355enc_debug_rate_bytes(self.h))

    def stage_rate(self, w256, a_y, a_uv, b_y, b_uv):
        """The mix launch alone on host planes of the coded size: (a (256 - w256) + b w256 + 128) >> 8, as the encoder runs it (in place, b kept where a was); returns (y, uv)."""
        pl = [np.ascontiguousarray(p, np.uint8) for p in (a_y, a_uv, b_y, b_uv)]
        assert pl[0].shape == pl[2].shape == (self.mbh * 16, self.mbw * 16) and pl[1].shape == pl[3].shape == (self.mbh * 8, self.mbw * 16)
        oy, ouv = self._surfaces()
        self._chk(self.L.mi355enc_stage_rate(self.h, int(w256), _p(pl[0]), _p(pl[1]), _p(pl[2]), _p(pl[3]), _p(oy), _p(ouv)), "stage_rate")
        return oy, ouv

    def collect(self, copy=True):
        n, key, pts, qp = C.c_size_t(0), C.c_int(0), C.c_int64(0), C.c_int(0)
        self._chk(self.L.mi355enc_collect(self.h, _p(self._out), self._out.size, C.byref(n), C.byref(key), C.byref(pts),
                                          C.byref(qp)), "collect")
        au = bytes(self._out[: n.value]) if copy else n.value
        return au, bool(key.value), pts.value, qp.value

    @property
    def last_drop(self):
        """drop level of the last collected picture (0, 1 .. DROP_MAX, DROP_SKIP)"""
        return int(self.stats().last_drop)

    @property
    def pending(self):
        return self.L.mi355enc_pending(self.h)

    def stats(self):
        s = Stats()
        self._chk(self.L.mi355enc_get_stats(self.h, C.byref(s)), "get_stats")
        return s

    def reset_stats(self):
        self.L.mi355enc_reset_stats(self.h)

    def fetch(self, what):
        H, W, n = self.mbh * 16, self.mbw * 16, self.mbw * self.mbh
        if what in (FETCH_RECON_Y, FETCH_PREFILTER_Y, FETCH_SOURCE_Y):
            a = np.empty((H, W), np.uint8)
        elif what in (FETCH_RECON_UV, FETCH_PREFILTER_UV, FETCH_SOURCE_UV):
            a = np.empty((H // 2, W), np.uint8)
        elif what == FETCH_MBINFO:
            a = np.empty(n, MBINFO_DTYPE)
        else:
            a = np.empty((n, LEVELS_PER_MB), np.int16)
        self._chk(self.L.mi355enc_fetch(self.h, what, _p(a), a.nbytes), "fetch")
        return a

    def band_cuts(self):
        """Development: what the band deblocker's last launch with the cut left (mi355enc_dev.h, d_part_cnt) -- a record with "count"
        (bands, 2): per band and plane the parts' counter; "cut" and "epoch" (bands, 2): per band and plane the column where the band
        was cut and the picture's epoch.  None where bands are walked whole (MI355ENC_NO_SPLIT)."""
        nb = (self.mbh + BAND_ROWS - 1) // BAND_ROWS
        layout = np.dtype([("count", "<u4", (nb, 2)), ("gran", [("cut", "<u4"), ("epoch", "<u4")], (nb, 2))])
        a = np.zeros(1, layout)
        r = self.L.mi355enc_fetch(self.h, FETCH_BAND_CUTS, _p(a), a.nbytes)
        if r == ERR_STATE:
            return None
        self._chk(r, "fetch")
        g = a[0]["gran"]
        return {"count": a[0]["count"].copy(), "cut": g["cut"].astype(np.int64), "epoch": g["epoch"].copy()}

    def error_word(self):
        """Development: the device's sticky error word (a bounded wait that ran out leaves its code there; 0: none did)."""
        a = np.zeros(1, np.uint32)
        self._chk(self.L.mi355enc_fetch(self.h, FETCH_ERROR_WORD, _p(a), a.nbytes), "fetch")
        return int(a[0])

    def sync_words(self):
        """Development: the device's side of debug_get_counters()'s four totals, read with the compute streams idle -- "db_started_total", "ip_done_total",
        "qpc_total": the three counting words; "row_done": every macroblock row's count (each equals pmb_rows_total once its launches are through)."""
        a = np.zeros(3 + self.mbh, np.uint32)
        self._chk(self.L.mi355enc_fetch(self.h, FETCH_SYNC_WORDS, _p(a), a.nbytes), "fetch")
        return {"db_started_total": int(a[0]), "ip_done_total": int(a[1]), "qpc_total": int(a[2]), "row_done": a[3:].copy()}

    # ---- single-stage entry points (coded-size host planes)
    def stage_me(self, cur_y, ref_y, qp):
        """-> (surfaces (n_mb, 35, 36) uint16: [dy+16][dx+16], first selection IMV_DTYPE (n_mb,))"""
        n = self.mbw * self.mbh
        imv = np.zeros(n, IMV_DTYPE)
        surf = np.zeros((n, SURF_ROWS, SURF_COLS), np.uint16)
        self._chk(self.L.mi355enc_stage_me(self.h, _p(np.ascontiguousarray(cur_y)), _p(np.ascontiguousarray(ref_y)), qp, _p(surf), _p(imv)), "stage_me")
        return surf, imv

    def stage_me_select(self, surf, imv, qp):
        out = np.zeros(imv.size, IMV_DTYPE)
        self._chk(self.L.mi355enc_stage_me_select(self.h, _p(np.ascontiguousarray(surf, np.uint16)), _p(np.ascontiguousarray(imv)), qp, _p(out)), "stage_me_select")
        return out

    def stage_me_select_next(self, surf, imv, prev, qp):
        """the same iteration as the encoder's later passes run it: macroblocks whose predictors are unchanged against `prev` (the field `imv` was selected from) are copied"""
        out = np.zeros(imv.size, IMV_DTYPE)
        self._chk(self.L.mi355enc_stage_me_select_next(self.h, _p(np.ascontiguousarray(surf, np.uint16)), _p(np.ascontiguousarray(imv)), _p(np.ascontiguousarray(prev)), qp, _p(out)), "stage_me_select_next")
        return out

    def stage_subpel(self, cur_y, ref_y, mbi, qp):
        mbi = np.ascontiguousarray(mbi).copy()
        self._chk(self.L.mi355enc_stage_subpel(self.h, _p(np.ascontiguousarray(cur_y)), _p(np.ascontiguousarray(ref_y)), qp, _p(mbi)), "stage_subpel")
        return mbi

    def stage_inter(self, src_y, src_uv, ref_y, ref_uv, mbi, qp):
        mbi = np.ascontiguousarray(mbi).copy()
        rec_y, rec_uv = np.empty_like(src_y), np.empty_like(src_uv)
        lev = np.empty((mbi.size, LEVELS_PER_MB), np.int16)
        self._chk(self.L.mi355enc_stage_inter(self.h, _p(np.ascontiguousarray(src_y)), _p(np.ascontiguousarray(src_uv)),
                                              _p(np.ascontiguousarray(ref_y)), _p(np.ascontiguousarray(ref_uv)), qp, _p(mbi),
                                              _p(rec_y), _p(rec_uv), _p(lev)), "stage_inter")
        return rec_y, rec_uv, mbi, lev

    def stage_pmb(self, src_y, src_uv, ref_y, ref_uv, imv, surf, qp, drop=0, refine=True, idec=None, run_intra_p=True):
        """surf: device layout (n_mb, 35, 36).  -> rec_y, rec_uv, records, levels"""
        n = self.mbw * self.mbh
        mbi = np.zeros(n, MBINFO_DTYPE)
        rec_y, rec_uv = np.empty_like(src_y), np.empty_like(src_uv)
        lev = np.empty((n, LEVELS_PER_MB), np.int16)
        dec = np.ascontiguousarray(idec) if idec is not None else None
        self._chk(self.L.mi355enc_stage_pmb(self.h, _p(np.ascontiguousarray(src_y)), _p(np.ascontiguousarray(src_uv)),
                                            _p(np.ascontiguousarray(ref_y)), _p(np.ascontiguousarray(ref_uv)), qp, int(drop), int(refine),
                                            _p(np.ascontiguousarray(imv)), _p(np.ascontiguousarray(surf, np.uint16)), _p(dec) if dec is not None else None,
                                            int(run_intra_p), _p(mbi), _p(rec_y), _p(rec_uv), _p(lev)), "stage_pmb")
        return rec_y, rec_uv, mbi, lev

    def stage_intra(self, src_y, src_uv, qp, drop=0):
        mbi = np.zeros(self.mbw * self.mbh, MBINFO_DTYPE)
        rec_y, rec_uv = np.empty_like(src_y), np.empty_like(src_uv)
        lev = np.empty((mbi.size, LEVELS_PER_MB), np.int16)
        self._chk(self.L.mi355enc_stage_intra(self.h, _p(np.ascontiguousarray(src_y)), _p(np.ascontiguousarray(src_uv)), qp, int(drop),
                                              _p(mbi), _p(rec_y), _p(rec_uv), _p(lev)), "stage_intra")
        return rec_y, rec_uv, mbi, lev

    def stage_intra_analyse(self, src_y, src_uv, qp=30):
        out = np.empty((self.mbw * self.mbh, 152), np.uint16)
        dec = np.zeros(self.mbw * self.mbh, IDEC)
        self._chk(self.L.mi355enc_stage_intra_analyse(self.h, _p(np.ascontiguousarray(src_y)), _p(np.ascontiguousarray(src_uv)), qp, _p(out), _p(dec)), "stage_intra_analyse")
        return out, dec

    def stage_deblock(self, rec_y, rec_uv, mbi):
        y, uv = np.ascontiguousarray(rec_y).copy(), np.ascontiguousarray(rec_uv).copy()
        self._chk(self.L.mi355enc_stage_deblock(self.h, _p(y), _p(uv), _p(np.ascontiguousarray(mbi))), "stage_deblock")
        return y, uv

    @property
    def slice_rows(self):
        """macroblock rows per slice of this encoder's I pictures (0: one slice)"""
        return int(self.L.mi355enc_slice_rows(self.h))

    @property
    def p_slice_rows(self):
        """... and of its P pictures"""
        return int(self.L.mi355enc_p_slice_rows(self.h))

    def stage_set_slice_deblock(self, idc):
        """the single-stage entry points: disable_deblocking_filter_idc of the picture's slices (0 or 2)"""
        self._chk(self.L.mi355enc_stage_set_slice_deblock(self.h, int(idc)), "stage_set_slice_deblock")

    def stage_set_slice_rows(self, rows):
        """the single-stage entry points treat the picture as slices of `rows` macroblock rows (0, the default: one slice)"""
        self._chk(self.L.mi355enc_stage_set_slice_rows(self.h, int(rows)), "stage_set_slice_rows")

    def debug_trip_wait(self, code):
        """fault injection: as if a bounded device-side wait had just run out (include/mi355enc.h)"""
        self._chk(self.L.mi355enc_debug_trip_wait(self.h, int(code)), "debug_trip_wait")

    def debug_get_counters(self):
        """Development: the long-run state as a dict (Counters.NAMES): the epoch of the last picture stamped, the four device-side totals, idr_count, frames_since_idr."""
        c = Counters()
        self._chk(self.L.mi355enc_debug_get_counters(self.h, C.byref(c)), "debug_get_counters")
        return {k: int(getattr(c, k)) for k in Counters.NAMES}

    def debug_set_counters(self, **values):
        """Development: puts the handle where a long run would have put it (include/mi355enc.h): host-side values and the device-side words they are compared
        with.  Only the fields named are touched; nothing may be pending (EncoderError, code ERR_STATE)."""
        c = Counters()
        c.keep = (1 << len(Counters.NAMES)) - 1
        for k, v in values.items():
            setattr(c, k, int(v) & 0xFFFFFFFF)
            c.keep &= ~(1 << Counters.NAMES.index(k))
        self._chk(self.L.mi355enc_debug_set_counters(self.h, C.byref(c)), "debug_set_counters")

    def time_stage(self, stage, iters=20):
        ms = C.c_double(0)
        self._chk(self.L.mi355enc_time_stage(self.h, stage, iters, C.byref(ms)), "time_stage")
        return ms.value
