// enc_internal.hpp -- what the translation units of the C-ABI shim share (not part of the ABI):
// the handle, the per-picture slot, and the helpers used by more than one of
//   enc_handle.cpp    open / close / setters / statistics / fetch
//   enc_input.cpp     the input path: submit*, from the caller's picture to the slot's source surfaces (upload, conversion, the sequence around them), and the
//                     table of the input steps (k_steps): the one list of what is latched, drawn, collected and freed, in chain order
//   enc_schedule.cpp  the picture pipeline: the stream schedule of one picture, the entropy worker, recovery, collect
//   enc_plan.hpp      ... and that schedule's decisions as a value: plan_picture(), and the launches that follow from a plan: plan_launches(); plain C++ (included here)
//   enc_sync.*        the words kernels wait on and the host's totals of them, under one owner: dev_words_t (mi355enc::words)
//   enc_overlay.cpp   the text overlay: setters, latch, layout, launch
//   enc_image.cpp    image layers: setters, latch, upload + prepare, blend launches, retirement
//   enc_orient.cpp    orientation of the input picture: setter, the slot's pre-orientation picture, launch, its stage entry points
//   enc_jpeg.cpp      MJPEG input: coefficient buffers, host decode, transfer + launch, its stage entry points
//   enc_snapshot.cpp  JPEG stills: request / take, the blocks the levels land in, the launch, its stage entry points
//   enc_csc.cpp       colorimetry: the setters, the RGB matrix and the YUV -> YUV table, the colour step's launch, their stage entry points
//   enc_adjust.cpp    picture controls: setter, latch, the two launch forms and the scratch plane, its stage entry point
//   enc_autolevel.cpp automatic levels and white balance: setter, latch, the three launches and the device block, the probes and the stage entry point
//   enc_lut3d.cpp     3D colour LUT: setter, latch, the table's way to the device, the launch, its probe and timed stage
//   enc_roi.cpp       region-of-interest quantisation: setter, the map's latch per picture and its pinned copies, the compose launch, the stage hook and the offsets probe
//   enc_mask.cpp      privacy masks: setter, the latch per output picture, the handle's result surface and ping-pong planes, the launches, the probe and timed stages
//   enc_dspatial.cpp  spatial noise reduction: setter, latch, the estimate's two launches, the filter launches and their scratch planes, probes, stage entry point
//   enc_denoise.cpp   temporal noise reduction: setter, latch, the launch and the handle's history, its stage entry point
//   enc_stab.cpp      electronic image stabilisation: setter, latch, the estimate in front of every scale launch, its probes and timed stages
//   enc_warp.cpp      lens, roll and keystone correction: setters, latch, the mesh's way to the device, the launch and the scratch pair, its stage entry point
//   enc_rate.cpp      frame-rate conversion: setter, the plan's step and commit per submit, keep buffer, mix / keep / repeat launches, its stage entry point
//   enc_hdr.cpp       HDR input: setter, the parameter block on the host and on the device, the tone-mapping conversion launch
//   enc_quality.cpp   quality metrics: setter, the accumulator and result blocks, enqueue / collect, the stage launch
//   enc_scale.cpp     input size and geometry: the one place both are decided, tables, the slots' plans, their stage entry points
//   enc_stage.hpp     the frame of every single-stage entry point: stage_enter, stage_in / stage_out, a call's own device buffers (included at the end)
//   enc_stages.cpp    single-stage entry points (parity tests, probes), mi355enc_time_stage and its table of stages, and the host-only stages
#ifndef MI355_ENC_INTERNAL_HPP
#define MI355_ENC_INTERNAL_HPP
#include "../../include/mi355enc.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>

#include "h264_host.h"
#include "mi355enc_dev.h"
#include "snapshot_host.h"
#include "hdr_host.h"
#include "adjust_host.h"
#include "denoise_host.h"
#include "stab_host.h"
#include "autolevel_host.h"
#include "dspatial_host.h"
#include "warp_host.h"
#include "lut3d_host.h"
#include "roi_host.h"
#include "mask_host.h"
#include "enc_plan.hpp"
#include "enc_sync.hpp"

#define HIPCHK(expr)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            fprintf(stderr, "mi355enc: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MI355ENC_ERR_HIP;                                                                 \
        }                                                                                            \
    } while (0)

static const uint8_t k_lambda[52] = {1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  2,  2,
                                     2,  2,  3,  3,  3,  4,  4,  4,  5,  6,  6,  7,  8,  9,  10, 11, 13, 14,
                                     16, 18, 20, 23, 25, 29, 32, 36, 40, 45, 51, 57, 64, 72, 81, 91};

#define NSLOT 3 /* pictures in flight: pipeline_depth + 1 */
#define NSET 3  /* device-side sets of what one picture's stages hand to each other (and to the host): one per picture in flight */
#define SURF_PAD 256 /* bytes past each surface: unaligned-pair loads may touch 4 bytes beyond */


// One image a layer was given (mi355enc_set_image).  The control thread makes it from the caller's pixels; the first picture that latches
// it uploads it from pinned staging and prepares it on the device, after which nothing writes it again.  refs (under mi355enc::img_mu): the layer that shows it
// and every slot whose picture latched it; at 0 it is retired -- its buffers go to the handle's pool for the next upload, nothing is freed before close.
struct image_buf_t { uint8_t *h_pin; uint32_t *d_pix; size_t cap; hipEvent_t ev; bool busy; image_buf_t *next; }; // pinned staging + device words of cap bytes; ev: behind the last transfer out of h_pin; busy: an image owns it
struct image_t {
    uint8_t *host;      // malloc: the caller's pixels, rows of 4 w bytes (freed once they are in pinned staging)
    image_buf_t *buf;   // null until the first picture that carries the image is submitted
    int fmt, w, h, refs;
};

// One still's landing place (mi355enc_request_snapshot): pinned host memory -- the quality's snapshot_tab_t (SNAP_TAB_BYTES), then the levels,
// then one hint byte per block -- and the table's copy on the device.  state (under mi355enc::snap_mu): 0 free, 1 a picture in flight owns it, 2 the ready
// still, 3 replaced by a newer still while `readers` takers were still coding it (the last one frees it).
#define SNAP_TAB_BYTES 1024
#define SNAP_BLOCKS (NSLOT + 3) /* one per picture in flight, the ready one, one replaced while being read; the last one belongs to the stage entry points */
struct snap_block_t {
    uint8_t *h_mem; void *d_tab; size_t cap;
    int state, readers, ow, oh;
    size_t nblk;
    uint16_t qt[2][64];
    mi355enc_snapshot_info_t info;
};

// Picture controls (mi355enc_set_adjust): a checked parameter set with what follows from it -- which parts are not neutral (ADJUST_*; 0: off),
// the luma table and the chroma rotation as built for the handle's output range by the thread that set it.
struct adjust_set_t { mi355enc_adjust_t a; int parts; uint8_t luma[256]; int32_t chroma[2]; };

// Temporal noise reduction (mi355enc_set_denoise): a checked parameter set with what follows from it -- which planes are filtered (DENOISE_*;
// 0: off) and the three tables (B, the luma's P, the chroma's P) as built by the thread that set it; range: the search range of the motion compensation
// (mi355enc_set_denoise_motion; section 25), 0: none.
struct denoise_set_t { mi355enc_denoise_t d; int parts; uint8_t tabs[768]; int range; };

struct slot_t {
    frame_ctx_t *h_ctx;   // pinned
    mb_info_t *h_mbi;     // pinned
    int16_t *h_levels;    // pinned: packed level stream, written by levels_pack_kernel over PCIe (no D2H copy)
    unsigned *h_hdr;      // pinned: [0] blocks in the stream, [1] error word of the band deblocker, [2 + r] first block of macroblock row r
    uint8_t *h_src;              // pinned staging for pictures submitted from pageable host memory (allocated on first use): rows at stride W
    uint8_t *d_src_y, *d_src_uv; // staging for host / unaligned input
    uint8_t *d_raw;              // staging of non-NV12 input before the conversion kernel, and of every input before the scale kernel (allocated on first use, raw_bytes())
    uint8_t *d_csc;              // the formats of k_csc.hip with an input size of their own: the NV12 picture of the input size between conversion and scale (allocated on first use)
    uint8_t *d_pre;              // orientation (allocated on first use): the NV12 picture of the pre-orientation visible size, which the decode / conversion / scale / copy writes instead of d_src_*
    uint8_t *h_jpeg, *d_jpeg;    // MJPEG input (allocated on first use): the quantisation tables and the coefficient blocks of the picture, pinned / on the device
    uint8_t *d_jpeg_planar;      // ... and the planar picture of a 4:4:4 one between the JPEG launch and the conversion
    hipEvent_t done, gpu_done, ev[12];
    hipEvent_t ev_up;          // the source has arrived (upload stream; only when that is a stream of its own)
    hipEvent_t ev_front;       // the front stream's part of the picture is done (source in place, search + selection + analysis)
    int prof;
    int all_skip;              // the picture is one run of P_Skip macroblocks: written by the host alone, no device work
    uint64_t index;            // position of the picture in the stream
    int is_idr, qp, drop, frame_num, idr_pic_id, rec_index, set;
    int ir_start;              // periodic intra refresh: the first picture of a refresh cycle (SPS, PPS and a recovery point SEI lead its access unit; a sync point)
    int fixed_qp, fixed_drop;  // the constant-QP override this picture was submitted under (-1: none): recover() re-encodes it under the same one
    int rc_picked;             // rate control booked this picture (rc_pick): its size is reported back (rc_update) or the booking taken back (rc_cancel)
    int64_t pts;
    // entropy coding on the handle's worker thread (pipeline_depth >= 1): the access unit is coded here while the caller submits the next picture
    uint8_t *au; size_t au_len; int au_state; // 0 not submitted to the worker, 1 queued / being coded, 2 coded (au_len 0: did not fit), 3 the hand-over carried an error word
    double au_ms;
    const uint8_t *src_y, *src_uv; int src_stride, force_idr; // what enqueue_picture() was given: a recovery re-enqueues the pictures in flight from here
    // text overlay: what submit latched for this picture and drew into its source surfaces (ov_len 0: nothing); a recovery keeps it -- the surfaces carry the text
    int ov_len; char ov_text[256]; mi355enc_overlay_style_t ov_style;
    // image layers: what submit latched for this picture and blended into its source surfaces (img[l] null: nothing of layer l); a recovery keeps it likewise
    image_t *img[MI355ENC_IMAGE_LAYERS]; int img_x[MI355ENC_IMAGE_LAYERS], img_y[MI355ENC_IMAGE_LAYERS], img_op[MI355ENC_IMAGE_LAYERS]; uint32_t img_serial[MI355ENC_IMAGE_LAYERS];
    // stills: the block this picture's still lands in, + 1 (0: the picture is not armed), and the request it was armed with; a recovery keeps both
    int snap; mi355enc_snapshot_req_t snap_req;
    // the colour step: this picture's samples are converted in ingest_end (latched with the slot; an RGB picture, converted straight to the output, clears it)
    bool yuv_step;
    // picture controls: what submit latched for this picture (adj.parts 0: nothing); applied once, to the input's own slot, in ingest_end
    adjust_set_t adj;
    // temporal noise reduction: what submit latched for this picture (dn.parts 0: nothing); applied once, to the input's own slot, in ingest_end
    denoise_set_t dn;
    // image stabilisation: what submit latched for this picture (stab.range 0: off), and whether the estimate ran for it (its record then lies in the handle's
    // pinned block at the slot's index once the picture is collected)
    mi355enc_stabilize_t stab; bool stab_done;
    // automatic levels and white balance: what submit latched for this picture (al_on false: nothing) with the output range it met, and whether the step ran
    // for it (its record and table then lie in the handle's pinned block at the slot's index once the picture is collected); applied once, to the input's own
    // slot, in ingest_end
    mi355enc_autolevel_t al; bool al_on, al_done; int al_full;
    // the spatial noise filter: what submit latched for this picture (ds_on false: nothing) with the output range it met, and whether the estimate ran for it
    // (its record then lies in the handle's pinned block at the slot's index once the picture is collected); applied once, to the input's own slot, in ingest_end
    mi355enc_denoise_spatial_t ds; bool ds_on, ds_done; int ds_full;
    // the warp: what submit latched for this picture (warp_on false: nothing; warp_gen: the count of sets its mesh belongs to); warp_send: the slot's pinned copy
    // holds that mesh and it travels in front of the launch; applied once, to the input's own slot, first in ingest_end
    bool warp_on, warp_send; mi355enc_warp_t warp; unsigned warp_gen;
    // the 3D LUT: what submit latched for this picture (lut_on false: nothing; lut_gen: the count of sets its table belongs to) with the coefficients of the
    // output matrix and range it met; lut_send: the slot's pinned copy holds that table and it travels in front of the launch; applied once, to the input's own
    // slot, in ingest_end
    bool lut_on, lut_send; mi355enc_lut3d_t lut; unsigned lut_gen; int32_t lut_coef[LUT3D_COEF_WORDS];
    // region-of-interest quantisation: what enqueue_picture latched for this picture (roi_on false: no map, or an inactive one) -- the map's own pinned copy h_roi
    // (nmb + 16 bytes, allocated by the slot's first picture with a map), which the compose launch reads and nothing writes again before the picture is collected,
    // its background offset and the sum of its values; a recovery keeps all of it
    bool roi_on; int roi_bg, roi_sum; int8_t *h_roi;
    // the privacy masks: what the picture latched in front of its draw (mask_on: some region reaches the visible picture and the launches run; mask: the
    // configuration it carries, n 0 for none; mask_gen: the count of sets it belongs to) -- every output picture its own, drawn first in draw_and_enqueue
    bool mask_on; mi355enc_mask_t mask; unsigned mask_gen;
};

struct mi355enc {
    mi355enc_cfg_t cfg;
    int mbw, mbh, W, H, nmb;
    size_t ysz, csz;
    hipStream_t stream;                  // "back" stream: everything of a picture that needs the picture before it -- fused P stage / intra wavefront, deblocking
    hipStream_t fstream;                 // "front" stream: source upload / conversion, and for P pictures the whole-sample search, the vector selection
                                         // and the gated intra analysis (source against source: nothing of the previous picture's coding is needed, so
                                         // they run beside its deblocking)
    frame_ctx_t *d_ctx, *d_ctx2[NSET];   // one context per picture in flight; d_ctx = d_ctx2[0]
    slot_t *prev_slot;                   // slot of the picture enqueued last
    mb_info_t *d_mbi, *d_mbi_set[NSET];  // record/level sets: the hand-over of picture n overlaps the kernels of n+1 (and n+2)
    int16_t *d_levels, *d_levels_set[NSET];
    hipStream_t cstream;                 // hand-over stream (scan + pack into pinned host memory)
    bool pgate;                          // the fused P stage runs beside the previous picture's deblocking launch, gated per band (pgate_on(), latched at open())
    bool wait_room[2];                   // [0] P, [1] IDR pictures: the picture's deblocking launch leaves a quarter of an MI355X's 256 compute units free, so its workgroups may wait on the device for another kernel (latched at open())
    bool fip_rows;                       // the intra macroblock rows of a P picture ride in its deblocking launch (fip_on(), latched at open())
    uint64_t n_submitted;
    uint64_t sc_sum, sc_force_at; int sc_cnt, sc_prev_skip; // scene-cut recovery: summed cost / number of the P pictures since the last IDR; picture to force
    uint8_t *d_rec_y[2], *d_rec_uv[2], *d_pre_y, *d_pre_uv;
    uint8_t *d_dbrec;     // deblocking records, 64 B per macroblock
    uint8_t *d_idec;      // intra decisions, IDEC_BYTES per macroblock
    uint16_t *d_isad;     // intra analysis SADs, ISAD_PER_MB u16 per macroblock
    uint2 *d_ib_gran;     // the intra band kernel's bottom lines between bands (tagged granules)
    hipEvent_t ev_dbI[2];  // [reconstruction buffer]: the deblocking of an IDR picture that ran beside its intra wavefront on the intra stream has finished
    int dbI_busy[2];
    unsigned *d_db_par;   // the band deblocker's table of per-edge parameter words (written by its prologue, read by its movers)
    dev_words_t words;    // every word a kernel waits on, with the host's totals (enc_sync.hpp; the table: DESIGN.md section 5, "The wait words")
    uint2 *d_db_gran;     // strips between deblocking bands, as epoch-tagged granules (never cleared)
    unsigned *d_off;      // per-macroblock block offsets of the packed stream (scan kernel -> pack kernel)
    uint16_t *d_surf[NSET]; // SAD surfaces of the motion search, SURF_U16 per macroblock; one set per picture in flight: the front stages of picture n+1 (n+2) run beside the back stages of n
    imv_t *d_imv[NSET][3];   // whole-sample vector fields (search result / selection iterations alternate), per set
    uint8_t *d_idec2[NSET];  // intra decisions per set (d_idec = set 0)
    int8_t *d_qp_off[NSET];  // adaptive quantisation: QP offset per macroblock, per set (null unless cfg.aq_mode, or a picture with an active region-of-interest map has been submitted: enc_roi.cpp)
    uint8_t *d_psrc[2];   // padded source luma of the last two coded pictures: the search runs source against source
    int psrc_cur;         // which of them holds the last coded picture
    uint8_t *d_ip_strips;    // intra macroblocks of P pictures: the bottom lines they publish for the row below, IP_STRIP_BYTES per macroblock
    uint32_t epoch;
    int islice_rows, stage_slice_rows;   // rows per slice of an I picture (cfg.intra_slices; 0: one slice) / what the single-stage entry points use
    int pslice_rows, slice_dbf, stage_slice_dbf; // ... of a P picture (cfg.slices); disable_deblocking_filter_idc of every slice (cfg.slice_deblock: 0 or 2) / of the single-stage entry points
    hipStream_t ustream;       // host-to-device copies of the source pictures (pipeline_depth >= 1): a copy engine's queue, so that a picture's transfer runs beside the
                               // previous picture's search instead of in front of this one's; nullptr: the front stream carries them
    hipStream_t istream;       // intra_p_kernel of a P picture: beside prep + the band deblocker, which follows it row by row
    hipEvent_t ev_pmb;         // the fused P stage of the picture is done
    slot_t slot[NSLOT];
    int head, tail, pending;
    int cur, have_ref, frames_since_idr, idr_count, last_collected_rec;
    // periodic intra refresh (mi355enc_set_intra_refresh): on, the cycle position j of the next P picture, the first column not yet
    // refreshed in the current cycle, and an all-skip picture that rate control wanted for the last picture of a cycle and that moves to the next picture
    int ir_on, ir_pos, ir_R, ir_skip_owed;
    slot_t *last_slot;
    hipGraphExec_t g_intra[NSET], g_deblock[NSET]; // per context
    h264_writer_t *writer;
    rc_state_t rc;
    std::atomic<uint32_t> want_bps;
    std::atomic<int> fixed_qp, fixed_drop;
    mi355enc_stats_t st;
    double ms_open;
    uint64_t n_skip_pictures;
    // Degradation ladder of the device-side waits (collect(): recover()).  0: kernels may wait on the device for other kernels' progress
    // (what exclusive_device and a single encoder per process allow); 1: kernels run in stream order, the only waits left are those between the
    // workgroups of ONE persistent launch (bands of the intra wavefront / the deblocker); 2: one launch per wavefront step, no wait on the device at all.
    int safe_level;
    // the input size (mi355enc_set_input_size): in_w x in_h, = cfg.width x cfg.height unless the picture is scaled down on the way in (scaling; the
    // scale kernel then writes the coded-size surfaces instead of the copy / conversion), the SAR the scale makes (0:0 = square, no VUI field), the
    // tables on the device and where the kernel finds them
    int in_w, in_h, sar_w, sar_h;
    bool scaling;
    // orientation (mi355enc_set_orientation): the method, and whether mi355enc_set_input_size has been called (otherwise the input size
    // follows the method: the pre-orientation target pre_w() x pre_h())
    int orient;
    bool in_set;
    uint8_t *d_scale_tab; size_t scale_tab_bytes;
    scale_plan_t scale;
    // the input geometry (mi355enc_set_input_geometry / mi355enc_set_crop).  d_scale_tab then holds NSLOT copies of the tables, geom_room bytes
    // apart, one per slot: a picture in flight keeps the crop it was submitted under.  h_geom_tab (pinned): the slots' copies on their way to the device, then the
    // current tables (what `scale` describes; its table pointers are null, geom_off says where the tables lie in a copy), then set_crop's candidate.  geom_gen counts
    // the changes of the current tables; a slot whose geom_slot_gen differs gets them in front of its next launch (scale_plan_for).
    bool geom_on;
    mi355enc_geometry_t geom;
    uint8_t *h_geom_tab; size_t geom_room, geom_bytes, geom_off[2 * SCALE_TABLES];
    uint32_t geom_gen, geom_slot_gen[NSLOT];
    scale_plan_t geom_plan[NSLOT];
    // colorimetry (mi355enc_set_colorimetry): what every SPS says about the samples (0, 2, 2, 2: nothing), and the RGB -> Y'CbCr matrix that follows from it
    // (csc_coef: the ten words of mi355enc_csc_coefficients; csc_ok false: the matrix code is not one RGB input can be converted with)
    int col_full, col_prim, col_trc, col_mat;
    int csc_coef[10]; bool csc_ok;
    // what submitted YUV samples mean (mi355enc_set_input_colorimetry).  in_col_set: the call was made; yuv_on: the resolved input differs from
    // the resolved output, so every YUV picture takes the colour step (yuv_coef: the nine words of mi355enc_yuv_coefficients); yuv_bad: the call was made and the
    // output matrix is not one the step can convert to -- a YUV submit is refused
    bool in_col_set, yuv_on, yuv_bad;
    int in_col_full, in_col_mat, yuv_coef[9];
    // HDR input (mi355enc_set_hdr_input).  hdr_on: the call was made -- P010, I420_10 and V210 pictures are tone-mapped in their conversion
    // launch, every other input is refused.  h_hdr / d_hdr: the parameter block (HDR_WORDS words of mi355enc_hdr_tables) as built for the output (matrix, range)
    // hdr_key names, on the host and on the device; built and uploaded in front of the first conversion, on its stream (hdr_stream), and again only if the
    // output's colorimetry was changed since (before the first submit).  Nothing of this is allocated on a handle that never made the call.
    bool hdr_on = false, hdr_arrived = false; // hdr_arrived: a stream other than hdr_stream has waited for the upload, no later launch needs to
    int hdr_transfer = 0, hdr_full = 0, hdr_peak = 0, hdr_target = 0, hdr_key = -1;
    int32_t *h_hdr = nullptr, *d_hdr = nullptr;
    hipStream_t hdr_stream = nullptr;
    // picture controls (mi355enc_set_adjust): what the control thread set last (under adj_mu; submit latches it per input picture), what the
    // last collected picture carried, and the scratch luma plane of the stencil form (W x H bytes, allocated by the first sharpened picture; adj_bytes: its size), which
    // changes places with a slot's luma surface whenever the stencil has written all of it
    std::mutex adj_mu;
    adjust_set_t adj_cur = {}, adj_last = {};
    bool adj_last_have = false;
    uint8_t *d_adj = nullptr;
    size_t adj_bytes = 0;
    // temporal noise reduction (mi355enc_set_denoise): what the control thread set last (under dn_mu; submit latches it per input picture), what
    // the last collected picture carried, and the history -- one uint16 per luma / chroma sample of the coded surfaces, allocated by the first filtered picture
    // (dn_bytes: both sizes), written only by the step's launches, which follow one another on the upload stream.  dn_prev: the strengths of the previous picture
    // that went through the step ({0, 0}: none, or it was off) -- a plane whose strength was 0 there primes.  recover() touches none of this.
    // Motion compensation (section 25): d_dn_y / d_dn_uv are the current histories; a compensated launch reads them, writes d_dn_y_alt / d_dn_uv_alt and swaps
    // the pointers.  Those and d_dn_vec (a word per 8 x 8 block: the search's result) are allocated by the first picture that is filtered with a range above 0.
    std::mutex dn_mu;
    denoise_set_t dn_cur = {}, dn_last = {};
    bool dn_last_have = false;
    uint16_t *d_dn_y = nullptr, *d_dn_uv = nullptr, *d_dn_y_alt = nullptr, *d_dn_uv_alt = nullptr;
    unsigned *d_dn_vec = nullptr;
    size_t dn_bytes = 0;
    mi355enc_denoise_t dn_prev = {0, 0};
    // electronic image stabilisation (mi355enc_set_stabilize): what the control thread set last (under stab_mu; submit latches it per input
    // picture) and what the last collected picture carried.  d_stab (one block, allocated by the first stabilised picture for the input size stab_w x stab_h;
    // stab_bytes: its size): the trajectory {Sx, Sy}, a record of STAB_REC_WORDS words per slot and one for the stage calls, then the two halves of the
    // projection buffer (4 (in_w + in_h) words each); h_stab: the records' pinned copies.  stab_half: the half the next picture's sums go into (the other one
    // holds the previous picture's); stab_primed false: the next stabilised picture primes.  Written only by launches that follow one another on the upload stream.
    std::mutex stab_mu;
    mi355enc_stabilize_t stab_cur = {0, 16, 0, 0}, stab_last = {0, 16, 0, 0};
    mi355enc_stabilize_info_t stab_last_info = {};
    bool stab_last_have = false, stab_primed = false;
    int *d_stab = nullptr, *h_stab = nullptr;
    size_t stab_bytes = 0;
    int stab_half = 0, stab_w = 0, stab_h = 0;
    // automatic levels and white balance (mi355enc_set_autolevel): what the control thread set last (under al_mu; submit latches it per
    // input picture) and what the last collected picture carried.  d_al (one block, allocated by the first autolevelled picture; al_bytes: its size): the state
    // {Lo, Hi, Du, Dv} (and four words of room), AL_SLOT_WORDS words per slot and for the stage calls (record, table), then AL_SLABS_MAX slabs; h_al: the
    // slots' pinned copies.  al_primed false: the next autolevelled picture primes.  Written only by launches that follow one another on one stream.
    std::mutex al_mu;
    mi355enc_autolevel_t al_cur = {0, 0, 16, 50, 50, 2000, 48}, al_last = {0, 0, 16, 50, 50, 2000, 48};
    mi355enc_autolevel_info_t al_last_info = {};
    uint8_t al_last_tab[256] = {};
    bool al_last_have = false, al_primed = false;
    int *d_al = nullptr, *h_al = nullptr;
    size_t al_bytes = 0;
    int al_time_n = 0; // (mi355enc_time_stage 32 .. 34: the slabs its prepare left)
    // the spatial noise filter (mi355enc_set_denoise_spatial): what the control thread set last (under ds_mu; submit latches it per input
    // picture) and what the last collected picture carried.  d_ds (one block, allocated by the first picture that is measured): the state X (and seven words of
    // room), DS_REC_WORDS words per slot and for the stage calls, DS_SLABS_MAX slabs, then the 33 tables R_s; h_ds: the slots' pinned records.  d_ds_y / d_ds_uv:
    // the scratch planes the filter launches write (allocated by the first picture whose plane is filtered), which then change places with the slot's.  ds_bytes:
    // all of it.  ds_primed false: the next measured picture primes.  Written only by launches that follow one another on one stream.
    std::mutex ds_mu;
    mi355enc_denoise_spatial_t ds_cur = {0, 0, 0, 25, 32}, ds_last = {0, 0, 0, 25, 32};
    mi355enc_denoise_spatial_info_t ds_last_info = {};
    bool ds_last_have = false, ds_primed = false;
    int *d_ds = nullptr, *h_ds = nullptr;
    uint8_t *d_ds_y = nullptr, *d_ds_uv = nullptr;
    size_t ds_bytes = 0;
    // lens, roll and keystone correction (mi355enc_set_warp / mi355enc_set_warp_mesh): what the control thread set last (under warp_mu: the
    // setting, its mesh of the coded visible size on the heap, the count of sets that turned it on; submit latches it per input picture) and what the last
    // collected picture carried.  Allocated by the first warped picture: the scratch pair d_warp_y / d_warp_uv (the launch writes it, then the slot and the handle
    // exchange planes), the mesh on the device and one pinned copy per slot (h_warp_mesh); warp_sent: the generation d_warp_mesh holds once the upload stream
    // has come that far (0: none).  Touched by the submitting thread only, apart from what warp_mu guards.
    std::mutex warp_mu;
    bool warp_on = false;
    mi355enc_warp_t warp_cur = {};
    int32_t *warp_mesh = nullptr;
    unsigned warp_gen = 0, warp_sent = 0, warp_last_gen = 0;
    bool warp_last_have = false;
    uint8_t *d_warp_y = nullptr, *d_warp_uv = nullptr;
    int32_t *d_warp_mesh = nullptr, *h_warp_mesh = nullptr;
    size_t warp_bytes = 0;
    // the 3D colour LUT (mi355enc_set_lut3d): what the control thread set last (under lut_mu: the setting, its table on the heap, the count of
    // sets that turned it on; submit latches it per input picture) and what the last collected picture carried.  Allocated by the first graded picture, for 65^3
    // nodes whatever the size set: d_lut (the table the launches read; lut_sent: the generation it holds, or will hold by the order of the upload stream) and h_lut
    // (pinned: one table per slot).  lut_bytes: the device bytes.
    std::mutex lut_mu;
    bool lut_on = false;
    mi355enc_lut3d_t lut_cur = {0, 0}, lut_last = {0, 0};
    uint32_t *lut_nodes = nullptr;
    unsigned lut_gen = 0, lut_sent = 0, lut_last_gen = 0;
    bool lut_last_have = false;
    uint32_t *d_lut = nullptr, *h_lut = nullptr;
    size_t lut_bytes = 0;
    int lut_form = -1; // (mi355enc_debug_lut3d_form: the launch form of the handle's own launches; -1: the plan's)
    // region-of-interest quantisation (mi355enc_set_roi): what the control thread set last (under roi_mu: the configuration, the map t it
    // stands for on the heap -- nmb bytes, kept from the first set on --, whether it is active, its background offset and sum; enqueue_picture latches it per
    // picture) and what the last collected picture carried.  The offsets themselves are d_qp_off's: without aq_mode the first picture with an active map
    // allocates the sets (roi_bytes: those bytes).  roi_stage: the map of the single-stage entry points (mi355enc_roi_probe_set_map; null: none).
    std::mutex roi_mu;
    std::atomic<bool> roi_set{false}; // (read without the mutex by every enqueue_picture: a handle the setter was never called on takes no lock per picture)
    bool roi_active = false;
    mi355enc_roi_t roi_cur = {};
    int8_t *roi_map = nullptr, *roi_stage = nullptr;
    int roi_bg = 0, roi_sum = 0;
    bool roi_last_have = false;
    int roi_last_active = 0, roi_last_bg = 0, roi_last_sum = 0;
    size_t roi_bytes = 0;
    // privacy masks (mi355enc_set_mask): what the control thread set last (under mask_mu; every drawn picture latches it) and what the last
    // collected picture carried.  d_mask: the result surface and the two ping-pong planes, a coded picture each, allocated by the first masked picture (mask_bytes)
    // and used on the upload stream alone (the probe and the timed stages: on the main stream, with nothing in flight).
    std::mutex mask_mu;
    std::atomic<bool> mask_set{false}; // (read without the mutex by every latch: a handle the setter was never called on takes no lock per picture)
    bool mask_on = false;
    mi355enc_mask_t mask_cur = {}, mask_last = {};
    unsigned mask_gen = 0, mask_last_gen = 0;
    bool mask_last_have = false;
    uint8_t *d_mask = nullptr;
    size_t mask_bytes = 0;
    bool warp_staging = true; // (mi355enc_debug_warp_staging: false -- every workgroup of the launch takes the direct form)
    // frame-rate conversion (mi355enc_set_rate_conversion).  rate.mode 0: off, and nothing below is used but last_count.  rate.max_fill is
    // clamped to pipeline_depth.  rate_plan: the rule's state; ingest_begin steps a copy of it (rate_next, with what the step yields: rate_n pictures, their pts
    // and weights) and ingest_end commits it once the pictures are enqueued -- a submit that fails in between has not advanced the plan.  d_keep: one NV12
    // picture of the coded size (luma, then chroma at ysz): blend -- the previous input after the colour step; hold with max_fill > 0 -- the previous output
    // picture before layers and text.  rate_idr_owed: the force_idr of submits that yielded no picture.  last_count: pictures the last successful submit enqueued.
    mi355enc_rate_t rate = {};
    mi355enc_rate_plan_t rate_plan = {}, rate_next = {};
    int rate_n = 0, rate_resync = 0, rate_w[MI355ENC_RATE_MAX_OUT] = {};
    int64_t rate_pts[MI355ENC_RATE_MAX_OUT] = {};
    int rate_idr_owed = 0, last_count = 0;
    uint8_t *d_keep = nullptr;
    mi355enc_rate_stats_t rate_st = {};
    uint32_t n_recoveries, last_error_word;
    // quality metrics (mi355enc_set_quality_metrics; everything null / 0 while they are off and no stage call has asked for them):
    // per slot, and one more for the single-stage entry points, a block of QUALITY_WORDS accumulator words on the device and of result words in pinned
    // host memory (the launch's last workgroup writes them); per slot the event behind the launch, which collect() waits for
    bool q_on;
    unsigned long long *d_qacc, *h_qres;
    hipEvent_t ev_q[NSLOT];
    mi355enc_quality_t q_last, q_tot; // the last collected picture's / the integer sums since open or reset_stats
    bool q_have;
    // text overlay (mi355enc_set_overlay_text / _style): what the control thread set last (under ov_mu; submit latches it per picture),
    // and the text of the last collected picture
    std::mutex ov_mu;
    int ov_len; char ov_text[256]; mi355enc_overlay_style_t ov_style;
    int ov_last_have, ov_last_len; char ov_last[256];
    // image layers (mi355enc_set_image / _set_image_place): per layer the image the control thread set last, its place, opacity and serial
    // (under img_mu; submit latches them per picture), every buffer made so far (those of retired images wait there for the next upload; freed at close), the
    // device bytes held, and what the last collected picture carried
    std::mutex img_mu;
    image_t *img_cur[MI355ENC_IMAGE_LAYERS]; int img_x[MI355ENC_IMAGE_LAYERS], img_y[MI355ENC_IMAGE_LAYERS], img_op[MI355ENC_IMAGE_LAYERS]; uint32_t img_serial[MI355ENC_IMAGE_LAYERS];
    image_buf_t *img_bufs;
    size_t img_dev_bytes;
    mi355enc_image_info_t img_last[MI355ENC_IMAGE_LAYERS];
    // stills: the request the control thread made last (armed: the next submitted picture takes it), the blocks, the ready one (-1: none),
    // all under snap_mu; per slot the event behind its still's launch, which collect() waits for (created with the first armed picture); recovering: recover()
    // is enqueueing the pictures in flight again (they keep their blocks)
    std::mutex snap_mu;
    std::atomic<bool> snap_armed; // (read without the mutex by every enqueue_picture: with no request the picture path takes no lock)
    bool recovering;
    mi355enc_snapshot_req_t snap_req, snap_last_req;
    snap_block_t snap_blk[SNAP_BLOCKS];
    int snap_ready;
    std::atomic<size_t> snap_bytes;
    hipEvent_t ev_snap[NSLOT];
    // the entropy-coding worker (started by open() when pipeline_depth >= 1)
    std::thread wk;
    std::mutex wk_mu;
    std::condition_variable wk_cv, wk_done_cv;
    int wk_q[NSLOT + 1], wk_qh, wk_qt;
    bool wk_stop, wk_on;
    size_t au_cap;
    // staging helpers (pageable host input at pipeline_depth >= 1): the pieces of a picture are copied into the slot's pinned buffer by the caller and
    // two helper threads side by side, each piece transferred as soon as it is staged; submit() returns when all of them are on their way
    struct stage_job { const uint8_t *src; uint8_t *dst, *dev; int src_stride, rows, width; size_t dst_stride; };
    std::thread stg_th[2];
    std::mutex stg_mu;
    std::condition_variable stg_cv, stg_done_cv;
    stage_job stg_job[8];
    int stg_n, stg_next, stg_done, stg_err;
    unsigned long long stg_gen;
    bool stg_stop, stg_on;
};
void stage_helper(mi355enc_t *h);
// mi355enc_time_stage (enc_stages.cpp): what a stage's preparation hands to its launches (14: the scale plan, 15: the image arguments); the features' *_time_* hooks have the signatures of its table's rows
struct ts_ctx_t { int stage; const scale_plan_t *scale; image_args_t img; };

static inline double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// enc_handle.cpp
extern std::atomic<int> g_open_encoders;
bool exclusive_device(const mi355enc_t *h);
bool pgate_on(int nmb);
bool fip_on(int nmb);
bool overlap_allowed(const mi355enc_t *h);
int sync_compute(mi355enc_t *h);
bool host_range_pinned(const void *p, size_t bytes); // inside memory handed out by mi355enc_host_alloc()
// enc_schedule.cpp
int run_intra(mi355enc_t *h, int ci, const frame_ctx_t *hc, unsigned *band_done = nullptr);
int run_pmb(mi355enc_t *h, const frame_ctx_t *hc, int refine, const pic_plan_t &plan, hipStream_t st); // the fused P stage as the plan gates it, booked (the default plan: in order)
int run_deblock(mi355enc_t *h, int ci, const frame_ctx_t *hc, const pic_plan_t &plan = pic_plan_t(), int rec = -1); // (the defaults: in order on the main stream, no band-done words)
void fill_ctx(mi355enc_t *h, frame_ctx_t *c, int qp, int drop, int idr, int set = 0, int roi = 0); // roi: the picture carries an active region-of-interest map
int enqueue_picture(mi355enc_t *h, slot_t *s, const uint8_t *src_y, const uint8_t *src_uv, int src_stride, int64_t pts, int force_idr);
void entropy_worker(mi355enc_t *h);
// enc_input.cpp
int upload_and_convert(mi355enc_t *h, slot_t *s, int fmt, const uint8_t *const planes[3], const int strides[3], hipStream_t up);
// a picture of the input size tightly into the slot's raw staging buffer (any format); p / st: where its planes lie on the device then
int upload_raw(mi355enc_t *h, slot_t *s, int fmt, const uint8_t *const planes[3], const int strides[3], hipStream_t up, const uint8_t *p[3], int st[3]);
// enc_scale.cpp
size_t raw_bytes(const mi355enc_t *h); // size of a slot's raw staging buffer
// enc_quality.cpp
int quality_alloc(mi355enc_t *h);   // the accumulator and result blocks (idempotent)
void quality_free(mi355enc_t *h);
// the picture of slot s: source (src_y, src_uv, src_stride) against reconstruction buffer `rec`, behind everything enqueued on st so far; records the slot's event
int quality_enqueue(mi355enc_t *h, slot_t *s, const uint8_t *src_y, const uint8_t *src_uv, int src_stride, int rec, hipStream_t st);
int quality_collect(mi355enc_t *h, slot_t *s); // waits for the slot's metrics, books them as the last picture's and into the totals
// one launch on the handle's main stream with the block of the stage entry points, waited for
int quality_run(mi355enc_t *h, const uint8_t *src_y, const uint8_t *src_uv, int src_stride, const uint8_t *rec_y, const uint8_t *rec_uv, mi355enc_quality_t *q);
// The input steps' hooks, as the rows of k_steps (enc_input.cpp) name them, in chain order.  One signature per kind, whatever the step:
//   latch      the value set last becomes the slot's; own: the slot the step is applied on, which also takes a new table or mesh (a per-output step is always
//              called with true).  stab_latch refuses there: ERR_STATE without a geometry, ERR_ARG for an input below 4 range; image_latch: ERR_ARG for an
//              active layer and a matrix RGB cannot be converted with; every other answer but OK is an allocation's
//   draw       the slot's step on its coded surfaces, behind everything enqueued on st so far; nothing where the slot latched none
//   collected  collect(): books what the picture carried as the last picture's (image_collected lets go of the slot's images)
//   free       close(): everything of the step (lut3d_close, warp_close: the heap table the latch reads too)
int stab_latch(mi355enc_t *h, slot_t *s, bool own); void stab_collected(mi355enc_t *h, slot_t *s); void stab_free(mi355enc_t *h);
int warp_latch(mi355enc_t *h, slot_t *s, bool own); int warp_draw(mi355enc_t *h, slot_t *s, hipStream_t st); void warp_collected(mi355enc_t *h, slot_t *s); void warp_close(mi355enc_t *h);
int yuv_draw(mi355enc_t *h, slot_t *s, hipStream_t st);
int dspatial_latch(mi355enc_t *h, slot_t *s, bool own); int dspatial_draw(mi355enc_t *h, slot_t *s, hipStream_t st); void dspatial_collected(mi355enc_t *h, slot_t *s); void dspatial_free(mi355enc_t *h);
int denoise_latch(mi355enc_t *h, slot_t *s, bool own); int denoise_draw(mi355enc_t *h, slot_t *s, hipStream_t st); void denoise_collected(mi355enc_t *h, slot_t *s); void denoise_free(mi355enc_t *h);
int lut3d_latch(mi355enc_t *h, slot_t *s, bool own); int lut3d_draw(mi355enc_t *h, slot_t *s, hipStream_t st); void lut3d_collected(mi355enc_t *h, slot_t *s); void lut3d_close(mi355enc_t *h);
int autolevel_latch(mi355enc_t *h, slot_t *s, bool own); int autolevel_draw(mi355enc_t *h, slot_t *s, hipStream_t st); void autolevel_collected(mi355enc_t *h, slot_t *s); void autolevel_free(mi355enc_t *h);
int adjust_latch(mi355enc_t *h, slot_t *s, bool own); int adjust_draw(mi355enc_t *h, slot_t *s, hipStream_t st); void adjust_collected(mi355enc_t *h, slot_t *s); void adjust_free(mi355enc_t *h);
int mask_latch(mi355enc_t *h, slot_t *s, bool own); int mask_draw(mi355enc_t *h, slot_t *s, hipStream_t st); void mask_collected(mi355enc_t *h, slot_t *s); void mask_free(mi355enc_t *h);
int image_latch(mi355enc_t *h, slot_t *s, bool own); int image_draw(mi355enc_t *h, slot_t *s, hipStream_t st); void image_collected(mi355enc_t *h, slot_t *s); void image_free(mi355enc_t *h);
int overlay_latch(mi355enc_t *h, slot_t *s, bool own); int overlay_draw(mi355enc_t *h, slot_t *s, hipStream_t st);
#pragma GCC visibility push(hidden)
void overlay_collected(mi355enc_t *h, slot_t *s);
int yuv_run(mi355enc_t *h, slot_t *s, hipStream_t st); // the colour step's launch whatever the slot latched: the stage entry points'
#pragma GCC visibility pop
// enc_image.cpp
static inline bool image_active(const slot_t *s) { for (int l = 0; l < MI355ENC_IMAGE_LAYERS; l++) if (s->img[l] && s->img_op[l]) return true; return false; }
int image_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *x); // mi355enc_time_stage 15: layer 0's image on the device, the launch's arguments (x->img) at its current place; ERR_STATE without one
// enc_scale.cpp
// the one place the input geometry of a handle is decided (both setters end here): validates, then rebuilds tables, sizes, SAR and staging buffers; ERR_ARG leaves the handle as it was
int geometry_apply(mi355enc_t *h, int orient, bool in_set, int in_w, int in_h, const mi355enc_geometry_t *geom = nullptr); // geom: the geometry in place of an input size
// the plan the scale launch of slot s's picture runs with, on stream `up` (with a geometry: the slot's copy of the tables, brought up to date in stream order); null: HIP error
const scale_plan_t *scale_plan_for(mi355enc_t *h, slot_t *s, hipStream_t up);
void scale_free(mi355enc_t *h); // the tables, on the device and pinned
// enc_orient.cpp
static inline bool orient_transposes(int m) { return m == MI355ENC_ORIENT_90R || m == MI355ENC_ORIENT_90L || m == MI355ENC_ORIENT_UL_LR || m == MI355ENC_ORIENT_UR_LL; }
static inline int pre_w(const mi355enc_t *h) { return orient_transposes(h->orient) ? h->cfg.height : h->cfg.width; } // the pre-orientation target: what decode / conversion / scale produce
static inline int pre_h(const mi355enc_t *h) { return orient_transposes(h->orient) ? h->cfg.width : h->cfg.height; }
// Where the step in front of the orientation writes its NV12 picture, and with what sizes: the slot's coded surfaces (identity: stride W, visible cfg size, margin up
// to W x H), or the slot's pre-orientation picture (visible size only: W = its stride, H = its height).  Every submit path asks here ...
struct in_target_t { uint8_t *y, *uv; int vw, vh, W, H; };
int input_target(mi355enc_t *h, slot_t *s, in_target_t *t);
// ... and ends here: with a method, the orientation launch from (src_y, src_uv; null: the slot's pre-orientation picture) into the slot's coded surfaces (nothing with identity)
int input_finish(mi355enc_t *h, slot_t *s, hipStream_t up, const uint8_t *src_y = nullptr, int y_stride = 0, const uint8_t *src_uv = nullptr, int uv_stride = 0);
void orient_free(slot_t *s);
// enc_input.cpp, what the other files share with it (these stay inside the library: the shared object exports what it did)
#pragma GCC visibility push(hidden)
// The planes of a w x h picture in `fmt`: how many, and per plane the bytes of a row and the rows.  0: not a format (YV12 is I420 once its planes are exchanged).
// The one description every upload and every validation of caller-owned planes goes by.
struct fmt_plane_t { int row, rows; };
int fmt_planes(int fmt, int w, int h, fmt_plane_t pl[3]);
bool planes_fit(int n, const fmt_plane_t pl[3], const uint8_t *const planes[3], const int strides[3]); // each of the n planes is there and its stride holds a row
int yv12_as_i420(int fmt, const uint8_t *p[3], int st[3]); // YV12 is I420 with V before U: exchanges the two planes and answers I420 (the only exchange); any other format as it is
// the two-launch form: the slot's NV12 picture of the input size (allocated on first use), which a conversion or decode launch writes, and the scale launch from
// such a picture into the input target with the slot's plan (k_launch_scale's answer)
struct nv12_pic_t { uint8_t *y, *uv; int stride; };
int input_nv12(mi355enc_t *h, slot_t *s, nv12_pic_t *c);
int scale_nv12(mi355enc_t *h, slot_t *s, const nv12_pic_t *c, const in_target_t *t, const scale_plan_t *pl, hipStream_t up);
// the planes' layout at rows of 16 n bytes, one behind the other from d on (a slot's raw staging buffer): where each lies and its stride -> the number of planes
int raw_layout(int fmt, int w, int h, const uint8_t *d, const uint8_t *p[3], int st[3], fmt_plane_t pl[3]);
// the walks over k_steps that other files need: some step changes the slot's picture (the in-place exit's test), collect()'s bookings, close()'s frees
bool steps_active(const slot_t *s);
void steps_collected(mi355enc_t *h, slot_t *s);
void steps_free(mi355enc_t *h);
#pragma GCC visibility pop
// enc_jpeg.cpp
int jpeg_alloc(mi355enc_t *h, slot_t *s);  // the slot's coefficient buffers (idempotent)
void jpeg_free(slot_t *s);
int jpeg_decode_host(mi355enc_t *h, slot_t *s, const uint8_t *data, size_t len, mi355enc_jpeg_info_t *info); // parse, check the size, entropy decode into the slot's pinned buffer
int jpeg_enqueue(mi355enc_t *h, slot_t *s, const mi355enc_jpeg_info_t *info, hipStream_t up);               // transfer + launch (+ scale) into the slot's staging surfaces
int jpeg_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x);
// enc_snapshot.cpp
void snapshot_latch(mi355enc_t *h, slot_t *s);  // enqueue_picture of a newly submitted picture: an armed request becomes the slot's, with a block to land in
// the slot's still from NV12 planes (the source, or the reconstruction) behind everything enqueued on st so far; records the slot's event
int snapshot_enqueue(mi355enc_t *h, slot_t *s, const uint8_t *y, const uint8_t *uv, int stride, hipStream_t st);
int snapshot_collect(mi355enc_t *h, slot_t *s); // waits for the slot's still and makes it the ready one
int snapshot_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *x); // mi355enc_time_stage 16: the stage block and its tables
int snapshot_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x);
void snapshot_init(mi355enc_t *h);
void snapshot_free(mi355enc_t *h);
// enc_csc.cpp
void csc_resolve(mi355enc_t *h); // fills csc_coef / csc_ok from col_mat, col_full and the coded size, and what the colour step follows from them
static inline bool fmt_is_rgb(int fmt) { return fmt >= MI355ENC_FMT_BGRX && fmt <= MI355ENC_FMT_RGB; }
// (the colour step, yuv_draw / yuv_run: the picture part -- with a geometry the oriented destination rectangle -- is converted in place, the border keeps its bytes)
void yuv_rect(const mi355enc_t *h, int rect[4]); // that picture part: x0, x1, y0, y1 in the coded surfaces (reaching their edge where it reaches the visible picture's)
// enc_adjust.cpp (picture controls)
void adjust_retable(mi355enc_t *h);                          // mi355enc_set_colorimetry: the current value's tables again, for the new output range
bool adjust_time_ready(mi355enc_t *h, int stage);            // mi355enc_time_stage 23 / 24: the value set last is active and of that form (24: the stencil form)
int adjust_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x); // ... and its launches on the main stream
// enc_denoise.cpp (temporal noise reduction)
bool denoise_time_ready(mi355enc_t *h, int stage);           // mi355enc_time_stage 25 .. 28: the value set last is active (27 / 28: with a range above 0)
int denoise_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x); // ... and its launch on the main stream: 25 filtering in place (priming where the history is not valid), 26 priming, 27 the search alone, 28 search and compensated filter
void denoise_time_done(mi355enc_t *h);                       // ... behind the timed launches: the history they left is no stream's, the next picture primes
// enc_stab.cpp (electronic image stabilisation)
// The one place a scale / geometry launch of a picture is enqueued (every submit path and mi355enc_stage_scale end here): with the slot stabilised, the estimate
// (clear, projection launch, match launch, the record's copy to pinned memory) in front of it on the same stream, and the launch reads the offset the match
// launch wrote.  An MI355ENC_* code
int input_scale(mi355enc_t *h, slot_t *s, int fmt, const uint8_t *p0, const uint8_t *p1, const uint8_t *p2, int s0, int s1, int s2, const in_target_t *t, const scale_plan_t *pl, hipStream_t up);
bool stab_time_ready(mi355enc_t *h, int stage);              // mi355enc_time_stage 29 / 30: the value set last is on, and the handle has a geometry of a size it takes
int stab_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *x);
int stab_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x); // 29 the clear and the projection launch on the raw staging buffer, 30 the match launch
void stab_time_done(mi355enc_t *h);                          // ... behind the timed launches: the next picture primes
// enc_autolevel.cpp (automatic levels and white balance)
bool autolevel_time_ready(mi355enc_t *h, int stage);         // mi355enc_time_stage 32 .. 34: the value set last is on
int autolevel_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *x); // the block, and a measure and a (priming) decide launch on slot 0's surfaces
int autolevel_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x); // 32 measure, 33 decide, 34 apply
void autolevel_time_done(mi355enc_t *h);                     // ... behind the timed launches: the next picture primes
// enc_dspatial.cpp (the spatial noise filter and its noise estimate)
bool dspatial_time_ready(mi355enc_t *h, int stage);          // mi355enc_time_stage 36 / 37: the value set last is on and manual / automatic
int dspatial_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x); // 36 the filter launches, 37 measure, decide and the filter launches
void dspatial_time_done(mi355enc_t *h);                      // ... behind the timed launches: the next picture primes
// enc_lut3d.cpp (3D colour LUT)
bool lut3d_time_ready(mi355enc_t *h, int stage);             // mi355enc_time_stage 35: the value set last is on
int lut3d_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *x); // the table set last onto the device
int lut3d_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x);
void lut3d_time_done(mi355enc_t *h);                         // ... behind the timed launches: the next graded picture sends its table again
// enc_roi.cpp (region-of-interest quantisation)
int roi_latch(mi355enc_t *h, slot_t *s);                     // enqueue_picture of a newly submitted picture: the map set last becomes the slot's, in its pinned copy (an active one: the offset sets exist from here on)
void roi_compose(mi355enc_t *h, const slot_t *s, int set, hipStream_t st); // the slot's map and (aq_mode) what aq_kernel left in d_qp_off[set] -> the picture's offsets there, behind everything enqueued on st so far
int roi_stage_ctx(mi355enc_t *h, frame_ctx_t *c);            // a single-stage call's context: one QP per picture, or the probe's map on its way into d_qp_off[0] on the main stream
void roi_collected(mi355enc_t *h, slot_t *s);                // collect(): books what the picture carried as the last picture's
void roi_free(mi355enc_t *h);
// enc_mask.cpp (privacy masks)
bool mask_time_ready(mi355enc_t *h, int stage);              // mi355enc_time_stage 38 / 39: the value set last holds a fill or pixelate / a blur region
int mask_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *x); // the surfaces, and the value set last as slot 0's
int mask_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x); // 38 the pixelate and commit launches, 39 the blur launches
// enc_warp.cpp (lens, roll and keystone correction)
bool warp_time_ready(mi355enc_t *h, int stage);              // mi355enc_time_stage 31: the warp is on
int warp_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *x);
int warp_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *x);
void warp_time_done(mi355enc_t *h);
// enc_hdr.cpp (HDR input)
// true: the handle tone-maps and this input is not one it takes (a format other than the three 10-bit ones -- fmt -1: an entry point that takes none of them --
// or an output matrix outside 1, 5, 6, 2): the submit fails with MI355ENC_ERR_ARG before anything is latched
bool hdr_refuses(const mi355enc_t *h, int fmt);
// the conversion launch of a 10-bit picture on a handle with hdr_on, in the place of k_launch_csc2 (same arguments); the block travels in front of the first one
int hdr_convert(mi355enc_t *h, int fmt, const uint8_t *const p[3], const int st[3], uint8_t *dy, uint8_t *duv, int vw, int vh, int W, int H, hipStream_t s);
void hdr_free(mi355enc_t *h);
// enc_rate.cpp (frame-rate conversion; every one of them is called with conversion on only)
#pragma GCC visibility push(hidden)
#define INGEST_DROP 1 /* ingest_begin's answer for a submit that yields no picture and needs no transfer (hold mode): the submit returns MI355ENC_OK at once */
// ingest_begin: steps a copy of the plan for an input at pts.  ERR_STATE with fewer free slots than the step needs (nothing has changed); INGEST_DROP: the input
// is dropped and booked; otherwise *ahead = pictures in front of the input's own (their slots follow the queue's head, the input goes into the slot behind them)
int rate_begin(mi355enc_t *h, int64_t pts, int force_idr, int *ahead);
int rate_keep(mi355enc_t *h, slot_t *s, hipStream_t st);                       // the slot's surfaces -> the keep buffer (nothing without one)
int rate_repeat(mi355enc_t *h, slot_t *t, hipStream_t st);                     // the keep buffer -> the slot's surfaces
int rate_mix(mi355enc_t *h, slot_t *b, slot_t *out, int w256, bool keep, hipStream_t st); // keep buffer x slot b -> slot out; keep: b replaces the keep buffer (out == b)
void rate_commit(mi355enc_t *h, int force_idr);                                // ingest_end: the step's pictures are enqueued (or it yields none): plan and statistics advance
void rate_free(mi355enc_t *h);
#pragma GCC visibility pop
#include "enc_stage.hpp"
#endif
