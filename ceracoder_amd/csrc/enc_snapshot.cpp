// enc_snapshot.cpp -- JPEG stills of the running stream: the request, the blocks of pinned host memory the device's levels land in, the
// launch of k_snapshot.hip in a picture's pipeline (enc_schedule.cpp says where), what collect() does with it, the take -- the Huffman coding, in the taker's
// thread (snapshot_host.c) -- and the single-stage entry points.
#include "enc_internal.hpp"

static int log2_reduce(int r) { return r == 1 ? 0 : r == 2 ? 1 : r == 4 ? 2 : r == 8 ? 3 : -1; }
static bool req_valid(const mi355enc_snapshot_req_t *q) { return q && (q->what == 0 || q->what == 1) && log2_reduce(q->reduce) >= 0 && q->quality >= 1 && q->quality <= 100; }

static int16_t *blk_levels(const snap_block_t *b) { return (int16_t *)(b->h_mem + SNAP_TAB_BYTES); }
static uint8_t *blk_hint(const snap_block_t *b) { return b->h_mem + SNAP_TAB_BYTES + b->nblk * 64 * sizeof(int16_t); }

void snapshot_init(mi355enc_t *h) {
    h->snap_armed.store(false); h->recovering = false; h->snap_ready = -1; h->snap_bytes.store(0);
    h->snap_req = h->snap_last_req = {0, 1, 75};
    memset((void *)h->snap_blk, 0, sizeof h->snap_blk);
    for (int i = 0; i < NSLOT; i++) h->ev_snap[i] = nullptr;
}
void snapshot_free(mi355enc_t *h) {
    for (snap_block_t &b : h->snap_blk) {
        if (b.h_mem) (void)hipHostFree(b.h_mem);
        if (b.d_tab) (void)hipFree(b.d_tab);
        b.h_mem = nullptr; b.d_tab = nullptr; b.cap = 0;
    }
    for (int i = 0; i < NSLOT; i++) if (h->ev_snap[i]) { (void)hipEventDestroy(h->ev_snap[i]); h->ev_snap[i] = nullptr; }
    h->snap_bytes.store(0);
}

static size_t block_bytes(int ow, int oh) {
    int bw[3], bh[3];
    size_t first[3];
    return SNAP_TAB_BYTES + snapshot_host_blocks(ow, oh, bw, bh, first) * (64 * sizeof(int16_t) + 1);
}
// Room, tables and sizes of a still of a w x ht picture in block b (which nothing else uses at this moment).  room_w x room_h: the still the block is sized for
// when it is allocated -- a picture's block takes the handle's picture at reduction 1 at its first use, so that no later still, whatever its reduction, allocates
// or frees on the submit path again; the stage entry points' block grows with the planes they are given.
static int block_prepare(mi355enc_t *h, snap_block_t *b, int w, int ht, int reduce, int quality, int room_w, int room_h) {
    int bw[3], bh[3];
    size_t first[3];
    b->ow = (w + reduce - 1) / reduce; b->oh = (ht + reduce - 1) / reduce;
    b->nblk = snapshot_host_blocks(b->ow, b->oh, bw, bh, first);
    size_t need = block_bytes(b->ow, b->oh);
    if (b->cap < need) {
        const size_t room = block_bytes(room_w, room_h);
        if (room > need) need = room;
        if (b->h_mem) { (void)hipHostFree(b->h_mem); b->h_mem = nullptr; h->snap_bytes.fetch_sub(b->cap); b->cap = 0; }
        HIPCHK(hipHostMalloc((void **)&b->h_mem, need, hipHostMallocDefault));
        b->cap = need; h->snap_bytes.fetch_add(need);
    }
    if (!b->d_tab) { HIPCHK(hipMalloc(&b->d_tab, SNAP_TAB_BYTES)); h->snap_bytes.fetch_add(SNAP_TAB_BYTES); }
    static_assert(sizeof(snapshot_tab_t) <= SNAP_TAB_BYTES, "the table leads the block");
    if (mi355enc_snapshot_tables(quality, b->qt)) return MI355ENC_ERR_ARG;
    snapshot_host_tab(b->qt, (snapshot_tab_t *)b->h_mem);
    return MI355ENC_OK;
}
// the table's transfer (1 KB, in stream order in front of the launch) and the launch, on st
static int block_table(snap_block_t *b, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(b->d_tab, b->h_mem, sizeof(snapshot_tab_t), hipMemcpyHostToDevice, st));
    return MI355ENC_OK;
}
static int block_launch(snap_block_t *b, const uint8_t *y, int ys, const uint8_t *uv, int uvs, int w, int ht, int reduce, hipStream_t st) {
    if (k_launch_snapshot(y, ys, uv, uvs, w, ht, log2_reduce(reduce), b->d_tab, blk_levels(b), blk_hint(b), st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}

void snapshot_latch(mi355enc_t *h, slot_t *s) {
    if (!s->snap && !h->snap_armed.load(std::memory_order_acquire)) return; // no request: no lock, nothing else
    std::lock_guard<std::mutex> g(h->snap_mu);
    if (s->snap) { h->snap_blk[s->snap - 1].state = 0; s->snap = 0; } // (left behind by a submit that failed)
    if (!h->snap_armed.load(std::memory_order_relaxed)) return;
    for (int i = 0; i < SNAP_BLOCKS - 1; i++)
        if (h->snap_blk[i].state == 0) {
            h->snap_blk[i].state = 1;
            s->snap = i + 1; s->snap_req = h->snap_req;
            h->snap_armed.store(false, std::memory_order_relaxed);
            return;
        }
    // every block is in flight, ready or being read: the request stays armed for the next picture
}

int snapshot_enqueue(mi355enc_t *h, slot_t *s, const uint8_t *y, const uint8_t *uv, int stride, hipStream_t st) {
    const int k = (int)(s - h->slot);
    snap_block_t *b = &h->snap_blk[s->snap - 1];
    if (!h->ev_snap[k]) HIPCHK(hipEventCreateWithFlags(&h->ev_snap[k], hipEventDisableTiming));
    int r = block_prepare(h, b, h->cfg.width, h->cfg.height, s->snap_req.reduce, s->snap_req.quality, h->cfg.width, h->cfg.height);
    if (!r) r = block_table(b, st);
    if (!r) r = block_launch(b, y, stride, uv, stride, h->cfg.width, h->cfg.height, s->snap_req.reduce, st);
    if (r) return r;
    HIPCHK(hipEventRecord(h->ev_snap[k], st));
    return MI355ENC_OK;
}

int snapshot_collect(mi355enc_t *h, slot_t *s) {
    const int k = (int)(s - h->slot), i = s->snap - 1;
    HIPCHK(hipEventSynchronize(h->ev_snap[k]));
    snap_block_t *b = &h->snap_blk[i];
    b->info = {s->pts, s->index, b->ow, b->oh, s->snap_req.what, s->snap_req.quality};
    std::lock_guard<std::mutex> g(h->snap_mu);
    if (h->snap_ready >= 0) { snap_block_t *o = &h->snap_blk[h->snap_ready]; o->state = o->readers ? 3 : 0; }
    b->state = 2; h->snap_ready = i;
    s->snap = 0;
    return MI355ENC_OK;
}

// (the table travels here, once, not inside the timed loop: stage 16 times the kernel alone, like the stages beside it)
int snapshot_time_prepare(mi355enc_t *h, slot_t *, ts_ctx_t *) {
    snap_block_t *b = &h->snap_blk[SNAP_BLOCKS - 1];
    int r = block_prepare(h, b, h->cfg.width, h->cfg.height, h->snap_last_req.reduce, h->snap_last_req.quality, 1, 1);
    if (!r) r = block_table(b, h->stream);
    return r;
}
int snapshot_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *) {
    return block_launch(&h->snap_blk[SNAP_BLOCKS - 1], s->d_src_y, h->W, s->d_src_uv, h->W, h->cfg.width, h->cfg.height, h->snap_last_req.reduce, h->stream);
}

// the stage entry points: planes on the device -> the stage block, waited for
static int stage_run(mi355enc_t *h, const uint8_t *d_y, int ys, const uint8_t *d_uv, int uvs, int w, int ht, int reduce, int quality, snap_block_t **out) {
    snap_block_t *b = &h->snap_blk[SNAP_BLOCKS - 1];
    int r = block_prepare(h, b, w, ht, reduce, quality, 1, 1);
    if (!r) r = block_table(b, h->stream);
    if (!r) r = block_launch(b, d_y, ys, d_uv, uvs, w, ht, reduce, h->stream);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = b;
    return MI355ENC_OK;
}
static bool stage_args_ok(const void *y, int ys, const void *uv, int uvs, int w, int ht, int reduce, int quality) {
    return y && uv && w >= 2 && ht >= 2 && !((w | ht) & 1) && w <= 16384 && ht <= 16384 && ys >= w && uvs >= w && log2_reduce(reduce) >= 0 && quality >= 1 && quality <= 100;
}
// host planes -> the call's own device planes of stride (w + 15) & ~15: luma, the chroma behind it
static int stage_upload(mi355enc_t *h, const uint8_t *y, int ys, const uint8_t *uv, int uvs, int w, int ht, stage_tmp_t *tmp, int *stride) {
    const int st = *stride = (w + 15) & ~15;
    if (tmp->alloc((size_t)st * ht * 3 / 2)) return MI355ENC_ERR_HIP;
    HIPCHK(hipMemcpy2DAsync(tmp->p, st, y, ys, w, ht, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpy2DAsync(tmp->as<uint8_t>() + (size_t)st * ht, st, uv, uvs, w, ht / 2, hipMemcpyHostToDevice, h->stream));
    return MI355ENC_OK;
}

extern "C" {

int mi355enc_request_snapshot(mi355enc_t *h, const mi355enc_snapshot_req_t *req) {
    if (!h || !req_valid(req)) return MI355ENC_ERR_ARG;
    std::lock_guard<std::mutex> g(h->snap_mu);
    h->snap_req = h->snap_last_req = *req;
    h->snap_armed.store(true, std::memory_order_release);
    return MI355ENC_OK;
}

int mi355enc_take_snapshot(mi355enc_t *h, uint8_t *out, size_t cap, size_t *len, mi355enc_snapshot_info_t *info) {
    if (!h || !len || (!out && cap)) return MI355ENC_ERR_ARG;
    snap_block_t *b;
    {
        std::lock_guard<std::mutex> g(h->snap_mu);
        if (h->snap_ready < 0) return MI355ENC_ERR_STATE;
        b = &h->snap_blk[h->snap_ready];
        b->readers++;
    }
    if (info) *info = b->info;
    const int r = snapshot_host_write(blk_levels(b), blk_hint(b), b->qt, b->ow, b->oh, out, cap, len);
    {
        std::lock_guard<std::mutex> g(h->snap_mu);
        if (--b->readers == 0 && b->state == 3) b->state = 0;
    }
    return r;
}

size_t mi355enc_debug_snapshot_bytes(const mi355enc_t *h) { return h ? h->snap_bytes.load() : 0; }

int mi355enc_stage_snapshot_blocks_device(mi355enc_t *h, const void *d_y, int y_stride, const void *d_uv, int uv_stride, int w, int ht, int reduce, int quality,
                                          int16_t *levels, uint16_t qt[2][64]) {
    if (!h || !levels || !qt || !stage_args_ok(d_y, y_stride, d_uv, uv_stride, w, ht, reduce, quality)) return MI355ENC_ERR_ARG;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    snap_block_t *b;
    int r = stage_run(h, (const uint8_t *)d_y, y_stride, (const uint8_t *)d_uv, uv_stride, w, ht, reduce, quality, &b);
    if (r) return r;
    memcpy(levels, blk_levels(b), b->nblk * 64 * sizeof(int16_t));
    memcpy(qt, b->qt, sizeof b->qt);
    return MI355ENC_OK;
}

int mi355enc_stage_snapshot_blocks(mi355enc_t *h, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride, int w, int ht, int reduce, int quality,
                                   int16_t *levels, uint16_t qt[2][64]) {
    if (!h || !levels || !qt || !stage_args_ok(y, y_stride, uv, uv_stride, w, ht, reduce, quality)) return MI355ENC_ERR_ARG;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    stage_tmp_t tmp(h->stream);
    int st = 0;
    int r = stage_upload(h, y, y_stride, uv, uv_stride, w, ht, &tmp, &st);
    const uint8_t *d = tmp.as<uint8_t>();
    return r ? r : mi355enc_stage_snapshot_blocks_device(h, d, st, d + (size_t)st * ht, st, w, ht, reduce, quality, levels, qt);
}

int mi355enc_stage_snapshot(mi355enc_t *h, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride, int w, int ht, int reduce, int quality,
                            uint8_t *out, size_t cap, size_t *len) {
    if (!h || !len || (!out && cap) || !stage_args_ok(y, y_stride, uv, uv_stride, w, ht, reduce, quality)) return MI355ENC_ERR_ARG;
    HIPCHK(hipSetDevice(h->cfg.device_id));
    stage_tmp_t tmp(h->stream);
    int st = 0;
    snap_block_t *b = nullptr;
    int r = stage_upload(h, y, y_stride, uv, uv_stride, w, ht, &tmp, &st);
    const uint8_t *d = tmp.as<uint8_t>();
    if (!r) r = stage_run(h, d, st, d + (size_t)st * ht, st, w, ht, reduce, quality, &b);
    return r ? r : snapshot_host_write(blk_levels(b), blk_hint(b), b->qt, b->ow, b->oh, out, cap, len);
}

} // extern "C"
