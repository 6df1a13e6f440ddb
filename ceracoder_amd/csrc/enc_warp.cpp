// enc_warp.cpp -- lens, roll and keystone correction of a handle (mi355enc_set_warp / mi355enc_set_warp_mesh): the setting and the mesh the
// control thread sets, their latch per input picture, the mesh's way to the device, the launch on the slot's coded surfaces with the handle's scratch pair, the
// stage entry point and the timed stage.  The rule itself is warp_host.h's and warp_host.c's, which need no device.
#include "enc_internal.hpp"

static int warp_words(const mi355enc_t *h) { return 2 * warp_nodes(h->cfg.width) * warp_nodes(h->cfg.height); }

void warp_free(mi355enc_t *h) {
    if (h->d_warp_y) (void)hipFree(h->d_warp_y);
    if (h->d_warp_uv) (void)hipFree(h->d_warp_uv);
    if (h->d_warp_mesh) (void)hipFree(h->d_warp_mesh);
    if (h->h_warp_mesh) (void)hipHostFree(h->h_warp_mesh);
    h->d_warp_y = h->d_warp_uv = nullptr; h->d_warp_mesh = h->h_warp_mesh = nullptr; h->warp_bytes = 0; h->warp_sent = 0;
}
void warp_close(mi355enc_t *h) { // (mi355enc_close: nothing sets any more)
    warp_free(h);
    free(h->warp_mesh);
    h->warp_mesh = nullptr;
}

// the scratch pair (surfaces like a slot's, SURF_PAD included), the mesh on the device and one pinned copy of a mesh per slot: allocated by the first warped picture
static int warp_alloc(mi355enc_t *h) {
    if (h->d_warp_y) return MI355ENC_OK;
    const size_t mesh = (size_t)warp_words(h) * sizeof(int32_t);
    if (hipMalloc((void **)&h->d_warp_y, h->ysz + SURF_PAD) != hipSuccess || hipMalloc((void **)&h->d_warp_uv, h->csz + SURF_PAD) != hipSuccess ||
        hipMalloc((void **)&h->d_warp_mesh, mesh) != hipSuccess || hipHostMalloc((void **)&h->h_warp_mesh, mesh * NSLOT, hipHostMallocDefault) != hipSuccess) {
        warp_free(h);
        return MI355ENC_ERR_HIP;
    }
    h->warp_bytes = h->ysz + h->csz + 2 * SURF_PAD + mesh;
    return MI355ENC_OK;
}

// The value set last becomes the slot's.  own (the slot the input goes into): where its generation is not the one the device mesh holds -- or will hold, by the
// order of the upload stream -- the mesh is copied, under the lock, into the slot's pinned copy, which nothing touches again before the picture is collected.
int warp_latch(mi355enc_t *h, slot_t *s, bool own) {
    s->warp_send = false;
    bool on;
    { std::lock_guard<std::mutex> g(h->warp_mu); on = h->warp_on; }
    if (own && on) { int r = warp_alloc(h); if (r) return r; }
    std::lock_guard<std::mutex> g(h->warp_mu);
    s->warp_on = h->warp_on && (!own || h->d_warp_y); // (set on between the two locks: this picture is not warped yet)
    s->warp = h->warp_cur;
    s->warp_gen = s->warp_on ? h->warp_gen : 0;
    if (own && s->warp_on && s->warp_gen != h->warp_sent) {
        memcpy(h->h_warp_mesh + (size_t)warp_words(h) * (s - h->slot), h->warp_mesh, (size_t)warp_words(h) * sizeof(int32_t));
        s->warp_send = true;
    }
    return MI355ENC_OK;
}

// the launch from the slot's surfaces into the scratch pair, then the exchange of both planes (the launch has written every byte; the planes the slot gives up
// were last read by this launch, and the next launch that writes them follows on the same stream)
static int warp_run(mi355enc_t *h, slot_t *s, const mi355enc_warp_t *set, const int32_t *d_mesh, hipStream_t st) {
    if (k_launch_warp(s->d_src_y, s->d_src_uv, h->d_warp_y, h->d_warp_uv, h->cfg.width, h->cfg.height, h->W, h->H, d_mesh, set->kind, set->fill, st, h->warp_staging ? 1 : 0)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    uint8_t *t = s->d_src_y; s->d_src_y = h->d_warp_y; h->d_warp_y = t;
    t = s->d_src_uv; s->d_src_uv = h->d_warp_uv; h->d_warp_uv = t;
    return MI355ENC_OK;
}

int warp_draw(mi355enc_t *h, slot_t *s, hipStream_t st) {
    if (!s->warp_on) return MI355ENC_OK;
    if (s->warp_send) { // (every warp launch of the stream and every transfer of a mesh is enqueued on this one stream: pictures in flight keep the mesh they latched)
        HIPCHK(hipMemcpyAsync(h->d_warp_mesh, h->h_warp_mesh + (size_t)warp_words(h) * (s - h->slot), (size_t)warp_words(h) * sizeof(int32_t), hipMemcpyHostToDevice, st));
        h->warp_sent = s->warp_gen; s->warp_send = false;
    }
    return warp_run(h, s, &s->warp, h->d_warp_mesh, st);
}

void warp_collected(mi355enc_t *h, slot_t *s) { h->warp_last_have = true; h->warp_last_gen = s->warp_on ? s->warp_gen : 0; }

bool warp_time_ready(mi355enc_t *h, int) { std::lock_guard<std::mutex> g(h->warp_mu); return h->warp_on; }
int warp_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *) { // the mesh set last, through slot 0's pinned copy, on the main stream
    { int r = warp_alloc(h); if (r) return r; }
    { std::lock_guard<std::mutex> g(h->warp_mu); if (!h->warp_on) return MI355ENC_ERR_STATE; s->warp = h->warp_cur; memcpy(h->h_warp_mesh, h->warp_mesh, (size_t)warp_words(h) * sizeof(int32_t)); }
    HIPCHK(hipMemcpyAsync(h->d_warp_mesh, h->h_warp_mesh, (size_t)warp_words(h) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    return MI355ENC_OK;
}
int warp_time_launch(mi355enc_t *h, slot_t *s, ts_ctx_t *) { return warp_run(h, s, &s->warp, h->d_warp_mesh, h->stream); }
void warp_time_done(mi355enc_t *h) { h->warp_sent = 0; } // (the next warped picture sends its mesh again, on its own stream)

// a checked setting and mesh become the handle's; a null setting: off
static int warp_set(mi355enc_t *h, const mi355enc_warp_t *s, int32_t *mesh) {
    std::lock_guard<std::mutex> g(h->warp_mu);
    if (!s) { h->warp_on = false; return MI355ENC_OK; }
    free(h->warp_mesh);
    h->warp_mesh = mesh; h->warp_cur = *s; h->warp_on = true; h->warp_gen++;
    return MI355ENC_OK;
}

extern "C" {

int mi355enc_set_warp(mi355enc_t *h, const mi355enc_warp_t *s, const mi355enc_warp_params_t *p) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!s) return warp_set(h, nullptr, nullptr);
    if (!p || (s->kind != 0 && s->kind != 1)) return MI355ENC_ERR_ARG;
    int32_t *mesh = (int32_t *)malloc((size_t)warp_words(h) * sizeof(int32_t)); // (built in the caller's thread, outside the lock)
    if (!mesh) return MI355ENC_ERR_ARG;
    if (mi355enc_warp_build(p, h->cfg.width, h->cfg.height, mesh, (size_t)warp_words(h))) { free(mesh); return MI355ENC_ERR_ARG; }
    return warp_set(h, s, mesh);
}

int mi355enc_set_warp_mesh(mi355enc_t *h, const mi355enc_warp_t *s, const int32_t *mesh, int nx, int ny) {
    if (!h) return MI355ENC_ERR_ARG;
    if (!s) return warp_set(h, nullptr, nullptr);
    if ((s->kind != 0 && s->kind != 1) || nx != warp_nodes(h->cfg.width) || ny != warp_nodes(h->cfg.height) || mi355enc_warp_mesh_check(mesh, nx, ny)) return MI355ENC_ERR_ARG;
    int32_t *copy = (int32_t *)malloc((size_t)warp_words(h) * sizeof(int32_t));
    if (!copy) return MI355ENC_ERR_ARG;
    memcpy(copy, mesh, (size_t)warp_words(h) * sizeof(int32_t));
    return warp_set(h, s, copy);
}

int mi355enc_get_warp(const mi355enc_t *h, int *on, mi355enc_warp_t *s) {
    if (!h) return MI355ENC_ERR_ARG;
    mi355enc_t *m = const_cast<mi355enc_t *>(h);
    std::lock_guard<std::mutex> g(m->warp_mu);
    if (on) *on = h->warp_on ? 1 : 0;
    if (s && h->warp_on) *s = h->warp_cur;
    return MI355ENC_OK;
}

int mi355enc_last_warp(mi355enc_t *h, unsigned *generation) {
    if (!h || !generation) return MI355ENC_ERR_ARG;
    if (!h->warp_last_have) return MI355ENC_ERR_STATE;
    *generation = h->warp_last_gen;
    return MI355ENC_OK;
}

size_t mi355enc_debug_warp_bytes(const mi355enc_t *h) { return h ? h->warp_bytes : 0; }

int mi355enc_debug_warp_staging(mi355enc_t *h, int on) {
    if (!h) return MI355ENC_ERR_ARG;
    h->warp_staging = on != 0;
    return MI355ENC_OK;
}

int mi355enc_warp_probe(mi355enc_t *h, const mi355enc_warp_t *set, const int32_t *mesh, uint8_t *y, uint8_t *uv) {
    if (!h || !set || (set->kind != 0 && set->kind != 1) || !y || !uv || mi355enc_warp_mesh_check(mesh, warp_nodes(h->cfg.width), warp_nodes(h->cfg.height))) return MI355ENC_ERR_ARG;
    slot_t *s = &h->slot[0];
    int r = stage_enter(h);
    if (!r) r = warp_alloc(h);
    if (r) return r;
    stage_tmp_t m(h->stream);
    if (m.alloc((size_t)warp_words(h) * sizeof(int32_t))) return MI355ENC_ERR_HIP;
    HIPCHK(hipMemcpyAsync(m.p, mesh, (size_t)warp_words(h) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    r = stage_in(h, s, y, uv);
    if (!r) r = warp_run(h, s, set, m.as<int32_t>(), h->stream);
    return r ? r : stage_out(h, s, y, uv);
}

} // extern "C"
