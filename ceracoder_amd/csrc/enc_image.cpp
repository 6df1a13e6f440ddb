// enc_image.cpp -- the image layers of a handle: the images and places the control thread sets, their latch per submitted
// picture, the upload and preparation of an image the device has not seen yet, the blend launches, the retirement of images nobody refers to
// any more, and the entry points that expose rule and kernels to tests.
#include "enc_internal.hpp"

#define IMAGE_PLACE_MAX 16384

static bool fmt_ok(int fmt) { return fmt >= MI355ENC_FMT_BGRX && fmt <= MI355ENC_FMT_XBGR; }
static bool place_ok(int x, int y, int opacity) {
    return x >= -IMAGE_PLACE_MAX && x <= IMAGE_PLACE_MAX && y >= -IMAGE_PLACE_MAX && y <= IMAGE_PLACE_MAX && opacity >= 0 && opacity <= 256;
}
static bool layer_ok(const mi355enc_image_layer_t *im) {
    return fmt_ok(im->fmt) && im->w >= 1 && im->w <= MI355ENC_IMAGE_MAX_DIM && im->h >= 1 && im->h <= MI355ENC_IMAGE_MAX_DIM && im->stride >= 4 * im->w &&
           place_ok(im->x, im->y, im->opacity);
}

// the caller's pixels as an image of the handle's own: rows of 4 w bytes in plain host memory (no GPU call); null: no memory
static image_t *image_new(const mi355enc_image_layer_t *im) {
    image_t *g = new (std::nothrow) image_t();
    if (!g) return nullptr;
    const size_t row = 4 * (size_t)im->w;
    g->host = (uint8_t *)malloc(row * (size_t)im->h);
    if (!g->host) { delete g; return nullptr; }
    for (int r = 0; r < im->h; r++) memcpy(g->host + (size_t)r * row, im->pixels + (size_t)r * (size_t)im->stride, row);
    g->buf = nullptr; g->fmt = im->fmt; g->w = im->w; g->h = im->h; g->refs = 1;
    return g;
}
// one reference less (img_mu held); the last one retires the image: its buffers are free for the next upload -- whatever read them was enqueued before that
// upload on the same stream, or has been waited for (the stage entry points) -- and nothing is freed on the device
static void image_unref(image_t *g) {
    if (!g || --g->refs > 0) return;
    if (g->buf) g->buf->busy = false;
    free(g->host);
    delete g;
}

// pinned staging and device words for `bytes`: a retired buffer that is large enough, or new ones (first use of a size; freed at close)
static int image_buf_get(mi355enc_t *h, size_t bytes, image_buf_t **out) {
    {
        std::lock_guard<std::mutex> g(h->img_mu);
        for (image_buf_t *b = h->img_bufs; b; b = b->next)
            if (!b->busy && b->cap >= bytes) { b->busy = true; *out = b; return MI355ENC_OK; }
    }
    image_buf_t *b = new (std::nothrow) image_buf_t();
    if (!b) return MI355ENC_ERR_NOMEM;
    b->h_pin = nullptr; b->d_pix = nullptr; b->ev = nullptr; b->cap = bytes; b->busy = true;
    { std::lock_guard<std::mutex> g(h->img_mu); b->next = h->img_bufs; h->img_bufs = b; h->img_dev_bytes += bytes; } // (on the list first: close() frees whatever of it exists)
    HIPCHK(hipHostMalloc((void **)&b->h_pin, bytes, hipHostMallocDefault));
    HIPCHK(hipMalloc((void **)&b->d_pix, bytes));
    HIPCHK(hipEventCreateWithFlags(&b->ev, hipEventDisableTiming));
    *out = b;
    return MI355ENC_OK;
}

// The image on the device, prepared, in stream order on st.  A buffer that comes back from the pool may still be the source of its previous image's transfer
// (a picture that was collected as a run of skipped macroblocks has not waited for its uploads): that one transfer, enqueued at least a whole picture ago on
// this handle's own upload stream, is waited for before the staging memory is written again.
static int image_upload(mi355enc_t *h, image_t *g, hipStream_t st) {
    if (g->buf) return MI355ENC_OK;
    const size_t bytes = 4 * (size_t)g->w * (size_t)g->h;
    image_buf_t *b = nullptr;
    { int r = image_buf_get(h, bytes, &b); if (r) return r; }
    if (!b->h_pin || !b->d_pix || !b->ev) return MI355ENC_ERR_HIP; // (an allocation that failed half way, earlier)
    HIPCHK(hipEventSynchronize(b->ev));
    memcpy(b->h_pin, g->host, bytes);
    free(g->host); g->host = nullptr;
    HIPCHK(hipMemcpyAsync(b->d_pix, b->h_pin, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(b->ev, st));
    if (k_launch_image_prepare(b->d_pix, (size_t)g->w * (size_t)g->h, g->fmt, h->csc_coef, st)) return MI355ENC_ERR_ARG;
    HIPCHK(hipGetLastError());
    g->buf = b;
    return MI355ENC_OK;
}

static bool image_args(const mi355enc_t *h, const slot_t *s, const image_t *g, int x, int y, int opacity, image_args_t *a) {
    memset(a, 0, sizeof *a);
    a->y = s->d_src_y; a->uv = s->d_src_uv; a->img = g->buf ? g->buf->d_pix : nullptr;
    a->stride = h->W; a->vw = h->cfg.width; a->vh = h->cfg.height; a->W = h->W; a->H = h->H;
    a->iw = g->w; a->ih = g->h; a->x = x; a->y0 = y; a->opacity = opacity;
    return k_image_grid(a);
}

static int image_blend(mi355enc_t *h, slot_t *s, image_t *g, int x, int y, int opacity, hipStream_t st) {
    image_args_t a;
    if (!opacity || !image_args(h, s, g, x, y, opacity, &a)) return MI355ENC_OK; // (nothing to change: no upload, no launch)
    { int r = image_upload(h, g, st); if (r) return r; }
    a.img = g->buf->d_pix;
    k_launch_image_blend(&a, st);
    HIPCHK(hipGetLastError());
    return MI355ENC_OK;
}

int image_latch(mi355enc_t *h, slot_t *s, bool) {
    std::lock_guard<std::mutex> g(h->img_mu);
    bool active = false;
    for (int l = 0; l < MI355ENC_IMAGE_LAYERS; l++) {
        image_unref(s->img[l]); // (what a submit that failed left behind)
        s->img[l] = h->img_cur[l];
        if (!s->img[l]) continue;
        s->img[l]->refs++;
        s->img_x[l] = h->img_x[l]; s->img_y[l] = h->img_y[l]; s->img_op[l] = h->img_op[l]; s->img_serial[l] = h->img_serial[l];
        active |= s->img_op[l] != 0;
    }
    if (active && !h->csc_ok) { // as an RGB submit: the colour cannot be converted
        for (int l = 0; l < MI355ENC_IMAGE_LAYERS; l++) { image_unref(s->img[l]); s->img[l] = nullptr; }
        return MI355ENC_ERR_ARG;
    }
    return MI355ENC_OK;
}

int image_draw(mi355enc_t *h, slot_t *s, hipStream_t st) {
    for (int l = 0; l < MI355ENC_IMAGE_LAYERS; l++)
        if (s->img[l]) { int r = image_blend(h, s, s->img[l], s->img_x[l], s->img_y[l], s->img_op[l], st); if (r) return r; }
    return MI355ENC_OK;
}

void image_collected(mi355enc_t *h, slot_t *s) {
    std::lock_guard<std::mutex> g(h->img_mu);
    for (int l = 0; l < MI355ENC_IMAGE_LAYERS; l++) {
        mi355enc_image_info_t *o = &h->img_last[l];
        memset(o, 0, sizeof *o);
        if (!s->img[l]) continue;
        o->w = s->img[l]->w; o->h = s->img[l]->h; o->x = s->img_x[l]; o->y = s->img_y[l]; o->opacity = s->img_op[l]; o->serial = s->img_serial[l];
        image_unref(s->img[l]);
        s->img[l] = nullptr;
    }
}

void image_free(mi355enc_t *h) {
    for (int l = 0; l < MI355ENC_IMAGE_LAYERS; l++) {
        for (int i = 0; i < NSLOT; i++) { image_unref(h->slot[i].img[l]); h->slot[i].img[l] = nullptr; }
        image_unref(h->img_cur[l]); h->img_cur[l] = nullptr;
    }
    while (h->img_bufs) {
        image_buf_t *b = h->img_bufs;
        h->img_bufs = b->next;
        if (b->h_pin) (void)hipHostFree(b->h_pin);
        if (b->d_pix) (void)hipFree(b->d_pix);
        if (b->ev) (void)hipEventDestroy(b->ev);
        delete b;
    }
    h->img_dev_bytes = 0;
}

extern "C" {

int mi355enc_set_image(mi355enc_t *h, int layer, const mi355enc_image_layer_t *img) {
    if (!h || layer < 0 || layer >= MI355ENC_IMAGE_LAYERS) return MI355ENC_ERR_ARG;
    image_t *g = nullptr;
    if (img && img->pixels) {
        if (!layer_ok(img)) return MI355ENC_ERR_ARG;
        g = image_new(img); // (the copy is made outside the lock: a running submit is not held up by it)
        if (!g) return MI355ENC_ERR_NOMEM;
    }
    std::lock_guard<std::mutex> lk(h->img_mu);
    image_unref(h->img_cur[layer]);
    h->img_cur[layer] = g;
    if (g) { h->img_x[layer] = img->x; h->img_y[layer] = img->y; h->img_op[layer] = img->opacity; }
    h->img_serial[layer]++;
    return MI355ENC_OK;
}

int mi355enc_set_image_place(mi355enc_t *h, int layer, int x, int y, int opacity) {
    if (!h || layer < 0 || layer >= MI355ENC_IMAGE_LAYERS || !place_ok(x, y, opacity)) return MI355ENC_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->img_mu);
    if (!h->img_cur[layer]) return MI355ENC_ERR_STATE;
    h->img_x[layer] = x; h->img_y[layer] = y; h->img_op[layer] = opacity;
    return MI355ENC_OK;
}

int mi355enc_last_image(mi355enc_t *h, int layer, mi355enc_image_info_t *info) {
    if (!h || !info || layer < 0 || layer >= MI355ENC_IMAGE_LAYERS) return MI355ENC_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->img_mu);
    *info = h->img_last[layer];
    return MI355ENC_OK;
}

size_t mi355enc_debug_image_bytes(const mi355enc_t *h) { return h ? h->img_dev_bytes : 0; }

int mi355enc_image_pixel(int matrix, int full_range, int r, int g, int b, uint8_t ycbcr[3]) {
    int32_t c[10];
    if (!ycbcr || ((r | g | b) & ~255) || mi355enc_csc_coefficients(matrix, full_range, c) != MI355ENC_OK) return MI355ENC_ERR_ARG;
    auto clip8 = [](int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); };
    ycbcr[0] = clip8((c[0] * r + c[1] * g + c[2] * b + (c[9] << 16) + (1 << 15)) >> 16);
    ycbcr[1] = clip8((c[3] * r + c[4] * g + c[5] * b + (128 << 16) + (1 << 15)) >> 16);
    ycbcr[2] = clip8((c[6] * r + c[7] * g + c[8] * b + (128 << 16) + (1 << 15)) >> 16);
    return MI355ENC_OK;
}

int mi355enc_stage_image(mi355enc_t *h, const mi355enc_image_layer_t *layers, int n, uint8_t *y, uint8_t *uv) {
    if (!h || !y || !uv || n < 0 || n > MI355ENC_IMAGE_LAYERS || (n && !layers)) return MI355ENC_ERR_ARG;
    for (int l = 0; l < n; l++) if (layers[l].pixels && !layer_ok(&layers[l])) return MI355ENC_ERR_ARG;
    { int r = stage_enter(h); if (r) return r; } // (its wait for every stream: the pool's buffers may have been read on the upload stream last)
    if (!h->csc_ok) return MI355ENC_ERR_ARG;
    slot_t *s = &h->slot[0];
    image_t *made[MI355ENC_IMAGE_LAYERS] = {nullptr, nullptr, nullptr, nullptr};
    int r = stage_in(h, s, y, uv);
    for (int l = 0; l < n && !r; l++) {
        if (!layers[l].pixels) continue;
        made[l] = image_new(&layers[l]);
        r = made[l] ? image_blend(h, s, made[l], layers[l].x, layers[l].y, layers[l].opacity, h->stream) : MI355ENC_ERR_NOMEM;
    }
    if (!r) r = stage_out(h, s, y, uv);
    if (r && hipStreamSynchronize(h->stream) != hipSuccess) r = MI355ENC_ERR_HIP;
    { std::lock_guard<std::mutex> lk(h->img_mu); for (int l = 0; l < n; l++) image_unref(made[l]); } // (everything that read them has completed)
    return r;
}

} // extern "C"

// mi355enc_time_stage 15: layer 0's image on the device (outside the timed loop), and the launch's arguments at its current place into slot 0's surfaces
int image_time_prepare(mi355enc_t *h, slot_t *s, ts_ctx_t *ctx) {
    image_args_t *a = &ctx->img;
    image_t *g;
    int x, y, op;
    {
        std::lock_guard<std::mutex> lk(h->img_mu);
        g = h->img_cur[0];
        if (!g) return MI355ENC_ERR_STATE;
        g->refs++; x = h->img_x[0]; y = h->img_y[0]; op = h->img_op[0];
    }
    int r = !h->csc_ok ? MI355ENC_ERR_ARG : image_upload(h, g, h->stream);
    if (!r && !image_args(h, s, g, x, y, op, a)) r = MI355ENC_ERR_STATE; // (nothing of it is visible: there is no launch to time)
    if (!r) a->img = g->buf->d_pix;
    { std::lock_guard<std::mutex> lk(h->img_mu); image_unref(g); } // (the layer keeps it: the buffer stays what it is while the caller times)
    return r;
}
