// ll_api_keyframe_bank.hip -- the key-frame descriptor bank of the C ABI (ll_keyframe_bank_*): the line and plane direction image of
// every processed key frame stay on the device with their norms, and "this key frame against these earlier ones" is one launch chain
// and one host wait for any number of pairs (ll_keyframe_bank_kernels.hip).  The floats are ll_keyframe_similarity's.
#include "ll_api_internal.h"
#include "ll_keyframe_bank.h"
#include "ll_keyframe_bank_core.h"

struct ll_keyframe_bank {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t cap = 0, n = 0;       // entries there is room for / entries held; an entry's id is its position and never changes
    float *d_img = nullptr;       // [cap][2][3600]: line image, plane image
    double *d_norm = nullptr;     // [cap][2]
    int64_t pair_cap = 0;
    int2 *d_pairs = nullptr, *hp_pairs = nullptr;  // device / page-locked host staging of a match's pairs
    double *d_partial = nullptr;  // [pair_cap][2][LL_KB_TILES]
    float *d_sim = nullptr, *hp_sim = nullptr;     // [2][n_pairs]
    double *d_surface = nullptr;  // [3600], ll_keyframe_bank_debug_surface
    int64_t work[4] = {0, 0, 0, 0};
};

static const int64_t kMaxEntries = (0x7fffffffLL) / LL_KB_ENTRY;  // the image array stays below 2^31 floats
static const int64_t kMaxPairs = 1 << 24;                         // 6 workgroups per pair in a one-dimensional grid

extern "C" void ll_keyframe_bank_destroy(ll_keyframe_bank *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    void *dev[] = {b->d_img, b->d_norm, b->d_pairs, b->d_partial, b->d_sim, b->d_surface};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (b->hp_pairs) (void)hipHostFree(b->hp_pairs);
    if (b->hp_sim) (void)hipHostFree(b->hp_sim);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

// room for `need` entries: the capacity doubles, content and ids kept.  The bank's stream is idle between calls, and is when this returns.
static int kb_room(ll_keyframe_bank *b, int64_t need, const char *where)
{
    if (need <= b->cap) return 0;
    if (need > kMaxEntries) return set_err(where, "the bank would pass 2^31 image floats");
    int64_t cap = std::max<int64_t>(2 * b->cap, need);
    if (cap > kMaxEntries) cap = kMaxEntries;
    float *img = nullptr;
    double *norm = nullptr;
    if (hipMalloc((void **)&img, (size_t)cap * LL_KB_ENTRY * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&norm, (size_t)cap * 2 * sizeof(double)) != hipSuccess) {
        if (img) (void)hipFree(img);
        return set_err(where, "allocation failed");
    }
    if (b->n > 0) {
        HC(hipMemcpyAsync(img, b->d_img, (size_t)b->n * LL_KB_ENTRY * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
        HC(hipMemcpyAsync(norm, b->d_norm, (size_t)b->n * 2 * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
        HC(hipStreamSynchronize(b->stream));
    }
    if (b->d_img) (void)hipFree(b->d_img);
    if (b->d_norm) (void)hipFree(b->d_norm);
    b->d_img = img;
    b->d_norm = norm;
    b->cap = cap;
    return 0;
}

static int kb_pair_room(ll_keyframe_bank *b, int64_t need, const char *where)
{
    if (need <= b->pair_cap) return 0;
    const int64_t cap = std::min<int64_t>(std::max<int64_t>(2 * b->pair_cap, need), kMaxPairs);
    void *dev[] = {b->d_pairs, b->d_partial, b->d_sim};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (b->hp_pairs) (void)hipHostFree(b->hp_pairs);
    if (b->hp_sim) (void)hipHostFree(b->hp_sim);
    b->d_pairs = b->hp_pairs = nullptr;
    b->d_partial = nullptr;
    b->d_sim = b->hp_sim = nullptr;
    b->pair_cap = 0;
    if (hipMalloc((void **)&b->d_pairs, (size_t)cap * sizeof(int2)) != hipSuccess ||
        hipMalloc((void **)&b->d_partial, (size_t)cap * 2 * LL_KB_TILES * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&b->d_sim, (size_t)cap * 2 * sizeof(float)) != hipSuccess ||
        hipHostMalloc((void **)&b->hp_pairs, (size_t)cap * sizeof(int2), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&b->hp_sim, (size_t)cap * 2 * sizeof(float), hipHostMallocDefault) != hipSuccess)
        return set_err(where, "allocation failed");
    b->pair_cap = cap;
    return 0;
}

extern "C" int ll_keyframe_bank_create(int32_t device, int64_t initial_entries, ll_keyframe_bank **out)
{
    const char *fn = "ll_keyframe_bank_create";
    if (!out) return set_err(fn, "null argument");
    if (initial_entries < 1) return set_err(fn, "initial_entries out of range");
    if (initial_entries > kMaxEntries) return set_err(fn, "the bank would pass 2^31 image floats");
    if (check_device(device)) return -1;
    ll_keyframe_bank *b = new ll_keyframe_bank();
    b->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess ||
        kb_room(b, initial_entries, fn) || kb_pair_room(b, 256, fn) || dmalloc(&b->d_surface, LL_KB_BINS)) {
        const std::string why = g_err;
        ll_keyframe_bank_destroy(b);
        g_err = why.empty() ? std::string(fn) + ": allocation failed" : why;
        return -1;
    }
    *out = b;
    return 0;
}

extern "C" int64_t ll_keyframe_bank_size(const ll_keyframe_bank *b)
{
    if (!b) return set_err("ll_keyframe_bank_size", "null argument");
    return b->n;
}

extern "C" int ll_keyframe_bank_add_cellmap(ll_keyframe_bank *b, ll_cellmap *c, float roi_ratio, float *images, float *ratio_nonzero,
                                            float *eigen_R, int32_t *n_vectors, float *centre_and_range, int64_t *id)
{
    const char *fn = "ll_keyframe_bank_add_cellmap";
    if (!b || !c || !id) return set_err(fn, "null argument");
    if (c->device != b->device) return set_err(fn, "the cell map lives on another device than the bank");
    if (!(roi_ratio >= 0.f && roi_ratio <= 1.f)) return set_err(fn, "roi_ratio must lie in [0, 1]");
    if (cellmap_settle(c)) return -1;  // (a history's cell map whose feeder has failed: its error)
    if (b->n >= kMaxEntries) return set_err(fn, "the bank would pass 2^31 image floats");
    HC(hipSetDevice(b->device));
    if (kb_room(b, b->n + 1, fn)) return -1;
    if (!c->d_stats) DM(c->d_stats, (size_t)c->dev.cap);
    if (!c->d_kf) DM(c->d_kf, 1);
    // ll_cellmap_keyframe_images, and behind it on the cell map's stream the two images into the entry, device to device, and their norms
    const char *err = nullptr;
    float *entry = b->d_img + (size_t)b->n * LL_KB_ENTRY;
    if (cellmap_keyframe_images(c->dev, c->d_stats, roi_ratio, c->d_kf, c->stream, &err)) return set_err(fn, err);
    HC(hipMemcpyAsync(entry, c->d_kf->img, (size_t)LL_KB_ENTRY * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (keyframe_bank_norms(entry, b->d_norm + 2 * (size_t)b->n, c->stream, &err)) return set_err(fn, err);
    std::vector<KfOut> h(1);
    HC(hipMemcpyAsync(h.data(), c->d_kf, sizeof(KfOut), hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    const KfOut &k = h[0];
    if (images) memcpy(images, k.img, sizeof(k.img));
    if (ratio_nonzero) memcpy(ratio_nonzero, k.ratio, sizeof(k.ratio));
    if (eigen_R) memcpy(eigen_R, k.R, sizeof(k.R));
    if (n_vectors)
        for (int i = 0; i < 4; i++) n_vectors[i] = k.n_vec[i];
    if (centre_and_range) {
        for (int d = 0; d < 3; d++) centre_and_range[d] = k.centre[d];
        centre_and_range[3] = k.roi_range;
    }
    *id = b->n++;
    return 0;
}

extern "C" int ll_keyframe_bank_add_images(ll_keyframe_bank *b, const float *img_line, const float *img_plane, int64_t *id)
{
    const char *fn = "ll_keyframe_bank_add_images";
    if (!b || !img_line || !img_plane || !id) return set_err(fn, "null argument");
    if (b->n >= kMaxEntries) return set_err(fn, "the bank would pass 2^31 image floats");
    HC(hipSetDevice(b->device));
    if (kb_room(b, b->n + 1, fn)) return -1;
    float *entry = b->d_img + (size_t)b->n * LL_KB_ENTRY;
    HC(hipMemcpyAsync(entry, img_line, LL_KB_BINS * sizeof(float), hipMemcpyHostToDevice, b->stream));
    HC(hipMemcpyAsync(entry + LL_KB_BINS, img_plane, LL_KB_BINS * sizeof(float), hipMemcpyHostToDevice, b->stream));
    const char *err = nullptr;
    if (keyframe_bank_norms(entry, b->d_norm + 2 * (size_t)b->n, b->stream, &err)) return set_err(fn, err);
    HC(hipStreamSynchronize(b->stream));
    *id = b->n++;
    return 0;
}

extern "C" int ll_keyframe_bank_images(ll_keyframe_bank *b, int64_t id, float *img_line, float *img_plane)
{
    const char *fn = "ll_keyframe_bank_images";
    if (!b || !img_line || !img_plane) return set_err(fn, "null argument");
    if (id < 0 || id >= b->n) return set_err(fn, "id out of range");
    HC(hipSetDevice(b->device));
    const float *entry = b->d_img + (size_t)id * LL_KB_ENTRY;
    HC(hipMemcpy(img_line, entry, LL_KB_BINS * sizeof(float), hipMemcpyDeviceToHost));
    HC(hipMemcpy(img_plane, entry + LL_KB_BINS, LL_KB_BINS * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int ll_keyframe_bank_match(ll_keyframe_bank *b, int64_t n_pairs, const int64_t *ids_a, const int64_t *ids_b, float *sim_line,
                                      float *sim_plane)
{
    const char *fn = "ll_keyframe_bank_match";
    if (!b) return set_err(fn, "null argument");
    if (n_pairs < 0 || n_pairs > kMaxPairs) return set_err(fn, "n_pairs out of range");
    if (n_pairs > 0 && (!ids_a || !ids_b || !sim_line || !sim_plane)) return set_err(fn, "null argument");
    for (int64_t p = 0; p < n_pairs; p++)
        if (ids_a[p] < 0 || ids_a[p] >= b->n || ids_b[p] < 0 || ids_b[p] >= b->n) return set_err(fn, "id out of range");
    int64_t *work = b->work;
    work[0] = work[1] = work[2] = 0;  // work[2]: no copy of this function moves an image; there is nothing to add to it
    work[3] = n_pairs;
    if (n_pairs == 0) return 0;
    HC(hipSetDevice(b->device));
    if (kb_pair_room(b, n_pairs, fn)) return -1;
    for (int64_t p = 0; p < n_pairs; p++) b->hp_pairs[p] = make_int2((int)ids_a[p], (int)ids_b[p]);
    const int n = (int)n_pairs;
    const char *err = nullptr;
    HC(hipMemcpyAsync(b->d_pairs, b->hp_pairs, (size_t)n * sizeof(int2), hipMemcpyHostToDevice, b->stream));
    if (keyframe_bank_match(b->d_img, b->d_norm, b->d_pairs, n, b->d_partial, b->d_sim, b->stream, &err)) return set_err(fn, err);
    HC(hipMemcpyAsync(b->hp_sim, b->d_sim, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    work[0] = 4;  // the pairs in, the correlation, the finish, the similarities out
    HC(hipStreamSynchronize(b->stream));  // the one wait
    work[1] = 1;
    memcpy(sim_line, b->hp_sim, (size_t)n * sizeof(float));
    memcpy(sim_plane, b->hp_sim + n, (size_t)n * sizeof(float));
    return 0;
}

extern "C" int ll_keyframe_bank_debug_surface(ll_keyframe_bank *b, int64_t id_a, int64_t id_b, int32_t kind, double *out)
{
    const char *fn = "ll_keyframe_bank_debug_surface";
    if (!b || !out) return set_err(fn, "null argument");
    if (id_a < 0 || id_a >= b->n || id_b < 0 || id_b >= b->n) return set_err(fn, "id out of range");
    if (kind != 0 && kind != 1) return set_err(fn, "kind must be 0 (line) or 1 (plane)");
    HC(hipSetDevice(b->device));
    if (kb_pair_room(b, 1, fn)) return -1;
    b->hp_pairs[0] = make_int2((int)id_a, (int)id_b);
    const char *err = nullptr;
    HC(hipMemcpyAsync(b->d_pairs, b->hp_pairs, sizeof(int2), hipMemcpyHostToDevice, b->stream));
    if (keyframe_bank_surface(b->d_img, b->d_pairs, kind, b->d_surface, b->stream, &err)) return set_err(fn, err);
    HC(hipMemcpyAsync(out, b->d_surface, LL_KB_BINS * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HC(hipStreamSynchronize(b->stream));
    return 0;
}

extern "C" int ll_keyframe_bank_work(ll_keyframe_bank *b, int64_t out[4])
{
    if (!b || !out) return set_err("ll_keyframe_bank_work", "null argument");
    for (int i = 0; i < 4; i++) out[i] = b->work[i];
    return 0;
}
