// ll_api_cellmap.hip -- the cell map handle (ll_cellmap_*) of the C ABI (ll_cellmap_kernels.hip), and ll_keyframe_similarity.
#include "ll_api_internal.h"

void ll::cellmap_release(ll_cellmap *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    cellmap_free(c->dev);
    if (c->d_in) (void)hipFree(c->d_in);
    if (c->d_pose) (void)hipFree(c->d_pose);
    if (c->d_stats) (void)hipFree(c->d_stats);
    if (c->d_kf) (void)hipFree(c->d_kf);
    if (c->d_list) (void)hipFree(c->d_list);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// A cell map owned by a history may be fed on that history's service thread (ll_history_set_cell_map_async): every public entry point
// that reads or changes a map first waits for the frames handed over so far (and reports the feeder's failure, if any), so a handle
// borrowed from ll_history_cell_map never sees an append in flight or a map swapped by cellmap_grow under it.
int ll::cellmap_settle(const ll_cellmap *c) { return (c && c->owner) ? history_cells_drain(c->owner) : 0; }

extern "C" int ll_cellmap_create(int32_t device, int64_t max_points, float resolution, int32_t minimum_revisit_threshold, ll_cellmap **out)
{
    if (!out) return set_err("ll_cellmap_create", "null argument");
    if (max_points < 1 || max_points >= 0x3fffffffLL) return set_err("ll_cellmap_create", "max_points out of range");
    if (!(resolution > 0.f)) return set_err("ll_cellmap_create", "resolution must be positive");
    if (check_device(device)) return -1;
    ll_cellmap *c = new ll_cellmap();
    c->device = device;
    const char *err = nullptr;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || cellmap_alloc(c->dev, (int)max_points, resolution, minimum_revisit_threshold, &err) ||
        hipMalloc((void **)&c->d_in, (size_t)max_points * sizeof(float4)) != hipSuccess || hipMalloc((void **)&c->d_pose, 8 * sizeof(double)) != hipSuccess) {
        cellmap_release(c);
        return set_err("ll_cellmap_create", err ? err : "allocation failed");
    }
    *out = c;
    return 0;
}

extern "C" void ll_cellmap_destroy(ll_cellmap *c) { cellmap_release(c); }

// capacity -> max_points (larger than the present one), content kept; the staging buffer follows
int ll::cellmap_make_room(ll_cellmap *c, int64_t max_points, const char *where)
{
    HC(hipSetDevice(c->device));
    const char *err = nullptr;
    if (cellmap_grow(c->dev, (int)max_points, c->stream, &err)) return set_err(where, err ? err : "allocation failed");
    float4 *d_new = nullptr;
    HC(hipMalloc((void **)&d_new, (size_t)max_points * sizeof(float4)));
    if (c->d_in) (void)hipFree(c->d_in);
    c->d_in = d_new;
    if (c->d_stats) {  // (sized by the capacity: allocated again by the next ll_cellmap_features / ll_cellmap_keyframe_images)
        (void)hipFree(c->d_stats);
        c->d_stats = nullptr;
    }
    return 0;
}

// Points_cloud_map grows on the heap without bound (CMK:619-672); the device map has a capacity: raise it, content kept.
extern "C" int ll_cellmap_reserve(ll_cellmap *c, int64_t max_points)
{
    if (!c) return set_err("ll_cellmap_reserve", "null argument");
    if (cellmap_settle(c)) return -1;
    if (max_points < 1 || max_points >= 0x3fffffffLL) return set_err("ll_cellmap_reserve", "max_points out of range");
    if (max_points <= c->dev.cap) return 0;
    return cellmap_make_room(c, max_points, "ll_cellmap_reserve");
}

extern "C" int ll_cellmap_append(ll_cellmap *c, const float *xyzi, int32_t n)
{
    if (!c || (n > 0 && !xyzi)) return set_err("ll_cellmap_append", "null argument");
    if (cellmap_settle(c)) return -1;
    if (n < 0 || n > c->dev.cap) return set_err("ll_cellmap_append", "cloud exceeds max_points");
    HC(hipSetDevice(c->device));
    if (n > 0) HC(hipMemcpyAsync(c->d_in, xyzi, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    const char *err = nullptr;
    if (cellmap_append(c->dev, c->d_in, n, c->stream, &err)) return set_err("ll_cellmap_append", err);
    HC(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int ll_cellmap_append_touched(ll_cellmap *c, const float *xyzi, int32_t n, int32_t min_points, int32_t *cell_ijk,
                                         int64_t capacity_cells, int64_t *n_touched)
{
    if (!c || (n > 0 && !xyzi) || !n_touched) return set_err("ll_cellmap_append_touched", "null argument");
    if (cellmap_settle(c)) return -1;
    if (n < 0 || n > c->dev.cap) return set_err("ll_cellmap_append_touched", "cloud exceeds max_points");
    HC(hipSetDevice(c->device));
    const bool first = c->dev.n_cells == 0;  // set_point_cloud: every cell that received a point (CMK:596-607)
    const int n_before = c->dev.n_pts;
    if (n > 0) HC(hipMemcpyAsync(c->d_in, xyzi, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    const char *err = nullptr;
    if (cellmap_append(c->dev, c->d_in, n, c->stream, &err)) return set_err("ll_cellmap_append_touched", err);
    if (cellmap_touch_counts(c->dev, n_before, n, c->stream, &err)) return set_err("ll_cellmap_append_touched", err);
    const int nc = c->dev.n_cells;
    std::vector<unsigned int> cnt(nc);
    std::vector<unsigned long long> keys(nc);
    if (nc > 0) {
        HC(hipMemcpyAsync(cnt.data(), c->dev.csel, (size_t)nc * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        HC(hipMemcpyAsync(keys.data(), c->dev.ckey, (size_t)nc * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    }
    HC(hipStreamSynchronize(c->stream));
    const unsigned int need = first ? 1u : (unsigned int)(min_points > 1 ? min_points : 1);
    int64_t k = 0;
    for (int i = 0; i < nc; i++) {
        if (cnt[i] < need) continue;
        // (the append is committed by now: a short buffer truncates the list, it does not fail the call -- a retry would append the
        //  cloud a second time.  *n_touched is always the full count; more than capacity_cells means the list was cut.)
        if (cell_ijk && k < capacity_cells) cell_unpack(keys[i], cell_ijk + 3 * (size_t)k);
        k++;
    }
    *n_touched = k;
    return 0;
}

extern "C" int ll_cellmap_query_filter(ll_cellmap *c, const double pose[7], float radius, float maximum_in_fov_angle, float leaf,
                                       int32_t down_sample_replace, int64_t *n_cells_selected, int64_t *n_out)
{
    if (!c || !pose) return set_err("ll_cellmap_query_filter", "null argument");
    if (cellmap_settle(c)) return -1;
    if (!(radius >= 0.f)) return set_err("ll_cellmap_query_filter", "radius must not be negative");
    HC(hipSetDevice(c->device));
    HC(hipMemcpyAsync(c->d_pose, pose, 7 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const char *err = nullptr;
    if (cellmap_query_filter(c->dev, c->d_pose, radius, maximum_in_fov_angle, leaf, down_sample_replace, c->stream, &err))
        return set_err("ll_cellmap_query_filter", err);
    HC(hipStreamSynchronize(c->stream));
    if (n_cells_selected) *n_cells_selected = c->dev.n_sel;
    if (n_out) *n_out = c->dev.n_filt;
    return 0;
}

extern "C" int64_t ll_cellmap_result(ll_cellmap *c, float *xyzi, int64_t capacity_points)
{
    if (!c) return set_err("ll_cellmap_result", "null argument");
    if (cellmap_settle(c)) return -1;
    const int64_t n = c->dev.n_filt;
    if (!xyzi) return n;
    if (capacity_points < n) return set_err("ll_cellmap_result", "buffer too small");
    if (hipSetDevice(c->device) != hipSuccess) return set_err("ll_cellmap_result", "hipSetDevice failed");
    if (n > 0 && hipMemcpy(xyzi, c->dev.filt, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess)
        return set_err("ll_cellmap_result", "copy failed");
    return n;
}

extern "C" int ll_cellmap_stats(const ll_cellmap *c, int64_t *n_cells, int64_t *n_points, int32_t *frame_idx)
{
    if (!c) return set_err("ll_cellmap_stats", "null argument");
    if (cellmap_settle(c)) return -1;
    if (n_cells) *n_cells = c->dev.n_cells;
    if (n_points) *n_points = c->dev.n_pts;
    if (frame_idx) *frame_idx = c->dev.frame;
    return 0;
}

extern "C" int ll_cellmap_features(ll_cellmap *c, int32_t *feature_type, float *feature_vector, float *mean, float *cov, float *eigen_val,
                                   int64_t capacity_cells)
{
    if (!c) return set_err("ll_cellmap_features", "null argument");
    if (cellmap_settle(c)) return -1;
    const int nc = c->dev.n_cells;
    if (capacity_cells < nc) return set_err("ll_cellmap_features", "buffer too small");
    if (nc == 0) return 0;
    HC(hipSetDevice(c->device));
    if (!c->d_stats) DM(c->d_stats, (size_t)c->dev.cap);  // a cell holds at least one point
    const char *err = nullptr;
    if (cellmap_stats(c->dev, c->d_stats, c->stream, &err)) return set_err("ll_cellmap_features", err);
    std::vector<CellStats> st(nc);
    HC(hipMemcpyAsync(st.data(), c->d_stats, (size_t)nc * sizeof(CellStats), hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    for (int i = 0; i < nc; i++) {
        if (feature_type) feature_type[i] = st[i].type;
        for (int d = 0; d < 3; d++) {
            if (feature_vector) feature_vector[3 * (size_t)i + d] = st[i].vec[d];
            if (mean) mean[3 * (size_t)i + d] = st[i].mean[d];
            if (eigen_val) eigen_val[3 * (size_t)i + d] = st[i].eval[d];
        }
        if (cov)
            for (int d = 0; d < 6; d++) cov[6 * (size_t)i + d] = st[i].cov[d];
    }
    return 0;
}

extern "C" int ll_cellmap_keyframe_images(ll_cellmap *c, float roi_ratio, float *images, float *ratio_nonzero, float *eigen_R,
                                          int32_t *n_vectors, float *centre_and_range)
{
    if (!c) return set_err("ll_cellmap_keyframe_images", "null argument");
    if (cellmap_settle(c)) return -1;
    if (!(roi_ratio >= 0.f && roi_ratio <= 1.f)) return set_err("ll_cellmap_keyframe_images", "roi_ratio must lie in [0, 1]");
    HC(hipSetDevice(c->device));
    if (!c->d_stats) DM(c->d_stats, (size_t)c->dev.cap);
    if (!c->d_kf) DM(c->d_kf, 1);
    const char *err = nullptr;
    if (cellmap_keyframe_images(c->dev, c->d_stats, roi_ratio, c->d_kf, c->stream, &err)) return set_err("ll_cellmap_keyframe_images", err);
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
    return 0;
}

extern "C" int ll_keyframe_similarity(int32_t device, const float *img_a, const float *img_b, float *similarity)
{
    if (!img_a || !img_b || !similarity) return set_err("ll_keyframe_similarity", "null argument");
    if (check_device(device)) return -1;
    const size_t n = (size_t)LL_KF_RES * LL_KF_RES;
    float *d = nullptr;
    DM(d, 2 * n + 1);
    int rc = 0;
    const char *err = nullptr;
    if (hipMemcpy(d, img_a, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + n, img_b, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || keyframe_similarity(d, d + n, d + 2 * n, nullptr, &err) ||
        hipMemcpy(similarity, d + 2 * n, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        rc = set_err("ll_keyframe_similarity", err ? err : "device copy failed");
    (void)hipFree(d);
    return rc;
}

extern "C" int ll_cellmap_dump(ll_cellmap *c, float *xyzi, int64_t capacity_points, int32_t *cell_ijk, int32_t *cell_start,
                               int32_t *cell_last_update, int64_t capacity_cells)
{
    if (!c) return set_err("ll_cellmap_dump", "null argument");
    if (cellmap_settle(c)) return -1;
    const int np = c->dev.n_pts, nc = c->dev.n_cells;
    if ((xyzi && capacity_points < np) || ((cell_ijk || cell_start || cell_last_update) && capacity_cells < nc))
        return set_err("ll_cellmap_dump", "buffer too small");
    HC(hipSetDevice(c->device));
    if (xyzi && np > 0) HC(hipMemcpy(xyzi, c->dev.pts, (size_t)np * sizeof(float4), hipMemcpyDeviceToHost));
    if (cell_start) {
        if (nc > 0)
            HC(hipMemcpy(cell_start, c->dev.cstart, (size_t)(nc + 1) * sizeof(int), hipMemcpyDeviceToHost));
        else
            cell_start[0] = 0;
    }
    if (cell_last_update && nc > 0) HC(hipMemcpy(cell_last_update, c->dev.clast, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost));
    if (cell_ijk && nc > 0) {
        std::vector<unsigned long long> keys(nc);
        HC(hipMemcpy(keys.data(), c->dev.ckey, (size_t)nc * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int i = 0; i < nc; i++) cell_unpack(keys[i], cell_ijk + 3 * (size_t)i);
    }
    return 0;
}

// The map where it lies: device pointers to the stored points ({x, y, z, 0}, ordered by (cell key, insertion order)) and to the 64-bit
// cell key of every point (21 bits per axis of the cell index + 2^20: ll_cellmap_core.h cell_pack).  Valid until the next call that
// changes this map; the handle's stream has been drained.  The input of the multi-GPU cell-map gather (multigpu.gather_cell_maps).
extern "C" int ll_cellmap_device_view(ll_cellmap *c, const float **dev_xyz0, const uint64_t **dev_point_keys, int64_t *n_points, int64_t *n_cells)
{
    if (!c || !dev_xyz0 || !dev_point_keys || !n_points) return set_err("ll_cellmap_device_view", "null argument");
    if (cellmap_settle(c)) return -1;
    HC(hipSetDevice(c->device));
    HC(hipStreamSynchronize(c->stream));
    *dev_xyz0 = (const float *)c->dev.pts;
    *dev_point_keys = (const uint64_t *)c->dev.pkey;
    *n_points = c->dev.n_pts;
    if (n_cells) *n_cells = c->dev.n_cells;
    return 0;
}

// A key frame's view of the shared cells (CMK:1243-1261): the cells of src named in the list, copied into dst where they lie
// (ll_cellmap_extract_kernels.hip).  Every refusal comes before the first launch; the one host wait before the points move returns
// {cells found, points}, which size dst and become its host mirrors.  The work runs on src's stream: dst's is idle between calls.
extern "C" int ll_cellmap_extract_cells(ll_cellmap *src, const int32_t *cell_ijk, int64_t n_list, ll_cellmap *dst, int64_t *n_cells_found,
                                        int64_t *n_points)
{
    const char *fn = "ll_cellmap_extract_cells";
    if (!src || !dst || (n_list > 0 && !cell_ijk)) return set_err(fn, "null argument");
    if (src == dst) return set_err(fn, "source and destination are the same map");
    if (dst->owner) return set_err(fn, "the destination is owned by a history");
    if (n_list < 0 || n_list >= 0x3fffffffLL) return set_err(fn, "n_list out of range");
    if (src->device != dst->device) return set_err(fn, "source and destination are on different devices");
    if (src->dev.resolution != dst->dev.resolution) return set_err(fn, "source and destination have different resolutions");
    if (cellmap_settle(src)) return -1;
    HC(hipSetDevice(src->device));
    if (n_list > src->list_cap) {
        int *d_new = nullptr;
        HC(hipMalloc((void **)&d_new, (size_t)n_list * 3 * sizeof(int)));
        if (src->d_list) (void)hipFree(src->d_list);
        src->d_list = d_new;
        src->list_cap = n_list;
    }
    if (n_list > 0) HC(hipMemcpyAsync(src->d_list, cell_ijk, (size_t)n_list * 3 * sizeof(int), hipMemcpyHostToDevice, src->stream));
    const char *err = nullptr;
    if (cellmap_extract_mark(src->dev, src->d_list, (int)n_list, src->stream, &err)) return set_err(fn, err);
    unsigned long long totals = 0;
    HC(hipMemcpyAsync(&totals, src->dev.skey2 + src->dev.n_cells, sizeof(totals), hipMemcpyDeviceToHost, src->stream));
    HC(hipStreamSynchronize(src->stream));
    const int found = (int)(totals >> 32), points = (int)(totals & 0xffffffffu);
    if (points > dst->dev.cap && cellmap_make_room(dst, points, fn)) return -1;
    if (cellmap_extract_cells(src->dev, dst->dev, found, points, src->stream, &err)) return set_err(fn, err);
    HC(hipStreamSynchronize(src->stream));
    if (n_cells_found) *n_cells_found = found;
    if (n_points) *n_points = points;
    return 0;
}
