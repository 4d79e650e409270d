// ll_api_map.hip -- the map handle (ll_map_*) of the C ABI: immutable search-grid snapshots (MapSnap, ll_api_internal.h), their
// publication and pinning, the stand-alone searches over them (ll_map_kernels.hip, ll_knn_kernels.hip).
#include "ll_api_internal.h"

std::shared_ptr<MapSnap> ll::map_pin(const ll_map *cm, int kind)
{
    ll_map *m = const_cast<ll_map *>(cm);
    std::lock_guard<std::mutex> lk(m->mu);
    return m->cur[kind];
}
std::shared_ptr<MapSnap> ll::map_build_target(ll_map *m, int kind)
{
    std::lock_guard<std::mutex> lk(m->mu);
    for (auto &s : m->pool[kind])
        if (s.use_count() == 1) return s;  // referenced by the pool only: not published, not pinned
    std::shared_ptr<MapSnap> s = std::make_shared<MapSnap>();
    s->device = m->device;
    m->pool[kind].push_back(s);
    return s;
}
// returns the generation number this publication got (read under the mutex: a concurrent publisher cannot slip in between)
int64_t ll::map_publish(ll_map *m, int kind, const std::shared_ptr<MapSnap> &s)
{
    std::lock_guard<std::mutex> lk(m->mu);
    m->cur[kind] = s;
    return ++m->generation[kind];
}
// builds the grid of `n` device-resident points into a fresh snapshot and publishes it
int ll::map_rebuild(ll_map *m, int kind, const float *d_raw, int stride, int64_t n, float cell, hipStream_t s, const char **err,
                    int64_t *generation)
{
    std::shared_ptr<MapSnap> t = map_build_target(m, kind);
    if (map_build(t->mk, d_raw, stride, n, cell, s, err)) return -1;  // returns with the stream drained
    const int64_t g = map_publish(m, kind, t);
    if (generation) *generation = g;
    return 0;
}

// the same from a bounding box the caller has read back already (map_bbox_enqueue): only enqueues on s, no host wait
int ll::map_rebuild_boxed(ll_map *m, int kind, const float *d_raw, int stride, int64_t n, float cell, const float mm[6], hipStream_t s, const char **err)
{
    std::shared_ptr<MapSnap> t = map_build_target(m, kind);
    if (map_build_boxed(t->mk, d_raw, stride, n, cell, mm, false, s, err)) return -1;
    map_publish(m, kind, t);
    return 0;
}

extern "C" int ll_map_create(int32_t device, ll_map **out)
{
    if (!out) return set_err("ll_map_create", "null argument");
    if (check_device(device)) return -1;
    ll_map *m = new ll_map();
    m->device = device;
    HC(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    *out = m;
    return 0;
}

extern "C" void ll_map_destroy(ll_map *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    for (int k = 0; k < 2; k++) {
        m->cur[k].reset();
        m->pool[k].clear();  // snapshots still pinned by a registrar die with its pin
    }
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

extern "C" int ll_map_upload(ll_map *m, int32_t kind, const float *xyz, int32_t stride_floats, int64_t n, float cell_size)
{
    return ll_map_upload_gen(m, kind, xyz, stride_floats, n, cell_size, nullptr);
}

extern "C" int ll_map_upload_gen(ll_map *m, int32_t kind, const float *xyz, int32_t stride_floats, int64_t n, float cell_size, int64_t *generation)
{
    if (!m || (!xyz && n > 0)) return set_err("ll_map_upload", "null argument");
    if (kind != LL_MAP_CORNER && kind != LL_MAP_SURF) return set_err("ll_map_upload", "bad kind");
    if (stride_floats < 3) return set_err("ll_map_upload", "stride_floats must be >= 3");
    if (n < 0 || n > 0x7fffffffLL) return set_err("ll_map_upload", "point count out of range");
    HC(hipSetDevice(m->device));
    if (!(cell_size > 0.f)) cell_size = (kind == LL_MAP_CORNER) ? 1.45f : 0.6f;  // corner: just above the line match radius sqrt(2) m (PCR:89)
    float *d_raw = nullptr;
    const size_t bytes = (size_t)(n > 0 ? n : 1) * stride_floats * sizeof(float);
    HC(hipMalloc(&d_raw, bytes));
    if (n > 0 && hipMemcpyAsync(d_raw, xyz, (size_t)n * stride_floats * sizeof(float), hipMemcpyHostToDevice, m->stream) != hipSuccess) {
        (void)hipFree(d_raw);
        return set_err("ll_map_upload", "host to device copy failed");
    }
    const char *err = nullptr;
    const int rc = map_rebuild(m, kind, d_raw, stride_floats, n, cell_size, m->stream, &err, generation);
    (void)hipFree(d_raw);
    if (rc != 0) return set_err("map_build", err ? err : "failed");
    return 0;
}

extern "C" int ll_map_to_f16(ll_map *m, int32_t kind)
{
    if (!m || kind < 0 || kind > 1) return set_err("ll_map_to_f16", "bad argument");
    HC(hipSetDevice(m->device));
    std::shared_ptr<MapSnap> snap = map_pin(m, kind);
    if (!snap) return set_err("ll_map_to_f16", "map kind not uploaded");
    // converts the published snapshot in place (C5 experiment path): the caller must not have a registration in flight
    if (snap.use_count() > 3) return set_err("ll_map_to_f16", "the snapshot is pinned by a registration in flight");
    if (snap->arena) return set_err("ll_map_to_f16", "the snapshot was built by ll_history_batch_refresh: its records live in a shared arena");
    const char *err = nullptr;
    if (map_to_f16(snap->mk, m->stream, &err)) return set_err("ll_map_to_f16", err ? err : "failed");
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->generation[kind]++;  // converted in place: not the structure a host-side cache uploaded any more
    }
    return 0;
}

extern "C" int ll_map_dequantized(ll_map *m, int32_t kind, float *xyz, int64_t capacity_points)
{
    if (!m || kind < 0 || kind > 1 || !xyz) return set_err("ll_map_dequantized", "bad argument");
    std::shared_ptr<MapSnap> snap = map_pin(m, kind);
    if (!snap) return set_err("ll_map_dequantized", "map kind not uploaded");
    const MapKind &mk = snap->mk;
    if (capacity_points < mk.n) return set_err("ll_map_dequantized", "buffer too small");
    HC(hipSetDevice(m->device));
    float *d_out = nullptr;
    const size_t bytes = (size_t)(mk.n > 0 ? mk.n : 1) * 3 * sizeof(float);
    HC(hipMalloc(&d_out, bytes));
    HC(hipMemsetAsync(d_out, 0xff, bytes, m->stream));  // NaN pattern for points that were dropped (non-finite input)
    const char *err = nullptr;
    const int rc = map_f16_dequant(mk, d_out, m->stream, &err);
    if (rc == 0 && mk.n > 0) HC(hipMemcpy(xyz, d_out, (size_t)mk.n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    (void)hipFree(d_out);
    if (rc) return set_err("ll_map_dequantized", err ? err : "failed");
    return 0;
}

extern "C" int64_t ll_map_generation(const ll_map *cm, int32_t kind)
{
    if (!cm || kind < 0 || kind > 1) return -1;
    ll_map *m = const_cast<ll_map *>(cm);
    std::lock_guard<std::mutex> lk(m->mu);
    return m->generation[kind];
}

extern "C" int64_t ll_map_size(const ll_map *m, int32_t kind)
{
    if (!m || kind < 0 || kind > 1) return -1;
    std::shared_ptr<MapSnap> snap = map_pin(m, kind);
    return snap ? snap->mk.n : 0;
}

// cells of the published grid of `kind` (its cell table holds one 32-bit start per cell + 1): the map's footprint in HBM is
// ll_map_size() records + this table (bench_c5.py's algorithmic bytes)
extern "C" int64_t ll_map_cells(const ll_map *m, int32_t kind)
{
    if (!m || kind < 0 || kind > 1) return -1;
    std::shared_ptr<MapSnap> snap = map_pin(m, kind);
    return snap ? (int64_t)snap->mk.ncell : 0;
}

extern "C" int ll_map_knn5(ll_map *m, int32_t kind, const float *queries_xyz, int32_t n_queries, float max_sq_dis, int32_t *idx5,
                           float *sq_dis5)
{
    if (!m || !queries_xyz || !idx5 || !sq_dis5) return set_err("ll_map_knn5", "null argument");
    std::shared_ptr<MapSnap> snap = (kind < 0 || kind > 1) ? nullptr : map_pin(m, kind);
    if (!snap || (!snap->mk.pts && !snap->mk.pts16)) return set_err("ll_map_knn5", "map kind not uploaded");
    if (n_queries <= 0) return 0;
    HC(hipSetDevice(m->device));
    float *d_q = nullptr, *d_d2 = nullptr;
    int *d_idx = nullptr;
    DM(d_q, (size_t)n_queries * 3);
    DM(d_d2, (size_t)n_queries * 5);
    DM(d_idx, (size_t)n_queries * 5);
    HC(hipMemcpyAsync(d_q, queries_xyz, (size_t)n_queries * 3 * sizeof(float), hipMemcpyHostToDevice, m->stream));
    launch_knn5(snap->mk.grid, d_q, n_queries, max_sq_dis, d_idx, d_d2, m->stream);
    HC(hipGetLastError());
    HC(hipMemcpyAsync(idx5, d_idx, (size_t)n_queries * 5 * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HC(hipMemcpyAsync(sq_dis5, d_d2, (size_t)n_queries * 5 * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HC(hipStreamSynchronize(m->stream));
    (void)hipFree(d_q);
    (void)hipFree(d_d2);
    (void)hipFree(d_idx);
    return 0;
}

// The same search with queries and results RESIDENT on the device (pointers from hipMalloc / a torch tensor's data_ptr): nothing crosses
// PCIe, and *kernel_ms (optional) is the search kernel's duration from HIP events on the map's stream -- the figure a roofline needs
// (bench_c5.py).  Synchronous.
extern "C" int ll_map_knn5_device(ll_map *m, int32_t kind, const float *dev_queries_xyz, int64_t n_queries, float max_sq_dis, int32_t *dev_idx5,
                                  float *dev_sq_dis5, float *kernel_ms)
{
    if (!m || !dev_queries_xyz || !dev_idx5 || !dev_sq_dis5) return set_err("ll_map_knn5_device", "null argument");
    if (n_queries < 0 || n_queries > 0x7fffffffLL / 5) return set_err("ll_map_knn5_device", "n_queries out of range");
    std::shared_ptr<MapSnap> snap = (kind < 0 || kind > 1) ? nullptr : map_pin(m, kind);
    if (!snap || (!snap->mk.pts && !snap->mk.pts16)) return set_err("ll_map_knn5_device", "map kind not uploaded");
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_queries == 0) return 0;
    HC(hipSetDevice(m->device));
    struct Events {  // (destroyed on every return path)
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events()
        {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    HC(hipEventCreate(&ev.e0));
    HC(hipEventCreate(&ev.e1));
    HC(hipDeviceSynchronize());  // (the caller's buffers may have been written on another stream)
    HC(hipEventRecord(ev.e0, m->stream));
    launch_knn5(snap->mk.grid, dev_queries_xyz, (int)n_queries, max_sq_dis, dev_idx5, dev_sq_dis5, m->stream);
    HC(hipEventRecord(ev.e1, m->stream));
    HC(hipGetLastError());
    HC(hipStreamSynchronize(m->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.e0, ev.e1);
    if (kernel_ms) *kernel_ms = ms;
    return 0;
}

extern "C" int ll_map_grid_geometry(const float bbox_min_max[6], float cell_size, int32_t dims[3], float *cell, float *slack)
{
    if (!bbox_min_max || !dims || !(cell_size > 0.f)) return set_err("ll_map_grid_geometry", "bad argument");
    Grid g{};
    map_grid_geometry(bbox_min_max, cell_size, g);
    dims[0] = g.nx;
    dims[1] = g.ny;
    dims[2] = g.nz;
    if (cell) *cell = g.h;
    if (slack) *slack = g.slack;
    return 0;
}
