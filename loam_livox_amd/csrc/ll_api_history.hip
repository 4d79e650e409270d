// ll_api_history.hip -- the match-buffer history handle (ll_history_*) of the C ABI: the frame ring, its cell maps and their
// service thread, the refreshes that publish a new search grid into an ll_map.
#include "ll_api_internal.h"

// history-owned cell maps grow with the sequence (the reference's cells live on the heap, CMK:619-672): twice the capacity when the
// next cloud would not fit
static int history_cells_append(ll_history *h, int kind, const float4 *d_src, int n, std::string *why)
{
    ll_cellmap *c = h->cells[kind];
    const char *err = nullptr;
    if ((long long)c->dev.n_pts + n > c->dev.cap) {
        long long want = 2LL * c->dev.cap;
        while (want < (long long)c->dev.n_pts + n) want *= 2;
        if (want >= 0x3fffffffLL) {
            *why = "cell map cannot grow further";
            return -1;
        }
        // the staging buffer of the new capacity first: a failure then leaves the map as it was (capacity and staging size agree)
        float4 *d_new = nullptr;
        if (hipMalloc((void **)&d_new, (size_t)want * sizeof(float4)) != hipSuccess) {
            *why = "allocation failed";
            return -1;
        }
        if (cellmap_grow(c->dev, (int)want, c->stream, &err)) {
            (void)hipFree(d_new);
            *why = err ? err : "cell map cannot grow further";
            return -1;
        }
        if (c->d_in) (void)hipFree(c->d_in);
        c->d_in = d_new;
        if (c->d_stats) {
            (void)hipFree(c->d_stats);
            c->d_stats = nullptr;
        }
    }
    if (cellmap_append(c->dev, d_src, n, c->stream, &err)) {
        *why = err ? err : "append failed";
        return -1;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
        *why = "stream error";
        return -1;
    }
    return 0;
}

static void history_feeder_main(ll_history *h)
{
    (void)hipSetDevice(h->device);
    for (;;) {
        ll_history::FeedJob job;
        {
            std::unique_lock<std::mutex> lk(h->mu);
            h->cv_job.wait(lk, [h] { return h->stop || !h->jobs.empty(); });
            if (h->jobs.empty()) return;  // (stop, and nothing left)
            job = h->jobs.front();
            h->jobs.pop_front();
        }
        std::string why;
        bool failed = false;
        bool skip = false;
        {
            std::lock_guard<std::mutex> lk(h->mu);
            skip = !h->feed_error.empty();  // latched: after a failure nothing more is appended (a map that silently lacks one frame is worse than none)
        }
        if (skip) {
            (void)hipEventSynchronize(job.ready);
        } else if (hipEventSynchronize(job.ready) != hipSuccess) {
            failed = true;
            why = "staging copy failed";
        } else if (history_cells_append(h, job.kind, h->stage[job.kind][job.slot], job.n, &why)) {
            failed = true;
        }
        (void)hipEventDestroy(job.ready);
        {
            std::lock_guard<std::mutex> lk(h->mu);
            if (failed && h->feed_error.empty()) h->feed_error = why;
            h->in_flight--;
        }
        h->cv_idle.notify_all();
    }
}

// every frame handed to the feeder has been appended; 0, or -1 with the feeder's first error.  The error is LATCHED: the feeder stops
// appending at its first failure and every reader / ll_history_add* reports it until ll_history_set_cell_map_async(h, 0) acknowledges
// it (the cell maps then lack the frames from the failing one on; the caller decides whether to go on inline or to start over).
int ll::history_cells_drain(ll_history *h)
{
    if (!h->cells_async) return 0;
    std::unique_lock<std::mutex> lk(h->mu);
    h->cv_idle.wait(lk, [h] { return h->in_flight == 0; });
    if (!h->feed_error.empty()) return set_err("ll_history (cell-map feeder)", ("feeding stopped at its first failure: " + h->feed_error).c_str());
    return 0;
}

extern "C" void ll_history_destroy(ll_history *h);
static int history_create_impl(int32_t device, int32_t maximum_history_size, int32_t max_points_per_frame, float line_res, float plane_res,
                               ll_history *h);
extern "C" int ll_history_create(int32_t device, int32_t maximum_history_size, int32_t max_points_per_frame, float line_res,
                                 float plane_res, ll_history **out)
{
    if (!out) return set_err("ll_history_create", "null argument");
    if (maximum_history_size < 1 || max_points_per_frame < 1) return set_err("ll_history_create", "bad capacity");
    if (!(line_res > 0.f) || !(plane_res > 0.f)) return set_err("ll_history_create", "resolutions must be positive");
    if ((int64_t)(maximum_history_size + 1) * max_points_per_frame >= 0x7fffffffLL) return set_err("ll_history_create", "history too large");
    if (check_device(device)) return -1;
    ll_history *h = new ll_history();
    if (history_create_impl(device, maximum_history_size, max_points_per_frame, line_res, plane_res, h)) {
        ll_history_destroy(h);
        return -1;
    }
    *out = h;
    return 0;
}

static int history_create_impl(int32_t device, int32_t maximum_history_size, int32_t max_points_per_frame, float line_res, float plane_res,
                               ll_history *h)
{
    h->device = device;
    h->max_hist = maximum_history_size;
    h->max_pts = max_points_per_frame;
    h->res[0] = line_res;
    h->res[1] = plane_res;
    HC(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const size_t slots = (size_t)maximum_history_size + 1, cap = slots * max_points_per_frame;
    for (int k = 0; k < 2; k++) {
        DM(h->frames[k], cap);
        DM(h->d_map[k], cap);
        h->count[k].assign(slots, 0);
    }
    DM(h->d_in, (size_t)max_points_per_frame);
    DM(h->d_xf, (size_t)max_points_per_frame);
    DM(h->d_concat, cap);
    DM(h->d_n, 1);
    DM(h->d_pose, 8);
    DM(h->d_table, 2 * (LL_HIST_CONCAT_MAX + 1));
    HC(hipHostMalloc((void **)&h->hp_table, 2 * (LL_HIST_CONCAT_MAX + 1) * sizeof(int2), hipHostMallocDefault));
    const char *err = nullptr;
    if (voxel_alloc(h->vox_frame, 1, max_points_per_frame, &err) || voxel_alloc(h->vox_map, 1, (int)cap, &err))
        return set_err("ll_history_create", err);
    return 0;
}

extern "C" void ll_history_destroy(ll_history *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    voxel_free(h->vox_frame);
    voxel_free(h->vox_map);
    voxel_free(h->vox_cells);
    if (h->feeder.joinable()) {
        {
            std::lock_guard<std::mutex> lk(h->mu);
            h->stop = true;
        }
        h->cv_job.notify_all();
        h->feeder.join();
    }
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < ll_history::kStage; i++)
            if (h->stage[k][i]) (void)hipFree(h->stage[k][i]);
    for (int k = 0; k < 2; k++) cellmap_release(h->cells[k]);
    if (h->hp_table) (void)hipHostFree(h->hp_table);
    void *ptrs[] = {h->frames[0], h->frames[1], h->d_map[0], h->d_map[1], h->d_in, h->d_xf, h->d_concat, h->d_n, h->d_pose, h->d_cmap[0], h->d_cmap[1], h->d_table, h->d_und};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (h->ev_und) (void)hipEventDestroy(h->ev_und);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

extern "C" int32_t ll_history_size(const ll_history *h) { return h ? h->size : -1; }

// one kind of one frame: d_src (sensor frame, n points on the device) -> map frame -> VoxelGrid.  The filtered frame stays
// in h->vox_frame.out; *n_out = its size.
static int history_filter_kind(ll_history *h, int kind, const float4 *d_src, int n, int *n_out)
{
    *n_out = 0;
    if (n <= 0) return 0;
    if (h->use_und)  // g_if_undistore = 1: every point with the pose interpolated at its time stamp (PCR:641-646)
        launch_cloud_undistort(h->d_und, nullptr, UndistortJob{0, n, 0, 0}, 1, n, d_src, nullptr, nullptr, h->d_xf, h->stream);
    else
        launch_cloud_transform(d_src, h->d_xf, n, h->d_pose, h->stream);  // laser_mapping.hpp:1421-1431
    HC(hipMemcpyAsync(h->d_n, &n, sizeof(int), hipMemcpyHostToDevice, h->stream));
    const float leaf[3] = {h->res[kind], h->res[kind], h->res[kind]};
    const char *err = nullptr;
    if (voxel_filter(h->vox_frame, h->d_xf, h->d_n, n, 1, leaf, h->stream, &err)) return set_err("ll_history_add", err);  // :1434-1437
    HC(hipMemcpyAsync(n_out, h->vox_frame.n_out, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HC(hipStreamSynchronize(h->stream));
    return 0;
}

// ... -> ring slot (when the frame is pushed) and -> cell map (when enabled; every registered frame, :1492-1493)
static int history_push_kind(ll_history *h, int kind, const float4 *d_src, int n, int slot, bool push)
{
    int n_out = 0;
    if (history_filter_kind(h, kind, d_src, n, &n_out)) return -1;
    if (push) {
        if (n_out > 0)
            HC(hipMemcpyAsync(h->frames[kind] + (size_t)slot * h->max_pts, h->vox_frame.out, (size_t)n_out * sizeof(float4),
                              hipMemcpyDeviceToDevice, h->stream));
        h->count[kind][slot] = n_out;
    }
    if (h->cells[kind] && h->cells_async) {
        // hand the filtered frame to the feeder: copy into the next staging slot (free again: at most kStage frames are in flight)
        {
            std::unique_lock<std::mutex> lk(h->mu);
            h->cv_idle.wait(lk, [h] { return h->in_flight < ll_history::kStage; });
            if (!h->feed_error.empty()) return set_err("ll_history_add (cell-map feeder)", ("feeding stopped at its first failure: " + h->feed_error).c_str());
        }
        const int slot = h->stage_next[kind];
        h->stage_next[kind] = (slot + 1) % ll_history::kStage;
        if (n_out > 0)
            HC(hipMemcpyAsync(h->stage[kind][slot], h->vox_frame.out, (size_t)n_out * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
        ll_history::FeedJob job{kind, slot, n_out, nullptr};
        HC(hipEventCreateWithFlags(&job.ready, hipEventDisableTiming));
        HC(hipEventRecord(job.ready, h->stream));
        {
            std::lock_guard<std::mutex> lk(h->mu);
            h->jobs.push_back(job);
            h->in_flight++;
        }
        h->cv_job.notify_one();
    } else if (h->cells[kind]) {
        std::string why;
        if (history_cells_append(h, kind, h->vox_frame.out, n_out, &why)) return set_err("ll_history_add (cell map)", why.c_str());
    }
    HC(hipStreamSynchronize(h->stream));
    return 0;
}

// The add-frame rule (laser_mapping.hpp:1439-1448): a history that is not full takes every frame; a full one takes a frame whose
// gate pose lies further than one of the two steps from the pose recorded at the last push.
bool ll::history_add_frame(const double gate_pose[7], const double last_q[4], const double last_t[3], int size, int capacity, double t_step,
                           double angle_step)
{
    const double r_diff = quat_angular_distance(gate_pose, last_q) * 57.3;
    const double dt[3] = {gate_pose[4] - last_t[0], gate_pose[5] - last_t[1], gate_pose[6] - last_t[2]};
    const double t_diff = sqrt(dot3(dt, dt));
    return size < capacity || t_diff > t_step || r_diff > angle_step * 57.3;  // :1446-1448
}

static int history_add_common(ll_history *h, const float4 *d_corner, int n_corner, const float4 *d_surf, int n_surf, const double pose[7],
                              double t_step, double angle_step, int32_t *added)
{
    if (n_corner > h->max_pts || n_surf > h->max_pts) return set_err("ll_history_add", "frame exceeds max_points_per_frame");
    // laser_mapping.hpp:1439-1440: the rule gates on the node's m_q_w_curr / m_t_w_curr -- still the pose BEFORE this
    // registration there (it is copied back at :1496-1500).  That gate pose is
    // handed over by ll_history_set_gate_pose (one-shot); without it the transform pose gates (identical results while
    // history_add_t_step = history_add_angle_step = 0, the reference's fixed values: every frame is pushed).
    const double *gp = h->has_gate ? h->gate : pose;
    h->has_gate = false;
    h->use_und = h->has_und;  // one-shot too (ll_history_set_undistort): this add's two clouds move with the registration's record
    h->has_und = false;
    const bool push = history_add_frame(gp, h->last_q, h->last_t, h->size, h->max_hist, t_step, angle_step);
    if (added) *added = push ? 1 : 0;
    if (!push && !h->cells[0]) return 0;
    const int slots = h->max_hist + 1;
    const int slot = (h->head + h->size) % slots;
    HC(hipMemcpyAsync(h->d_pose, pose, 7 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (history_push_kind(h, 0, d_corner, n_corner, slot, push)) return -1;
    if (history_push_kind(h, 1, d_surf, n_surf, slot, push)) return -1;
    if (!push) return 0;
    for (int i = 0; i < 4; i++) h->last_q[i] = gp[i];  // :1450-1451
    for (int i = 0; i < 3; i++) h->last_t[i] = gp[4 + i];
    h->size++;
    if (h->size > h->max_hist) {  // :1463-1473 pop_front
        h->head = (h->head + 1) % slots;
        h->size--;
    }
    HC(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int ll_history_set_gate_pose(ll_history *h, const double pose[7])
{
    if (!h || !pose) return set_err("ll_history_set_gate_pose", "null argument");
    for (int i = 0; i < 7; i++) h->gate[i] = pose[i];
    h->has_gate = true;
    return 0;
}

// g_if_undistore = 1 for the next add (laser_mapping.hpp:1424,1430): slot `slot` of the registration r collected last.  The record is copied
// on the registrar's stream into memory of this handle -- the registrar's next enqueue may follow at once -- and this handle's stream
// waits for the copy on the device; the host waits for nothing.
extern "C" int ll_history_set_undistort(ll_history *h, ll_reg *r, int32_t slot)
{
    static const char *where = "ll_history_set_undistort";
    if (!h || !r) return set_err(where, "null argument");
    if (r->device != h->device) return set_err(where, "registrar lives on another device");
    if (slot < 0) return set_err(where, "negative slot");
    if (reg_undistort_records(where, r, slot + 1)) return -1;
    if (!h->d_und) {
        DM(h->d_und, 1);
        HC(hipEventCreateWithFlags(&h->ev_und, hipEventDisableTiming));
    }
    HC(hipMemcpyAsync(h->d_und, r->d_und + slot, sizeof(UndistortRec), hipMemcpyDeviceToDevice, r->stream));
    HC(hipEventRecord(h->ev_und, r->stream));
    HC(hipStreamWaitEvent(h->stream, h->ev_und, 0));
    h->has_und = true;
    return 0;
}

extern "C" int ll_history_add(ll_history *h, const float *corner_xyzi, int32_t n_corner, const float *surf_xyzi, int32_t n_surf,
                              const double pose[7], double history_add_t_step, double history_add_angle_step, int32_t *added)
{
    if (!h || !pose || (n_corner > 0 && !corner_xyzi) || (n_surf > 0 && !surf_xyzi)) return set_err("ll_history_add", "null argument");
    if (n_corner < 0 || n_surf < 0 || n_corner > h->max_pts || n_surf > h->max_pts) return set_err("ll_history_add", "frame exceeds max_points_per_frame");
    HC(hipSetDevice(h->device));
    // the two kinds are staged one after the other through d_in: copy the surface cloud to the concat scratch first
    if (n_corner > 0) HC(hipMemcpyAsync(h->d_in, corner_xyzi, (size_t)n_corner * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    if (n_surf > 0) HC(hipMemcpyAsync(h->d_concat, surf_xyzi, (size_t)n_surf * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    return history_add_common(h, h->d_in, n_corner, h->d_concat, n_surf, pose, history_add_t_step, history_add_angle_step, added);
}

// slot `slot` of a device-resident producer: wait for it, read the two counts, offset the two stacks
static int history_add_view(ll_history *h, const FeatView &v, int slot, const double pose[7], double t_step, double angle_step, int32_t *added)
{
    HC(hipSetDevice(h->device));
    if (feat_sync(v)) return -1;
    int nc = 0, ns = 0;
    HC(hipMemcpy(&nc, v.n_corner + slot, sizeof(int), hipMemcpyDeviceToHost));
    HC(hipMemcpy(&ns, v.n_surf + slot, sizeof(int), hipMemcpyDeviceToHost));
    return history_add_common(h, v.corner + (size_t)slot * v.stride_c, nc, v.surf + (size_t)slot * v.stride_s, ns, pose, t_step, angle_step, added);
}

extern "C" int ll_history_add_fe(ll_history *h, ll_fe *fe, int32_t scan, const double pose[7], double history_add_t_step,
                                 double history_add_angle_step, int32_t *added)
{
    if (!h || !fe || !pose) return set_err("ll_history_add_fe", "null argument");
    if (fe->prm.device != h->device) return set_err("ll_history_add_fe", "extractor lives on another device");
    if (scan < 0 || scan >= fe->prm.max_scans) return set_err("ll_history_add_fe", "scan slot out of range");
    return history_add_view(h, feat_view(fe), scan, pose, history_add_t_step, history_add_angle_step, added);
}

extern "C" int ll_history_add_voxel(ll_history *h, ll_voxel *vc, ll_voxel *vs, int32_t cloud, const double pose[7],
                                    double history_add_t_step, double history_add_angle_step, int32_t *added)
{
    if (!h || !vc || !vs || !pose) return set_err("ll_history_add_voxel", "null argument");
    if (vc->device != h->device || vs->device != h->device) return set_err("ll_history_add_voxel", "handles live on different devices");
    if (cloud < 0 || cloud >= vc->dev.max_clouds || cloud >= vs->dev.max_clouds) return set_err("ll_history_add_voxel", "cloud index out of range");
    return history_add_view(h, feat_view(vc, vs), cloud, pose, history_add_t_step, history_add_angle_step, added);
}

// a spin handle's stacks (ll_spin_api.hip spin_handoff), device to device
extern "C" int ll_history_add_spin(ll_history *h, ll_spin *sp, int32_t scan, const double pose[7], double history_add_t_step,
                                   double history_add_angle_step, int32_t *added)
{
    if (!h || !sp || !pose) return set_err("ll_history_add_spin", "null argument");
    if (h->has_und) {  // (dropped with the refusal: the handle goes on with plain adds)
        h->has_und = false;
        return set_err("ll_history_add_spin", "ll_history_set_undistort does not apply: the spinning extractor writes intensity = scanID + scanPeriod * relTime "
                                              "(laser_feature_extractor.hpp:502), which is no time stamp of refine_blur (point_cloud_registration.hpp:128-141)");
    }
    SpinView v;
    spin_view(sp, &v);
    if (v.device != h->device) return set_err("ll_history_add_spin", "extractor lives on another device");
    if (scan < 0 || scan >= v.max_scans) return set_err("ll_history_add_spin", "scan slot out of range");
    if (spin_handoff(sp, scan + 1, &v)) return -1;
    return history_add_view(h, feat_view(v), scan, pose, history_add_t_step, history_add_angle_step, added);
}

extern "C" int ll_history_refresh(ll_history *h, ll_map *map, int64_t *n_map_corner, int64_t *n_map_surf)
{
    if (!h || !map) return set_err("ll_history_refresh", "null argument");
    if (map->device != h->device) return set_err("ll_history_refresh", "map lives on another device");
    HC(hipSetDevice(h->device));
    const int slots = h->max_hist + 1;
    for (int kind = 0; kind < 2; kind++) {
        // laser_mapping.hpp:519-530: concatenate the history, oldest frame first
        int total = 0;
        if (h->size <= LL_HIST_CONCAT_MAX && h->hp_table) {  // one gather launch (the table travels as one small pinned copy)
            int2 *tab = h->hp_table + (size_t)kind * (LL_HIST_CONCAT_MAX + 1);
            int n_seg = 0;
            for (int i = 0; i < h->size; i++) {
                const int slot = (h->head + i) % slots;
                const int c = h->count[kind][slot];
                if (c > 0) tab[n_seg++] = make_int2((int)((size_t)slot * h->max_pts), total);  // (ring size x max_pts < 2^31: ll_history_create)
                total += c;
            }
            tab[n_seg] = make_int2(0, total);
            if (total > 0) {
                int2 *d_tab = h->d_table + (size_t)kind * (LL_HIST_CONCAT_MAX + 1);
                HC(hipMemcpyAsync(d_tab, tab, (size_t)(n_seg + 1) * sizeof(int2), hipMemcpyHostToDevice, h->stream));
                launch_history_concat(h->frames[kind], d_tab, n_seg, total, h->d_concat, h->stream);
            }
        } else {
            for (int i = 0; i < h->size; i++) {
                const int slot = (h->head + i) % slots;
                const int c = h->count[kind][slot];
                if (c > 0)
                    HC(hipMemcpyAsync(h->d_concat + total, h->frames[kind] + (size_t)slot * h->max_pts, (size_t)c * sizeof(float4),
                                      hipMemcpyDeviceToDevice, h->stream));
                total += c;
            }
        }
        int n_out = 0;
        if (total > 0) {
            HC(hipMemcpyAsync(h->d_n, &total, sizeof(int), hipMemcpyHostToDevice, h->stream));
            const float leaf[3] = {h->res[kind], h->res[kind], h->res[kind]};
            const char *err = nullptr;
            if (voxel_filter(h->vox_map, h->d_concat, h->d_n, total, 1, leaf, h->stream, &err)) return set_err("ll_history_refresh", err);  // :533-537
            HC(hipMemcpyAsync(&n_out, h->vox_map.n_out, sizeof(int), hipMemcpyDeviceToHost, h->stream));
            HC(hipStreamSynchronize(h->stream));
            HC(hipMemcpyAsync(h->d_map[kind], h->vox_map.out, (size_t)n_out * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
        }
        h->n_map[kind] = n_out;
        h->map_src[kind] = h->d_map[kind];
        // the search structure (laser_mapping.hpp:539-546: two KdTreeFLANN::setInputCloud) is the device grid
        const char *err = nullptr;
        const float cell = match_cell_size(kind, h->res[kind]);
        if (map_rebuild(map, kind, (const float *)h->d_map[kind], 4, n_out, cell, h->stream, &err)) return set_err("map_build", err ? err : "failed");
    }
    HC(hipStreamSynchronize(h->stream));
    if (n_map_corner) *n_map_corner = h->n_map[0];
    if (n_map_surf) *n_map_surf = h->n_map[1];
    return 0;
}

extern "C" int64_t ll_history_map_cloud(ll_history *h, int32_t kind, float *xyzi, int64_t capacity_points)
{
    if (!h || kind < 0 || kind > 1) return set_err("ll_history_map_cloud", "bad argument");
    const int64_t n = h->n_map[kind];
    if (!xyzi) return n;
    if (capacity_points < n) return set_err("ll_history_map_cloud", "buffer too small");
    if (hipSetDevice(h->device) != hipSuccess) return set_err("ll_history_map_cloud", "hipSetDevice failed");
    if (n > 0 && hipMemcpy(xyzi, h->map_src[kind], (size_t)n * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess)
        return set_err("ll_history_map_cloud", "copy failed");
    return n;
}

extern "C" int ll_history_map_cloud_device(ll_history *h, int32_t kind, const float **dev_xyzi, int64_t *n_points)
{
    if (!h || !dev_xyzi || !n_points || kind < 0 || kind > 1) return set_err("ll_history_map_cloud_device", "bad argument");
    HC(hipSetDevice(h->device));
    HC(hipStreamSynchronize(h->stream));
    *dev_xyzi = (const float *)h->map_src[kind];
    *n_points = h->n_map[kind];
    return 0;
}

float ll::match_cell_size(int kind, float leaf)
{
    // Cell size from the voxel leaf the buffer has just been filtered with: the points are about one leaf apart (along
    // the edges for the corner cloud, across the surfaces for the other), and a search is fastest with a handful of
    // points per cell.  The default corner cell (1.45 m, sized for a sparse edge map and the sqrt(2) m line radius)
    // would put hundreds of candidates of a dense local edge map into the query's own cells.
    return (kind == LL_MAP_CORNER) ? fminf(fmaxf(4.0f * leaf, 0.4f), 1.45f) : fminf(fmaxf(3.0f * leaf, 0.45f), 1.2f);
}

extern "C" int ll_history_enable_cell_map(ll_history *h, int64_t max_points, float cell_resolution, int32_t threshold_cell_revisit)
{
    if (!h) return set_err("ll_history_enable_cell_map", "null argument");
    if (h->cells[0]) return set_err("ll_history_enable_cell_map", "already enabled");
    if (max_points < h->max_pts) return set_err("ll_history_enable_cell_map", "max_points below max_points_per_frame");
    HC(hipSetDevice(h->device));
    const char *err = nullptr;
    bool ok = true;
    for (int k = 0; k < 2 && ok; k++) {
        // laser_mapping.hpp:620-624: set_resolution( m_pt_cell_resolution ), m_minimum_revisit_threshold
        ok = ll_cellmap_create(h->device, max_points, cell_resolution, threshold_cell_revisit, &h->cells[k]) == 0 &&
             hipMalloc((void **)&h->d_cmap[k], (size_t)max_points * sizeof(float4)) == hipSuccess;
    }
    if (ok && voxel_alloc(h->vox_cells, 1, (int)max_points, &err)) ok = false;
    if (ok) h->cells[0]->owner = h->cells[1]->owner = h;  // (every ll_cellmap_* call on them settles the service thread first, cellmap_settle)
    if (!ok) {  // all or nothing: a half-enabled history would fail later in ll_history_refresh_cells
        const std::string why = err ? std::string(err) : g_err;
        voxel_free(h->vox_cells);
        for (int k = 0; k < 2; k++) {
            cellmap_release(h->cells[k]);
            h->cells[k] = nullptr;
            if (h->d_cmap[k]) (void)hipFree(h->d_cmap[k]);
            h->d_cmap[k] = nullptr;
        }
        return set_err("ll_history_enable_cell_map", why.empty() ? "allocation failed" : why.c_str());
    }
    return 0;
}

// NULL with ll_last_error() set: bad argument, cell maps not enabled, or the service thread failed.  The handle stays the history's: every
// ll_cellmap_* call on it waits for the frames handed to the service thread so far, so it may be kept across ll_history_add*; what
// ll_cellmap_device_view returns for it is valid only until the next ll_history_add* (which may grow and move the map).
extern "C" ll_cellmap *ll_history_cell_map(ll_history *h, int32_t kind)
{
    if (!h || kind < 0 || kind > 1) {
        set_err("ll_history_cell_map", "bad argument");
        return nullptr;
    }
    if (!h->cells[kind]) {
        set_err("ll_history_cell_map", "cell maps are not enabled (ll_history_enable_cell_map)");
        return nullptr;
    }
    if (history_cells_drain(h)) return nullptr;  // (the caller is about to read the map)
    return h->cells[kind];
}

// enable != 0: the frames ll_history_add* receives from now on reach the cell maps through a service thread, in order, beside the caller
// (matching mode 0: nothing reads the cell maps between frames); every entry point that reads them -- ll_history_cell_map,
// ll_history_refresh_cells, ll_history_sync_cell_maps -- waits for the frames handed over so far.  enable == 0: drain and append inline
// again (the default).
extern "C" int ll_history_set_cell_map_async(ll_history *h, int32_t enable)
{
    if (!h) return set_err("ll_history_set_cell_map_async", "null argument");
    if (!h->cells[0]) return set_err("ll_history_set_cell_map_async", "cell maps are not enabled (ll_history_enable_cell_map)");
    HC(hipSetDevice(h->device));
    if (!enable) {
        const int rc = history_cells_drain(h);  // (reports a latched feeder error one last time ...)
        h->cells_async = false;
        std::lock_guard<std::mutex> lk(h->mu);
        h->feed_error.clear();                  // (... and acknowledges it)
        return rc;
    }
    if (h->cells_async) return 0;
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < ll_history::kStage; i++)
            if (!h->stage[k][i]) DM(h->stage[k][i], (size_t)h->max_pts);
    if (!h->feeder.joinable()) h->feeder = std::thread(history_feeder_main, h);
    h->cells_async = true;
    return 0;
}

extern "C" int ll_history_sync_cell_maps(ll_history *h)
{
    if (!h) return set_err("ll_history_sync_cell_maps", "null argument");
    return history_cells_drain(h);
}

// update_buff_for_matching with m_matching_mode == 1 (laser_mapping.hpp:471-546)
extern "C" int ll_history_refresh_cells(ll_history *h, ll_map *map, const double pose[7], float maximum_search_range_corner,
                                        float maximum_search_range_surface, float maximum_in_fov_angle, int32_t down_sample_replace,
                                        int64_t *n_map_corner, int64_t *n_map_surf)
{
    if (!h || !map || !pose) return set_err("ll_history_refresh_cells", "null argument");
    if (!h->cells[0]) return set_err("ll_history_refresh_cells", "cell maps are not enabled (ll_history_enable_cell_map)");
    if (map->device != h->device) return set_err("ll_history_refresh_cells", "map lives on another device");
    if (history_cells_drain(h)) return -1;
    HC(hipSetDevice(h->device));
    const float range[2] = {maximum_search_range_corner, maximum_search_range_surface};
    for (int kind = 0; kind < 2; kind++) {
        ll_cellmap *c = h->cells[kind];
        const float leaf1 = h->res[kind];
        // :475-513: cells in range and in the field of view, each through the VoxelGrid, concatenated
        if (ll_cellmap_query_filter(c, pose, range[kind], maximum_in_fov_angle, leaf1, down_sample_replace, nullptr, nullptr)) return -1;
        const int total = c->dev.n_filt;
        int n_out = 0;
        if (total > 0) {
            HC(hipMemcpyAsync(h->d_n, &total, sizeof(int), hipMemcpyHostToDevice, h->stream));
            const float leaf[3] = {leaf1, leaf1, leaf1};
            const char *err = nullptr;
            if (voxel_filter(h->vox_cells, c->dev.filt, h->d_n, total, 1, leaf, h->stream, &err)) return set_err("ll_history_refresh_cells", err);  // :533-537
            HC(hipMemcpyAsync(&n_out, h->vox_cells.n_out, sizeof(int), hipMemcpyDeviceToHost, h->stream));
            HC(hipStreamSynchronize(h->stream));
            HC(hipMemcpyAsync(h->d_cmap[kind], h->vox_cells.out, (size_t)n_out * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
        }
        h->n_map[kind] = n_out;
        h->map_src[kind] = h->d_cmap[kind];
        const char *err = nullptr;
        if (map_rebuild(map, kind, (const float *)h->d_cmap[kind], 4, n_out, match_cell_size(kind, leaf1), h->stream, &err))
            return set_err("map_build", err ? err : "failed");
    }
    HC(hipStreamSynchronize(h->stream));
    if (n_map_corner) *n_map_corner = h->n_map[0];
    if (n_map_surf) *n_map_surf = h->n_map[1];
    return 0;
}
