// ll_api_history_batch_buffer.hip -- the batched match buffer of the C ABI: the handle, the adds, the refresh.
// One handle for the histories of S sequences (ll_history_batch_*).  Per slot the semantics are ll_history's; the device work of an
// add and of a refresh is one fixed chain of launches over all slots (ll_history_batch_kernels.hip), and the search grids of one
// refresh live in ONE pooled pair of buffers, an arena.  Every MapSnap built in an arena holds a reference to it, so the immutable
// snapshot contract of ll_map carries over: an arena is taken for the next refresh only when nothing but the handle's pool refers
// to it -- no snapshot built in it is published by a map or pinned by a registration any more.
//
// The deferred stores the handle can keep beside the buffer, and what reads them, are the other three units.
#include "ll_api_history_batch_internal.h"

// grow-only device buffer, half again as large as asked when it has to move
template <typename T>
static int hb_grow(T **p, size_t *cap, size_t need)
{
    if (need <= *cap && *p) return 0;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const size_t want = need + need / 2 + 16;
    HC(hipMalloc((void **)p, want * sizeof(T)));
    *cap = want;
    return 0;
}

static int history_batch_create_impl(ll_history_batch *h)
{
    const size_t S = (size_t)h->S, ring = S * h->slots * h->max_pts, cat = S * h->cstride;
    HC(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (int k = 0; k < 2; k++) {
        DM(h->frames[k], ring);
        h->count[k].assign(S * h->slots, 0);
        h->n_map[k].assign(S, 0);
    }
    h->head.assign(S, 0);
    h->size.assign(S, 0);
    h->last_q.assign(4 * S, 0.0);
    h->last_t.assign(3 * S, 0.0);
    for (size_t s = 0; s < S; s++) h->last_q[4 * s + 3] = 1.0;
    DM(h->d_xf, 2 * S * h->max_pts);
    DM(h->d_nxf, 2 * S);
    DM(h->d_concat, 2 * cat);
    DM(h->d_map, 2 * cat);
    DM(h->d_add, S);
    DM(h->d_cnt, 2 * S);
    h->ref_seg_off = (3 * S * sizeof(int) + 15) / 16 * 16;
    h->ref_bytes = h->ref_seg_off + 2 * S * h->max_hist * sizeof(HbSeg);
    DM(h->d_ref, h->ref_bytes);
    DM(h->d_mm, 2 * S * 8);
    DM(h->d_grid, 2 * S);
    DM(h->d_nvalid, 2 * S);
    HC(hipHostMalloc((void **)&h->hp_add, S * sizeof(HbAddSlot), hipHostMallocDefault));
    HC(hipHostMalloc((void **)&h->hp_cnt, 4 * S * sizeof(int), hipHostMallocDefault));
    HC(hipHostMalloc((void **)&h->hp_ref, h->ref_bytes, hipHostMallocDefault));
    HC(hipHostMalloc((void **)&h->hp_mm_init, 2 * S * 8 * sizeof(unsigned int), hipHostMallocDefault));
    HC(hipHostMalloc((void **)&h->hp_mm, 2 * S * 8 * sizeof(unsigned int), hipHostMallocDefault));
    HC(hipHostMalloc((void **)&h->hp_grid, 2 * S * sizeof(HbGrid), hipHostMallocDefault));
    HC(hipHostMalloc((void **)&h->hp_nvalid, 2 * S * sizeof(int), hipHostMallocDefault));
    for (size_t g = 0; g < 2 * S; g++) hb_aabb_identity(h->hp_mm_init + 8 * g);
    const char *err = nullptr;
    for (int k = 0; k < 2; k++)
        if (voxel_alloc(h->vf[k], h->S, h->max_pts, &err) || voxel_alloc(h->vm[k], h->S, (int)h->cstride, &err))
            return set_err("ll_history_batch_create", err);
    return 0;
}

extern "C" void ll_history_batch_destroy(ll_history_batch *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (int k = 0; k < 2; k++) {
        voxel_free(h->vf[k]);
        voxel_free(h->vm[k]);
    }
    void *dev[] = {h->frames[0], h->frames[1], h->d_xf, h->d_nxf, h->d_concat, h->d_map, h->d_add, h->d_cnt, h->d_ref, h->d_mm, h->d_grid,
                   h->d_nvalid, h->keys, h->keys2, h->vals, h->vals2, h->counts, h->tmp, h->d_cq_tab, h->d_cx_in, h->d_cx_out, h->d_cx_dst, h->d_und};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (h->ev_und) (void)hipEventDestroy(h->ev_und);
    for (int k = 0; k < 2; k++) hb_store_free(h->st[k]);
    hb_full_free(h);
    hb_scan_log_free(h);
    for (const CmbDev &q : h->cq) {
        void *ptrs[] = {q.csel, q.cflag, q.crank, q.ccell, q.key, q.key2, q.val, q.val2, q.hflag, q.hrank, q.head, q.leaf, q.leaf_cell, q.out, q.tmp};
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
    }
    void *host[] = {h->hp_add, h->hp_cnt, h->hp_ref, h->hp_mm_init, h->hp_mm, h->hp_grid, h->hp_nvalid, h->hp_cq_tab, h->hp_cq, h->hp_cx_in,
                    h->hp_cx_out, h->hp_cx_dst};
    for (void *p : host)
        if (p) (void)hipHostFree(p);
    h->arenas.clear();  // (an arena still referenced by a published or pinned snapshot dies with that snapshot)
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

extern "C" int ll_history_batch_create(int32_t device, int32_t n_sequences, int32_t maximum_history_size, int32_t max_points_per_frame,
                                       float line_res, float plane_res, ll_history_batch **out)
{
    static const char *where = "ll_history_batch_create";
    if (!out) return set_err(where, "null argument");
    if (n_sequences < 1) return set_err(where, "n_sequences must be at least 1");
    if (n_sequences > 16384) return set_err(where, "n_sequences above 16384 (a launch covers the slots with its grid's y dimension)");
    if (maximum_history_size < 1 || max_points_per_frame < 1) return set_err(where, "bad capacity");
    if (!(line_res > 0.f) || !(plane_res > 0.f)) return set_err(where, "resolutions must be positive");
    if ((double)n_sequences * (double)maximum_history_size * (double)max_points_per_frame >= 2147483648.0)
        return set_err(where, "n_sequences * maximum_history_size * max_points_per_frame must stay below 2^31 (the sorts index with 32 bits)");
    if (check_device(device)) return -1;
    ll_history_batch *h = new ll_history_batch();
    h->device = device;
    h->S = n_sequences;
    h->max_hist = maximum_history_size;
    h->max_pts = max_points_per_frame;
    h->slots = maximum_history_size + 1;
    h->cstride = (size_t)maximum_history_size * max_points_per_frame;
    h->res[0] = line_res;
    h->res[1] = plane_res;
    if (history_batch_create_impl(h)) {
        const std::string keep = g_err;
        ll_history_batch_destroy(h);
        g_err = keep;
        return -1;
    }
    *out = h;
    return 0;
}

extern "C" int32_t ll_history_batch_size(const ll_history_batch *h, int32_t sequence)
{
    return (h && sequence >= 0 && sequence < h->S) ? h->size[sequence] : -1;
}

// one-shot (ll_history_batch_set_undistort): the records pending for the next add, taken by that add whatever becomes of it -- the
// first thing both entry points do with their handle, ahead of their own refusals
static bool history_batch_take_undistort(ll_history_batch *h)
{
    const bool und = h && h->has_und;
    if (h) h->has_und = false;
    return und;
}

// slots 0 .. S-1 of a device-resident producer; und: this add's clouds move with the registration's records (h->d_und)
static int history_batch_add_common(const char *where, ll_history_batch *h, const FeatView &v, const int32_t *active, const double *poses7,
                                    const double *gate_poses7, double t_step, double angle_step, int32_t *added, bool und)
{
    const int S = h->S;
    HC(hipSetDevice(h->device));
    if (feat_sync(v)) return -1;
    if (added)
        for (int s = 0; s < S; s++) added[s] = 0;
    int *in_n = h->hp_cnt;  // [2][S]
    HC(hipMemcpy(in_n, v.n_corner, (size_t)S * sizeof(int), hipMemcpyDeviceToHost));
    HC(hipMemcpy(in_n + S, v.n_surf, (size_t)S * sizeof(int), hipMemcpyDeviceToHost));
    for (int s = 0; s < S; s++) {
        if (active && !active[s]) continue;
        if (in_n[s] > h->max_pts || in_n[S + s] > h->max_pts || in_n[s] > v.stride_c || in_n[S + s] > v.stride_s)
            return set_err(where, "frame exceeds max_points_per_frame");
    }
    // the add-frame rule per slot (history_add_frame): host arithmetic on the gate poses
    // With cell maps every active slot goes through the transform and the VoxelGrid, pushed or not (laser_mapping.hpp:1492-1493 feeds
    // the cell maps with every registered frame); only the scatter into the ring is left to the rule.
    for (int k = 0; h->cm_on && k < 2; k++) {  // (a store stays below 2^31 points per kind even if the VoxelGrid drops nothing)
        long long bound = h->st[k].dev.n_log;
        for (int s = 0; s < S; s++)
            if (!active || active[s]) bound += in_n[k * S + s] > 0 ? in_n[k * S + s] : 0;
        if (bound >= kCbLimit) return set_err(where, "the cell maps would pass 2^31 stored points per kind");
    }
    int n_work = 0, max_in[2] = {0, 0};
    for (int s = 0; s < S; s++) {
        HbAddSlot &a = h->hp_add[s];
        memset(&a, 0, sizeof(a));
        if (active && !active[s]) continue;
        const double *pose = poses7 + 7 * (size_t)s, *gp = gate_poses7 ? gate_poses7 + 7 * (size_t)s : pose;
        const bool push = history_add_frame(gp, &h->last_q[4 * (size_t)s], &h->last_t[3 * (size_t)s], h->size[s], h->max_hist, t_step, angle_step);
        if (!push && !h->cm_on) continue;
        for (int i = 0; i < 7; i++) a.pose[i] = pose[i];
        a.work = 1;
        a.push = push ? 1 : 0;
        a.ring = (h->head[s] + h->size[s]) % h->slots;
        n_work++;
        for (int k = 0; k < 2; k++) {
            const int n = in_n[k * S + s] > 0 ? in_n[k * S + s] : 0;
            max_in[k] = n > max_in[k] ? n : max_in[k];
        }
    }
    if (n_work == 0) return 0;
    HC(hipMemcpyAsync(h->d_add, h->hp_add, (size_t)S * sizeof(HbAddSlot), hipMemcpyHostToDevice, h->stream));
    if (und)  // g_if_undistore = 1: every point with the pose interpolated at its time stamp (PCR:641-646); the poses still serve the rule and the cell maps
        launch_hb_transform_undistort(v.corner, v.n_corner, v.stride_c, v.surf, v.n_surf, v.stride_s, h->d_add, h->d_und, S, h->max_pts, h->d_xf, h->d_nxf, h->stream);
    else
        launch_hb_transform(v.corner, v.n_corner, v.stride_c, v.surf, v.n_surf, v.stride_s, h->d_add, S, h->max_pts, h->d_xf, h->d_nxf, h->stream);  // :1421-1431
    const char *err = nullptr;
    for (int k = 0; k < 2; k++) {  // :1434-1437
        const float leaf[3] = {h->res[k], h->res[k], h->res[k]};
        if (voxel_filter_bounded(h->vf[k], h->d_xf + (size_t)k * S * h->max_pts, h->d_nxf + (size_t)k * S, h->max_pts, S, leaf, max_in[k], h->stream, &err))
            return set_err(where, err);
    }
    launch_hb_scatter(h->vf[0].out, h->vf[0].n_out, h->vf[1].out, h->vf[1].n_out, h->max_pts, h->d_add, S, h->max_pts, h->slots, h->frames[0],
                      h->frames[1], h->d_cnt, h->stream);
    HC(hipGetLastError());
    int *out_n = h->hp_cnt + 2 * S;
    HC(hipMemcpyAsync(out_n, h->d_cnt, (size_t)2 * S * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (h->cm_on)
        for (int k = 0; k < 2; k++) HC(hipMemcpyAsync(h->st[k].hp_n, h->vf[k].n_out, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HC(hipStreamSynchronize(h->stream));
    for (int s = 0; s < S; s++) {
        const HbAddSlot &a = h->hp_add[s];
        if (!a.push) continue;
        const double *gp = gate_poses7 ? gate_poses7 + 7 * (size_t)s : poses7 + 7 * (size_t)s;
        for (int k = 0; k < 2; k++) h->count[k][(size_t)s * h->slots + a.ring] = out_n[k * S + s];
        for (int i = 0; i < 4; i++) h->last_q[4 * (size_t)s + i] = gp[i];  // :1450-1451
        for (int i = 0; i < 3; i++) h->last_t[3 * (size_t)s + i] = gp[4 + i];
        if (++h->size[s] > h->max_hist) {  // :1463-1473 pop_front
            h->head[s] = (h->head[s] + 1) % h->slots;
            h->size[s]--;
        }
        if (added) added[s] = 1;
    }
    if (h->cm_on) return hb_cells_append(where, h);
    return 0;
}

extern "C" int ll_history_batch_add_voxel(ll_history_batch *h, ll_voxel *vc, ll_voxel *vs, const int32_t *active, const double *poses7,
                                          const double *gate_poses7, double history_add_t_step, double history_add_angle_step, int32_t *added)
{
    static const char *where = "ll_history_batch_add_voxel";
    const bool und = history_batch_take_undistort(h);
    if (!h || !vc || !vs || !poses7) return set_err(where, "null argument");
    if (vc->device != h->device || vs->device != h->device) return set_err(where, "handles live on different devices");
    if (vc->dev.max_clouds < h->S || vs->dev.max_clouds < h->S) return set_err(where, "the voxel filters hold fewer clouds than n_sequences");
    return history_batch_add_common(where, h, feat_view(vc, vs), active, poses7, gate_poses7, history_add_t_step, history_add_angle_step, added, und);
}

extern "C" int ll_history_batch_add_fe(ll_history_batch *h, ll_fe *fe, const int32_t *active, const double *poses7, const double *gate_poses7,
                                       double history_add_t_step, double history_add_angle_step, int32_t *added)
{
    static const char *where = "ll_history_batch_add_fe";
    const bool und = history_batch_take_undistort(h);
    if (!h || !fe || !poses7) return set_err(where, "null argument");
    if (fe->prm.device != h->device) return set_err(where, "extractor lives on another device");
    if (fe->prm.max_scans < h->S) return set_err(where, "the extractor holds fewer scans than n_sequences");
    return history_batch_add_common(where, h, feat_view(fe), active, poses7, gate_poses7, history_add_t_step, history_add_angle_step, added, und);
}

// g_if_undistore = 1 for the next add (laser_mapping.hpp:1424,1430), the batch form of ll_history_set_undistort: slot s of the registration
// r collected last moves sequence s's clouds.  The S records are copied on the registrar's stream into memory of this handle -- the
// registrar's next enqueue may follow at once -- and this handle's stream waits for the copy on the device; the host waits for nothing.
extern "C" int ll_history_batch_set_undistort(ll_history_batch *h, ll_reg *r)
{
    static const char *where = "ll_history_batch_set_undistort";
    if (!h || !r) return set_err(where, "null argument");
    if (r->device != h->device) return set_err(where, "registrar lives on another device");
    if (reg_undistort_records(where, r, h->S)) return -1;  // (refuses an uncollected enqueue and a registration of fewer than S scans)
    if (!h->d_und) {
        DM(h->d_und, (size_t)h->S);
        HC(hipEventCreateWithFlags(&h->ev_und, hipEventDisableTiming));
    }
    HC(hipMemcpyAsync(h->d_und, r->d_und, (size_t)h->S * sizeof(UndistortRec), hipMemcpyDeviceToDevice, r->stream));
    HC(hipEventRecord(h->ev_und, r->stream));
    HC(hipStreamWaitEvent(h->stream, h->ev_und, 0));
    h->has_und = true;
    return 0;
}

void hb_sizes_out(const ll_history_batch *h, int64_t *n_map_corner, int64_t *n_map_surf)
{
    for (int s = 0; s < h->S; s++) {
        if (n_map_corner) n_map_corner[s] = h->n_map[0][s];
        if (n_map_surf) n_map_surf[s] = h->n_map[1][s];
    }
}

// what a refresh checks before it touches anything: a map of the handle's device in every active slot, none of them twice
int hb_check_maps(const char *where, const ll_history_batch *h, ll_map *const *maps, const int32_t *active, bool *any)
{
    std::vector<const ll_map *> seen;
    for (int s = 0; s < h->S; s++) {
        if (active && !active[s]) continue;
        if (!maps[s]) return set_err(where, "null map in an active slot");
        if (maps[s]->device != h->device) return set_err(where, "map lives on another device");
        seen.push_back(maps[s]);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return set_err(where, "the same map in two active slots");
    *any = !seen.empty();
    return 0;
}

extern "C" int ll_history_batch_refresh(ll_history_batch *h, ll_map *const *maps, const int32_t *active, int64_t *n_map_corner,
                                        int64_t *n_map_surf)
{
    static const char *where = "ll_history_batch_refresh";
    if (!h || !maps) return set_err(where, "null argument");
    const int S = h->S;
    bool any = false;
    if (hb_check_maps(where, h, maps, active, &any)) return -1;
    if (!any) {
        hb_sizes_out(h, n_map_corner, n_map_surf);
        return 0;
    }
    HC(hipSetDevice(h->device));
    // ---- concatenations, oldest frame first (laser_mapping.hpp:519-530), and their VoxelGrid (:533-537)
    int *t_active = (int *)h->hp_ref, *t_ncat = t_active + S;
    HbSeg *segs = (HbSeg *)(h->hp_ref + h->ref_seg_off);
    // The concatenations of one kind share a stride, and VoxelGrid's general path sorts the padded [S][stride] index space: the stride
    // is the longest concatenation of THIS refresh, not the capacity (a slot's result does not depend on it).
    int n_seg = 0, max_cat[2] = {0, 0};
    for (int s = 0; s < S; s++) {
        const bool on = !active || active[s];
        t_active[s] = on ? 1 : 0;
        for (int k = 0; k < 2; k++) {
            int total = 0;
            for (int i = 0; on && i < h->size[s]; i++) total += h->count[k][(size_t)s * h->slots + (h->head[s] + i) % h->slots];
            t_ncat[k * S + s] = total;
            max_cat[k] = total > max_cat[k] ? total : max_cat[k];
        }
    }
    const int cat_stride[2] = {max_cat[0] > 0 ? max_cat[0] : 1, max_cat[1] > 0 ? max_cat[1] : 1};
    for (int s = 0; s < S; s++) {
        for (int k = 0; k < 2; k++) {
            int total = 0;
            for (int i = 0; t_active[s] && i < h->size[s]; i++) {
                const int slot = (h->head[s] + i) % h->slots;
                const int c = h->count[k][(size_t)s * h->slots + slot];
                if (c > 0) {
                    HbSeg &sg = segs[n_seg++];
                    sg.src = (long long)(((size_t)s * h->slots + slot) * h->max_pts);
                    sg.dst = (long long)((size_t)k * S * h->cstride + (size_t)s * cat_stride[k] + total);
                    sg.n = c;
                    sg.kind = k;
                }
                total += c;
            }
        }
    }
    HC(hipMemcpyAsync(h->d_ref, h->hp_ref, h->ref_seg_off + (size_t)n_seg * sizeof(HbSeg), hipMemcpyHostToDevice, h->stream));
    HC(hipMemcpyAsync(h->d_mm, h->hp_mm_init, (size_t)2 * S * 8 * sizeof(unsigned int), hipMemcpyHostToDevice, h->stream));
    launch_hb_gather_frames(h->frames[0], h->frames[1], (const HbSeg *)(h->d_ref + h->ref_seg_off), n_seg, h->max_pts, h->d_concat, h->stream);
    return hb_refresh_second_half(where, h, maps, max_cat, cat_stride, n_map_corner, n_map_surf);
}

// The second half of a refresh, shared by the history mode and the cell mode: the VoxelGrid over the concatenations
// (laser_mapping.hpp:533-537; h->d_concat holds them per kind as [S][cat_stride[kind]], the tables of the call are on their way to
// h->d_ref), then the search grids of all active slots in one arena, published into maps[s].  Two host waits.
int hb_refresh_second_half(const char *where, ll_history_batch *h, ll_map *const *maps, const int max_cat[2], const int cat_stride[2],
                           int64_t *n_map_corner, int64_t *n_map_surf)
{
    const int S = h->S;
    const int *t_active = (const int *)h->hp_ref;
    const int *d_active = (const int *)h->d_ref, *d_ncat = d_active + S;
    const char *err = nullptr;
    for (int k = 0; k < 2; k++) {
        const float leaf[3] = {h->res[k], h->res[k], h->res[k]};
        if (voxel_filter_bounded(h->vm[k], h->d_concat + (size_t)k * S * h->cstride, d_ncat + (size_t)k * S, cat_stride[k], S, leaf, max_cat[k],
                                 h->stream, &err))
            return set_err(where, err);
    }
    // ---- bounding boxes and sizes of all filtered clouds: one launch, one copy, the first of the two waits
    launch_hb_aabb(h->vm[0].out, h->vm[0].n_out, cat_stride[0], h->vm[1].out, h->vm[1].n_out, cat_stride[1], d_active, S,
                   max_cat[0] > max_cat[1] ? max_cat[0] : max_cat[1], (int)h->cstride, h->d_map, h->d_mm, h->stream);
    HC(hipGetLastError());
    HC(hipMemcpyAsync(h->hp_mm, h->d_mm, (size_t)2 * S * 8 * sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
    HC(hipStreamSynchronize(h->stream));
    // ---- grid geometry per (slot, kind) by map_build's arithmetic; the grids' places in the pooled buffers
    int n_grids = 0, max_n = 0;
    long long n_total = 0, n_cells = 0;
    unsigned long long max_ncell = 1;
    for (int s = 0; s < S; s++) {
        if (!t_active[s]) continue;
        for (int k = 0; k < 2; k++) {
            HbGrid &t = h->hp_grid[n_grids++];
            memset(&t, 0, sizeof(t));
            float mm[6];
            int n_out = 0;
            hb_aabb_decode(h->hp_mm + 8 * ((size_t)k * S + s), mm, &n_out);
            if (n_out < 0 || (size_t)n_out > h->cstride) return set_err(where, "filtered cloud size out of range");
            map_grid_geometry(mm, match_cell_size(k, h->res[k]), t.g);
            t.src = k * S + s;
            t.n = n_out;
            t.ncell = t.g.nx * t.g.ny * t.g.nz;
            t.pt_off = n_total;
            t.cell_off = n_cells;
            n_total += n_out;
            n_cells += (long long)t.ncell + 1;
            max_n = n_out > max_n ? n_out : max_n;
            max_ncell = (unsigned long long)t.ncell > max_ncell ? (unsigned long long)t.ncell : max_ncell;
        }
    }
    if (n_total >= 0x7fffffffLL || n_cells >= 0x7fffffffLL) return set_err(where, "the pooled grids exceed 2^31 entries");
    int cbits = 1, gbits = 1;
    while ((1ull << cbits) <= max_ncell) cbits++;
    while ((1 << gbits) < n_grids) gbits++;
    size_t tmp_bytes = 0;
    if (hb_sort_scan_bytes(n_total, n_cells, &tmp_bytes, &err)) return set_err(where, err);
    {   // scratch: buffers of one group share a capacity (the stream is idle here)
        size_t c[4] = {h->cap_n, h->cap_n, h->cap_n, h->cap_n}, cc = h->cap_cells;
        h->cap_n = h->cap_cells = 0;
        const size_t nn = (size_t)(n_total > 0 ? n_total : 1);
        if (hb_grow(&h->keys, &c[0], nn) || hb_grow(&h->keys2, &c[1], nn) || hb_grow(&h->vals, &c[2], nn) || hb_grow(&h->vals2, &c[3], nn) ||
            hb_grow(&h->counts, &cc, (size_t)n_cells) || hb_grow(&h->tmp, &h->cap_tmp, tmp_bytes))
            return -1;
        h->cap_n = c[0];
        h->cap_cells = cc;
    }
    std::shared_ptr<HbArena> arena;
    for (auto &a : h->arenas)
        if (a.use_count() == 1) {  // referenced by the pool only: no snapshot built in it is published or pinned
            arena = a;
            break;
        }
    if (!arena) {
        arena = std::make_shared<HbArena>();
        arena->device = h->device;
        h->arenas.push_back(arena);
    }
    if (hb_grow(&arena->pts, &arena->cap_pts, (size_t)(n_total > 0 ? n_total : 1)) || hb_grow(&arena->cells, &arena->cap_cells, (size_t)n_cells)) return -1;
    // ---- keys of all grids, one stable sort by (grid, cell), one scan over the concatenated cell tables, one gather
    HC(hipMemcpyAsync(h->d_grid, h->hp_grid, (size_t)n_grids * sizeof(HbGrid), hipMemcpyHostToDevice, h->stream));
    HC(hipMemsetAsync(h->counts, 0, (size_t)n_cells * sizeof(int), h->stream));
    launch_hb_cellkey(h->d_map, (int)h->cstride, h->d_grid, n_grids, max_n, cbits, h->keys, h->vals, h->counts, h->stream);
    if (hb_sort_scan(h->tmp, h->cap_tmp, h->keys, h->keys2, h->vals, h->vals2, n_total, cbits + gbits, h->counts, arena->cells, n_cells, h->stream, &err))
        return set_err(where, err);
    for (int g = 0; g < n_grids; g++) h->hp_nvalid[g] = 0;
    HC(hipMemcpyAsync(h->d_nvalid, h->hp_nvalid, (size_t)n_grids * sizeof(int), hipMemcpyHostToDevice, h->stream));
    launch_hb_gather_points(h->d_map, (int)h->cstride, h->d_grid, cbits, h->keys2, h->vals2, n_total, arena->cells, arena->pts, h->d_nvalid, h->stream);
    HC(hipGetLastError());
    HC(hipMemcpyAsync(h->hp_nvalid, h->d_nvalid, (size_t)n_grids * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HC(hipStreamSynchronize(h->stream));  // the second wait: the snapshots are complete before they are published
    // ---- one new snapshot per grid, each pointing into the arena and keeping it alive
    for (int g = 0; g < n_grids; g++) {
        const HbGrid &t = h->hp_grid[g];
        const int k = t.src / S, s = t.src % S;
        std::shared_ptr<MapSnap> sn = std::make_shared<MapSnap>();
        sn->device = h->device;
        sn->arena = arena;
        MapKind &mk = sn->mk;
        mk.pts = arena->pts + t.pt_off;
        mk.cell_start = arena->cells + t.cell_off;
        mk.n = t.n;
        mk.n_valid = h->hp_nvalid[g];
        mk.ncell = (size_t)t.ncell;
        mk.grid = t.g;
        mk.grid.pts = mk.pts;
        mk.grid.cell_start = mk.cell_start;
        (void)map_publish(maps[s], k, sn);
        h->n_map[k][s] = t.n;
    }
    hb_sizes_out(h, n_map_corner, n_map_surf);
    return 0;
}

extern "C" int64_t ll_history_batch_map_cloud(ll_history_batch *h, int32_t sequence, int32_t kind, float *xyzi, int64_t capacity_points)
{
    if (!h || kind < 0 || kind > 1 || sequence < 0 || sequence >= h->S) return set_err("ll_history_batch_map_cloud", "bad argument");
    const int64_t n = h->n_map[kind][sequence];
    if (!xyzi) return n;
    if (capacity_points < n) return set_err("ll_history_batch_map_cloud", "buffer too small");
    if (hipSetDevice(h->device) != hipSuccess) return set_err("ll_history_batch_map_cloud", "hipSetDevice failed");
    if (n > 0 && hipMemcpy(xyzi, h->d_map + ((size_t)kind * h->S + sequence) * h->cstride, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess)
        return set_err("ll_history_batch_map_cloud", "copy failed");
    return n;
}
