// ll_api_scene_align.hip -- the scene alignment of two key frames without a host hop (ll_scene_align_*), and the host read-back of
// the selection it starts from (ll_cellmap_feature_clouds).  Scene_alignment::find_tranfrom_of_two_mappings
// (source/scene_alignment.hpp:269-391) as loam_livox_amd/scene_alignment.py states it, with the clouds staying where they are:
// ll_cellmap_select_kernels.hip turns each cell map into its line and plane cloud, the voxel filter reads those at all three scales,
// the search grids are built from the source key frame's filtered clouds and the registrar binds the target's.  Everything the host
// has to know -- sizes, centres, the grids' bounding boxes -- comes back in ONE wait; after it a run waits only to collect a registration.
#include "ll_api_internal.h"

// cell labels, centre and the selection of one key frame, enqueued on s: the centre lands in c->d_kf->centre.  Five enqueues.
static const int kSelectEnqueues = 5;  // cellmap_stats 1, cellmap_centre 1, cellmap_select_features 3
int ll::cellmap_feature_clouds_enqueue(ll_cellmap *c, float4 *d_line, float4 *d_plane, int *d_n_line, int *d_n_plane, hipStream_t s, const char *where)
{
    if (!c->d_stats) DM(c->d_stats, (size_t)c->dev.cap);  // a cell holds at least one point
    if (!c->d_kf) DM(c->d_kf, 1);
    const size_t need = cellmap_select_scratch(c->dev);
    if (need > c->dev.tmp_bytes) {  // (a map of a few points: its scratch was sized for its own sorts and 32-bit scans; nothing of the map is in flight)
        void *t = nullptr;
        HC(hipMalloc(&t, need));
        if (c->dev.tmp) (void)hipFree(c->dev.tmp);
        c->dev.tmp = t;
        c->dev.tmp_bytes = need;
    }
    const char *err = nullptr;
    if (cellmap_stats(c->dev, c->d_stats, s, &err) || cellmap_centre(c->dev, c->d_kf, s, &err) ||
        cellmap_select_features(c->dev, c->d_stats, d_line, d_plane, d_n_line, d_n_plane, s, &err))
        return set_err(where, err ? err : "launch failed");
    return 0;
}

extern "C" int ll_cellmap_feature_clouds(ll_cellmap *c, float *line_xyzi, int64_t capacity_line, int64_t *n_line, float *plane_xyzi,
                                         int64_t capacity_plane, int64_t *n_plane, float centre[3])
{
    const char *fn = "ll_cellmap_feature_clouds";
    if (!c || !n_line || !n_plane) return set_err(fn, "null argument");
    if (capacity_line < 0 || capacity_plane < 0 || (!line_xyzi && capacity_line != 0) || (!plane_xyzi && capacity_plane != 0))
        return set_err(fn, "a null buffer must come with capacity 0");
    if (cellmap_settle(c)) return -1;
    HC(hipSetDevice(c->device));
    // the append / replace scratch is free between calls and 2 * cap points long: the line cloud in its first half, the plane cloud in its second
    float4 *d_line = c->dev.pts2, *d_plane = c->dev.pts2 + c->dev.cap;
    int *d_n = c->dev.counts + 4;  // (entries [4], [5] of the device scalars: no kernel of the map uses them)
    if (cellmap_feature_clouds_enqueue(c, d_line, d_plane, d_n, d_n + 1, c->stream, fn)) return -1;
    int n[2] = {0, 0};
    float ctr[3] = {0.f, 0.f, 0.f};
    HC(hipMemcpyAsync(n, d_n, sizeof(n), hipMemcpyDeviceToHost, c->stream));
    HC(hipMemcpyAsync(ctr, c->d_kf->centre, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    if ((line_xyzi && capacity_line < n[0]) || (plane_xyzi && capacity_plane < n[1])) return set_err(fn, "buffer too small");
    if (line_xyzi && n[0] > 0) HC(hipMemcpy(line_xyzi, d_line, (size_t)n[0] * sizeof(float4), hipMemcpyDeviceToHost));
    if (plane_xyzi && n[1] > 0) HC(hipMemcpy(plane_xyzi, d_plane, (size_t)n[1] * sizeof(float4), hipMemcpyDeviceToHost));
    *n_line = n[0];
    *n_plane = n[1];
    if (centre)
        for (int d = 0; d < 3; d++) centre[d] = ctr[d];
    return 0;
}

extern "C" void ll_scene_align_default_params(ll_scene_align_params *p)
{
    if (!p) return;
    p->line_res = 0.4f;                // SA:27
    p->plane_res = 0.4f;               // SA:28
    p->maximum_icp_iteration = 10;     // SA:35
    p->accepted_threshold = 0.2f;      // SA:36
    p->maximum_residual_block = 5000;  // SA:34
    p->registrar_init = 1;             // Scene_alignment::init, SA:233-243 (the loop detector calls it, laser_mapping.hpp:896)
    p->subsample_seed = 1;
}

extern "C" void ll_scene_align_destroy(ll_scene_align *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->reg) ll_reg_destroy(h->reg);  // (first: it drains the stream everything of a run was enqueued on)
    if (h->vox) ll_voxel_destroy(h->vox);
    if (h->map) ll_map_destroy(h->map);
    for (float4 *p : h->sel)
        if (p) (void)hipFree(p);
    for (auto &scale : h->filt)
        for (float4 *p : scale)
            if (p) (void)hipFree(p);
    if (h->d_ints) (void)hipFree(h->d_ints);
    if (h->d_mm) (void)hipFree(h->d_mm);
    delete h;
}

// capacities: the larger of what is asked for and twice what is there, never below initial_points
static int64_t sa_grown(const ll_scene_align *h, int64_t have, int64_t need)
{
    int64_t cap = have > 0 ? 2 * have : h->initial_points;
    if (cap < need) cap = need;
    return cap < 0x3fffffffLL ? cap : 0x3fffffffLL - 1;
}

// the selected clouds of key frame `which` (0: a, 1: b) and their filtered forms with room for n points each; nothing of an earlier
// run is kept
static int sa_room_clouds(ll_scene_align *h, int which, int64_t n)
{
    if (n <= h->sel_cap[which]) return 0;
    const int64_t cap = sa_grown(h, h->sel_cap[which], n);
    h->sel_cap[which] = 0;
    for (int k = 2 * which; k < 2 * which + 2; k++) {
        float4 **bufs[4] = {&h->sel[k], &h->filt[0][k], &h->filt[1][k], &h->filt[2][k]};
        for (float4 **b : bufs) {
            if (*b) (void)hipFree(*b);
            *b = nullptr;
            DM(*b, (size_t)cap);
        }
    }
    h->sel_cap[which] = cap;
    return 0;
}

static int sa_room_filter(ll_scene_align *h, int64_t n)
{
    if (n <= h->vox_cap) return 0;
    const int64_t cap = sa_grown(h, h->vox_cap, n);
    h->vox_cap = 0;
    if (h->vox) ll_voxel_destroy(h->vox);
    h->vox = nullptr;
    if (ll_voxel_create(h->device, 1, (int32_t)cap, &h->vox)) return -1;
    h->vox_cap = cap;
    return 0;
}

static int sa_room_registrar(ll_scene_align *h, int64_t n)
{
    if (n <= h->reg_cap) return 0;
    const int64_t cap = sa_grown(h, h->reg_cap, n);
    if (h->reg) ll_reg_destroy(h->reg);
    h->reg = nullptr;
    h->reg_cap = 0;
    if (ll_reg_create(h->device, 1, (int32_t)cap, &h->reg)) return -1;
    h->reg_cap = cap;
    return 0;
}

extern "C" int ll_scene_align_create(int32_t device, int64_t initial_points, ll_scene_align **out)
{
    const char *fn = "ll_scene_align_create";
    if (!out) return set_err(fn, "null argument");
    if (initial_points < 1 || initial_points >= 0x3fffffffLL) return set_err(fn, "initial_points out of range");
    if (check_device(device)) return -1;
    ll_scene_align *h = new ll_scene_align();
    h->device = device;
    h->initial_points = initial_points;
    if (hipSetDevice(device) != hipSuccess || dmalloc(&h->d_ints, 28) || dmalloc(&h->d_mm, 36) || ll_map_create(device, &h->map) ||
        sa_room_registrar(h, initial_points) || sa_room_filter(h, initial_points) || sa_room_clouds(h, 0, initial_points) ||
        sa_room_clouds(h, 1, initial_points)) {
        const std::string why = g_err;  // (the destroy calls below do not touch it, but a copy says so)
        ll_scene_align_destroy(h);
        g_err = why.empty() ? std::string(fn) + ": allocation failed" : why;
        return -1;
    }
    *out = h;
    return 0;
}

extern "C" int ll_scene_align_work(ll_scene_align *h, int64_t out[4])
{
    if (!h || !out) return set_err("ll_scene_align_work", "null argument");
    for (int i = 0; i < 4; i++) out[i] = h->work[i];
    return 0;
}

extern "C" int ll_scene_align_run(ll_scene_align *h, ll_cellmap *a, ll_cellmap *b, const ll_scene_align_params *p, double pose[7],
                                  double *inlier_threshold, ll_reg_report reports[3], int32_t *n_reports)
{
    const char *fn = "ll_scene_align_run";
    if (!h || !a || !b || !p || !pose || !inlier_threshold || !reports || !n_reports) return set_err(fn, "null argument");
    if (a == b) return set_err(fn, "the two key frames are the same map");
    if (a->device != h->device || b->device != h->device) return set_err(fn, "a cell map lives on another device than the handle");
    if (!(p->line_res > 0.f) || !(p->plane_res > 0.f)) return set_err(fn, "resolutions must be positive");
    if (p->maximum_icp_iteration < 1) return set_err(fn, "maximum_icp_iteration must be positive");
    if (cellmap_settle(a) || cellmap_settle(b)) return -1;
    HC(hipSetDevice(h->device));
    int64_t *work = h->work;
    work[0] = work[1] = work[2] = work[3] = 0;  // work[0]: no copy of this function moves a point; there is nothing to add to it
    // The maps' host mirrors bound every cloud of a run, selected or filtered: all room is made before anything is enqueued, without a wait.
    const int n_pts[2] = {a->dev.n_pts, b->dev.n_pts};
    if (sa_room_clouds(h, 0, n_pts[0]) || sa_room_clouds(h, 1, n_pts[1]) || sa_room_filter(h, std::max(1, std::max(n_pts[0], n_pts[1]))) ||
        sa_room_registrar(h, std::max(1, n_pts[1])))
        return -1;
    // everything of a run goes onto the registrar's stream, in order: the cell maps' own streams are idle between calls
    hipStream_t s = h->reg->stream;
    int *d_sel = h->d_ints, *d_filt = h->d_ints + 4, *d_status = h->d_ints + 16;
    if (cellmap_feature_clouds_enqueue(a, h->sel[0], h->sel[1], d_sel, d_sel + 1, s, fn) ||
        cellmap_feature_clouds_enqueue(b, h->sel[2], h->sel[3], d_sel + 2, d_sel + 3, s, fn))
        return -1;
    work[3] = 2 * kSelectEnqueues;
    // The three scales (SA:313-327) do not depend on each other's registrations: all twelve filtered clouds, and the bounding boxes of
    // a's six, are enqueued now, so that their sizes come back with the selection's.
    const int scales[3] = {8, 4, 0};
    float res[3][2];  // [scale][line, plane]
    bool finest[3];
    for (int si = 0; si < 3; si++) {
        float line_res = p->line_res * (float)scales[si], plane_res = p->plane_res * (float)scales[si];
        if (line_res < p->line_res) line_res = p->line_res;
        finest[si] = plane_res < p->plane_res;
        if (finest[si]) plane_res = p->plane_res;
        res[si][0] = line_res;
        res[si][1] = plane_res;
    }
    HC(hipMemsetAsync(d_filt, 0, 24 * sizeof(int), s));  // (a map without points is not filtered: its clouds are empty at every scale)
    for (int si = 0; si < 3; si++)
        for (int k = 0; k < 4; k++) {
            const int bound = n_pts[k >> 1];
            if (bound > 0) {
                // the handle's filter with its outputs pointed at this cloud's own places; stride and bound = the map's points, which no
                // cloud exceeds (the filter takes the cloud's size from the device); an empty cloud comes out empty
                VoxelDev v = h->vox->dev;
                v.out = h->filt[si][k];
                v.n_out = d_filt + 4 * si + k;
                v.status = d_status + 4 * si + k;
                const float leaf[3] = {res[si][k & 1], res[si][k & 1], res[si][k & 1]};
                const char *err = nullptr;
                if (voxel_filter_bounded(v, h->sel[k], d_sel + k, bound, 1, leaf, bound, s, &err)) return set_err(fn, err);
            }
            const char *err = nullptr;
            if (k < 2 && map_bbox_enqueue((const float *)h->filt[si][k], 4, d_filt + 4 * si + k, bound, h->d_mm + 6 * (2 * si + k), s, &err))
                return set_err(fn, err ? err : "launch failed");
        }
    int n_f[3][4];
    float ca[3], cb[3], mm[3][2][6];
    HC(hipMemcpyAsync(n_f, d_filt, sizeof(n_f), hipMemcpyDeviceToHost, s));
    HC(hipMemcpyAsync(mm, h->d_mm, sizeof(mm), hipMemcpyDeviceToHost, s));
    HC(hipMemcpyAsync(ca, a->d_kf->centre, sizeof(ca), hipMemcpyDeviceToHost, s));
    HC(hipMemcpyAsync(cb, b->d_kf->centre, sizeof(cb), hipMemcpyDeviceToHost, s));
    HC(hipStreamSynchronize(s));  // the one wait for sizes, centres and boxes
    work[1]++;

    ll_reg_params prm;
    ll_reg_default_params(&prm);
    if (p->registrar_init) {  // Scene_alignment::init, SA:233-243
        prm.icp_line = 0;
        prm.max_final_cost = 20000.0f;
        prm.para_max_speed = 1000.0f;
        prm.para_max_angular_rate = (float)(360 * 57.3);
        prm.inliner_dis = 0.2;
    }
    prm.current_frame_index = 10000000;                        // SA:296
    prm.icp_max_iterations = p->maximum_icp_iteration;         // SA:300
    prm.ceres_max_iterations = 50;                             // SA:301
    prm.ceres_prerun_times = 2;                                // SA:302
    prm.maximum_allow_residual_block = p->maximum_residual_block;  // SA:303
    prm.subsample_seed = p->subsample_seed;
    const double last[7] = {0, 0, 0, 1, 0, 0, 0};              // SA:297-299
    double curr[7] = {0, 0, 0, 1, 0, 0, 0}, incre[7] = {0, 0, 0, 1, 0, 0, 0};
    for (int d = 0; d < 3; d++) curr[4 + d] = incre[4 + d] = (double)(float)(ca[d] - cb[d]);  // SA:307, 309-310: nothing of the previous pair
    double thr = 0.0;
    int n_rep = 0;
    for (int si = 0; si < 3; si++) {
        if (finest[si]) prm.icp_max_iterations = p->maximum_icp_iteration * 2;  // SA:327
        const int *nf = n_f[si];
        if (nf[0] > 0 && nf[1] > 0) {  // PCR:595-602: otherwise "return 1" without solving
            const char *err = nullptr;
            // KdTreeFLANN::setInputCloud twice (PCR:596-597) with ll_map_upload's default cells, from the boxes read above: enqueued only
            if (map_rebuild_boxed(h->map, LL_MAP_CORNER, (const float *)h->filt[si][0], 4, nf[0], 1.45f, mm[si][0], s, &err) ||
                map_rebuild_boxed(h->map, LL_MAP_SURF, (const float *)h->filt[si][1], 4, nf[1], 0.6f, mm[si][1], s, &err))
                return set_err(fn, err ? err : "map build failed");
            if (reg_enqueue_device_clouds(fn, h->reg, h->map, h->filt[si][2], d_filt + 4 * si + 2, nf[2], h->filt[si][3], d_filt + 4 * si + 3, nf[3], &prm,
                                          last, curr, incre))
                return -1;
            int32_t result = 0;
            if (ll_reg_collect(h->reg, 1, curr, incre, &reports[n_rep], &result) < 0) return -1;  // the early stop needs this scale's report
            work[1]++;
            work[2]++;
            thr = reports[n_rep].inlier_threshold;
            n_rep++;
        }
        if (thr > (double)p->accepted_threshold * 2) break;  // SA:350-351
    }
    for (int i = 0; i < 7; i++) pose[i] = curr[i];
    *inlier_threshold = thr;
    *n_reports = n_rep;
    return 0;
}
