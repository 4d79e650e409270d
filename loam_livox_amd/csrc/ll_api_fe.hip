// ll_api_fe.hip -- the extractor handle (ll_fe_*) of the C ABI: uploads, the launch order of ll_fe_kernels.hip, the host-libm
// resolve of ambiguous view angles, downloads.
#include "ll_api_internal.h"

extern "C" void ll_fe_default_params(ll_fe_params *p)
{
    memset(p, 0, sizeof(*p));
    p->thr_corner_curvature = 0.05f;   // LFX:152 default
    p->thr_surface_curvature = 0.01f;  // LFX:153
    p->minimum_view_angle = 10.0f;     // LFX:154
    p->livox_min_allow_dis = 0.1f;     // LFX:854
    p->livox_min_sigma = 7e-4f;        // LFX:859
    p->max_fov = 17.0f;                // LFE:143
    p->time_internal_pts = 1.0e-5f;    // LFE:145
    p->device = 0;
    p->max_points = 24000;
    p->max_scans = 1;
    p->piecewise_number = 3;           // LFX:142
}

static FeConst make_fe_const(const ll_fe_params &p)
{
    FeConst c;
    c.thr_corner_curvature = p.thr_corner_curvature;
    c.thr_surface_curvature = p.thr_surface_curvature;
    c.minimum_view_angle = p.minimum_view_angle;
    c.min_dis_sq = p.livox_min_allow_dis * p.livox_min_allow_dis;
    c.min_sigma = p.livox_min_sigma;
    c.max_edge_polar_pos = (float)pow(tan((double)p.max_fov / 57.3) * 1, 2);  // LFE:185
    c.time_internal_pts = p.time_internal_pts;
    // acosf implementations differ by <= 1 ulp; *57.3 and the float store add < 1 ulp more: 8 ulp of the
    // threshold is a generous band
    c.view_angle_band = 8.0f * (nextafterf(fabsf(p.minimum_view_angle) + 1.0f, INFINITY) - (fabsf(p.minimum_view_angle) + 1.0f));
    return c;
}

extern "C" void ll_fe_destroy(ll_fe *h);
static int fe_create_impl(const ll_fe_params *p, ll_fe *h)
{
    h->prm = *p;
    h->fc = make_fe_const(*p);
    const size_t B = p->max_scans, N = p->max_points, BN = B * N;
    FeDev &d = h->dev;
    memset(&d, 0, sizeof(d));
    d.stride = (int)N;
    d.split_cap = (int)(N / 50 + 8);
    // view-angle ambiguity list (ll_fe_resolve): sized for the whole batch -- 1/16 of the points, at least 4096; a batch that
    // still overflows it makes ll_fe_resolve fail instead of silently keeping device-libm labels
    d.ambig_cap = (int)((BN / 16 > 4096 ? BN / 16 : 4096) < 0x7fffffffull ? (BN / 16 > 4096 ? BN / 16 : 4096) : 0x7fffffffull);
    HC(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HC(hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming));
    HC(hipEventCreateWithFlags(&h->ev_staged, hipEventDisableTiming));
    DM(h->d_xyzi, BN);
    DM(h->d_npts, B);
    DM(h->d_time0, B);
    d.xyzi = h->d_xyzi;
    d.npts = h->d_npts;
    d.time0 = h->d_time0;
    DM(d.type, BN);
    DM(d.label, BN);
    DM(d.depth2, BN);
    DM(d.polar2, BN);
    DM(d.curv, BN);
    DM(d.view, BN);
    DM(d.tstamp, BN);
    DM(d.polar_angle, BN);
    DM(d.img, BN);
    DM(d.flags, BN);
    DM(d.cand, BN);
    DM(d.split_idx, B * d.split_cap);
    DM(d.petal_first, B * d.split_cap);
    DM(d.petal_last, B * d.split_cap);
    DM(d.run_angle, B * d.split_cap);
    DM(d.info, B);
    DM(d.corner_idx, BN);
    DM(d.surf_idx, BN);
    DM(d.full_idx, BN);
    DM(d.corner_feat, BN);
    DM(d.surf_feat, BN);
    DM(d.n_corner, B);
    DM(d.n_surf, B);
    DM(d.n_full, B);
    DM(d.n_ambig, 1);
    DM(d.ambig_list, d.ambig_cap);
    // On the handle's own stream, ahead of everything it will ever run.  (A hipMemset on the null stream is asynchronous to the host
    // and NOT ordered with a non-blocking stream: issued behind a busy null stream -- a 5 M-point map upload just before -- the
    // zeroing of d_npts landed after the first upload's copy into it, and the first extraction of a fresh handle saw zero points.)
    HC(hipMemsetAsync(d.n_ambig, 0, sizeof(int), h->stream));
    HC(hipMemsetAsync(h->d_npts, 0, B * sizeof(int), h->stream));
    HC(hipMemsetAsync(d.n_corner, 0, B * sizeof(int), h->stream));
    HC(hipMemsetAsync(d.n_surf, 0, B * sizeof(int), h->stream));
    HC(hipMemsetAsync(d.n_full, 0, B * sizeof(int), h->stream));
    HC(hipMemsetAsync(d.info, 0, B * sizeof(FeScanInfo), h->stream));
    h->h_npts.assign(B, 0);
    HC(hipHostMalloc((void **)&h->hp_npts, B * sizeof(int), hipHostMallocDefault));
    HC(hipHostMalloc((void **)&h->hp_time0, B * sizeof(double), hipHostMallocDefault));
    return 0;
}

extern "C" int ll_fe_create(const ll_fe_params *p, ll_fe **out)
{
    if (!p || !out) return set_err("ll_fe_create", "null argument");
    if (p->max_points < 1 || p->max_scans < 1) return set_err("ll_fe_create", "bad capacity");
    if (p->piecewise_number < 1 || p->piecewise_number > LL_MAX_PIECES) return set_err("ll_fe_create", "piecewise_number out of range");
    if (check_device(p->device)) return -1;
    ll_fe *h = new ll_fe();
    if (fe_create_impl(p, h)) {  // a failed allocation half way: release what was built (fields start out null)
        ll_fe_destroy(h);
        return -1;
    }
    *out = h;
    return 0;
}

extern "C" void ll_fe_destroy(ll_fe *h)
{
    if (!h) return;
    (void)hipSetDevice(h->prm.device);
    FeDev &d = h->dev;
    void *ptrs[] = {h->d_xyzi, h->d_npts, h->d_time0, d.type, d.label, d.depth2, d.polar2, d.curv, d.view, d.tstamp,
                    d.polar_angle, d.img, d.flags, d.cand, d.split_idx, d.petal_first, d.petal_last, d.run_angle, d.info,
                    d.corner_idx, d.surf_idx, d.full_idx, d.corner_feat, d.surf_feat, d.n_corner, d.n_surf, d.n_full,
                    d.n_ambig, d.ambig_list, h->d_last};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (h->hp_npts) (void)hipHostFree(h->hp_npts);
    if (h->hp_time0) (void)hipHostFree(h->hp_time0);
    if (h->ev_done) (void)hipEventDestroy(h->ev_done);
    if (h->ev_staged) (void)hipEventDestroy(h->ev_staged);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

extern "C" void *ll_fe_stream(ll_fe *h) { return h ? (void *)h->stream : nullptr; }
extern "C" int ll_fe_sync(ll_fe *h)
{
    if (!h) return set_err("ll_fe_sync", "null handle");
    HC(hipSetDevice(h->prm.device));
    HC(hipStreamSynchronize(h->stream));
    return 0;
}

static int fe_upload_impl(ll_fe *h, int32_t first_scan, int32_t n_scans, const float *xyzi, int32_t n_points, const double *current_time,
                          bool wait);
extern "C" int ll_fe_upload(ll_fe *h, int32_t first_scan, int32_t n_scans, const float *xyzi, int32_t n_points,
                            const double *current_time)
{
    return fe_upload_impl(h, first_scan, n_scans, xyzi, n_points, current_time, true);
}
extern "C" int ll_fe_upload_async(ll_fe *h, int32_t first_scan, int32_t n_scans, const float *xyzi, int32_t n_points,
                                  const double *current_time)
{
    return fe_upload_impl(h, first_scan, n_scans, xyzi, n_points, current_time, false);
}
static int fe_upload_impl(ll_fe *h, int32_t first_scan, int32_t n_scans, const float *xyzi, int32_t n_points, const double *current_time,
                          bool wait)
{
    if (!h || !xyzi || !current_time) return set_err("ll_fe_upload", "null argument");
    if (first_scan < 0 || n_scans < 0 || first_scan + n_scans > h->prm.max_scans) return set_err("ll_fe_upload", "scan range exceeds max_scans");
    if (n_points < 0 || n_points > h->prm.max_points) return set_err("ll_fe_upload", "n_points exceeds max_points");
    HC(hipSetDevice(h->prm.device));
    const size_t N = h->prm.max_points;
    // The page-locked staging slots of an upload still in flight are not rewritten: wait for the earlier upload's two small
    // copies (an event right behind them) -- not for the stream, which may hold a whole batch of extraction kernels.
    if (h->staged_pending) {
        HC(hipEventSynchronize(h->ev_staged));
        h->staged_pending = false;
    }
    for (int i = 0; i < n_scans; i++) {
        h->h_npts[first_scan + i] = n_points;
        h->hp_npts[first_scan + i] = n_points;
        h->hp_time0[first_scan + i] = current_time[i];
    }
    HC(hipMemcpyAsync(h->d_npts + first_scan, h->hp_npts + first_scan, n_scans * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HC(hipMemcpyAsync(h->d_time0 + first_scan, h->hp_time0 + first_scan, n_scans * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HC(hipEventRecord(h->ev_staged, h->stream));
    h->staged_pending = true;
    if (n_points > 0 && (size_t)n_points == N)  // full slots: one linear copy (a pitched copy of the same bytes does not run at link speed)
        HC(hipMemcpyAsync(h->d_xyzi + (size_t)first_scan * N, xyzi, (size_t)n_scans * N * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    else if (n_points > 0)
        HC(hipMemcpy2DAsync(h->d_xyzi + (size_t)first_scan * N, N * sizeof(float4), xyzi, (size_t)n_points * sizeof(float4),
                            (size_t)n_points * sizeof(float4), n_scans, hipMemcpyHostToDevice, h->stream));
    if (wait) HC(hipStreamSynchronize(h->stream));  // the caller's buffers may be reused right away
    return 0;
}

extern "C" int ll_fe_extract_batch(ll_fe *h, int32_t n_scans)
{
    if (!h) return set_err("ll_fe_extract_batch", "null handle");
    if (n_scans < 1 || n_scans > h->prm.max_scans) return set_err("ll_fe_extract_batch", "n_scans out of range");
    HC(hipSetDevice(h->prm.device));
    int max_n = 0;
    for (int i = 0; i < n_scans; i++) max_n = h->h_npts[i] > max_n ? h->h_npts[i] : max_n;
    HC(hipMemsetAsync(h->dev.n_ambig, 0, sizeof(int), h->stream));
    if (max_n > 0) launch_fe_point(h->dev, h->fc, n_scans, max_n, h->stream);
    launch_fe_split(h->dev, h->prm.piecewise_number, n_scans, h->stream);
    HC(hipGetLastError());
    return 0;
}

// Re-derive, with the host libm acosf the reference uses, the labels of the (very rare) points whose view angle
// fell inside the acosf ambiguity band.  Synchronises.  Returns the number of such points.
static int fe_resolve_ambiguous(ll_fe *h)
{
    int n_amb = 0;
    HC(hipMemcpyAsync(&n_amb, h->dev.n_ambig, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HC(hipStreamSynchronize(h->stream));
    if (n_amb <= 0) return 0;
    if (n_amb > h->dev.ambig_cap)
        return set_err("ll_fe_resolve", "more points inside the view-angle ambiguity band than the list holds (degenerate minimum_view_angle?)");
    const int n_list = n_amb;
    std::vector<int2> list(n_list);
    HC(hipMemcpy(list.data(), h->dev.ambig_list, n_list * sizeof(int2), hipMemcpyDeviceToHost));
    const size_t N = h->prm.max_points;
    // the re-derived labels are applied behind the loop: copies queued on the handle's stream from staging that outlives them, one wait
    // (a pair of copies and a stream drain per point made a batch with a few thousand flagged points thousands of round trips)
    std::vector<int> fix_label(n_list);
    std::vector<float> fix_view(n_list);
    std::vector<size_t> fix_at;
    fix_at.reserve(n_list);
    for (const int2 &e : list) {
        const int b = e.x, i = e.y, n = h->h_npts[b];
        if (i < 2 || i >= n - 2) continue;
        float4 raw[5];
        HC(hipMemcpy(raw, h->d_xyzi + (size_t)b * N + i - 2, sizeof(raw), hipMemcpyDeviceToHost));
        float p[5][3], d[5];
        int t[5];
        for (int k = 0; k < 5; k++) {
            const PointOwn o = point_own(raw[k].x, raw[k].y, raw[k].z, raw[k].w, i - 2 + k, h->fc);
            p[k][0] = raw[k].x;
            p[k][1] = raw[k].y;
            p[k][2] = raw[k].z;
            t[k] = o.type_self;
            d[k] = o.depth_sq2;
        }
        const LabelOut lo = point_label(p, t, d, h->fc);  // host build: glibc acosf
        fix_label[fix_at.size()] = lo.label;
        fix_view[fix_at.size()] = lo.view_angle;
        fix_at.push_back((size_t)b * N + i);
    }
    // on the handle's stream and waited for: the selection kernel that reads these runs on that stream, and a null-stream copy from
    // pageable memory is not ordered with it
    for (size_t k = 0; k < fix_at.size(); k++) {
        HC(hipMemcpyAsync(h->dev.label + fix_at[k], &fix_label[k], sizeof(int), hipMemcpyHostToDevice, h->stream));
        HC(hipMemcpyAsync(h->dev.view + fix_at[k], &fix_view[k], sizeof(float), hipMemcpyHostToDevice, h->stream));
    }
    if (!fix_at.empty()) HC(hipStreamSynchronize(h->stream));
    return n_amb;
}

extern "C" int ll_fe_counts(ll_fe *h, int32_t n_scans, int32_t *n_corner, int32_t *n_surf, int32_t *n_full, int32_t *n_ambiguous)
{
    if (!h) return set_err("ll_fe_counts", "null handle");
    if (n_scans < 1 || n_scans > h->prm.max_scans) return set_err("ll_fe_counts", "n_scans out of range");
    HC(hipSetDevice(h->prm.device));
    HC(hipStreamSynchronize(h->stream));
    if (n_corner) HC(hipMemcpy(n_corner, h->dev.n_corner, n_scans * sizeof(int), hipMemcpyDeviceToHost));
    if (n_surf) HC(hipMemcpy(n_surf, h->dev.n_surf, n_scans * sizeof(int), hipMemcpyDeviceToHost));
    if (n_full) HC(hipMemcpy(n_full, h->dev.n_full, n_scans * sizeof(int), hipMemcpyDeviceToHost));
    if (n_ambiguous) HC(hipMemcpy(n_ambiguous, h->dev.n_ambig, sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int ll_fe_resolve(ll_fe *h)
{
    if (!h) return set_err("ll_fe_resolve", "null handle");
    HC(hipSetDevice(h->prm.device));
    return fe_resolve_ambiguous(h);
}

extern "C" int ll_fe_extract(ll_fe *h, const float *xyzi, int32_t n, double time_stamp, int32_t *n_petal_clouds)
{
    if (!h || (!xyzi && n > 0)) return set_err("ll_fe_extract", "null argument");
    if (time_stamp < 0.0) return set_err("ll_fe_extract", "time_stamp must be >= 0 (assert at livox_feature_extractor.hpp:724)");
    if (n < 0 || n > h->prm.max_points) return set_err("ll_fe_extract", "n exceeds max_points");
    // LFE:724-736
    double current_time;
    if (time_stamp <= 0.0000001 || (time_stamp < h->last_maximum_time_stamp))
        current_time = h->last_maximum_time_stamp;
    else
        current_time = time_stamp - h->first_receive_time;
    if (h->first_receive_time <= 0) h->first_receive_time = time_stamp;
    static const float dummy[4] = {0, 0, 0, 0};
    if (ll_fe_upload(h, 0, 1, n > 0 ? xyzi : dummy, n, &current_time)) return -1;
    if (ll_fe_extract_batch(h, 1)) return -1;
    if (fe_resolve_ambiguous(h) < 0) return -1;
    if (n > 0) h->last_maximum_time_stamp = (double)point_time_stamp(current_time, n - 1, h->prm.time_internal_pts);  // LFE:482
    FeScanInfo info;
    HC(hipMemcpy(&info, h->dev.info, sizeof(info), hipMemcpyDeviceToHost));
    if (n_petal_clouds) *n_petal_clouds = info.n_petal_clouds;
    return 0;
}

extern "C" int ll_fe_labels(ll_fe *h, int32_t scan, int32_t *pt_type, int32_t *pt_label, float *depth_sq2, float *polar_dis_sq2,
                            float *curvature, float *view_angle, float *time_stamp, float *polar_angle)
{
    if (!h) return set_err("ll_fe_labels", "null handle");
    if (scan < 0 || scan >= h->prm.max_scans) return set_err("ll_fe_labels", "scan out of range");
    HC(hipSetDevice(h->prm.device));
    HC(hipStreamSynchronize(h->stream));
    const size_t off = (size_t)scan * h->prm.max_points;
    const int n = h->h_npts[scan];
    D2H_OPT(pt_type, h->dev.type + off, n, int);
    D2H_OPT(pt_label, h->dev.label + off, n, int);
    D2H_OPT(depth_sq2, h->dev.depth2 + off, n, float);
    D2H_OPT(polar_dis_sq2, h->dev.polar2 + off, n, float);
    D2H_OPT(curvature, h->dev.curv + off, n, float);
    D2H_OPT(view_angle, h->dev.view + off, n, float);
    D2H_OPT(time_stamp, h->dev.tstamp + off, n, float);
    D2H_OPT(polar_angle, h->dev.polar_angle + off, n, float);
    return 0;
}

extern "C" int ll_fe_splits(ll_fe *h, int32_t scan, int32_t *split_idx, int32_t *n_split, int32_t *clutter_size,
                            int32_t *n_petal_clouds, int32_t *first_idx, int32_t *last_idx, float *piece_start, float *piece_end)
{
    if (!h) return set_err("ll_fe_splits", "null handle");
    if (scan < 0 || scan >= h->prm.max_scans) return set_err("ll_fe_splits", "scan out of range");
    HC(hipSetDevice(h->prm.device));
    HC(hipStreamSynchronize(h->stream));
    FeScanInfo info;
    HC(hipMemcpy(&info, h->dev.info + scan, sizeof(info), hipMemcpyDeviceToHost));
    if (n_split) *n_split = info.n_split;
    if (clutter_size) *clutter_size = info.clutter_size;
    if (n_petal_clouds) *n_petal_clouds = info.n_petal_clouds;
    const size_t off = (size_t)scan * h->dev.split_cap;
    D2H_OPT(split_idx, h->dev.split_idx + off, info.n_split, int);
    D2H_OPT(first_idx, h->dev.petal_first + off, info.n_petal_clouds, int);
    D2H_OPT(last_idx, h->dev.petal_last + off, info.n_petal_clouds, int);
    for (int i = 0; i < h->prm.piecewise_number; i++) {
        if (piece_start) piece_start[i] = info.piece_start[i];
        if (piece_end) piece_end[i] = info.piece_end[i];
    }
    return 0;
}

extern "C" int ll_fe_select_batch(ll_fe *h, int32_t n_scans, int32_t piece, float minimum_blur, float maximum_blur)
{
    if (!h) return set_err("ll_fe_select_batch", "null handle");
    if (n_scans < 1 || n_scans > h->prm.max_scans) return set_err("ll_fe_select_batch", "n_scans out of range");
    if (piece >= h->prm.piecewise_number) return set_err("ll_fe_select_batch", "piece out of range");
    HC(hipSetDevice(h->prm.device));
    launch_fe_select(h->dev, n_scans, piece, minimum_blur, maximum_blur, h->stream);
    HC(hipGetLastError());
    return 0;
}

extern "C" int ll_fe_select(ll_fe *h, float minimum_blur, float maximum_blur, int32_t *corner_idx, int32_t *n_corner,
                            int32_t *surf_idx, int32_t *n_surf, int32_t *full_idx, int32_t *n_full, float *corner_xyzi,
                            float *surf_xyzi)
{
    if (ll_fe_select_batch(h, 1, -1, minimum_blur, maximum_blur)) return -1;
    HC(hipStreamSynchronize(h->stream));
    int nc = 0, ns = 0, nf = 0;
    HC(hipMemcpy(&nc, h->dev.n_corner, sizeof(int), hipMemcpyDeviceToHost));
    HC(hipMemcpy(&ns, h->dev.n_surf, sizeof(int), hipMemcpyDeviceToHost));
    HC(hipMemcpy(&nf, h->dev.n_full, sizeof(int), hipMemcpyDeviceToHost));
    if (n_corner) *n_corner = nc;
    if (n_surf) *n_surf = ns;
    if (n_full) *n_full = nf;
    D2H_OPT(corner_idx, h->dev.corner_idx, nc, int);
    D2H_OPT(surf_idx, h->dev.surf_idx, ns, int);
    D2H_OPT(full_idx, h->dev.full_idx, nf, int);
    D2H_OPT(corner_xyzi, h->dev.corner_feat, nc, float4);
    D2H_OPT(surf_xyzi, h->dev.surf_feat, ns, float4);
    return 0;
}

// The last (largest: a selection is ascending) position of every slot's selection of `kind` (0 corner, 1 surface, 2 full), -1 where it
// is empty: what the time range of a motion-deblur frame needs of the full selection (laser_mapping.hpp:1336: its largest stamp), as
// one small launch and one copy of n_scans ints instead of a selection per slot.
extern "C" int ll_fe_selection_last(ll_fe *h, int32_t n_scans, int32_t kind, int32_t *last_position)
{
    static const char *where = "ll_fe_selection_last";
    if (!h) return set_err(where, "null handle");
    if (!last_position) return set_err(where, "null argument");
    if (n_scans < 1 || n_scans > h->prm.max_scans) return set_err(where, "n_scans out of range");
    if (kind < 0 || kind > 2) return set_err(where, "kind must be 0 (corner), 1 (surface) or 2 (full)");
    if (kind == 2 && !h->dev.full_idx) return set_err(where, "the extractor keeps no full selection");
    HC(hipSetDevice(h->prm.device));
    if (!h->d_last) DM(h->d_last, (size_t)h->prm.max_scans);
    launch_fe_selection_last(h->dev, n_scans, kind, h->d_last, h->stream);
    HC(hipGetLastError());
    HC(hipMemcpyAsync(last_position, h->d_last, (size_t)n_scans * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HC(hipStreamSynchronize(h->stream));
    return 0;
}

// the selection ll_fe_select_batch left in slot `scan` (the batched counterpart of ll_fe_select's downloads)
extern "C" int ll_fe_selection(ll_fe *h, int32_t scan, int32_t *corner_idx, int32_t *n_corner, int32_t *surf_idx, int32_t *n_surf,
                               int32_t *full_idx, int32_t *n_full, float *corner_xyzi, float *surf_xyzi)
{
    if (!h) return set_err("ll_fe_selection", "null handle");
    if (scan < 0 || scan >= h->prm.max_scans) return set_err("ll_fe_selection", "scan out of range");
    HC(hipSetDevice(h->prm.device));
    HC(hipStreamSynchronize(h->stream));
    int nc = 0, ns = 0, nf = 0;
    HC(hipMemcpy(&nc, h->dev.n_corner + scan, sizeof(int), hipMemcpyDeviceToHost));
    HC(hipMemcpy(&ns, h->dev.n_surf + scan, sizeof(int), hipMemcpyDeviceToHost));
    HC(hipMemcpy(&nf, h->dev.n_full + scan, sizeof(int), hipMemcpyDeviceToHost));
    if (n_corner) *n_corner = nc;
    if (n_surf) *n_surf = ns;
    if (n_full) *n_full = nf;
    const size_t off = (size_t)scan * h->dev.stride;
    D2H_OPT(corner_idx, h->dev.corner_idx + off, nc, int);
    D2H_OPT(surf_idx, h->dev.surf_idx + off, ns, int);
    D2H_OPT(full_idx, h->dev.full_idx + off, nf, int);
    D2H_OPT(corner_xyzi, h->dev.corner_feat + off, nc, float4);
    D2H_OPT(surf_xyzi, h->dev.surf_feat + off, ns, float4);
    return 0;
}
