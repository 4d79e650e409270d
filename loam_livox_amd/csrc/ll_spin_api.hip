// ll_spin_api.hip -- host side of the ll_spin_* entry points of include/loam_livox_hip.h (spinning-lidar feature
// extraction, hku-mars/loam_livox source/laser_feature_extractor.hpp:393-787).  Device memory, launch order and the
// host-libm resolve of ambiguous atanf / atan2f decisions; the arithmetic runs in ll_spin_kernels.hip.
#include "ll_api_internal.h"

struct ll_spin {
    ll_spin_params prm;
    int n_vlines = 0;  // lines that can hold points: 16, or 51 for the 64-line rule (IDs 0..50)
    SpinDev d;
    VoxelDev vox;
    hipStream_t stream = nullptr;
    hipEvent_t ev[8] = {};  // [0]-[1] assign; [2] start of the later phases, [3]-[7] after lines, curvature, sort, select, VoxelGrid
    std::vector<int> h_n;      // points per slot as uploaded
    int last_batch = 0;        // n_scans of the last ll_spin_extract_batch
    // hand-off to device consumers (ll_reg_enqueue_spin, ll_history_add_spin, ll_cloud_transform_spin_device): allocated by the first
    // hand-off, so that callers who only extract and download pay nothing
    int pack_stride = 0;
    float4 *pack = nullptr;    // [S][pack_stride] the less-sharp cloud (corner stack)
    int *pack_nc = nullptr, *pack_ns = nullptr;  // [S] sizes of the corner and the surface stack
    int packed_n = 0;          // slots 0 .. packed_n-1 of `pack` hold the handle's current outputs (0 after every extraction)
    float4 *pack_x = nullptr;  // [S][pack_stride] the cloud ll_cloud_transform_spin_device asked for (the corner stack may be in use)
    int *pack_xn = nullptr;    // [S]
    hipEvent_t ev_pack[2] = {};  // around the last pack of the corner stack (ll_spin_handoff_time)
};

extern "C" void ll_spin_default_params(ll_spin_params *p)
{
    memset(p, 0, sizeof(*p));
    p->scan_line = 16;           // :137
    p->minimum_range = 0.1f;     // :140
    p->plane_resolution = 0.8f;  // :138
    p->device = 0;
    p->max_points = 32768;
    p->max_scans = 1;
    p->max_line_points = 8192;
}

static int spin_create_impl(const ll_spin_params *p, ll_spin *h)
{
    h->prm = *p;
    h->n_vlines = p->scan_line == 16 ? 16 : 51;
    {  // at most 200 less-sharp picks per sub-region (:667-676), 6 sub-regions per line
        const long long bound = 1200ll * p->scan_line;
        h->pack_stride = (int)(bound < p->max_points ? bound : p->max_points);
    }
    const int S = p->max_scans;
    const size_t P = (size_t)p->max_points, SP = (size_t)S * P;
    SpinDev &d = h->d;
    memset(&d, 0, sizeof(d));
    d.stride = p->max_points;
    d.line_cap = p->max_line_points;
    d.ambig_cap = (int)(SP / 16 > 4096 ? SP / 16 : 4096);
    d.thres = p->minimum_range;
    if (dmalloc(&d.in, SP) || dmalloc(&d.n_in, S) || dmalloc(&d.ori_se, S) || dmalloc(&d.raw_sid, SP) || dmalloc(&d.raw_ori, SP) || dmalloc(&d.n_ambig, 1) ||
        dmalloc(&d.ambig, d.ambig_cap) || dmalloc(&d.ambig_p, d.ambig_cap) || dmalloc(&d.ambig_sid, d.ambig_cap) || dmalloc(&d.ambig_ori, d.ambig_cap) || dmalloc(&d.line_off, (size_t)S * (SPIN_MAX_LINES + 1)) || dmalloc(&d.full, SP) || dmalloc(&d.full_src, SP) ||
        dmalloc(&d.curv, SP) || dmalloc(&d.flags, SP) || dmalloc(&d.label, SP) || dmalloc(&d.order, SP) || dmalloc(&d.sharp, SP) || dmalloc(&d.less_sharp, SP) ||
        dmalloc(&d.flat, SP) || dmalloc(&d.lf_pos, SP) || dmalloc(&d.vox_in, (size_t)S * h->n_vlines * p->max_line_points) ||
        dmalloc(&d.vox_n, (size_t)S * h->n_vlines) || dmalloc(&d.less_flat, SP) || dmalloc(&d.cnt, (size_t)S * SPIN_NCNT))
        return -1;
    const char *err = nullptr;
    if (voxel_alloc(h->vox, S * h->n_vlines, p->max_line_points, &err)) return set_err("ll_spin_create", err);
    HC(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    // zeroed on the handle's own stream: a non-blocking stream is not ordered after the null stream, so a null-stream hipMemset could
    // still land after the first extraction's kernels and wipe the counts and line offsets they wrote
    HC(hipMemsetAsync(d.n_in, 0, S * sizeof(int), h->stream));
    HC(hipMemsetAsync(d.cnt, 0, (size_t)S * SPIN_NCNT * sizeof(int), h->stream));
    HC(hipMemsetAsync(d.line_off, 0, (size_t)S * (SPIN_MAX_LINES + 1) * sizeof(int), h->stream));
    HC(hipStreamSynchronize(h->stream));
    for (auto &e : h->ev) HC(hipEventCreate(&e));
    h->h_n.assign(S, 0);
    return 0;
}

extern "C" int ll_spin_create(const ll_spin_params *p, ll_spin **out)
{
    if (!p || !out) return set_err("ll_spin_create", "null argument");
    if (p->scan_line != 16 && p->scan_line != 64) return set_err("ll_spin_create", "only support velodyne with 16 or 64 scan line!");
    if (p->max_points < 1 || p->max_points > LL_SPIN_MAX_POINTS || p->max_scans < 1 || p->max_line_points < 1)
        return set_err("ll_spin_create", "bad capacity (max_points must be in 1 .. 400000)");
    if (!(p->plane_resolution > 0.f)) return set_err("ll_spin_create", "plane_resolution must be positive");
    if ((size_t)p->max_scans * p->max_points >= 0x7fffffffull) return set_err("ll_spin_create", "max_scans * max_points must stay below 2^31");
    if (check_device(p->device)) return -1;
    ll_spin *h = new ll_spin();
    if (spin_create_impl(p, h)) {
        ll_spin_destroy(h);
        return -1;
    }
    *out = h;
    return 0;
}

extern "C" void ll_spin_destroy(ll_spin *h)
{
    if (!h) return;
    (void)hipSetDevice(h->prm.device);
    SpinDev &d = h->d;
    void *ptrs[] = {d.in, d.n_in, d.ori_se, d.raw_sid, d.raw_ori, d.n_ambig, d.ambig, d.ambig_p, d.ambig_sid, d.ambig_ori, d.line_off, d.full, d.full_src, d.curv, d.flags,
                    d.label, d.order, d.sharp, d.less_sharp, d.flat, d.lf_pos, d.vox_in, d.vox_n, d.less_flat, d.cnt,
                    h->pack, h->pack_nc, h->pack_ns, h->pack_x, h->pack_xn};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    voxel_free(h->vox);
    for (auto &e : h->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : h->ev_pack)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

static bool survives(const float *q, float thres)
{
    return isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) && !(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] < thres * thres);
}

extern "C" int ll_spin_upload(ll_spin *h, int32_t first_scan, int32_t n_scans, const float *xyzi, const int32_t *n_points, int32_t stride_points)
{
    if (!h || (!xyzi && n_scans > 0) || !n_points) return set_err("ll_spin_upload", "null argument");
    if (first_scan < 0 || n_scans < 0 || first_scan + n_scans > h->prm.max_scans) return set_err("ll_spin_upload", "scan slots out of range");
    for (int b = 0; b < n_scans; b++) {
        if (n_points[b] < 0 || n_points[b] > stride_points) return set_err("ll_spin_upload", "n_points out of range");
        if (n_points[b] > h->prm.max_points) return set_err("ll_spin_upload", "scan has more points than max_points");
    }
    HC(hipSetDevice(h->prm.device));
    HC(hipStreamSynchronize(h->stream));
    const float thres = h->prm.minimum_range;
    std::vector<float2> se(n_scans);
    for (int b = 0; b < n_scans; b++) {
        const float *c = xyzi + (size_t)b * stride_points * 4;
        const int n = n_points[b];
        int first = 0, last = n - 1;
        while (first < n && !survives(c + 4 * first, thres)) first++;
        while (last > first && !survives(c + 4 * last, thres)) last--;
        float startOri = 0.f, endOri = 0.f;
        if (first < n) {  // :403-415 on the filtered cloud
            startOri = -atan2f(c[4 * first + 1], c[4 * first]);
            endOri = -atan2f(c[4 * last + 1], c[4 * last]) + 2 * M_PI;
            if (endOri - startOri > 3 * M_PI)
                endOri -= 2 * M_PI;
            else if (endOri - startOri < M_PI)
                endOri += 2 * M_PI;
        }
        se[b] = make_float2(startOri, endOri);
        if (n > 0)
            HC(hipMemcpyAsync(h->d.in + (size_t)(first_scan + b) * h->d.stride, c, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
        h->h_n[first_scan + b] = n;
    }
    if (n_scans > 0) {
        HC(hipMemcpyAsync(h->d.n_in + first_scan, n_points, n_scans * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HC(hipMemcpyAsync(h->d.ori_se + first_scan, se.data(), n_scans * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    }
    HC(hipStreamSynchronize(h->stream));
    return 0;
}

static int max_n(const ll_spin *h, int n_scans)
{
    int m = 0;
    for (int b = 0; b < n_scans; b++) m = h->h_n[b] > m ? h->h_n[b] : m;
    return m;
}

// everything after the per-point assignment: lines, curvature, sort, select, VoxelGrid
static int spin_run_rest(ll_spin *h, int n_scans)
{
    const int L = h->prm.scan_line;
    const int mn = max_n(h, n_scans);
    h->packed_n = 0;  // the packed corner stack no longer holds the handle's outputs
    HC(hipEventRecord(h->ev[2], h->stream));
    spin_launch_lines(h->d, n_scans, L, h->stream);
    HC(hipEventRecord(h->ev[3], h->stream));
    spin_launch_curv(h->d, n_scans, mn, h->stream);
    HC(hipEventRecord(h->ev[4], h->stream));
    spin_launch_sort(h->d, n_scans, L, h->stream);
    HC(hipEventRecord(h->ev[5], h->stream));
    spin_launch_select(h->d, n_scans, L, h->n_vlines, h->stream);
    HC(hipEventRecord(h->ev[6], h->stream));
    const float leaf1 = h->prm.plane_resolution / 2;  // :192 setLeafSize(m_plane_resolution / 2, ...) in float
    const float leaf[3] = {leaf1, leaf1, leaf1};
    const char *err = nullptr;
    if (voxel_filter(h->vox, h->d.vox_in, h->d.vox_n, h->prm.max_line_points, n_scans * h->n_vlines, leaf, h->stream, &err))
        return set_err("ll_spin_extract_batch", err);
    spin_launch_gather(h->d, h->vox.out, h->vox.n_out, h->vox.out_stride, n_scans, h->n_vlines, h->stream);
    HC(hipEventRecord(h->ev[7], h->stream));
    HC(hipGetLastError());
    return 0;
}

extern "C" int ll_spin_extract_batch(ll_spin *h, int32_t n_scans)
{
    if (!h) return set_err("ll_spin_extract_batch", "null handle");
    if (n_scans < 1 || n_scans > h->prm.max_scans) return set_err("ll_spin_extract_batch", "n_scans out of range");
    HC(hipSetDevice(h->prm.device));
    HC(hipMemsetAsync(h->d.n_ambig, 0, sizeof(int), h->stream));
    HC(hipEventRecord(h->ev[0], h->stream));
    spin_launch_assign(h->d, n_scans, h->prm.scan_line, max_n(h, n_scans), h->stream);
    HC(hipEventRecord(h->ev[1], h->stream));
    h->last_batch = n_scans;
    return spin_run_rest(h, n_scans);
}

extern "C" int ll_spin_sync(ll_spin *h)
{
    if (!h) return set_err("ll_spin_sync", "null handle");
    HC(hipSetDevice(h->prm.device));
    HC(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int ll_spin_resolve(ll_spin *h)
{
    if (!h) return set_err("ll_spin_resolve", "null handle");
    HC(hipSetDevice(h->prm.device));
    HC(hipStreamSynchronize(h->stream));
    int n_amb = 0;
    HC(hipMemcpy(&n_amb, h->d.n_ambig, sizeof(int), hipMemcpyDeviceToHost));
    if (n_amb == 0) return 0;
    if (n_amb > h->d.ambig_cap) return set_err("ll_spin_resolve", "more points near an atanf / atan2f decision than the list holds");
    // the listed points and their device decisions come back in one copy, the host decisions go out in one copy
    spin_launch_ambig(h->d, n_amb, false, h->stream);
    HC(hipGetLastError());
    std::vector<float4> p(n_amb);
    std::vector<int> sid_d(n_amb), sid(n_amb);
    std::vector<float> ori_d(n_amb), ori(n_amb);
    HC(hipMemcpyAsync(p.data(), h->d.ambig_p, n_amb * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    HC(hipMemcpyAsync(sid_d.data(), h->d.ambig_sid, n_amb * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HC(hipMemcpyAsync(ori_d.data(), h->d.ambig_ori, n_amb * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HC(hipStreamSynchronize(h->stream));
    bool changed = false;
    for (int k = 0; k < n_amb; k++) {
        // the same decisions as spin_assign_kernel, with the host libm
        sid[k] = spin_scan_id(spin_angle(p[k].x, p[k].y, p[k].z), h->prm.scan_line);
        ori[k] = sid[k] >= 0 ? spin_ori(p[k].x, p[k].y) : 0.f;
        changed |= sid[k] != sid_d[k] || memcmp(&ori[k], &ori_d[k], sizeof(float)) != 0;
    }
    if (changed) {
        HC(hipMemcpyAsync(h->d.ambig_sid, sid.data(), n_amb * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HC(hipMemcpyAsync(h->d.ambig_ori, ori.data(), n_amb * sizeof(float), hipMemcpyHostToDevice, h->stream));
        spin_launch_ambig(h->d, n_amb, true, h->stream);
        if (spin_run_rest(h, h->last_batch)) return -1;
        HC(hipStreamSynchronize(h->stream));
    }
    return n_amb;
}

extern "C" int ll_spin_counts(ll_spin *h, int32_t n_scans, int32_t *counts, int32_t *status)
{
    if (!h || !counts) return set_err("ll_spin_counts", "null argument");
    if (n_scans < 1 || n_scans > h->prm.max_scans) return set_err("ll_spin_counts", "n_scans out of range");
    HC(hipSetDevice(h->prm.device));
    HC(hipStreamSynchronize(h->stream));
    std::vector<int> c((size_t)n_scans * SPIN_NCNT);
    HC(hipMemcpy(c.data(), h->d.cnt, c.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < n_scans; b++) {
        const int *cb = &c[(size_t)b * SPIN_NCNT];
        for (int k = 0; k < 5; k++) counts[5 * b + k] = cb[k];
        if (status) status[b] = cb[SPIN_C_STATUS];
    }
    return 0;
}

extern "C" int ll_spin_cloud(ll_spin *h, int32_t scan, int32_t which, float *xyzi, int32_t *idx, int32_t *n)
{
    if (!h || !n) return set_err("ll_spin_cloud", "null argument");
    if (scan < 0 || scan >= h->prm.max_scans) return set_err("ll_spin_cloud", "scan out of range");
    if (which < LL_SPIN_FULL || which > LL_SPIN_LESS_FLAT_PRE) return set_err("ll_spin_cloud", "unknown cloud");
    if (which == LL_SPIN_LESS_FLAT && idx) return set_err("ll_spin_cloud", "the less-flat cloud (voxel centroids) has no index");
    HC(hipSetDevice(h->prm.device));
    HC(hipStreamSynchronize(h->stream));
    int c[SPIN_NCNT];
    HC(hipMemcpy(c, h->d.cnt + (size_t)scan * SPIN_NCNT, sizeof(c), hipMemcpyDeviceToHost));
    static const int slot[6] = {SPIN_C_FULL, SPIN_C_SHARP, SPIN_C_LESS_SHARP, SPIN_C_FLAT, SPIN_C_LESS_FLAT, SPIN_C_LF_PRE};
    const int m = c[slot[which]];
    *n = m;
    const size_t base = (size_t)scan * h->d.stride;
    if (m <= 0) return 0;
    const float4 *full = h->d.full + base;
    if (which == LL_SPIN_FULL) {
        if (xyzi) HC(hipMemcpy(xyzi, full, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost));
        if (idx) HC(hipMemcpy(idx, h->d.full_src + base, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
        return 0;
    }
    if (which == LL_SPIN_LESS_FLAT) {
        if (xyzi) HC(hipMemcpy(xyzi, h->d.less_flat + base, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost));
        return 0;
    }
    const int *src = which == LL_SPIN_SHARP ? h->d.sharp : which == LL_SPIN_LESS_SHARP ? h->d.less_sharp : which == LL_SPIN_FLAT ? h->d.flat : h->d.lf_pos;
    std::vector<int> pos(m);
    HC(hipMemcpy(pos.data(), src + base, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
    if (idx) memcpy(idx, pos.data(), (size_t)m * sizeof(int));
    if (xyzi) {
        std::vector<float4> f(c[SPIN_C_FULL]);
        HC(hipMemcpy(f.data(), full, f.size() * sizeof(float4), hipMemcpyDeviceToHost));
        for (int k = 0; k < m; k++) memcpy(xyzi + 4 * (size_t)k, &f[pos[k]], sizeof(float4));
    }
    return 0;
}

extern "C" int ll_spin_lines(ll_spin *h, int32_t scan, int32_t *line_start, int32_t *line_n)
{
    if (!h || !line_start || !line_n) return set_err("ll_spin_lines", "null argument");
    if (scan < 0 || scan >= h->prm.max_scans) return set_err("ll_spin_lines", "scan out of range");
    HC(hipSetDevice(h->prm.device));
    HC(hipStreamSynchronize(h->stream));
    int off[SPIN_MAX_LINES + 1];
    HC(hipMemcpy(off, h->d.line_off + (size_t)scan * (SPIN_MAX_LINES + 1), sizeof(off), hipMemcpyDeviceToHost));
    for (int l = 0; l < h->prm.scan_line; l++) {
        line_start[l] = off[l];
        line_n[l] = off[l + 1] - off[l];
    }
    return 0;
}

extern "C" int ll_spin_extract(ll_spin *h, const float *xyzi, int32_t n)
{
    if (!h) return set_err("ll_spin_extract", "null handle");
    const int32_t np = n;
    if (ll_spin_upload(h, 0, 1, xyzi, &np, n) || ll_spin_extract_batch(h, 1) || ll_spin_resolve(h) < 0) return -1;
    int32_t counts[5], status = 0;
    if (ll_spin_counts(h, 1, counts, &status)) return -1;
    return status;
}

// ---------------------------------------------------------------------------------------------------- hand-off
namespace ll {

void spin_view(const ll_spin *h, SpinView *v)
{
    memset(v, 0, sizeof(*v));
    v->device = h->prm.device;
    v->max_scans = h->prm.max_scans;
    v->max_points = h->prm.max_points;
    v->scan_line = h->prm.scan_line;
    v->pack_stride = h->pack_stride;
    v->stream = h->stream;
}

int spin_handoff(ll_spin *h, int n_scans, SpinView *v)
{
    if (n_scans < 1 || n_scans > h->prm.max_scans) return set_err("ll_spin (hand-off)", "n_scans out of range");
    HC(hipSetDevice(h->prm.device));
    const size_t S = h->prm.max_scans;
    if (!h->pack) {
        if (dmalloc(&h->pack, S * h->pack_stride) || dmalloc(&h->pack_nc, S) || dmalloc(&h->pack_ns, S)) return -1;
        for (auto &e : h->ev_pack) HC(hipEventCreate(&e));
    }
    // On the handle's own stream: behind the extraction that wrote the lists, and ahead of the event every consumer waits for.  Nothing
    // is zeroed: the kernel writes both counts of every slot it hands over, and no consumer reads a cloud beyond its count.
    if (h->packed_n < n_scans) {
        HC(hipEventRecord(h->ev_pack[0], h->stream));
        spin_launch_pack(h->d, h->d.less_sharp, SPIN_C_LESS_SHARP, h->pack, h->pack_stride, h->pack_nc, h->pack_ns, n_scans, h->stream);
        HC(hipEventRecord(h->ev_pack[1], h->stream));
        HC(hipGetLastError());
        h->packed_n = n_scans;
    }
    spin_view(h, v);
    v->corner = h->pack;
    v->n_corner = h->pack_nc;
    v->surf = h->d.less_flat;
    v->n_surf = h->pack_ns;
    return 0;
}

int spin_device_cloud(ll_spin *h, int n_scans, int which, const float4 **src, int *stride, int *counts)
{
    if (n_scans < 1 || n_scans > h->prm.max_scans) return set_err("ll_spin (hand-off)", "n_scans out of range");
    HC(hipSetDevice(h->prm.device));
    const size_t S = h->prm.max_scans;
    static const int slot[5] = {SPIN_C_FULL, SPIN_C_SHARP, SPIN_C_LESS_SHARP, SPIN_C_FLAT, SPIN_C_LESS_FLAT};
    if (which == LL_SPIN_FULL || which == LL_SPIN_LESS_FLAT) {
        *src = which == LL_SPIN_FULL ? h->d.full : h->d.less_flat;
        *stride = h->d.stride;
    } else {
        if (!h->pack_x) {
            if (dmalloc(&h->pack_x, S * h->pack_stride) || dmalloc(&h->pack_xn, S)) return -1;
        }
        const int *list = which == LL_SPIN_SHARP ? h->d.sharp : which == LL_SPIN_LESS_SHARP ? h->d.less_sharp : h->d.flat;
        spin_launch_pack(h->d, list, slot[which], h->pack_x, h->pack_stride, h->pack_xn, nullptr, n_scans, h->stream);
        HC(hipGetLastError());
        *src = h->pack_x;
        *stride = h->pack_stride;
    }
    HC(hipStreamSynchronize(h->stream));
    std::vector<int> c((size_t)n_scans * SPIN_NCNT);
    HC(hipMemcpy(c.data(), h->d.cnt, c.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < n_scans; b++) {
        const int m = c[(size_t)b * SPIN_NCNT + slot[which]];
        counts[b] = m < *stride ? m : *stride;
    }
    return 0;
}

}  // namespace ll

extern "C" int ll_spin_kernel_times(ll_spin *h, float ms[6])
{
    if (!h || !ms) return set_err("ll_spin_kernel_times", "null argument");
    HC(hipSetDevice(h->prm.device));
    HC(hipEventSynchronize(h->ev[7]));
    HC(hipEventElapsedTime(&ms[0], h->ev[0], h->ev[1]));
    for (int k = 1; k < 6; k++) HC(hipEventElapsedTime(&ms[k], h->ev[k + 1], h->ev[k + 2]));
    return 0;
}

extern "C" int ll_spin_handoff_time(ll_spin *h, float *ms)
{
    if (!h || !ms) return set_err("ll_spin_handoff_time", "null argument");
    if (!h->ev_pack[1]) return set_err("ll_spin_handoff_time", "nothing has been handed over yet");
    HC(hipSetDevice(h->prm.device));
    HC(hipEventSynchronize(h->ev_pack[1]));
    HC(hipEventElapsedTime(ms, h->ev_pack[0], h->ev_pack[1]));
    return 0;
}
