// ll_api_map_refine.hip -- the key-frame map refinement of the C ABI (ll_map_refine_*): the key frames' accumulated clouds stay on
// the device in one ragged store, and "these key frames into their corrected frames, filtered" is one launch chain and one host wait
// for any number of them (ll_map_refine_kernels.hip).  Mapping_refine of the reference, ceres_pose_graph_3d.hpp:368-538.
// ll_map_refine_add_logged takes the clouds of several key frames out of the scan log of a batched match buffer, device to device.
#include "ll_api_history_batch_internal.h"
#include "ll_map_refine.h"

struct ll_map_refine {
    int device = 0;
    hipStream_t stream = nullptr;
    float4 *d_store = nullptr;          // the stored clouds, one after the other
    int64_t cap = 0;                    // points the store has room for
    std::vector<int64_t> off{0};        // cloud id -> first point; off.back() = points held.  An id is a position and never changes.
    float4 *d_stage = nullptr;          // an add's upload
    int64_t stage_cap = 0;
    MrDev dev;
    float4 *d_out = nullptr;            // the last run's outputs, packed in selection order
    int64_t out_cap = 0;
    std::vector<int64_t> out_off;       // [n_sel + 1] of the last run; empty before the first
    float4 *d_merged = nullptr;         // the last merge's output
    int64_t merged_cap = 0, n_merged = -1;
    char *hp = nullptr;                 // page-locked staging: selections and work list in, offsets and status out
    size_t hp_bytes = 0;
    int64_t work[4] = {0, 0, 0, 0};
    // ll_map_refine_add_logged: the gather's work list (page-locked / device) and the event that orders this stream behind the log's
    SlCopy *hp_gwork = nullptr, *d_gwork = nullptr;
    int64_t gwork_cap = 0;
    hipEvent_t ev_log = nullptr;
};

static const int64_t kMrMaxPoints = 0x7ffffffeLL;  // the store, like a run, stays below 2^31 points

extern "C" void ll_map_refine_destroy(ll_map_refine *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    map_refine_free(h->dev);
    void *dev[] = {h->d_store, h->d_stage, h->d_out, h->d_merged};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (h->hp) (void)hipHostFree(h->hp);
    if (h->d_gwork) (void)hipFree(h->d_gwork);
    if (h->hp_gwork) (void)hipHostFree(h->hp_gwork);
    if (h->ev_log) (void)hipEventDestroy(h->ev_log);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// room for `need` points in the store: the capacity doubles, content and ids kept.  The stream is idle between calls, and is when this returns.
static int mr_store_room(ll_map_refine *h, int64_t need, const char *where)
{
    if (need <= h->cap) return 0;
    if (need > kMrMaxPoints) return set_err(where, "the store would pass 2^31 points");
    int64_t cap = std::max<int64_t>(2 * h->cap, need);
    if (cap > kMrMaxPoints) cap = kMrMaxPoints;
    float4 *store = nullptr;
    if (hipMalloc((void **)&store, (size_t)cap * sizeof(float4)) != hipSuccess) return set_err(where, "allocation failed");
    if (h->off.back() > 0) {
        HC(hipMemcpyAsync(store, h->d_store, (size_t)h->off.back() * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
        HC(hipStreamSynchronize(h->stream));
    }
    if (h->d_store) (void)hipFree(h->d_store);
    h->d_store = store;
    h->cap = cap;
    return 0;
}

// a scratch buffer whose content need not survive
static int mr_scratch_room(float4 **p, int64_t *cap, int64_t need, const char *where)
{
    if (need <= *cap) return 0;
    const int64_t c = std::min<int64_t>(std::max<int64_t>(2 * *cap, need), kMrMaxPoints);
    if (*p) (void)hipFree(*p);
    *p = nullptr, *cap = 0;
    if (hipMalloc((void **)p, (size_t)c * sizeof(float4)) != hipSuccess) return set_err(where, "allocation failed");
    *cap = c;
    return 0;
}

static int mr_host_room(ll_map_refine *h, size_t bytes, const char *where)
{
    if (bytes <= h->hp_bytes) return 0;
    const size_t b = std::max(2 * h->hp_bytes, bytes);
    if (h->hp) (void)hipHostFree(h->hp);
    h->hp = nullptr, h->hp_bytes = 0;
    if (hipHostMalloc((void **)&h->hp, b, hipHostMallocDefault) != hipSuccess) return set_err(where, "allocation failed");
    h->hp_bytes = b;
    return 0;
}

// A planned chain over src into out: the selections and the work list go up in one copy, the offsets and the status values come back
// in one, and the host waits once.  offsets [n_sel + 1] and status [n_sel] are filled.  Counts launches, waits and bytes into h->work.
static int mr_run_plan(ll_map_refine *h, const MrPlan &plan, const float4 *src, int mode, float leaf, float4 *out, int64_t *offsets, int32_t *status,
                       const char *where)
{
    const int n_sel = (int)plan.sel.size(), n_work = (int)plan.work.size();
    if (plan.total == 0) {  // nothing to key or sort: every selection is empty
        for (int s = 0; s <= n_sel; s++) offsets[s] = 0;
        for (int s = 0; s < n_sel; s++) status[s] = VOX_EMPTY;
        return 0;
    }
    const char *err = nullptr;
    if (map_refine_room(h->dev, plan.total, n_sel, n_work, &err)) return set_err(where, err);
    const size_t sel_bytes = (size_t)n_sel * sizeof(MrSel), work_bytes = (size_t)n_work * sizeof(MrWork), res_bytes = ((size_t)2 * n_sel + 1) * sizeof(int);
    if (mr_host_room(h, sel_bytes + work_bytes + res_bytes, where)) return -1;
    memcpy(h->hp, plan.sel.data(), sel_bytes);
    memcpy(h->hp + sel_bytes, plan.work.data(), work_bytes);
    int *res = (int *)(h->hp + sel_bytes + work_bytes);
    // whatever fails once something is enqueued, the stream is idle again when this returns: the staging, the scratch and the store
    // are reused by the next call (mr_store_room relies on it)
    hipError_t e = hipMemcpyAsync(h->dev.sel, h->hp, sel_bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->dev.work, h->hp + sel_bytes, work_bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && map_refine_chain(h->dev, src, mode, n_sel, n_work, (int)plan.total, leaf, out, h->stream, &err)) {
        (void)hipStreamSynchronize(h->stream);
        return set_err(where, err);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(res, h->dev.result, res_bytes, hipMemcpyDeviceToHost, h->stream);
    const hipError_t waited = hipStreamSynchronize(h->stream);  // the one wait
    if (e != hipSuccess || waited != hipSuccess) return set_err(where, hipGetErrorString(e != hipSuccess ? e : waited));
    h->work[0] += MR_CHAIN_LAUNCHES + 3;
    h->work[1] += 1;
    h->work[2] += (int64_t)(sel_bytes + work_bytes + res_bytes);
    for (int s = 0; s <= n_sel; s++) offsets[s] = res[s];
    for (int s = 0; s < n_sel; s++) status[s] = res[n_sel + 1 + s];
    return 0;
}

extern "C" int ll_map_refine_create(int32_t device, int64_t initial_points, ll_map_refine **out)
{
    const char *fn = "ll_map_refine_create";
    if (!out) return set_err(fn, "null argument");
    if (initial_points < 1) return set_err(fn, "initial_points out of range");
    if (initial_points > kMrMaxPoints) return set_err(fn, "the store would pass 2^31 points");
    if (check_device(device)) return -1;
    ll_map_refine *h = new ll_map_refine();
    h->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        mr_store_room(h, initial_points, fn)) {
        const std::string why = g_err;
        ll_map_refine_destroy(h);
        g_err = why.empty() ? std::string(fn) + ": allocation failed" : why;
        return -1;
    }
    *out = h;
    return 0;
}

extern "C" int ll_map_refine_add_cloud(ll_map_refine *h, const float *xyzi, int64_t n, float leaf, int64_t *id, int64_t *n_kept, int32_t *status)
{
    const char *fn = "ll_map_refine_add_cloud";
    if (!h || !id || (n > 0 && !xyzi)) return set_err(fn, "null argument");
    if (n < 0) return set_err(fn, "negative count");
    if (!(leaf > 0.f) || !std::isfinite(leaf)) return set_err(fn, "the leaf must be positive and finite");
    const int64_t used = h->off.back();
    if (n > kMrMaxPoints - used) return set_err(fn, "the store would pass 2^31 points");
    // the upload as one cloud, filtered straight into the store behind the clouds it holds (the filter keeps at most n points)
    const std::vector<int64_t> one{0, n};
    const int64_t zero = 0;
    MrPlan plan;
    const std::string why = mr_plan(MR_FILTER_ONLY, 1, &zero, nullptr, nullptr, leaf, one, &plan);
    if (!why.empty()) return set_err(fn, why.c_str());
    HC(hipSetDevice(h->device));
    if (mr_store_room(h, used + n, fn) || mr_scratch_room(&h->d_stage, &h->stage_cap, n, fn)) return -1;
    h->work[0] = h->work[1] = h->work[2] = 0;
    h->work[3] = n;
    if (n > 0) {
        HC(hipMemcpyAsync(h->d_stage, xyzi, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
        h->work[0] += 1;
        h->work[2] += n * (int64_t)sizeof(float4);
    }
    int64_t offsets[2];
    int32_t st = 0;
    if (mr_run_plan(h, plan, h->d_stage, MR_FILTER_ONLY, leaf, h->d_store + used, offsets, &st, fn)) return -1;
    h->off.push_back(used + offsets[1]);
    *id = (int64_t)h->off.size() - 2;
    if (n_kept) *n_kept = offsets[1];
    if (status) *status = st;
    return 0;
}

// room for the work list of a gather of n_work items (the stream is idle)
static int mr_gather_room(ll_map_refine *h, int64_t n_work, const char *where)
{
    if (!h->ev_log && hipEventCreateWithFlags(&h->ev_log, hipEventDisableTiming) != hipSuccess) return set_err(where, "allocation failed");
    if (n_work <= h->gwork_cap) return 0;
    const int64_t cap = std::max<int64_t>(2 * h->gwork_cap, n_work);
    if (h->d_gwork) (void)hipFree(h->d_gwork);
    if (h->hp_gwork) (void)hipHostFree(h->hp_gwork);
    h->d_gwork = nullptr, h->hp_gwork = nullptr, h->gwork_cap = 0;
    if (hipMalloc((void **)&h->d_gwork, (size_t)cap * sizeof(SlCopy)) != hipSuccess ||
        hipHostMalloc((void **)&h->hp_gwork, (size_t)cap * sizeof(SlCopy), hipHostMallocDefault) != hipSuccess)
        return set_err(where, "allocation failed");
    h->gwork_cap = cap;
    return 0;
}

// ll_map_refine_add_cloud for the key frames of a round, device to device: request r is the concatenation of the logged scans of its
// groups (the scan log of a batched match buffer, ll_api_history_batch_scanlog.hip).  One gather launch puts all requests into the
// staging array, one MR_FILTER_ONLY chain over n_req selections filters them into the store, the host waits once.
extern "C" int ll_map_refine_add_logged(ll_map_refine *h, ll_history_batch *hb, int64_t n_req, const int64_t *group_off, const int64_t *group_ids,
                                        float leaf, int64_t *ids, int64_t *n_kept, int32_t *status)
{
    const char *fn = "ll_map_refine_add_logged";
    if (!h || !hb || !group_off || (n_req > 0 && !ids)) return set_err(fn, "null argument");
    if (n_req < 0) return set_err(fn, "negative count");
    if (n_req > MR_MAX_SEL) return set_err(fn, "a run holds at most 2^20 selections");
    if (!(leaf > 0.f) || !std::isfinite(leaf)) return set_err(fn, "the leaf must be positive and finite");
    if (!hb->sl.on) return set_err(fn, "the scan log is not enabled (ll_history_batch_enable_scan_log)");
    if (hb->device != h->device) return set_err(fn, "the scan log lives on another device");
    if (group_off[0] != 0) return set_err(fn, "group offsets must start at 0");
    for (int64_t r = 0; r < n_req; r++)
        if (group_off[r + 1] < group_off[r]) return set_err(fn, "group offsets must ascend");
    const int64_t n_groups = group_off[n_req];
    if (n_groups > 0 && !group_ids) return set_err(fn, "null argument");
    SlBook &book = hb->sl.book;
    std::string why = sl_check_groups(book, n_groups, group_ids);
    if (!why.empty()) return set_err(fn, why.c_str());
    const int64_t used = h->off.back();
    int64_t total = 0;
    for (int64_t g = 0; g < n_groups; g++)
        for (const SlScan &e : *sl_group(book, group_ids[g])) {
            total += e.n;
            if (total > kMrMaxPoints - used) return set_err(fn, "the store would pass 2^31 points");
        }
    SlPlan gather;
    sl_gather_plan(book, n_req, group_off, group_ids, &gather);
    std::vector<int64_t> req_ids((size_t)n_req);
    for (int64_t r = 0; r < n_req; r++) req_ids[(size_t)r] = r;
    MrPlan plan;
    why = mr_plan(MR_FILTER_ONLY, n_req, req_ids.data(), nullptr, nullptr, leaf, gather.req_off, &plan);
    if (!why.empty()) return set_err(fn, why.c_str());
    HC(hipSetDevice(h->device));
    const int64_t n_work = (int64_t)gather.items.size();
    if (mr_store_room(h, used + total, fn) || mr_scratch_room(&h->d_stage, &h->stage_cap, total, fn) || mr_gather_room(h, n_work, fn)) return -1;
    h->work[0] = h->work[1] = h->work[2] = 0;
    h->work[3] = total;
    if (n_work > 0) {
        for (int64_t w = 0; w < n_work; w++) {
            const SlItem &it = gather.items[(size_t)w];
            h->hp_gwork[w] = SlCopy{hb_scan_log_block(hb, it.block) + it.first, it.dst, it.n, it.req};
        }
        // this stream behind the log kernels that filled the blocks; then the work list up and the one gather.  A failure leaves the
        // stream idle, as mr_run_plan does.
        const char *err = nullptr;
        hipError_t e = hipEventRecord(h->ev_log, hb->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, h->ev_log, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(h->d_gwork, h->hp_gwork, (size_t)n_work * sizeof(SlCopy), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess && sl_gather(h->d_gwork, (int)n_work, h->d_stage, h->stream, &err)) e = hipErrorUnknown;
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);
            return set_err(fn, err ? err : hipGetErrorString(e));
        }
        h->work[0] += 4;
        h->work[2] += n_work * (int64_t)sizeof(SlCopy);
    }
    std::vector<int64_t> offsets((size_t)n_req + 1, 0);
    std::vector<int32_t> st((size_t)n_req, 0);
    if (mr_run_plan(h, plan, h->d_stage, MR_FILTER_ONLY, leaf, h->d_store + used, offsets.data(), st.data(), fn)) return -1;
    for (int64_t r = 0; r < n_req; r++) {  // consecutive ids, as n_req add_cloud calls would give
        h->off.push_back(used + offsets[(size_t)r + 1]);
        ids[r] = (int64_t)h->off.size() - 2;
        if (n_kept) n_kept[r] = offsets[(size_t)r + 1] - offsets[(size_t)r];
        if (status) status[r] = st[(size_t)r];
    }
    for (int64_t g = 0; g < n_groups; g++) sl_drop(book, group_ids[g]);  // consumed: the host has waited for the chain that read them
    return 0;
}

extern "C" int ll_map_refine_add_stored(ll_map_refine *h, const float *xyzi, int64_t n, int64_t *id)
{
    const char *fn = "ll_map_refine_add_stored";
    if (!h || !id || (n > 0 && !xyzi)) return set_err(fn, "null argument");
    if (n < 0) return set_err(fn, "negative count");
    const int64_t used = h->off.back();
    if (n > kMrMaxPoints - used) return set_err(fn, "the store would pass 2^31 points");
    HC(hipSetDevice(h->device));
    if (mr_store_room(h, used + n, fn)) return -1;
    h->work[0] = h->work[1] = h->work[2] = 0;
    h->work[3] = n;
    if (n > 0) {
        HC(hipMemcpyAsync(h->d_store + used, xyzi, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
        const hipError_t e = hipStreamSynchronize(h->stream);  // (the caller's buffer is its own again)
        if (e != hipSuccess) return set_err(fn, hipGetErrorString(e));
        h->work[0] = h->work[1] = 1;
        h->work[2] = n * (int64_t)sizeof(float4);
    }
    h->off.push_back(used + n);
    *id = (int64_t)h->off.size() - 2;
    return 0;
}

extern "C" int64_t ll_map_refine_size(const ll_map_refine *h)
{
    if (!h) return set_err("ll_map_refine_size", "null argument");
    return (int64_t)h->off.size() - 1;
}

extern "C" int ll_map_refine_cloud(ll_map_refine *h, int64_t id, float *xyzi_out, int64_t capacity_points, int64_t *n)
{
    const char *fn = "ll_map_refine_cloud";
    if (!h || !n) return set_err(fn, "null argument");
    if (id < 0 || id >= (int64_t)h->off.size() - 1) return set_err(fn, "id out of range");
    const int64_t cnt = h->off[id + 1] - h->off[id];
    *n = cnt;
    if (!xyzi_out) return 0;  // (the size alone)
    if (capacity_points < cnt) return set_err(fn, "capacity below the cloud's size");
    HC(hipSetDevice(h->device));
    if (cnt > 0) HC(hipMemcpy(xyzi_out, h->d_store + h->off[id], (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int ll_map_refine_affine(const double *ori7, const double *opm7, float *R9_out, float *T3_out)
{
    const char *fn = "ll_map_refine_affine";
    if (!ori7 || !opm7 || !R9_out || !T3_out) return set_err(fn, "null argument");
    for (int i = 0; i < 7; i++)
        if (!std::isfinite(ori7[i]) || !std::isfinite(opm7[i])) return set_err(fn, "a pose is not finite");
    mr_affine(ori7, opm7, R9_out, T3_out);
    return 0;
}

extern "C" int ll_map_refine_run(ll_map_refine *h, int32_t mode, int64_t n_sel, const int64_t *ids, const double *poses_ori7, const double *poses_opm7,
                                 float leaf, int64_t *offsets_out, int32_t *status_out)
{
    const char *fn = "ll_map_refine_run";
    if (!h || !offsets_out) return set_err(fn, "null argument");
    if (mode != MR_FILTER_THEN_MOVE && mode != MR_MOVE_THEN_FILTER) return set_err(fn, "mode must be 0 (filter, then move) or 1 (move, then filter)");
    if (n_sel > 0 && !status_out) return set_err(fn, "null argument");
    MrPlan plan;
    const std::string why = mr_plan(mode, n_sel, ids, poses_ori7, poses_opm7, leaf, h->off, &plan);
    if (!why.empty()) return set_err(fn, why.c_str());
    // nothing below refuses on the arguments: from here the last outputs are replaced
    HC(hipSetDevice(h->device));
    if (plan.total > 0 && mr_scratch_room(&h->d_out, &h->out_cap, plan.total, fn)) {
        h->out_off.clear();
        return -1;
    }
    h->work[0] = h->work[1] = h->work[2] = 0;
    h->work[3] = plan.total;
    h->n_merged = -1;
    h->out_off.assign((size_t)n_sel + 1, 0);
    if (n_sel == 0) {
        offsets_out[0] = 0;
        return 0;
    }
    if (mr_run_plan(h, plan, h->d_store, mode, leaf, h->d_out, h->out_off.data(), status_out, fn)) {
        h->out_off.clear();
        return -1;
    }
    for (int64_t s = 0; s <= n_sel; s++) offsets_out[s] = h->out_off[(size_t)s];
    return 0;
}

extern "C" int ll_map_refine_fetch(ll_map_refine *h, float *xyzi_out, int64_t capacity_points)
{
    const char *fn = "ll_map_refine_fetch";
    if (!h) return set_err(fn, "null argument");
    if (h->out_off.empty()) return set_err(fn, "no run to fetch");
    const int64_t cnt = h->out_off.back();
    if (cnt > 0 && !xyzi_out) return set_err(fn, "null argument");
    if (capacity_points < cnt) return set_err(fn, "capacity below the outputs' size");
    if (cnt == 0) return 0;
    HC(hipSetDevice(h->device));
    HC(hipMemcpyAsync(xyzi_out, h->d_out, (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    HC(hipStreamSynchronize(h->stream));
    h->work[0] += 1;
    h->work[1] += 1;
    h->work[2] += cnt * (int64_t)sizeof(float4);
    return 0;
}

extern "C" int ll_map_refine_merge(ll_map_refine *h, float leaf, int64_t *n_out, int32_t *status)
{
    const char *fn = "ll_map_refine_merge";
    if (!h || !n_out) return set_err(fn, "null argument");
    if (h->out_off.empty()) return set_err(fn, "no run to merge");
    const std::vector<int64_t> one{0, h->out_off.back()};
    const int64_t zero = 0;
    MrPlan plan;
    const std::string why = mr_plan(MR_FILTER_ONLY, 1, &zero, nullptr, nullptr, leaf, one, &plan);
    if (!why.empty()) return set_err(fn, why.c_str());
    HC(hipSetDevice(h->device));
    if (mr_scratch_room(&h->d_merged, &h->merged_cap, plan.total, fn)) return -1;
    h->work[0] = h->work[1] = h->work[2] = 0;
    h->work[3] = plan.total;
    int64_t offsets[2];
    int32_t st = 0;
    h->n_merged = -1;
    if (mr_run_plan(h, plan, h->d_out, MR_FILTER_ONLY, leaf, h->d_merged, offsets, &st, fn)) return -1;
    h->n_merged = offsets[1];
    *n_out = offsets[1];
    if (status) *status = st;
    return 0;
}

extern "C" int ll_map_refine_fetch_merged(ll_map_refine *h, float *xyzi_out, int64_t capacity_points)
{
    const char *fn = "ll_map_refine_fetch_merged";
    if (!h) return set_err(fn, "null argument");
    if (h->n_merged < 0) return set_err(fn, "no merge to fetch");
    if (h->n_merged > 0 && !xyzi_out) return set_err(fn, "null argument");
    if (capacity_points < h->n_merged) return set_err(fn, "capacity below the merged cloud's size");
    if (h->n_merged == 0) return 0;
    HC(hipSetDevice(h->device));
    HC(hipMemcpyAsync(xyzi_out, h->d_merged, (size_t)h->n_merged * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    HC(hipStreamSynchronize(h->stream));
    h->work[0] += 1;
    h->work[1] += 1;
    h->work[2] += h->n_merged * (int64_t)sizeof(float4);
    return 0;
}

extern "C" int ll_map_refine_work(ll_map_refine *h, int64_t out[4])
{
    if (!h || !out) return set_err("ll_map_refine_work", "null argument");
    for (int i = 0; i < 4; i++) out[i] = h->work[i];
    return 0;
}
