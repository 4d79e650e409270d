// ll_api_history_batch_scanlog.hip -- the scan log of the batched match buffer: m_laser_cloud_full_history of every slot kept on the
// device (laser_mapping.hpp:1456, 1480-1486, 1545-1558).  The blocks' lives are host bookkeeping (ll_scan_log.h); a log call is one
// launch for all slots and no host wait (ll_scan_log_kernels.hip); hand-over and drop touch no device memory.
#include "ll_api_history_batch_internal.h"

void hb_scan_log_free(ll_history_batch *h)
{
    HbScanLog &l = h->sl;
    for (float4 *p : l.chunks)
        if (p) (void)hipFree(p);
    l.chunks.clear();
    if (l.d_tab) (void)hipFree(l.d_tab);
    if (l.hp_tab) (void)hipHostFree(l.hp_tab);
    if (l.ev) (void)hipEventDestroy(l.ev);
    l.d_tab = nullptr, l.hp_tab = nullptr, l.ev = nullptr;
    l.on = l.pending = false;
    l.book = SlBook();
}

// `want` free blocks: the pool grows by whole chunks; the chunks it has stay where they are
static int hb_scan_log_room(const char *where, ll_history_batch *h, int want)
{
    HbScanLog &l = h->sl;
    for (int c = sl_chunks_short(l.book, want); c > 0; c--) {
        float4 *p = nullptr;
        if (hipMalloc((void **)&p, (size_t)l.book.chunk_blocks * (size_t)h->max_pts * sizeof(float4)) != hipSuccess)
            return set_err(where, "allocation failed");
        l.chunks.push_back(p);
        sl_add_chunk(l.book);
    }
    return 0;
}

extern "C" int ll_history_batch_enable_scan_log(ll_history_batch *h, int32_t maximum_history_size, int64_t initial_scans)
{
    static const char *where = "ll_history_batch_enable_scan_log";
    if (!h) return set_err(where, "null argument");
    if (!h->fm_on) return set_err(where, "full maps are not enabled (ll_history_batch_enable_full_maps)");
    if (h->sl.on) return set_err(where, "already enabled");
    if (maximum_history_size < 1) return set_err(where, "maximum_history_size must be at least 1");
    if (initial_scans < 1 || initial_scans > (1 << 24)) return set_err(where, "initial_scans out of range");
    HC(hipSetDevice(h->device));
    HbScanLog &l = h->sl;
    sl_init(l.book, h->S, maximum_history_size, (int)initial_scans);
    const bool ok = hipHostMalloc((void **)&l.hp_tab, (size_t)h->S * sizeof(SlSlot), hipHostMallocDefault) == hipSuccess &&
                    hipMalloc((void **)&l.d_tab, (size_t)h->S * sizeof(SlSlot)) == hipSuccess &&
                    hipEventCreateWithFlags(&l.ev, hipEventDisableTiming) == hipSuccess && hb_scan_log_room(where, h, (int)initial_scans) == 0;
    if (!ok) {  // all or nothing
        hb_scan_log_free(h);
        return set_err(where, "allocation failed");
    }
    l.n.assign((size_t)h->S, -1);
    l.on = true;
    return 0;
}

// :1456 + :1480-1486 for all slots of the step.  The pinned table is rewritten only by a call that launches, which an append with
// points precedes -- and that append has waited for the handle's stream, so the previous call's copy out of the table is over.
extern "C" int ll_history_batch_log_full_fe(ll_history_batch *h, ll_fe *fe, const int32_t *active)
{
    static const char *where = "ll_history_batch_log_full_fe";
    if (!h || !fe) return set_err(where, "null argument");
    HbScanLog &l = h->sl;
    if (!l.on) return set_err(where, "the scan log is not enabled (ll_history_batch_enable_scan_log)");
    if (!l.pending) return set_err(where, "no ll_history_batch_append_full_fe to log (one log call per append)");
    if (fe != l.fe) return set_err(where, "not the extractor of the append");
    const int S = h->S;
    auto named = [&](int s) { return l.n[(size_t)s] >= 0 && (!active || active[s]); };
    int want = 0, max_n = 0;
    for (int s = 0; s < S; s++)
        if (named(s)) want++, max_n = std::max(max_n, l.n[(size_t)s]);
    HC(hipSetDevice(h->device));
    if (hb_scan_log_room(where, h, want)) return -1;
    // ---- nothing refuses below
    l.pending = false;
    std::vector<int> block((size_t)S, -1);
    for (int s = 0; s < S; s++)
        if (named(s)) block[(size_t)s] = sl_take(l.book);
    int enq = 0;
    hipError_t e = hipSuccess;
    const char *err = nullptr;
    if (max_n > 0) {
        for (int s = 0; s < S; s++) l.hp_tab[s] = SlSlot{named(s) ? hb_scan_log_block(h, block[(size_t)s]) : nullptr, named(s) ? l.n[(size_t)s] : 0, 0};
        e = hipMemcpyAsync(l.d_tab, l.hp_tab, (size_t)S * sizeof(SlSlot), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess && sl_log(l.d_tab, h->fm.xf, h->max_pts, fe->dev.xyzi, fe->dev.full_idx, fe->dev.stride, S, max_n, h->stream, &err)) e = hipErrorUnknown;
        // the next upload into the extractor must not replace a scan this launch still reads
        if (e == hipSuccess) e = hipEventRecord(l.ev, h->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(fe->stream, l.ev, 0);
        enq = 4;
    }
    if (e != hipSuccess) {  // the blocks go back; the FIFOs are as they were
        for (int s = 0; s < S; s++)
            if (block[(size_t)s] >= 0) sl_release(l.book, block[(size_t)s]);
        return set_err(where, err ? err : hipGetErrorString(e));
    }
    for (int s = 0; s < S; s++) {
        if (l.n[(size_t)s] < 0) continue;  // (not in the append: the node did not reach :1456 for it)
        if (named(s)) sl_push(l.book, s, block[(size_t)s], l.n[(size_t)s]);
        sl_trim(l.book, s);
    }
    l.work[0] = enq;
    l.work[1] = 0;
    return 0;
}

extern "C" int ll_history_batch_scan_log_hand_over(ll_history_batch *h, int32_t sequence, int64_t *group_id)
{
    static const char *where = "ll_history_batch_scan_log_hand_over";
    if (!h || !group_id) return set_err(where, "null argument");
    if (!h->sl.on) return set_err(where, "the scan log is not enabled (ll_history_batch_enable_scan_log)");
    if (sequence < 0 || sequence >= h->S) return set_err(where, "sequence out of range");
    *group_id = sl_hand_over(h->sl.book, sequence);
    return 0;
}

extern "C" int ll_history_batch_scan_log_drop(ll_history_batch *h, int64_t n, const int64_t *group_ids)
{
    static const char *where = "ll_history_batch_scan_log_drop";
    if (!h || (n > 0 && !group_ids)) return set_err(where, "null argument");
    if (!h->sl.on) return set_err(where, "the scan log is not enabled (ll_history_batch_enable_scan_log)");
    if (n < 0) return set_err(where, "negative count");
    const std::string why = sl_check_groups(h->sl.book, n, group_ids);
    if (!why.empty()) return set_err(where, why.c_str());
    for (int64_t i = 0; i < n; i++) sl_drop(h->sl.book, group_ids[i]);
    return 0;
}

extern "C" int ll_history_batch_scan_log_read(ll_history_batch *h, int64_t group_id, float *xyzi, int64_t capacity_points, int64_t *n)
{
    static const char *where = "ll_history_batch_scan_log_read";
    if (!h || !n) return set_err(where, "null argument");
    if (!h->sl.on) return set_err(where, "the scan log is not enabled (ll_history_batch_enable_scan_log)");
    const std::vector<SlScan> *g = sl_group(h->sl.book, group_id);
    if (!g) return set_err(where, "unknown or consumed group");
    int64_t total = 0;
    for (const SlScan &e : *g) total += e.n;
    *n = total;
    if (!xyzi) return 0;  // (the size alone)
    if (capacity_points < total) return set_err(where, "buffer too small");
    HC(hipSetDevice(h->device));
    int64_t at = 0;
    for (const SlScan &e : *g) {
        if (e.n > 0) HC(hipMemcpyAsync(xyzi + 4 * at, hb_scan_log_block(h, e.block), (size_t)e.n * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
        at += e.n;
    }
    HC(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int ll_history_batch_scan_log_work(ll_history_batch *h, int64_t out[4])
{
    static const char *where = "ll_history_batch_scan_log_work";
    if (!h || !out) return set_err(where, "null argument");
    if (!h->sl.on) return set_err(where, "the scan log is not enabled (ll_history_batch_enable_scan_log)");
    out[0] = h->sl.work[0];
    out[1] = h->sl.work[1];
    out[2] = h->sl.book.in_use;
    out[3] = h->sl.book.n_blocks;
    return 0;
}
