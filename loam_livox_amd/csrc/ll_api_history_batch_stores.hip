// ll_api_history_batch_stores.hip -- the deferred stores of the batched match buffer: the two cell maps of every slot, fed by every
// add (ll_cellmap_batch_kernels.hip), and the full-cloud map of every slot, fed by ll_history_batch_append_full_fe
// (ll_fullmap_batch_kernels.hip).  What the three have in common is written once, for an HbStore.
#include "ll_api_history_batch_internal.h"

// ================================================================================================ one store
void hb_store_free(HbStore &st)
{
    CbDev &m = st.dev;
    (void)(cb_each_log(m, 0, hb_free) || cb_each_table(m, 0, hb_free) || cb_each_append(m, 0, hb_free) || cb_each_mat(m, 0, hb_free) || cb_each_fixed(m, hb_free));
    if (m.tmp) (void)hipFree(m.tmp);
    memset(&m, 0, sizeof(m));
    if (st.hp_tab) (void)hipHostFree(st.hp_tab);
    if (st.hp_n) (void)hipHostFree(st.hp_n);
    st.hp_tab = nullptr;
    st.hp_n = st.hp_coff = st.hp_poff = st.hp_counts = nullptr;
}

// Room for `need` entries of the log, or of the cell table: twice the capacity when they would not fit -- for the log the only time
// stored points are copied outside a materialisation.  A capacity is raised only after every array of its group has moved, so a
// failure leaves the store consistent.
int hb_cells_reserve_log(ll_history_batch *h, CbDev &m, long long need)
{
    if (need <= (long long)m.cap) return 0;
    const long long twice = 2LL * (long long)m.cap, want = twice < need ? need : twice;
    const size_t n = (size_t)(want < kCbLimit ? want : kCbLimit);
    if (cb_each_log(m, n, hb_mover(h, (size_t)m.n_log))) return -1;
    m.cap = n;
    return 0;
}

static int hb_cells_reserve_table(ll_history_batch *h, CbDev &m, long long need)
{
    if (need <= (long long)m.ccap) return 0;
    const long long twice = 2LL * (long long)m.ccap;
    const size_t n = (size_t)(twice < need ? need : twice);
    if (cb_each_table(m, n, hb_mover(h, (size_t)m.n_cells))) return -1;
    HC(hipMemset(m.cstart, 0, (n + (size_t)m.S + 1) * sizeof(int)));  // (rebuilt by the next materialisation)
    HC(hipDeviceSynchronize());
    m.ccap = n;
    return 0;
}

int hb_cells_reserve_mat(ll_history_batch *h, CbDev &m, size_t n)
{
    if (cb_each_mat(m, n, hb_mover(h, 0))) return -1;
    m.mcap = n;
    return 0;
}

// An enabled, empty store: laser_mapping.hpp:616-624, every map has m_pt_cell_resolution and m_minimum_revisit_threshold.  The
// caller waits for the device afterwards (null-stream memsets are not ordered with the handle's non-blocking stream).
static int hb_store_setup(ll_history_batch *h, HbStore &st, int64_t initial_points_per_map, float cell_resolution, int32_t threshold)
{
    const size_t S = (size_t)h->S;
    HC(hipHostMalloc((void **)&st.hp_tab, S * sizeof(CbSlot), hipHostMallocDefault));
    HC(hipHostMalloc((void **)&st.hp_n, (S + 2 * (S + 1) + 4) * sizeof(int), hipHostMallocDefault));
    st.hp_coff = st.hp_n + S;
    st.hp_poff = st.hp_coff + S + 1;
    st.hp_counts = st.hp_poff + S + 1;
    CbDev &m = st.dev;
    m.S = h->S;
    m.geom = cell_geom(cell_resolution);
    m.threshold = threshold;
    if (cb_each_fixed(m, [](auto *&p, size_t n, bool) { return dmalloc(&p, n); })) return -1;
    HC(hipMemset(m.coff, 0, (S + 1) * sizeof(int)));
    HC(hipMemset(m.poff, 0, (S + 1) * sizeof(int)));
    HC(hipMemset(m.counts, 0, 4 * sizeof(int)));
    if (hb_cells_reserve_log(h, m, (long long)(S * (size_t)initial_points_per_map)) || hb_cells_reserve_table(h, m, (long long)h->max_pts)) return -1;
    st.frame.assign(S, 0);
    st.coff.assign(S + 1, 0);
    st.poff.assign(S + 1, 0);
    st.res = cell_resolution;
    return 0;
}

// room for an append of n_new points whose merge leaves at most table_need cells (the stream is idle)
static int hb_store_reserve(ll_history_batch *h, CbDev &m, long long n_new, long long table_need)
{
    if (hb_cells_reserve_log(h, m, m.n_log + n_new) || hb_cells_reserve_table(h, m, table_need) ||
        hb_reserve_tmp("ll_history_batch (cell maps)", h, m.tmp, m.tmp_bytes, cb_tmp_bytes, n_new))
        return -1;
    if ((long long)m.acap < n_new) {
        const size_t n = (size_t)(n_new + n_new / 2);
        if (cb_each_append(m, n, hb_mover(h, 0))) return -1;
        m.acap = n;
    }
    return 0;
}

// put the stores of the kinds k0 .. k1 - 1 in order: one chain per store, one wait for all
static int hb_stores_materialise(const char *where, ll_history_batch *h, int k0, int k1)
{
    const int S = h->S;
    HC(hipSetDevice(h->device));
    for (int k = k0; k < k1; k++) {
        CbDev &m = h->st[k].dev;
        if (m.n_log <= 0) continue;
        if (hb_reserve_tmp("ll_history_batch (cell maps)", h, m.tmp, m.tmp_bytes, cb_tmp_bytes, m.n_log)) return -1;
        if ((long long)m.mcap < m.n_log && hb_cells_reserve_mat(h, m, m.cap)) return -1;  // (the log's capacity: grows as rarely as the log does)
    }
    int launches = 0;
    const char *err = nullptr;
    for (int k = k0; k < k1; k++) {
        if (cb_materialise(h->st[k].dev, h->stream, &launches, &err)) return set_err(where, err);
        HC(hipMemcpyAsync(h->st[k].hp_poff, h->st[k].dev.poff, (size_t)(S + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HC(hipStreamSynchronize(h->stream));
    for (int k = k0; k < k1; k++) {
        HbStore &st = h->st[k];
        st.poff.assign(st.hp_poff, st.hp_poff + S + 1);
        st.dev.n_log = st.poff[S];  // the ordered store replaces the log: later adds write behind it
    }
    return 0;
}

// put the stores of both feature kinds in order (a read after an add); nothing to do when no add came since the last time
int hb_cells_materialise(const char *where, ll_history_batch *h)
{
    if (!h->cm_dirty) return 0;
    if (hb_stores_materialise(where, h, 0, 2)) return -1;
    h->cm_dirty = false;
    h->cm_work[2]++;
    return 0;
}

// the same for the full-cloud store alone: a read of kind 2 never orders the feature stores, and the other way round
static int hb_full_materialise(const char *where, ll_history_batch *h)
{
    if (!h->fm_dirty) return 0;
    if (hb_stores_materialise(where, h, 2, 3)) return -1;
    h->fm_dirty = false;
    h->fm_work[3]++;
    return 0;
}

// ================================================================================================ the cell maps of the slots
// The cell-map part of an add: the filtered frames of the working slots (h->vf[k].out, their sizes in st[k].hp_n) behind the logs of
// the two kinds.  One chain per kind, one wait for both.  (Room is made kind by kind: the corner store may have grown when the
// surface store's 2^31 check refuses, which history_batch_add_common has already ruled out for both.)
int hb_cells_append(const char *where, ll_history_batch *h)
{
    const int S = h->S;
    long long n_new[2] = {0, 0};
    int max_n[2] = {0, 0}, launches = 0;
    for (int k = 0; k < 2; k++) {
        HbStore &st = h->st[k];
        auto n_of = [&](int s) {
            const int n = st.hp_n[s];
            return !h->hp_add[s].work ? -1 : (n < 0 ? 0 : (n < h->max_pts ? n : h->max_pts));
        };
        CbDev &m = st.dev;
        n_new[k] = cb_fill_slots(st.hp_tab, S, n_of, st.frame.data(), m.n_log, &max_n[k]);
        if (n_new[k] == 0) continue;
        if (m.n_log + n_new[k] >= kCbLimit) return set_err(where, "the cell maps would pass 2^31 stored points per kind");
        if (hb_store_reserve(h, m, n_new[k], (long long)m.n_cells + n_new[k])) return -1;
    }
    const char *err = nullptr;
    for (int k = 0; k < 2; k++) {
        HbStore &st = h->st[k];
        if (n_new[k] == 0) continue;
        HC(hipMemcpyAsync(st.dev.tab, st.hp_tab, (size_t)S * sizeof(CbSlot), hipMemcpyHostToDevice, h->stream));
        if (cb_append(st.dev, h->vf[k].out, h->max_pts, max_n[k], n_new[k], h->stream, &launches, &err)) return set_err(where, err);
        HC(hipMemcpyAsync(st.hp_counts, st.dev.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HC(hipMemcpyAsync(st.hp_coff, st.dev.coff, (size_t)(S + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HC(hipStreamSynchronize(h->stream));
    for (int k = 0; k < 2; k++) {
        HbStore &st = h->st[k];  // (the frame counters step; the mirrors take what the chain left)
        cb_after_append(st.frame.data(), st.coff.data(), S, [&](int s) { return h->hp_add[s].work != 0; }, n_new[k] ? st.hp_coff : nullptr);
        if (n_new[k]) st.dev.n_cells = st.hp_counts[1];
        h->cm_work[0] += n_new[k];
        h->cm_work[1] += n_new[k];  // (the candidates' keys: two sorts over the new points, nothing else is sorted or gathered here)
    }
    h->cm_work[3] = launches;
    h->cm_dirty = true;
    return 0;
}

// what every reader checks first; 0 with the stores in order
int hb_cells_reader(const char *where, ll_history_batch *h, int32_t sequence, int32_t kind)
{
    if (!h) return set_err(where, "null argument");
    if (kind == 2 && h->fm_on) {  // the full-cloud store, on its own
        if (sequence < 0 || sequence >= h->S) return set_err(where, "sequence out of range");
        return hb_full_materialise(where, h);
    }
    if (!h->cm_on) return set_err(where, "cell maps are not enabled (ll_history_batch_enable_cell_maps)");
    if (sequence < 0 || sequence >= h->S) return set_err(where, "sequence out of range");
    if (kind < 0 || kind > 1) return set_err(where, "kind out of range");
    return hb_cells_materialise(where, h);
}

extern "C" int ll_history_batch_sync_cell_maps(ll_history_batch *h)
{
    static const char *where = "ll_history_batch_sync_cell_maps";
    if (h && h->fm_on) {  // whatever is enabled
        if (h->cm_on && hb_cells_materialise(where, h)) return -1;
        return hb_full_materialise(where, h);
    }
    return hb_cells_reader(where, h, 0, 0);
}

extern "C" int ll_history_batch_cell_map_stats(ll_history_batch *h, int32_t sequence, int32_t kind, int64_t *n_cells, int64_t *n_points,
                                               int32_t *frame_idx)
{
    if (hb_cells_reader("ll_history_batch_cell_map_stats", h, sequence, kind)) return -1;
    const HbStore &st = h->st[kind];
    if (n_cells) *n_cells = st.coff[sequence + 1] - st.coff[sequence];
    if (n_points) *n_points = st.poff[sequence + 1] - st.poff[sequence];
    if (frame_idx) *frame_idx = st.frame[sequence];
    return 0;
}

extern "C" int ll_history_batch_cell_map_dump(ll_history_batch *h, int32_t sequence, int32_t kind, float *xyzi, int64_t capacity_points,
                                              int32_t *cell_ijk, int32_t *cell_start, int32_t *cell_last_update, int64_t capacity_cells)
{
    static const char *where = "ll_history_batch_cell_map_dump";
    if (!h) return set_err(where, "null argument");
    auto too_small = [&](const HbStore &st) {
        const int np = st.poff[sequence + 1] - st.poff[sequence], nc = st.coff[sequence + 1] - st.coff[sequence];
        return (xyzi && capacity_points < np) || ((cell_ijk || cell_start || cell_last_update) && capacity_cells < nc);
    };
    // (sizes known: refuse short buffers before any work)
    if (sequence >= 0 && sequence < h->S && ((kind == 2 && h->fm_on && !h->fm_dirty) || (h->cm_on && kind >= 0 && kind <= 1 && !h->cm_dirty)) &&
        too_small(h->st[kind]))
        return set_err(where, "buffer too small");
    if (hb_cells_reader(where, h, sequence, kind)) return -1;
    const HbStore &st = h->st[kind];
    const CbDev &m = st.dev;
    const int p0 = st.poff[sequence], c0 = st.coff[sequence];
    const int np = st.poff[sequence + 1] - p0, nc = st.coff[sequence + 1] - c0;
    if (too_small(st)) return set_err(where, "buffer too small");
    if (xyzi && np > 0) HC(hipMemcpy(xyzi, m.pts + p0, (size_t)np * sizeof(float4), hipMemcpyDeviceToHost));
    if (cell_start) {
        if (nc > 0)
            HC(hipMemcpy(cell_start, m.cstart + c0 + sequence, (size_t)(nc + 1) * sizeof(int), hipMemcpyDeviceToHost));
        else
            cell_start[0] = 0;
    }
    if (cell_last_update && nc > 0) HC(hipMemcpy(cell_last_update, m.clast + c0, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost));
    if (cell_ijk && nc > 0) {
        std::vector<unsigned long long> keys(nc);
        HC(hipMemcpy(keys.data(), m.ckey + c0, (size_t)nc * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int i = 0; i < nc; i++) cell_unpack(keys[i], cell_ijk + 3 * (size_t)i);
    }
    return 0;
}

// One slot's map where it lies, in the layout of ll_cellmap_device_view.  Valid until the next add on this handle (which writes behind
// the store and may move it); the handle's stream has been drained.
extern "C" int ll_history_batch_cell_map_device_view(ll_history_batch *h, int32_t sequence, int32_t kind, const float **dev_xyz0,
                                                     const uint64_t **dev_point_keys, int64_t *n_points, int64_t *n_cells)
{
    static const char *where = "ll_history_batch_cell_map_device_view";
    if (!h || !dev_xyz0 || !dev_point_keys || !n_points) return set_err(where, "null argument");
    if (hb_cells_reader(where, h, sequence, kind)) return -1;
    const HbStore &st = h->st[kind];
    const int p0 = st.poff[sequence];
    *dev_xyz0 = (const float *)(st.dev.pts + p0);
    *dev_point_keys = (const uint64_t *)(st.dev.pkey + p0);
    *n_points = st.poff[sequence + 1] - p0;
    if (n_cells) *n_cells = st.coff[sequence + 1] - st.coff[sequence];
    return 0;
}

extern "C" int ll_history_batch_cell_map_work(ll_history_batch *h, int64_t out[4])
{
    static const char *where = "ll_history_batch_cell_map_work";
    if (!h || !out) return set_err(where, "null argument");
    if (!h->cm_on) return set_err(where, "cell maps are not enabled (ll_history_batch_enable_cell_maps)");
    for (int i = 0; i < 4; i++) out[i] = h->cm_work[i];
    return 0;
}

// ================================================================================================ the full-cloud maps of the slots
void hb_full_free(ll_history_batch *h)
{
    FbDev &t = h->fm;
    void *ptrs[] = {t.xf, t.tab, t.cnt, t.flag, t.rank, t.cells, t.toff, t.tmp};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    memset(&t, 0, sizeof(t));
    hb_store_free(h->st[2]);
    void *host[] = {h->hp_fb_tab, h->hp_fm_toff, h->hp_fm_cells};
    for (void *p : host)
        if (p) (void)hipHostFree(p);
    h->hp_fb_tab = nullptr;
    h->hp_fm_toff = nullptr;
    h->hp_fm_cells = nullptr;
    h->fm_cells_cap = 0;
}

// the stores of one enable call: both feature stores, or the full-cloud store with what its appends need on top
static int hb_enable_impl(ll_history_batch *h, bool full, int64_t initial_points_per_map, float cell_resolution, int32_t threshold)
{
    const size_t S = (size_t)h->S;
    for (int k = full ? 2 : 0; k < (full ? 3 : 2); k++)
        if (hb_store_setup(h, h->st[k], initial_points_per_map, cell_resolution, threshold)) return -1;
    if (full) {
        HC(hipHostMalloc((void **)&h->hp_fb_tab, S * sizeof(FbSlot), hipHostMallocDefault));
        HC(hipHostMalloc((void **)&h->hp_fm_toff, (S + 1) * sizeof(int), hipHostMallocDefault));
        h->fm_cells_cap = 4096;
        HC(hipHostMalloc((void **)&h->hp_fm_cells, h->fm_cells_cap * 3 * sizeof(int), hipHostMallocDefault));
        DM(h->fm.xf, S * (size_t)h->max_pts);
        DM(h->fm.tab, S);
        DM(h->fm.toff, S + 1);
        HC(hipMemset(h->fm.toff, 0, (S + 1) * sizeof(int)));
        h->fm_touched.assign(S, std::vector<int32_t>());
    }
    HC(hipDeviceSynchronize());  // (null-stream memsets are not ordered with the handle's non-blocking stream)
    return 0;
}

// the checks and the all-or-nothing frame of both enable calls; full: the full-cloud store, else the two feature stores
static int hb_enable(const char *where, ll_history_batch *h, bool full, int64_t initial_points_per_map, float cell_resolution, int32_t threshold)
{
    if (!h) return set_err(where, "null argument");
    if (full ? h->fm_on : h->cm_on) return set_err(where, "already enabled");
    if (!(cell_resolution > 0.f)) return set_err(where, "cell_resolution must be positive");
    if (initial_points_per_map < h->max_pts) return set_err(where, "initial_points_per_map below max_points_per_frame");
    if ((double)initial_points_per_map * (double)h->S >= 2147483647.0)
        return set_err(where, full ? "n_sequences * initial_points_per_map must stay below 2^31 stored points"
                                   : "n_sequences * initial_points_per_map must stay below 2^31 stored points per kind");
    HC(hipSetDevice(h->device));
    HC(hipStreamSynchronize(h->stream));
    if (hb_enable_impl(h, full, initial_points_per_map, cell_resolution, threshold)) {  // all or nothing
        const std::string keep = g_err;
        if (full) hb_full_free(h);
        for (int k = 0; !full && k < 2; k++) hb_store_free(h->st[k]);
        g_err = keep;
        return -1;
    }
    (full ? h->fm_on : h->cm_on) = true;
    return 0;
}

extern "C" int ll_history_batch_enable_cell_maps(ll_history_batch *h, int64_t initial_points_per_map, float cell_resolution,
                                                 int32_t threshold_cell_revisit)
{
    return hb_enable("ll_history_batch_enable_cell_maps", h, false, initial_points_per_map, cell_resolution, threshold_cell_revisit);
}

extern "C" int ll_history_batch_enable_full_maps(ll_history_batch *h, int64_t initial_points_per_map, float cell_resolution,
                                                 int32_t threshold_cell_revisit)
{
    return hb_enable("ll_history_batch_enable_full_maps", h, true, initial_points_per_map, cell_resolution, threshold_cell_revisit);
}

// the scratch of the touched chain follows the cell table's capacity (the stream is idle)
static int hb_full_reserve_scratch(ll_history_batch *h, long long n_upper)
{
    FbDev &t = h->fm;
    const size_t want = h->st[2].dev.ccap;
    if (t.tcap < want) {
        if (hb_cells_move(h, &t.cnt, want, 0) || hb_cells_move(h, &t.flag, want, 0) || hb_cells_move(h, &t.rank, want, 0) ||
            hb_cells_move(h, &t.cells, 3 * want, 0))
            return -1;
        t.tcap = want;
    }
    return hb_reserve_tmp("ll_history_batch_append_full_fe", h, t.tmp, t.tmp_bytes, fb_tmp_bytes, n_upper);
}

// laser_mapping.hpp:1442 + 1527 for all active slots: the scan's full cloud (the extractor's full selection) into the map frame with
// the slot's pose and behind the full-cloud store, and per slot the cells the scan touched.  One gather, the append chain of
// ll_cellmap_batch_kernels.hip, the touched chain; the host waits for the selection sizes, for the tables of the append, and for
// the touched cells themselves.  A growth of the store waits on top, as it does for the feature stores.
extern "C" int ll_history_batch_append_full_fe(ll_history_batch *h, ll_fe *fe, const int32_t *active, const double *poses7, int32_t min_points,
                                               int64_t *n_touched)
{
    static const char *where = "ll_history_batch_append_full_fe";
    if (!h || !fe || !poses7 || !n_touched) return set_err(where, "null argument");
    if (!h->fm_on) return set_err(where, "full maps are not enabled (ll_history_batch_enable_full_maps)");
    if (fe->prm.device != h->device) return set_err(where, "extractor lives on another device");
    if (fe->prm.max_scans < h->S) return set_err(where, "the extractor holds fewer scans than n_sequences");
    if (min_points < 1) return set_err(where, "min_points must be at least 1");
    const int S = h->S;
    HbStore &st = h->st[2];
    CbDev &m = st.dev;
    FbDev &t = h->fm;
    HC(hipSetDevice(h->device));
    int enq = 0, waits = 0;
    int *in_n = st.hp_n, *h_toff = h->hp_fm_toff;
    HC(hipMemcpyAsync(in_n, fe->dev.n_full, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, fe->stream));  // (behind the selection)
    HC(hipStreamSynchronize(fe->stream));
    enq++;
    waits++;
    // ---- the checks: nothing is enqueued on the handle's stream and nothing of the store is changed before they have passed (the
    // pinned tables of the call are scratch: filled between the checks, rewritten by every call)
    auto on = [&](int s) { return !active || active[s]; };
    for (int s = 0; s < S; s++)
        if (on(s) && (in_n[s] > h->max_pts || in_n[s] > fe->dev.stride)) return set_err(where, "full selection exceeds max_points_per_frame");
    int max_n = 0;
    const long long n_new = fb_fill_slots(st.hp_tab, h->hp_fb_tab, S, [&](int s) { return !on(s) ? -1 : (in_n[s] > 0 ? in_n[s] : 0); }, st.frame.data(),
                                          st.coff.data(), min_points, poses7, m.n_log, &max_n);
    if (m.n_log + n_new >= kCbLimit) return set_err(where, "the full maps would pass 2^31 stored points");
    const long long n_upper = (long long)m.n_cells + n_new;  // bound of the cell table after the merge
    if (n_upper >= kCbLimit) return set_err(where, "the full maps would pass 2^31 cells");
    if (n_new > 0 && (hb_store_reserve(h, m, n_new, n_upper) || hb_full_reserve_scratch(h, n_upper))) return -1;
    int total = 0;
    if (n_new > 0) {
        const char *err = nullptr;
        HC(hipMemcpyAsync(m.tab, st.hp_tab, (size_t)S * sizeof(CbSlot), hipMemcpyHostToDevice, h->stream));
        HC(hipMemcpyAsync(t.tab, h->hp_fb_tab, (size_t)S * sizeof(FbSlot), hipMemcpyHostToDevice, h->stream));
        enq += 2;
        if (fb_gather(t, fe->dev.xyzi, fe->dev.full_idx, fe->dev.stride, S, h->max_pts, max_n, h->stream, &enq, &err)) return set_err(where, err);
        if (cb_append(m, t.xf, h->max_pts, max_n, n_new, h->stream, &enq, &err)) return set_err(where, err);
        if (fb_touched_chain(m, t, max_n, (int)n_upper, h->stream, &enq, &err)) return set_err(where, err);
        HC(hipMemcpyAsync(st.hp_counts, st.dev.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HC(hipMemcpyAsync(st.hp_coff, st.dev.coff, (size_t)(S + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HC(hipMemcpyAsync(h_toff, t.toff, (size_t)(S + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        enq += 3;
        HC(hipStreamSynchronize(h->stream));
        waits++;
        total = h_toff[S];
        if (total < 0 || total > st.hp_counts[1] || st.hp_counts[1] > n_upper) return set_err(where, "touched-cell counts out of range");
        if ((size_t)total > h->fm_cells_cap) {  // (the stream is idle)
            const size_t want = (size_t)total + (size_t)total / 2;
            int *p = nullptr;
            HC(hipHostMalloc((void **)&p, want * 3 * sizeof(int), hipHostMallocDefault));
            (void)hipHostFree(h->hp_fm_cells);
            h->hp_fm_cells = p;
            h->fm_cells_cap = want;
        }
        // the lists themselves; the copy and its wait are there for every call that appended, so that their number does not depend on the data
        HC(hipMemcpyAsync(h->hp_fm_cells, t.cells, (size_t)(total > 0 ? total : 1) * 3 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        enq++;
        HC(hipStreamSynchronize(h->stream));
        waits++;
    }
    cb_after_append(st.frame.data(), st.coff.data(), S, on, n_new > 0 ? st.hp_coff : nullptr);  // (an inactive slot keeps its map, its counter and its list)
    if (n_new > 0) m.n_cells = st.hp_counts[1];
    for (int s = 0; s < S; s++) {
        std::vector<int32_t> &list = h->fm_touched[s];
        if (on(s)) list.clear();
        if (on(s) && n_new > 0) list.assign(h->hp_fm_cells + 3 * (size_t)h_toff[s], h->hp_fm_cells + 3 * (size_t)h_toff[s + 1]);
        n_touched[s] = (int64_t)(list.size() / 3);
    }
    if (n_new > 0) h->fm_dirty = true;
    if (h->sl.on) {  // what ll_history_batch_log_full_fe logs: this call's slots and sizes, out of t.xf as it stands now
        for (int s = 0; s < S; s++) h->sl.n[(size_t)s] = !on(s) ? -1 : (in_n[s] > 0 ? in_n[s] : 0);
        h->sl.fe = fe;
        h->sl.pending = true;
    }
    h->fm_work[0] = enq;
    h->fm_work[1] = waits;
    return 0;
}

extern "C" int ll_history_batch_full_touched(ll_history_batch *h, int32_t sequence, int32_t *cell_ijk, int64_t capacity_cells, int64_t *n)
{
    static const char *where = "ll_history_batch_full_touched";
    if (!h || !n) return set_err(where, "null argument");
    if (!h->fm_on) return set_err(where, "full maps are not enabled (ll_history_batch_enable_full_maps)");
    if (sequence < 0 || sequence >= h->S) return set_err(where, "sequence out of range");
    const std::vector<int32_t> &list = h->fm_touched[sequence];
    *n = (int64_t)(list.size() / 3);
    if (!cell_ijk) return 0;
    if (capacity_cells < *n) return set_err(where, "buffer too small");
    if (!list.empty()) memcpy(cell_ijk, list.data(), list.size() * sizeof(int32_t));
    return 0;
}

// test tap of the full-cloud maps (out[] as loam_livox_hip.h describes it)
extern "C" int ll_history_batch_full_map_work(ll_history_batch *h, int64_t out[4])
{
    static const char *where = "ll_history_batch_full_map_work";
    if (!h || !out) return set_err(where, "null argument");
    if (!h->fm_on) return set_err(where, "full maps are not enabled (ll_history_batch_enable_full_maps)");
    for (int i = 0; i < 4; i++) out[i] = h->fm_work[i];
    return 0;
}
