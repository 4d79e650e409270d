// ll_api_history_batch.hip -- the batched match buffer of the C ABI.
// One handle for the histories of S sequences (ll_history_batch_*).  Per slot the semantics are ll_history's; the device work of an
// add and of a refresh is one fixed chain of launches over all slots (ll_history_batch_kernels.hip), and the search grids of one
// refresh live in ONE pooled pair of buffers, an arena.  Every MapSnap built in an arena holds a reference to it, so the immutable
// snapshot contract of ll_map carries over: an arena is taken for the next refresh only when nothing but the handle's pool refers
// to it -- no snapshot built in it is published by a map or pinned by a registration any more.
//
// The handle can keep the two cell maps of every slot as well (ll_history_batch_enable_cell_maps): every active slot of an add
// appends its filtered frame to them, through one more fixed chain whose work is that of the new points and the cell tables
// (ll_cellmap_batch_kernels.hip); the stored points are put in order when somebody reads.
//
// Independently of those it can keep the full-cloud map of every slot (ll_history_batch_enable_full_maps): a third store of the same
// kind, fed by ll_history_batch_append_full_fe with the extractor's full selections and reporting the cells each scan touched
// (ll_fullmap_batch_kernels.hip).  Nothing of an add or of a refresh reads it.
//
// Chosen cells of any of the three stores leave it on the device, for several slots in one call (ll_history_batch_extract_cells,
// ll_cellmap_batch_extract_kernels.hip): the key frames the sequences close in the same step, each into a cell map of its own.
#include "ll_api_internal.h"
#include "ll_cellmatch_batch.h"
#include "ll_fullmap_batch.h"

struct HbArena {
    int device = 0;
    f4 *pts = nullptr;
    int *cells = nullptr;
    size_t cap_pts = 0, cap_cells = 0;
    ~HbArena()
    {
        (void)hipSetDevice(device);
        if (pts) (void)hipFree(pts);
        if (cells) (void)hipFree(cells);
    }
};

struct ll_history_batch {
    int device = 0, S = 0, max_hist = 0, max_pts = 0, slots = 0;
    size_t cstride = 0;  // points per slot of the concatenation / match-buffer buffers: maximum_history_size * max_points_per_frame
    float res[2] = {0.1f, 0.4f};
    hipStream_t stream = nullptr;
    float4 *frames[2] = {nullptr, nullptr};  // [S][max_hist + 1][max_pts] rings per kind
    float4 *d_xf = nullptr;                  // [2][S][max_pts] the frames in the map frame
    int *d_nxf = nullptr;                    // [2][S]
    float4 *d_concat = nullptr, *d_map = nullptr;  // [2][S][cstride] concatenations / filtered match buffers of the last refresh
    VoxelDev vf[2]{}, vm[2]{};               // VoxelGrid of the frames / of the concatenations, per kind
    std::vector<int> count[2];               // [S][slots] points per ring slot
    std::vector<int> head, size;             // [S] FIFO windows
    std::vector<double> last_q, last_t;      // [S][4], [S][3] m_last_his_add_q / m_last_his_add_t
    std::vector<int64_t> n_map[2];           // [S]
    // tables: pinned host copies and their device mirrors
    HbAddSlot *hp_add = nullptr, *d_add = nullptr;  // [S]
    int *hp_cnt = nullptr, *d_cnt = nullptr;        // host [4 S]: input counts [2][S], filtered counts [2][S]; device [2][S] filtered counts
    char *hp_ref = nullptr, *d_ref = nullptr;       // refresh: int active[S], int n_concat[2][S], (16-byte aligned) HbSeg segs[2 S max_hist]
    size_t ref_seg_off = 0, ref_bytes = 0;
    unsigned int *hp_mm_init = nullptr, *hp_mm = nullptr, *d_mm = nullptr;  // [2 S][8]
    HbGrid *hp_grid = nullptr, *d_grid = nullptr;   // [2 S]
    int *hp_nvalid = nullptr, *d_nvalid = nullptr;  // [2 S]
    // scratch of the grid build, grown geometrically
    unsigned long long *keys = nullptr, *keys2 = nullptr;
    int *vals = nullptr, *vals2 = nullptr, *counts = nullptr;
    char *tmp = nullptr;
    size_t cap_n = 0, cap_cells = 0, cap_tmp = 0;
    std::vector<std::shared_ptr<HbArena>> arenas;
    // the cell maps of all slots, one deferred store per kind (ll_history_batch_enable_cell_maps)
    bool cm_on = false, cm_dirty = false;    // dirty: an add came after the last materialisation
    CbDev cm[3]{};                           // corner, surface; [2]: the full-cloud store (ll_history_batch_enable_full_maps)
    std::vector<int> cm_frame[3];            // [S] m_current_frame_idx of every map
    std::vector<int> cm_coff[3], cm_poff[3]; // [S + 1] host copies: first cell / first stored point of every slot
    CbSlot *hp_cm_tab = nullptr;             // pinned [2][S]
    int *hp_cm = nullptr;                    // pinned: filtered counts [2][S], coff [2][S + 1], poff [2][S + 1], counts [2][4]
    int64_t cm_work[4] = {0, 0, 0, 0};       // ll_history_batch_cell_map_work
    // the cell-mode refresh (ll_history_batch_refresh_cells): scratch per kind, the slots' poses, the drained counts
    CmbDev cq[2]{};
    CmbSlot *hp_cq_tab = nullptr, *d_cq_tab = nullptr;  // [S]
    int *hp_cq = nullptr;                    // pinned [2][S + 4]: first leaf of every slot, leaves, candidates, live entries
    int64_t cq_work[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // ll_history_batch_cell_match_work
    // the full-cloud maps of all slots: cm[2] and what an append needs on top of it (ll_history_batch_enable_full_maps)
    bool fm_on = false, fm_dirty = false;
    FbDev fm{};
    CbSlot *hp_fm_tab = nullptr;             // pinned [S]
    FbSlot *hp_fb_tab = nullptr;             // pinned [S]
    int *hp_fm = nullptr;                    // pinned: full-selection sizes [S], coff [S + 1], poff [S + 1], counts [4], toff [S + 1]
    int *hp_fm_cells = nullptr;              // pinned [fm_cells_cap][3]: the touched cells of the last append on their way to the lists
    size_t fm_cells_cap = 0;
    std::vector<std::vector<int32_t>> fm_touched;  // [S] the {i, j, k} of the cells the slot's last appended scan touched
    int64_t fm_work[4] = {0, 0, 0, 0};       // ll_history_batch_full_map_work
    // cells of several slots into cell maps (ll_history_batch_extract_cells): the staged requests and lists, the totals, the destinations
    float cm_res[3] = {0.f, 0.f, 0.f};       // the cell resolution every kind was enabled with
    int *hp_cx_in = nullptr, *d_cx_in = nullptr;
    size_t cx_in_cap = 0;                    // ints
    int *hp_cx_out = nullptr, *d_cx_out = nullptr;      // [4 S + 2]
    CxbDst *hp_cx_dst = nullptr, *d_cx_dst = nullptr;   // [S]
    int64_t cx_work[4] = {0, 0, 0, 0};       // ll_history_batch_extract_work
};

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

static void hb_cells_free(CbDev &m)
{
    void *ptrs[] = {m.pts,   m.pts2, m.pkey,  m.pkey2, m.pslot, m.pslot2, m.pep,    m.pep2,  m.ckey,  m.ckey2, m.cslot, m.cslot2, m.clast,
                    m.clast2, m.cep, m.cep2,  m.coff,  m.coff2, m.poff,   m.cstart, m.akey,  m.akey2, m.aslot, m.aslot2, m.aflag, m.arank,
                    m.mkey,  m.mkey2, m.mval, m.mval2, m.mslot, m.mslot2, m.tmp,    m.counts, m.tab};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    memset(&m, 0, sizeof(m));
}

static void hb_full_free(ll_history_batch *h)
{
    FbDev &t = h->fm;
    void *ptrs[] = {t.xf, t.tab, t.cnt, t.flag, t.rank, t.cells, t.toff, t.tmp};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    memset(&t, 0, sizeof(t));
    hb_cells_free(h->cm[2]);
    void *host[] = {h->hp_fm_tab, h->hp_fb_tab, h->hp_fm, h->hp_fm_cells};
    for (void *p : host)
        if (p) (void)hipHostFree(p);
    h->hp_fm_tab = nullptr;
    h->hp_fb_tab = nullptr;
    h->hp_fm = nullptr;
    h->hp_fm_cells = nullptr;
    h->fm_cells_cap = 0;
}

static void hb_cellmatch_free(CmbDev &q)
{
    void *ptrs[] = {q.csel, q.cflag, q.crank, q.ccell, q.key, q.key2, q.val, q.val2, q.hflag, q.hrank, q.head, q.leaf, q.leaf_cell, q.out, q.tmp};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    memset(&q, 0, sizeof(q));
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
                   h->d_nvalid, h->keys, h->keys2, h->vals, h->vals2, h->counts, h->tmp};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    for (int k = 0; k < 2; k++) hb_cells_free(h->cm[k]);
    hb_full_free(h);
    for (int k = 0; k < 2; k++) hb_cellmatch_free(h->cq[k]);
    if (h->d_cq_tab) (void)hipFree(h->d_cq_tab);
    void *cx_dev[] = {h->d_cx_in, h->d_cx_out, h->d_cx_dst};
    for (void *p : cx_dev)
        if (p) (void)hipFree(p);
    void *cx_host[] = {h->hp_cx_in, h->hp_cx_out, h->hp_cx_dst};
    for (void *p : cx_host)
        if (p) (void)hipHostFree(p);
    void *host[] = {h->hp_add, h->hp_cnt, h->hp_ref, h->hp_mm_init, h->hp_mm, h->hp_grid, h->hp_nvalid, h->hp_cm_tab, h->hp_cm, h->hp_cq_tab, h->hp_cq};
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


// ================================================================================================ the cell maps of the slots
static const long long kCbLimit = 0x7fffffffLL;  // a store holds fewer than 2^31 points per kind (the sorts index with 32 bits)

// a device array of `count` entries that keeps its first `keep`
template <typename T>
static int hb_cells_move(ll_history_batch *h, T **p, size_t count, size_t keep)
{
    T *q = nullptr;
    HC(hipMalloc((void **)&q, (count > 0 ? count : 1) * sizeof(T)));
    if (*p && keep > 0) {
        hipError_t e = hipMemcpyAsync(q, *p, keep * sizeof(T), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            (void)hipFree(q);
            return set_err("ll_history_batch (cell maps)", hipGetErrorString(e));
        }
    }
    if (*p) (void)hipFree(*p);
    *p = q;
    return 0;
}

// Room for `need` logged points: twice the capacity when they would not fit -- the only time stored points are copied outside a
// materialisation.  A capacity is raised only after every array of its group has moved, so a failure leaves the store consistent.
static int hb_cells_reserve_log(ll_history_batch *h, CbDev &m, long long need)
{
    if (need <= (long long)m.cap) return 0;
    long long want = 2LL * (long long)m.cap;
    want = want < need ? need : want;
    want = want < kCbLimit ? want : kCbLimit;
    const size_t n = (size_t)want, keep = (size_t)m.n_log;
    if (hb_cells_move(h, &m.pts, n, keep) || hb_cells_move(h, &m.pkey, n, keep) || hb_cells_move(h, &m.pslot, n, keep) ||
        hb_cells_move(h, &m.pep, n, keep) || hb_cells_move(h, &m.pts2, n, 0) || hb_cells_move(h, &m.pkey2, n, 0) ||
        hb_cells_move(h, &m.pslot2, n, 0) || hb_cells_move(h, &m.pep2, n, 0))
        return -1;
    m.cap = n;
    return 0;
}

static int hb_cells_reserve_table(ll_history_batch *h, CbDev &m, long long need)
{
    if (need <= (long long)m.ccap) return 0;
    long long want = 2LL * (long long)m.ccap;
    want = want < need ? need : want;
    const size_t n = (size_t)want, keep = (size_t)m.n_cells;
    if (hb_cells_move(h, &m.ckey, n, keep) || hb_cells_move(h, &m.cslot, n, keep) || hb_cells_move(h, &m.clast, n, keep) ||
        hb_cells_move(h, &m.cep, n, keep) || hb_cells_move(h, &m.ckey2, n, 0) || hb_cells_move(h, &m.cslot2, n, 0) ||
        hb_cells_move(h, &m.clast2, n, 0) || hb_cells_move(h, &m.cep2, n, 0) || hb_cells_move(h, &m.cstart, n + (size_t)m.S + 1, 0))
        return -1;
    HC(hipMemset(m.cstart, 0, (n + (size_t)m.S + 1) * sizeof(int)));  // (rebuilt by the next materialisation)
    HC(hipDeviceSynchronize());
    m.ccap = n;
    return 0;
}

static int hb_cells_reserve_tmp(ll_history_batch *h, CbDev &m, long long n)
{
    size_t bytes = 0;
    const char *err = nullptr;
    if (cb_tmp_bytes(n, &bytes, &err)) return set_err("ll_history_batch (cell maps)", err);
    if (bytes <= m.tmp_bytes) return 0;
    char *p = (char *)m.tmp;
    if (hb_cells_move(h, &p, bytes + bytes / 2, 0)) return -1;
    m.tmp = p;
    m.tmp_bytes = bytes + bytes / 2;
    return 0;
}

// before an add enqueues anything: the store stays below 2^31 points per kind even if the VoxelGrid drops nothing
static int hb_cells_room(const char *where, ll_history_batch *h, const int32_t *active, const int *in_n)
{
    for (int k = 0; k < 2; k++) {
        long long bound = h->cm[k].n_log;
        for (int s = 0; s < h->S; s++)
            if (!active || active[s]) bound += in_n[k * h->S + s] > 0 ? in_n[k * h->S + s] : 0;
        if (bound >= kCbLimit) return set_err(where, "the cell maps would pass 2^31 stored points per kind");
    }
    return 0;
}

// The cell-map part of an add: the filtered frames of the working slots (h->vf[k].out, their sizes in hp_cm) behind the logs of the
// two kinds.  One chain per kind, one wait for both.
static int hb_cells_append(const char *where, ll_history_batch *h)
{
    const int S = h->S;
    long long n_new[2] = {0, 0};
    int max_n[2] = {0, 0}, launches = 0;
    for (int k = 0; k < 2; k++) {
        CbSlot *tab = h->hp_cm_tab + (size_t)k * S;
        for (int s = 0; s < S; s++) {
            memset(&tab[s], 0, sizeof(CbSlot));
            if (!h->hp_add[s].work) continue;
            int n = h->hp_cm[(size_t)k * S + s];
            n = n < 0 ? 0 : (n < h->max_pts ? n : h->max_pts);
            tab[s].off = h->cm[k].n_log + n_new[k];
            tab[s].n = n;
            tab[s].frame = h->cm_frame[k][s];
            tab[s].active = 1;
            n_new[k] += n;
            max_n[k] = n > max_n[k] ? n : max_n[k];
        }
    }
    for (int k = 0; k < 2; k++) {
        CbDev &m = h->cm[k];
        if (n_new[k] == 0) continue;
        if (m.n_log + n_new[k] >= kCbLimit) return set_err(where, "the cell maps would pass 2^31 stored points per kind");
        if (hb_cells_reserve_log(h, m, m.n_log + n_new[k]) || hb_cells_reserve_table(h, m, (long long)m.n_cells + n_new[k]) ||
            hb_cells_reserve_tmp(h, m, n_new[k]))
            return -1;
        if ((long long)m.acap < n_new[k]) {
            const size_t n = (size_t)(n_new[k] + n_new[k] / 2);
            if (hb_cells_move(h, &m.akey, n, 0) || hb_cells_move(h, &m.akey2, n, 0) || hb_cells_move(h, &m.aslot, n, 0) ||
                hb_cells_move(h, &m.aslot2, n, 0) || hb_cells_move(h, &m.aflag, n, 0) || hb_cells_move(h, &m.arank, n, 0))
                return -1;
            m.acap = n;
        }
    }
    int *h_coff = h->hp_cm + (size_t)2 * S, *h_counts = h->hp_cm + (size_t)2 * S + 4 * ((size_t)S + 1);
    const char *err = nullptr;
    for (int k = 0; k < 2; k++) {
        CbDev &m = h->cm[k];
        if (n_new[k] == 0) continue;
        HC(hipMemcpyAsync(m.tab, h->hp_cm_tab + (size_t)k * S, (size_t)S * sizeof(CbSlot), hipMemcpyHostToDevice, h->stream));
        if (cb_append(m, h->vf[k].out, h->max_pts, max_n[k], n_new[k], h->stream, &launches, &err)) return set_err(where, err);
        HC(hipMemcpyAsync(h_counts + 4 * k, m.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HC(hipMemcpyAsync(h_coff + (size_t)k * (S + 1), m.coff, (size_t)(S + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HC(hipStreamSynchronize(h->stream));
    for (int k = 0; k < 2; k++) {
        CbDev &m = h->cm[k];
        for (int s = 0; s < S; s++)  // (the cell counts at the call decide the step of the frame counter)
            if (h->hp_add[s].work) h->cm_frame[k][s] += cb_frame_step(h->cm_coff[k][s + 1] == h->cm_coff[k][s]);
        if (n_new[k] == 0) continue;
        m.n_cells = h_counts[4 * k + 1];
        for (int s = 0; s <= S; s++) h->cm_coff[k][s] = h_coff[(size_t)k * (S + 1) + s];
        h->cm_work[0] += n_new[k];
        h->cm_work[1] += n_new[k];  // (the candidates' keys: two sorts over the new points, nothing else is sorted or gathered here)
    }
    h->cm_work[3] = launches;
    h->cm_dirty = true;
    return 0;
}

// put the stores of the kinds k0 .. k1 - 1 in order; h_poff: pinned, S + 1 entries per kind
static int hb_stores_materialise(const char *where, ll_history_batch *h, int k0, int k1, int *h_poff)
{
    const int S = h->S;
    HC(hipSetDevice(h->device));
    for (int k = k0; k < k1; k++) {
        CbDev &m = h->cm[k];
        if (m.n_log <= 0) continue;
        if (hb_cells_reserve_tmp(h, m, m.n_log)) return -1;
        if ((long long)m.mcap < m.n_log) {
            const size_t n = m.cap;  // (the log's capacity: grows as rarely as the log does)
            if (hb_cells_move(h, &m.mkey, n, 0) || hb_cells_move(h, &m.mkey2, n, 0) || hb_cells_move(h, &m.mval, n, 0) ||
                hb_cells_move(h, &m.mval2, n, 0) || hb_cells_move(h, &m.mslot, n, 0) || hb_cells_move(h, &m.mslot2, n, 0))
                return -1;
            m.mcap = n;
        }
    }
    int launches = 0;
    const char *err = nullptr;
    for (int k = k0; k < k1; k++) {
        CbDev &m = h->cm[k];
        if (cb_materialise(m, h->stream, &launches, &err)) return set_err(where, err);
        HC(hipMemcpyAsync(h_poff + (size_t)(k - k0) * (S + 1), m.poff, (size_t)(S + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HC(hipStreamSynchronize(h->stream));
    for (int k = k0; k < k1; k++) {
        for (int s = 0; s <= S; s++) h->cm_poff[k][s] = h_poff[(size_t)(k - k0) * (S + 1) + s];
        h->cm[k].n_log = h->cm_poff[k][S];  // the ordered store replaces the log: later adds write behind it
    }
    return 0;
}

// put the stores of both feature kinds in order (a read after an add); nothing to do when no add came since the last time
static int hb_cells_materialise(const char *where, ll_history_batch *h)
{
    if (!h->cm_dirty) return 0;
    if (hb_stores_materialise(where, h, 0, 2, h->hp_cm + (size_t)2 * h->S + 2 * ((size_t)h->S + 1))) return -1;
    h->cm_dirty = false;
    h->cm_work[2]++;
    return 0;
}

// the same for the full-cloud store alone: a read of kind 2 never orders the feature stores, and the other way round
static int hb_full_materialise(const char *where, ll_history_batch *h)
{
    if (!h->fm_dirty) return 0;
    if (hb_stores_materialise(where, h, 2, 3, h->hp_fm + (size_t)h->S + ((size_t)h->S + 1))) return -1;
    h->fm_dirty = false;
    h->fm_work[3]++;
    return 0;
}


// slots 0 .. S-1 of a device-resident producer
static int history_batch_add_common(const char *where, ll_history_batch *h, const FeatView &v, const int32_t *active, const double *poses7,
                                    const double *gate_poses7, double t_step, double angle_step, int32_t *added)
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
    if (h->cm_on && hb_cells_room(where, h, active, in_n)) return -1;
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
        for (int k = 0; k < 2; k++) HC(hipMemcpyAsync(h->hp_cm + (size_t)k * S, h->vf[k].n_out, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, h->stream));
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
    if (!h || !vc || !vs || !poses7) return set_err(where, "null argument");
    if (vc->device != h->device || vs->device != h->device) return set_err(where, "handles live on different devices");
    if (vc->dev.max_clouds < h->S || vs->dev.max_clouds < h->S) return set_err(where, "the voxel filters hold fewer clouds than n_sequences");
    return history_batch_add_common(where, h, feat_view(vc, vs), active, poses7, gate_poses7, history_add_t_step, history_add_angle_step, added);
}

extern "C" int ll_history_batch_add_fe(ll_history_batch *h, ll_fe *fe, const int32_t *active, const double *poses7, const double *gate_poses7,
                                       double history_add_t_step, double history_add_angle_step, int32_t *added)
{
    static const char *where = "ll_history_batch_add_fe";
    if (!h || !fe || !poses7) return set_err(where, "null argument");
    if (fe->prm.device != h->device) return set_err(where, "extractor lives on another device");
    if (fe->prm.max_scans < h->S) return set_err(where, "the extractor holds fewer scans than n_sequences");
    return history_batch_add_common(where, h, feat_view(fe), active, poses7, gate_poses7, history_add_t_step, history_add_angle_step, added);
}

// what a refresh checks before it touches anything: a map of the handle's device in every active slot, none of them twice
static int hb_check_maps(const char *where, const ll_history_batch *h, ll_map *const *maps, const int32_t *active, bool *any)
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

static void hb_sizes_out(const ll_history_batch *h, int64_t *n_map_corner, int64_t *n_map_surf)
{
    for (int s = 0; s < h->S; s++) {
        if (n_map_corner) n_map_corner[s] = h->n_map[0][s];
        if (n_map_surf) n_map_surf[s] = h->n_map[1][s];
    }
}

static int hb_refresh_second_half(const char *where, ll_history_batch *h, ll_map *const *maps, const int max_cat[2], const int cat_stride[2],
                                  int64_t *n_map_corner, int64_t *n_map_surf);

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
static int hb_refresh_second_half(const char *where, ll_history_batch *h, ll_map *const *maps, const int max_cat[2], const int cat_stride[2],
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

static int hb_cells_enable_impl(ll_history_batch *h, int64_t initial_points_per_map, float cell_resolution, int32_t threshold)
{
    const size_t S = (size_t)h->S;
    HC(hipHostMalloc((void **)&h->hp_cm_tab, 2 * S * sizeof(CbSlot), hipHostMallocDefault));
    HC(hipHostMalloc((void **)&h->hp_cm, (2 * S + 4 * (S + 1) + 8) * sizeof(int), hipHostMallocDefault));
    for (int k = 0; k < 2; k++) {
        CbDev &m = h->cm[k];
        m.S = h->S;
        m.geom = cell_geom(cell_resolution);  // laser_mapping.hpp:620-624: set_resolution( m_pt_cell_resolution ), m_minimum_revisit_threshold
        m.threshold = threshold;
        DM(m.coff, S + 1);
        DM(m.coff2, S + 1);
        DM(m.poff, S + 1);
        DM(m.counts, 4);
        DM(m.tab, S);
        HC(hipMemset(m.coff, 0, (S + 1) * sizeof(int)));
        HC(hipMemset(m.poff, 0, (S + 1) * sizeof(int)));
        HC(hipMemset(m.counts, 0, 4 * sizeof(int)));
        if (hb_cells_reserve_log(h, m, (long long)(S * (size_t)initial_points_per_map)) || hb_cells_reserve_table(h, m, (long long)h->max_pts)) return -1;
        h->cm_frame[k].assign(S, 0);
        h->cm_coff[k].assign(S + 1, 0);
        h->cm_poff[k].assign(S + 1, 0);
    }
    HC(hipDeviceSynchronize());  // (null-stream memsets are not ordered with the handle's non-blocking stream)
    return 0;
}

extern "C" int ll_history_batch_enable_cell_maps(ll_history_batch *h, int64_t initial_points_per_map, float cell_resolution,
                                                 int32_t threshold_cell_revisit)
{
    static const char *where = "ll_history_batch_enable_cell_maps";
    if (!h) return set_err(where, "null argument");
    if (h->cm_on) return set_err(where, "already enabled");
    if (!(cell_resolution > 0.f)) return set_err(where, "cell_resolution must be positive");
    if (initial_points_per_map < h->max_pts) return set_err(where, "initial_points_per_map below max_points_per_frame");
    if ((double)initial_points_per_map * (double)h->S >= 2147483647.0)
        return set_err(where, "n_sequences * initial_points_per_map must stay below 2^31 stored points per kind");
    HC(hipSetDevice(h->device));
    HC(hipStreamSynchronize(h->stream));
    if (hb_cells_enable_impl(h, initial_points_per_map, cell_resolution, threshold_cell_revisit)) {  // all or nothing
        const std::string keep = g_err;
        for (int k = 0; k < 2; k++) hb_cells_free(h->cm[k]);
        if (h->hp_cm_tab) (void)hipHostFree(h->hp_cm_tab);
        if (h->hp_cm) (void)hipHostFree(h->hp_cm);
        h->hp_cm_tab = nullptr;
        h->hp_cm = nullptr;
        g_err = keep;
        return -1;
    }
    h->cm_on = true;
    h->cm_res[0] = h->cm_res[1] = cell_resolution;
    return 0;
}

// what every reader checks first; 0 with the stores in order
static int hb_cells_reader(const char *where, ll_history_batch *h, int32_t sequence, int32_t kind)
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
    if (n_cells) *n_cells = h->cm_coff[kind][sequence + 1] - h->cm_coff[kind][sequence];
    if (n_points) *n_points = h->cm_poff[kind][sequence + 1] - h->cm_poff[kind][sequence];
    if (frame_idx) *frame_idx = h->cm_frame[kind][sequence];
    return 0;
}

extern "C" int ll_history_batch_cell_map_dump(ll_history_batch *h, int32_t sequence, int32_t kind, float *xyzi, int64_t capacity_points,
                                              int32_t *cell_ijk, int32_t *cell_start, int32_t *cell_last_update, int64_t capacity_cells)
{
    static const char *where = "ll_history_batch_cell_map_dump";
    if (!h) return set_err(where, "null argument");
    if (sequence >= 0 && sequence < h->S && ((kind == 2 && h->fm_on && !h->fm_dirty) || (h->cm_on && kind >= 0 && kind <= 1 && !h->cm_dirty))) {
        // (sizes known: refuse short buffers before any work)
        const int np = h->cm_poff[kind][sequence + 1] - h->cm_poff[kind][sequence], nc = h->cm_coff[kind][sequence + 1] - h->cm_coff[kind][sequence];
        if ((xyzi && capacity_points < np) || ((cell_ijk || cell_start || cell_last_update) && capacity_cells < nc)) return set_err(where, "buffer too small");
    }
    if (hb_cells_reader(where, h, sequence, kind)) return -1;
    const CbDev &m = h->cm[kind];
    const int p0 = h->cm_poff[kind][sequence], c0 = h->cm_coff[kind][sequence];
    const int np = h->cm_poff[kind][sequence + 1] - p0, nc = h->cm_coff[kind][sequence + 1] - c0;
    if ((xyzi && capacity_points < np) || ((cell_ijk || cell_start || cell_last_update) && capacity_cells < nc)) return set_err(where, "buffer too small");
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
    const CbDev &m = h->cm[kind];
    const int p0 = h->cm_poff[kind][sequence];
    *dev_xyz0 = (const float *)(m.pts + p0);
    *dev_point_keys = (const uint64_t *)(m.pkey + p0);
    *n_points = h->cm_poff[kind][sequence + 1] - p0;
    if (n_cells) *n_cells = h->cm_coff[kind][sequence + 1] - h->cm_coff[kind][sequence];
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
static int hb_full_enable_impl(ll_history_batch *h, int64_t initial_points_per_map, float cell_resolution, int32_t threshold)
{
    const size_t S = (size_t)h->S;
    HC(hipHostMalloc((void **)&h->hp_fm_tab, S * sizeof(CbSlot), hipHostMallocDefault));
    HC(hipHostMalloc((void **)&h->hp_fb_tab, S * sizeof(FbSlot), hipHostMallocDefault));
    HC(hipHostMalloc((void **)&h->hp_fm, (S + 3 * (S + 1) + 4) * sizeof(int), hipHostMallocDefault));
    h->fm_cells_cap = 4096;
    HC(hipHostMalloc((void **)&h->hp_fm_cells, h->fm_cells_cap * 3 * sizeof(int), hipHostMallocDefault));
    CbDev &m = h->cm[2];
    m.S = h->S;
    m.geom = cell_geom(cell_resolution);  // laser_mapping.hpp:616-617: m_pt_cell_map_full has the feature maps' resolution and threshold
    m.threshold = threshold;
    DM(m.coff, S + 1);
    DM(m.coff2, S + 1);
    DM(m.poff, S + 1);
    DM(m.counts, 4);
    DM(m.tab, S);
    HC(hipMemset(m.coff, 0, (S + 1) * sizeof(int)));
    HC(hipMemset(m.poff, 0, (S + 1) * sizeof(int)));
    HC(hipMemset(m.counts, 0, 4 * sizeof(int)));
    if (hb_cells_reserve_log(h, m, (long long)(S * (size_t)initial_points_per_map)) || hb_cells_reserve_table(h, m, (long long)h->max_pts)) return -1;
    FbDev &t = h->fm;
    DM(t.xf, S * (size_t)h->max_pts);
    DM(t.tab, S);
    DM(t.toff, S + 1);
    HC(hipMemset(t.toff, 0, (S + 1) * sizeof(int)));
    h->cm_frame[2].assign(S, 0);
    h->cm_coff[2].assign(S + 1, 0);
    h->cm_poff[2].assign(S + 1, 0);
    h->fm_touched.assign(S, std::vector<int32_t>());
    HC(hipDeviceSynchronize());  // (null-stream memsets are not ordered with the handle's non-blocking stream)
    return 0;
}

extern "C" int ll_history_batch_enable_full_maps(ll_history_batch *h, int64_t initial_points_per_map, float cell_resolution,
                                                 int32_t threshold_cell_revisit)
{
    static const char *where = "ll_history_batch_enable_full_maps";
    if (!h) return set_err(where, "null argument");
    if (h->fm_on) return set_err(where, "already enabled");
    if (!(cell_resolution > 0.f)) return set_err(where, "cell_resolution must be positive");
    if (initial_points_per_map < h->max_pts) return set_err(where, "initial_points_per_map below max_points_per_frame");
    if ((double)initial_points_per_map * (double)h->S >= 2147483647.0)
        return set_err(where, "n_sequences * initial_points_per_map must stay below 2^31 stored points");
    HC(hipSetDevice(h->device));
    HC(hipStreamSynchronize(h->stream));
    if (hb_full_enable_impl(h, initial_points_per_map, cell_resolution, threshold_cell_revisit)) {  // all or nothing
        const std::string keep = g_err;
        hb_full_free(h);
        g_err = keep;
        return -1;
    }
    h->fm_on = true;
    h->cm_res[2] = cell_resolution;
    return 0;
}

// the scratch of the touched chain follows the cell table's capacity (the stream is idle)
static int hb_full_reserve_scratch(ll_history_batch *h, long long n_upper)
{
    FbDev &t = h->fm;
    const size_t want = h->cm[2].ccap;
    if (t.tcap < want) {
        if (hb_cells_move(h, &t.cnt, want, 0) || hb_cells_move(h, &t.flag, want, 0) || hb_cells_move(h, &t.rank, want, 0) ||
            hb_cells_move(h, &t.cells, 3 * want, 0))
            return -1;
        t.tcap = want;
    }
    size_t bytes = 0;
    const char *err = nullptr;
    if (fb_tmp_bytes(n_upper, &bytes, &err)) return set_err("ll_history_batch_append_full_fe", err);
    if (bytes > t.tmp_bytes) {
        char *p = (char *)t.tmp;
        if (hb_cells_move(h, &p, bytes + bytes / 2, 0)) return -1;
        t.tmp = p;
        t.tmp_bytes = bytes + bytes / 2;
    }
    return 0;
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
    CbDev &m = h->cm[2];
    FbDev &t = h->fm;
    HC(hipSetDevice(h->device));
    int enq = 0, waits = 0;
    int *in_n = h->hp_fm, *h_coff = in_n + S, *h_counts = h_coff + 2 * ((size_t)S + 1), *h_toff = h_counts + 4;
    HC(hipMemcpyAsync(in_n, fe->dev.n_full, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, fe->stream));  // (behind the selection)
    HC(hipStreamSynchronize(fe->stream));
    enq++;
    waits++;
    // ---- the checks: nothing is enqueued on the handle's stream and nothing is changed before they have passed
    long long n_new = 0;
    int max_n = 0;
    for (int s = 0; s < S; s++) {
        if (active && !active[s]) continue;
        if (in_n[s] > h->max_pts || in_n[s] > fe->dev.stride) return set_err(where, "full selection exceeds max_points_per_frame");
        const int n = in_n[s] > 0 ? in_n[s] : 0;
        n_new += n;
        max_n = n > max_n ? n : max_n;
    }
    if (m.n_log + n_new >= kCbLimit) return set_err(where, "the full maps would pass 2^31 stored points");
    const long long n_upper = (long long)m.n_cells + n_new;  // bound of the cell table after the merge
    if (n_upper >= kCbLimit) return set_err(where, "the full maps would pass 2^31 cells");
    if (n_new > 0) {
        if (hb_cells_reserve_log(h, m, m.n_log + n_new) || hb_cells_reserve_table(h, m, n_upper) || hb_cells_reserve_tmp(h, m, n_new) ||
            hb_full_reserve_scratch(h, n_upper))
            return -1;
        if ((long long)m.acap < n_new) {
            const size_t n = (size_t)(n_new + n_new / 2);
            if (hb_cells_move(h, &m.akey, n, 0) || hb_cells_move(h, &m.akey2, n, 0) || hb_cells_move(h, &m.aslot, n, 0) ||
                hb_cells_move(h, &m.aslot2, n, 0) || hb_cells_move(h, &m.aflag, n, 0) || hb_cells_move(h, &m.arank, n, 0))
                return -1;
            m.acap = n;
        }
    }
    // ---- the tables of the call
    long long off = m.n_log;
    for (int s = 0; s < S; s++) {
        CbSlot &c = h->hp_fm_tab[s];
        FbSlot &f = h->hp_fb_tab[s];
        memset(&c, 0, sizeof(c));
        memset(&f, 0, sizeof(f));
        if (active && !active[s]) continue;
        const int n = in_n[s] > 0 ? in_n[s] : 0;
        c.off = off;
        c.n = f.n = n;
        c.frame = h->cm_frame[2][s];
        c.active = f.active = 1;
        f.need = fb_need(h->cm_coff[2][s + 1] == h->cm_coff[2][s], min_points);
        for (int i = 0; i < 7; i++) f.pose[i] = poses7[7 * (size_t)s + i];
        off += n;
    }
    int total = 0;
    if (n_new > 0) {
        const char *err = nullptr;
        HC(hipMemcpyAsync(m.tab, h->hp_fm_tab, (size_t)S * sizeof(CbSlot), hipMemcpyHostToDevice, h->stream));
        HC(hipMemcpyAsync(t.tab, h->hp_fb_tab, (size_t)S * sizeof(FbSlot), hipMemcpyHostToDevice, h->stream));
        enq += 2;
        if (fb_gather(t, fe->dev.xyzi, fe->dev.full_idx, fe->dev.stride, S, h->max_pts, max_n, h->stream, &enq, &err)) return set_err(where, err);
        if (cb_append(m, t.xf, h->max_pts, max_n, n_new, h->stream, &enq, &err)) return set_err(where, err);
        if (fb_touched_chain(m, t, max_n, (int)n_upper, h->stream, &enq, &err)) return set_err(where, err);
        HC(hipMemcpyAsync(h_counts, m.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HC(hipMemcpyAsync(h_coff, m.coff, (size_t)(S + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HC(hipMemcpyAsync(h_toff, t.toff, (size_t)(S + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        enq += 3;
        HC(hipStreamSynchronize(h->stream));
        waits++;
        total = h_toff[S];
        if (total < 0 || total > h_counts[1] || h_counts[1] > n_upper) return set_err(where, "touched-cell counts out of range");
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
    for (int s = 0; s < S; s++) {
        if (active && !active[s]) continue;  // (an inactive slot keeps its map, its counter and its list)
        h->cm_frame[2][s] += cb_frame_step(h->cm_coff[2][s + 1] == h->cm_coff[2][s]);  // (the cell counts at the call)
        std::vector<int32_t> &list = h->fm_touched[s];
        list.clear();
        if (n_new > 0) list.assign(h->hp_fm_cells + 3 * (size_t)h_toff[s], h->hp_fm_cells + 3 * (size_t)h_toff[s + 1]);
    }
    if (n_new > 0) {
        m.n_cells = h_counts[1];
        for (int s = 0; s <= S; s++) h->cm_coff[2][s] = h_coff[s];
        h->fm_dirty = true;
    }
    for (int s = 0; s < S; s++) n_touched[s] = (int64_t)(h->fm_touched[s].size() / 3);
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

// Test tap of the full-cloud maps: [0] enqueues (launches, library calls, copies) of the last ll_history_batch_append_full_fe, [1] its
// host waits (a growth of the store waits on top and is not counted), [2] stored points that went through a sort or a gather inside
// append calls so far -- no kernel of an append takes a stored point, so nothing ever adds to it: the number is there to be
// asserted -- [3] materialisations of the full store so far.
extern "C" int ll_history_batch_full_map_work(ll_history_batch *h, int64_t out[4])
{
    static const char *where = "ll_history_batch_full_map_work";
    if (!h || !out) return set_err(where, "null argument");
    if (!h->fm_on) return set_err(where, "full maps are not enabled (ll_history_batch_enable_full_maps)");
    for (int i = 0; i < 4; i++) out[i] = h->fm_work[i];
    return 0;
}


// ================================================================================================ cells of the slots into cell maps
// the staging of a call and the scratch of its chain (the stream is idle: the store has just been put in order)
static int hb_extract_reserve(const char *where, ll_history_batch *h, CbDev &m, size_t n_in)
{
    const size_t S = (size_t)h->S;
    if (!h->hp_cx_out) HC(hipHostMalloc((void **)&h->hp_cx_out, (4 * S + 2) * sizeof(int), hipHostMallocDefault));
    if (!h->hp_cx_dst) HC(hipHostMalloc((void **)&h->hp_cx_dst, S * sizeof(CxbDst), hipHostMallocDefault));
    if (!h->d_cx_out) DM(h->d_cx_out, 4 * S + 2);
    if (!h->d_cx_dst) DM(h->d_cx_dst, S);
    if (n_in > h->cx_in_cap) {
        const size_t want = n_in + n_in / 2 + 64;
        int *hp = nullptr, *d = nullptr;
        HC(hipHostMalloc((void **)&hp, want * sizeof(int), hipHostMallocDefault));
        if (hipMalloc((void **)&d, want * sizeof(int)) != hipSuccess) {
            (void)hipHostFree(hp);
            return set_err(where, "allocation failed");
        }
        if (h->hp_cx_in) (void)hipHostFree(h->hp_cx_in);
        if (h->d_cx_in) (void)hipFree(h->d_cx_in);
        h->hp_cx_in = hp;
        h->d_cx_in = d;
        h->cx_in_cap = want;
    }
    if (m.mcap < (size_t)m.n_cells + 1) {  // (a store that was never materialised, or one whose every point opened a cell)
        const size_t n = m.cap > (size_t)m.n_cells + 1 ? m.cap : (size_t)m.n_cells + 1;
        if (hb_cells_move(h, &m.mkey, n, 0) || hb_cells_move(h, &m.mkey2, n, 0) || hb_cells_move(h, &m.mval, n, 0) ||
            hb_cells_move(h, &m.mval2, n, 0) || hb_cells_move(h, &m.mslot, n, 0) || hb_cells_move(h, &m.mslot2, n, 0))
            return -1;
        m.mcap = n;
    }
    size_t bytes = 0;
    const char *err = nullptr;
    if (cxb_tmp_bytes(m.n_cells, &bytes, &err)) return set_err(where, err);
    if (bytes > m.tmp_bytes) {
        char *p = (char *)m.tmp;
        if (hb_cells_move(h, &p, bytes + bytes / 2, 0)) return -1;
        m.tmp = p;
        m.tmp_bytes = bytes + bytes / 2;
    }
    return 0;
}

// Key frames' views of the shared cells (CMK:1243-1261) for several slots at once: request r copies the cells of slot sequences[r]'s
// map of `kind` named in cell_ijk[list_offsets[r] .. list_offsets[r + 1]) into dst[r], where they lie (ll_cellmap_batch_extract_kernels.hip).
// Every refusal comes before anything is enqueued; the store is put in order as every reader does; then one fixed chain, one wait
// for the totals -- which size the destinations: all that need room grow before any is overwritten -- and a final wait.
extern "C" int ll_history_batch_extract_cells(ll_history_batch *h, int32_t kind, int32_t n_requests, const int32_t *sequences,
                                              const int64_t *list_offsets, const int32_t *cell_ijk, ll_cellmap *const *dst, int64_t *n_cells_found,
                                              int64_t *n_points)
{
    static const char *where = "ll_history_batch_extract_cells";
    if (!h) return set_err(where, "null argument");
    if (kind == 2) {
        if (!h->fm_on) return set_err(where, "full maps are not enabled (ll_history_batch_enable_full_maps)");
    } else if (kind == 0 || kind == 1) {
        if (!h->cm_on) return set_err(where, "cell maps are not enabled (ll_history_batch_enable_cell_maps)");
    } else {
        return set_err(where, "kind out of range");
    }
    const int S = h->S, R = n_requests;
    if (R < 1 || R > S) return set_err(where, "n_requests must lie in 1 .. n_sequences");
    if (!sequences || !list_offsets || !dst || !n_cells_found || !n_points) return set_err(where, "null argument");
    if (list_offsets[0] < 0) return set_err(where, "list_offsets must not be negative");
    for (int r = 0; r < R; r++)
        if (list_offsets[r + 1] < list_offsets[r]) return set_err(where, "list_offsets must not descend");
    const int64_t n_list64 = list_offsets[R] - list_offsets[0];
    if (n_list64 >= 0x3fffffffLL / 3) return set_err(where, "the cell lists are too long");
    if (n_list64 > 0 && !cell_ijk) return set_err(where, "null argument");
    std::vector<char> named((size_t)S, 0);
    for (int r = 0; r < R; r++) {
        const int s = sequences[r];
        if (s < 0 || s >= S) return set_err(where, "sequence out of range");
        if (named[s]) return set_err(where, "a sequence is named twice");
        named[s] = 1;
        const ll_cellmap *d = dst[r];
        if (!d) return set_err(where, "null argument");
        for (int o = 0; o < r; o++)
            if (dst[o] == d) return set_err(where, "a destination is named twice");
        if (d->owner) return set_err(where, "a destination is owned by a history");
        if (d->device != h->device) return set_err(where, "a destination is on another device");
        if (d->dev.resolution != h->cm_res[kind]) return set_err(where, "a destination has another resolution than the store");
    }
    HC(hipSetDevice(h->device));
    const int64_t mats = kind == 2 ? h->fm_work[3] : h->cm_work[2];
    if (hb_cells_reader(where, h, sequences[0], kind)) return -1;  // at most one materialisation, with its own wait
    h->cx_work[3] += (kind == 2 ? h->fm_work[3] : h->cm_work[2]) - mats;
    CbDev &m = h->cm[kind];
    const int n_list = (int)n_list64;
    const size_t n_in = (size_t)3 * R + 1 + (size_t)3 * n_list;
    if (hb_extract_reserve(where, h, m, n_in)) return -1;
    // ---- the requests in ascending slot order: the order of the table, and so of the scan
    std::vector<int> order((size_t)R);
    for (int r = 0; r < R; r++) order[r] = r;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return sequences[a] < sequences[b]; });
    int *in = h->hp_cx_in;
    for (int r = 0; r <= R; r++) in[r] = (int)(list_offsets[r] - list_offsets[0]);
    for (int r = 0; r < R; r++) in[R + 1 + r] = sequences[r];
    for (int q = 0; q < R; q++) in[2 * R + 1 + q] = sequences[order[q]];
    if (n_list > 0) memcpy(in + 3 * R + 1, cell_ijk + 3 * (size_t)list_offsets[0], (size_t)3 * n_list * sizeof(int));
    int enq = 0, waits = 0;
    const char *err = nullptr;
    HC(hipMemcpyAsync(h->d_cx_in, in, n_in * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (cxb_mark(m, h->d_cx_in, R, n_list, h->d_cx_out, h->stream, &enq, &err)) return set_err(where, err);
    HC(hipMemcpyAsync(h->hp_cx_out, h->d_cx_out, ((size_t)4 * R + 2) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    enq += 2;
    HC(hipStreamSynchronize(h->stream));  // the only wait before points move
    waits++;
    const int *found = h->hp_cx_out, *points = found + R, *qrank = points + R, *qpos = qrank + R + 1;
    const int n_found = qrank[R], n_pts = qpos[R];
    for (int q = 0; q < R; q++) {
        const int s = sequences[order[q]];
        if (found[q] < 0 || points[q] < found[q] || found[q] > h->cm_coff[kind][s + 1] - h->cm_coff[kind][s] ||
            points[q] > h->cm_poff[kind][s + 1] - h->cm_poff[kind][s] || points[q] >= 0x3fffffff)
            return set_err(where, "cell selection out of range");
    }
    // ---- every destination that needs room grows (content kept) before any is overwritten: a failure here leaves all as they were
    for (int q = 0; q < R; q++) {
        ll_cellmap *d = dst[order[q]];
        if (points[q] > d->dev.cap && cellmap_make_room(d, points[q], where)) return -1;
    }
    for (int q = 0; q < R; q++) {
        const CellMapDev &d = dst[order[q]]->dev;
        h->hp_cx_dst[q] = CxbDst{d.ckey, d.cstart, d.clast, d.pts, d.pkey};
    }
    HC(hipMemcpyAsync(h->d_cx_dst, h->hp_cx_dst, (size_t)R * sizeof(CxbDst), hipMemcpyHostToDevice, h->stream));
    enq++;
    if (cxb_extract(m, h->d_cx_in, R, h->d_cx_out, h->d_cx_dst, n_found, n_pts, h->stream, &enq, &err)) return set_err(where, err);
    HC(hipStreamSynchronize(h->stream));  // the destinations are readable from their own streams
    waits++;
    for (int q = 0; q < R; q++) {
        const int r = order[q];
        CellMapDev &d = dst[r]->dev;
        d.n_pts = points[q];
        d.n_cells = points[q] > 0 ? found[q] : 0;
        d.frame = points[q] > 0 ? 2 : 0;  // the double increment of an append on an empty map (cellmap_append)
        d.n_filt = d.n_sel = 0;
        n_cells_found[r] = found[q];
        n_points[r] = points[q];
    }
    h->cx_work[0] = enq;
    h->cx_work[1] = waits;
    return 0;
}

// Test tap of the extraction: [0] enqueues (launches, library calls, copies) of the last ll_history_batch_extract_cells behind the
// store's being put in order, [1] its host waits (a materialisation and a growth of a destination wait on top), [2] stored points
// sorted or moved by extraction calls so far -- the chain copies points out and never touches the store, so nothing ever adds to it:
// the number is there to be asserted -- [3] materialisations extraction calls caused so far.
extern "C" int ll_history_batch_extract_work(ll_history_batch *h, int64_t out[4])
{
    static const char *where = "ll_history_batch_extract_work";
    if (!h || !out) return set_err(where, "null argument");
    if (!h->cm_on && !h->fm_on) return set_err(where, "neither cell maps nor full maps are enabled");
    for (int i = 0; i < 4; i++) out[i] = h->cx_work[i];
    return 0;
}


// ================================================================================================ the cell-mode refresh
// scratch of one kind for a store of n_log logged points and n_cells table entries (the stream is idle)
static int hb_cellmatch_reserve(ll_history_batch *h, CmbDev &q, long long n_log, int n_cells)
{
    if (!q.out) DM(q.out, (size_t)h->S + 4);
    if ((long long)q.ncap < n_log) {
        const size_t n = (size_t)(n_log + n_log / 2 + 16);
        if (hb_cells_move(h, &q.cflag, n, 0) || hb_cells_move(h, &q.crank, n, 0) || hb_cells_move(h, &q.ccell, n, 0) || hb_cells_move(h, &q.key, n, 0) ||
            hb_cells_move(h, &q.key2, n, 0) || hb_cells_move(h, &q.val, n, 0) || hb_cells_move(h, &q.val2, n, 0) || hb_cells_move(h, &q.hflag, n, 0) ||
            hb_cells_move(h, &q.hrank, n, 0) || hb_cells_move(h, &q.head, n, 0) || hb_cells_move(h, &q.leaf, n, 0) || hb_cells_move(h, &q.leaf_cell, n, 0))
            return -1;
        q.ncap = n;
    }
    if (q.ccap < (size_t)n_cells) {
        const size_t n = (size_t)n_cells + (size_t)n_cells / 2 + 16;
        if (hb_cells_move(h, &q.csel, n, 0)) return -1;
        q.ccap = n;
    }
    size_t bytes = 0;
    const char *err = nullptr;
    if (cmb_tmp_bytes(n_log, &bytes, &err)) return set_err("ll_history_batch_refresh_cells", err);
    if (bytes > q.tmp_bytes) {
        char *p = (char *)q.tmp;
        if (hb_cells_move(h, &p, bytes + bytes / 2, 0)) return -1;
        q.tmp = p;
        q.tmp_bytes = bytes + bytes / 2;
    }
    return 0;
}

// update_buff_for_matching with m_matching_mode == 1 (laser_mapping.hpp:471-546) for all slots: per kind one chain over the deferred
// store (ll_cellmatch_batch_kernels.hip), one drain for the leaf counts of both kinds, the checks, then the scatter into the
// concatenation buffers, the replace, and the second half of ll_history_batch_refresh.
extern "C" int ll_history_batch_refresh_cells(ll_history_batch *h, ll_map *const *maps, const int32_t *active, const double *poses7,
                                              float maximum_search_range_corner, float maximum_search_range_surface,
                                              float maximum_in_fov_angle, int32_t down_sample_replace, int64_t *n_map_corner,
                                              int64_t *n_map_surf)
{
    static const char *where = "ll_history_batch_refresh_cells";
    if (!h || !maps) return set_err(where, "null argument");
    if (!h->cm_on) return set_err(where, "cell maps are not enabled (ll_history_batch_enable_cell_maps)");
    if (!poses7) return set_err(where, "null argument (poses7)");
    const float range[2] = {maximum_search_range_corner, maximum_search_range_surface};
    if (!(range[0] >= 0.f) || !(range[1] >= 0.f)) return set_err(where, "a search range must not be negative");
    for (int k = 0; k < 2; k++)
        if (!cmb_leaf_fits(h->cm[k].geom, h->res[k]))
            return set_err(where, "leaf size too small for the cell size (more than 1020 leaves across one cell)");
    const int S = h->S;
    bool any = false;
    if (hb_check_maps(where, h, maps, active, &any)) return -1;
    if (!any) {
        hb_sizes_out(h, n_map_corner, n_map_surf);
        return 0;
    }
    HC(hipSetDevice(h->device));
    if (!h->hp_cq) {
        HC(hipHostMalloc((void **)&h->hp_cq_tab, (size_t)S * sizeof(CmbSlot), hipHostMallocDefault));
        HC(hipHostMalloc((void **)&h->hp_cq, 2 * ((size_t)S + 4) * sizeof(int), hipHostMallocDefault));
        DM(h->d_cq_tab, (size_t)S);
    }
    int *t_active = (int *)h->hp_ref, *t_ncat = t_active + S;
    for (int s = 0; s < S; s++) {
        CmbSlot &t = h->hp_cq_tab[s];
        memset(&t, 0, sizeof(t));
        t.active = t_active[s] = (!active || active[s]) ? 1 : 0;
        for (int i = 0; t.active && i < 7; i++) t.pose[i] = poses7[7 * (size_t)s + i];
    }
    bool run[2];
    for (int k = 0; k < 2; k++) {
        run[k] = h->cm[k].n_log > 0 && h->cm[k].n_cells > 0;
        if (run[k] && hb_cellmatch_reserve(h, h->cq[k], h->cm[k].n_log, h->cm[k].n_cells)) return -1;
    }
    // ---- per kind: select, candidates, per-cell VoxelGrid, counts; one copy each, one drain for both
    int enq = 0, waits = 0;
    const char *err = nullptr;
    memset(h->hp_cq, 0, 2 * ((size_t)S + 4) * sizeof(int));
    HC(hipMemcpyAsync(h->d_cq_tab, h->hp_cq_tab, (size_t)S * sizeof(CmbSlot), hipMemcpyHostToDevice, h->stream));
    enq++;
    for (int k = 0; k < 2; k++) {
        if (!run[k]) continue;
        if (cmb_query(h->cm[k], h->cq[k], h->d_cq_tab, range[k], maximum_in_fov_angle, h->res[k], h->stream, &enq, &err)) return set_err(where, err);
        HC(hipMemcpyAsync(h->hp_cq + (size_t)k * (S + 4), h->cq[k].out, ((size_t)S + 3) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        enq++;
    }
    HC(hipStreamSynchronize(h->stream));
    waits++;
    // ---- the checks, before anything is changed
    int max_cat[2] = {0, 0}, n_leaves[2] = {0, 0};
    long long n_cand[2] = {0, 0}, n_live[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        const int *loff = h->hp_cq + (size_t)k * (S + 4);
        n_leaves[k] = loff[S];
        n_cand[k] = loff[S + 1];
        n_live[k] = loff[S + 2];
        for (int s = 0; s < S; s++) {
            const int n = loff[s + 1] - loff[s];
            if (n < 0 || (!t_active[s] && n != 0)) return set_err(where, "leaf counts out of range");
            if ((size_t)n > h->cstride) {
                char msg[200];
                snprintf(msg, sizeof(msg), "the cells selected for slot %d hold %d %s leaves, the match buffer of a slot holds %zu points "
                         "(maximum_history_size * max_points_per_frame)", s, n, k ? "surface" : "corner", h->cstride);
                return set_err(where, msg);
            }
            t_ncat[k * S + s] = n;
            max_cat[k] = n > max_cat[k] ? n : max_cat[k];
        }
        if (down_sample_replace && h->cm[k].n_log + n_leaves[k] >= kCbLimit) return set_err(where, "the cell maps would pass 2^31 stored points per kind");
    }
    if (down_sample_replace)
        for (int k = 0; k < 2; k++)
            if (n_leaves[k] > 0 && hb_cells_reserve_log(h, h->cm[k], h->cm[k].n_log + n_leaves[k])) return -1;
    const int cat_stride[2] = {max_cat[0] > 0 ? max_cat[0] : 1, max_cat[1] > 0 ? max_cat[1] : 1};
    // ---- the leaves into the concatenations (:496-512)
    HC(hipMemcpyAsync(h->d_ref, h->hp_ref, h->ref_seg_off, hipMemcpyHostToDevice, h->stream));
    HC(hipMemcpyAsync(h->d_mm, h->hp_mm_init, (size_t)2 * S * 8 * sizeof(unsigned int), hipMemcpyHostToDevice, h->stream));
    enq += 2;
    for (int k = 0; k < 2; k++)
        if (run[k] && cmb_scatter(h->cm[k], h->cq[k], n_leaves[k], h->d_concat + (size_t)k * S * h->cstride, cat_stride[k], h->stream, &enq, &err))
            return set_err(where, err);
    // The stores are still as they were: a second half that fails (an allocation, a size out of range) leaves no replace behind.
    if (hb_refresh_second_half(where, h, maps, max_cat, cat_stride, n_map_corner, n_map_surf)) return -1;
    waits += 2;
    // ---- the replace (:492-495), once the maps are published; the second half uses none of the chain's scratch
    for (int k = 0; k < 2; k++) {
        if (!run[k] || !down_sample_replace || n_leaves[k] <= 0) continue;
        if (cmb_replace(h->cm[k], h->cq[k], n_leaves[k], h->stream, &enq, &err)) return set_err(where, err);
        n_live[k] += n_leaves[k] - n_cand[k];
        h->cm_dirty = true;  // (dead entries in the log: a reader puts the stores in order first)
    }
    h->cq_work[0] = enq;
    h->cq_work[1] = waits;
    h->cq_work[7] = n_cand[0] + n_cand[1];
    for (int k = 0; k < 2; k++) {
        h->cq_work[3 + 2 * k] = h->cm[k].n_log;
        h->cq_work[4 + 2 * k] = run[k] ? n_live[k] : 0;
    }
    // ---- the handle puts the stores in order by itself once the dead entries outnumber the live ones
    if (h->cm_dirty && ((run[0] && cmb_compact_now(h->cm[0].n_log, n_live[0])) || (run[1] && cmb_compact_now(h->cm[1].n_log, n_live[1])))) {
        if (hb_cells_materialise(where, h)) return -1;
        h->cq_work[2]++;
        for (int k = 0; k < 2; k++) h->cq_work[3 + 2 * k] = h->cq_work[4 + 2 * k] = h->cm[k].n_log;
    }
    return 0;
}

// Test tap of the cell-mode refresh: [0] enqueues (launches, library calls, copies) of the cell-mode part of the last refresh, the
// replace included, ll_history_batch_refresh's second half not, [1] the host waits of the refresh proper, second half included --
// a compaction or a growth of the log waits on top and is not counted here, [2] compactions so far (each costs a materialisation
// and its wait), [3] / [4] log entries and live entries of the corner stores after the last
// refresh, [5] / [6] of the surface stores, [7] candidates of the last refresh, both kinds.
extern "C" int ll_history_batch_cell_match_work(ll_history_batch *h, int64_t out[8])
{
    static const char *where = "ll_history_batch_cell_match_work";
    if (!h || !out) return set_err(where, "null argument");
    if (!h->cm_on) return set_err(where, "cell maps are not enabled (ll_history_batch_enable_cell_maps)");
    for (int i = 0; i < 8; i++) out[i] = h->cq_work[i];
    return 0;
}
