// ll_api_history_batch_internal.h -- what the units of the batched match buffer share (ll_api_history_batch_*.hip): the handle, the
// pooled search-grid arena, the host side of one deferred store, and the helpers more than one unit calls.
#pragma once
#include "ll_api_internal.h"
#include "ll_cellmap_batch_extract_core.h"
#include "ll_cellmatch_batch.h"
#include "ll_fullmap_batch.h"
#include "ll_scan_log.h"

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

// One deferred store of S slots (ll_cellmap_batch.h) with its host side: the mirrors every reader answers from, and the pinned
// tables of an append.  hp_n .. hp_counts name the parts of one pinned block.  (Hidden, like the helpers below: no symbol of its
// implicit members joins the library's surface; HbArena and the handle had theirs exported before and keep them.)
struct __attribute__((visibility("hidden"))) HbStore {
    CbDev dev{};
    float res = 0.f;               // the cell resolution the store was enabled with
    std::vector<int> frame;        // [S] m_current_frame_idx of every map
    std::vector<int> coff, poff;   // [S + 1] host copies: first cell / first stored point of every slot
    CbSlot *hp_tab = nullptr;      // pinned [S]
    int *hp_n = nullptr;           // [S] points per slot of the call (filtered counts / full-selection sizes)
    int *hp_coff = nullptr, *hp_poff = nullptr;  // [S + 1] each
    int *hp_counts = nullptr;      // [4]
};

// The scan log (ll_history_batch_enable_scan_log, ll_api_history_batch_scanlog.hip): the book of ll_scan_log.h, the chunks its blocks
// lie in, and what the last append_full_fe left for the log call behind it.
struct __attribute__((visibility("hidden"))) HbScanLog {
    bool on = false;
    SlBook book;
    std::vector<float4 *> chunks;      // chunk c holds blocks c * chunk_blocks ..; never moved, freed with the handle
    SlSlot *hp_tab = nullptr, *d_tab = nullptr;  // [S] the table of a log call, pinned / device
    hipEvent_t ev = nullptr;           // behind the last log kernel: the extractor's stream waits for it before a scan is replaced
    bool pending = false;              // an append_full_fe came and no log call yet
    const ll_fe *fe = nullptr;         // that append's extractor
    std::vector<int> n;                // [S] that append's selection sizes, -1 for a slot it left out
    int64_t work[2] = {0, 0};          // enqueue calls and host waits of the last log call
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
    // ll_history_batch_set_undistort: the next add moves slot s's clouds with record s (copies this handle owns, made on the registrar's
    // stream; ev_und orders this handle's stream behind them).  Both allocated by the first call.
    UndistortRec *d_und = nullptr;                  // [S]
    hipEvent_t ev_und = nullptr;
    bool has_und = false;
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
    // The deferred stores: corner and surface cell maps (ll_history_batch_enable_cell_maps), the full-cloud maps
    // (ll_history_batch_enable_full_maps).  A read of kind 0 or 1 puts both feature stores in order with one wait; kind 2 is on its own.
    HbStore st[3];
    bool cm_on = false, cm_dirty = false;    // dirty: an add came after the last materialisation
    bool fm_on = false, fm_dirty = false;
    int64_t cm_work[4] = {0, 0, 0, 0};       // ll_history_batch_cell_map_work
    // the cell-mode refresh (ll_history_batch_refresh_cells): scratch per kind, the slots' poses, the drained counts
    CmbDev cq[2]{};
    CmbSlot *hp_cq_tab = nullptr, *d_cq_tab = nullptr;  // [S]
    int *hp_cq = nullptr;                    // pinned [2][S + 4]: first leaf of every slot, leaves, candidates, live entries
    int64_t cq_work[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // ll_history_batch_cell_match_work
    // what an append to the full-cloud store needs on top of st[2]
    FbDev fm{};
    FbSlot *hp_fb_tab = nullptr;             // pinned [S]
    int *hp_fm_toff = nullptr;               // pinned [S + 1]: first touched cell of every slot
    int *hp_fm_cells = nullptr;              // pinned [fm_cells_cap][3]: the touched cells of the last append on their way to the lists
    size_t fm_cells_cap = 0;
    std::vector<std::vector<int32_t>> fm_touched;  // [S] the {i, j, k} of the cells the slot's last appended scan touched
    int64_t fm_work[4] = {0, 0, 0, 0};       // ll_history_batch_full_map_work
    // cells of several slots into cell maps (ll_history_batch_extract_cells): the staged requests and lists, the totals, the destinations
    int *hp_cx_in = nullptr, *d_cx_in = nullptr;
    size_t cx_in_cap = 0;                    // ints
    int *hp_cx_out = nullptr, *d_cx_out = nullptr;      // [4 S + 2]
    CxbDst *hp_cx_dst = nullptr, *d_cx_dst = nullptr;   // [S]
    int64_t cx_work[4] = {0, 0, 0, 0};       // ll_history_batch_extract_work
    HbScanLog sl;
};

#pragma GCC visibility push(hidden)  // what follows is shared by the units and no part of the library's surface

static const long long kCbLimit = 0x7fffffffLL;  // a store holds fewer than 2^31 points per kind (the sorts index with 32 bits)

// a device array of `count` entries that keeps its first `keep`
template <typename T>
int hb_cells_move(ll_history_batch *h, T **p, size_t count, size_t keep)
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
// the visitors of ll_cellmap_batch.h's array enumerations: free; move to `count` entries, the marked arrays keeping their first `keep`
static const auto hb_free = [](auto *&p, size_t, bool) { if (p) (void)hipFree(p); p = nullptr; return 0; };
static inline auto hb_mover(ll_history_batch *h, size_t keep) { return [=](auto *&p, size_t n, bool kept) { return hb_cells_move(h, &p, n, kept ? keep : 0); }; }
// temporary storage for what bytes_of(n, ..) asks, half again as much when it has to move
template <typename F, typename N>
int hb_reserve_tmp(const char *where, ll_history_batch *h, void *&tmp, size_t &tmp_bytes, F bytes_of, N n)
{
    size_t bytes = 0;
    const char *err = nullptr;
    if (bytes_of(n, &bytes, &err)) return set_err(where, err);
    if (bytes <= tmp_bytes) return 0;
    char *p = (char *)tmp;
    if (hb_cells_move(h, &p, bytes + bytes / 2, 0)) return -1;
    tmp = p;
    tmp_bytes = bytes + bytes / 2;
    return 0;
}

// ---- defined in the stores unit, the buffer unit (hb_check_maps .. hb_refresh_second_half) and the cells unit (hb_cellmatch_free)
int hb_cells_reserve_log(ll_history_batch *h, CbDev &m, long long need);
int hb_cells_reserve_mat(ll_history_batch *h, CbDev &m, size_t n);   // the materialise scratch at n entries
void hb_store_free(HbStore &st);
void hb_full_free(ll_history_batch *h);
int hb_cells_append(const char *where, ll_history_batch *h);
int hb_cells_materialise(const char *where, ll_history_batch *h);
int hb_cells_reader(const char *where, ll_history_batch *h, int32_t sequence, int32_t kind);
int hb_check_maps(const char *where, const ll_history_batch *h, ll_map *const *maps, const int32_t *active, bool *any);
void hb_sizes_out(const ll_history_batch *h, int64_t *n_map_corner, int64_t *n_map_surf);
int hb_refresh_second_half(const char *where, ll_history_batch *h, ll_map *const *maps, const int max_cat[2], const int cat_stride[2],
                           int64_t *n_map_corner, int64_t *n_map_surf);
// ---- defined in the scan-log unit
void hb_scan_log_free(ll_history_batch *h);
// where a block of the scan log lies
inline float4 *hb_scan_log_block(const ll_history_batch *h, int block)
{
    const int per = h->sl.book.chunk_blocks;
    return h->sl.chunks[(size_t)(block / per)] + (size_t)(block % per) * (size_t)h->max_pts;
}

#pragma GCC visibility pop
