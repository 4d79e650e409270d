// ll_api_history_batch_extract.hip -- ll_history_batch_extract_cells: chosen cells of several slots of a deferred store into one cell
// map each, where they lie (ll_cellmap_batch_extract_kernels.hip).
#include "ll_api_history_batch_internal.h"

// the staging of a call and the scratch of its chain (the stream is idle: the store has just been put in order)
static int hb_extract_reserve(const char *where, ll_history_batch *h, CbDev &m, size_t n_in)
{
    const size_t S = (size_t)h->S;
    if (!h->hp_cx_out) HC(hipHostMalloc((void **)&h->hp_cx_out, cxb_out_ints(h->S) * sizeof(int), hipHostMallocDefault));
    if (!h->hp_cx_dst) HC(hipHostMalloc((void **)&h->hp_cx_dst, S * sizeof(CxbDst), hipHostMallocDefault));
    if (!h->d_cx_out) DM(h->d_cx_out, cxb_out_ints(h->S));
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
    // (a store that was never materialised, or one whose every point opened a cell)
    if (m.mcap < (size_t)m.n_cells + 1 && hb_cells_reserve_mat(h, m, m.cap > (size_t)m.n_cells + 1 ? m.cap : (size_t)m.n_cells + 1)) return -1;
    return hb_reserve_tmp(where, h, m.tmp, m.tmp_bytes, cxb_tmp_bytes, m.n_cells);
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
        if (d->dev.resolution != h->st[kind].res) return set_err(where, "a destination has another resolution than the store");
    }
    HC(hipSetDevice(h->device));
    const int64_t mats = kind == 2 ? h->fm_work[3] : h->cm_work[2];
    if (hb_cells_reader(where, h, sequences[0], kind)) return -1;  // at most one materialisation, with its own wait
    h->cx_work[3] += (kind == 2 ? h->fm_work[3] : h->cm_work[2]) - mats;
    HbStore &st = h->st[kind];
    CbDev &m = st.dev;
    const int n_list = (int)n_list64;
    const size_t n_in = cxb_in_ints(R, n_list);
    if (hb_extract_reserve(where, h, m, n_in)) return -1;
    std::vector<int> order((size_t)R);
    int *in = h->hp_cx_in;
    cxb_stage(in, order.data(), R, sequences, list_offsets, cell_ijk);
    int enq = 0, waits = 0;
    const char *err = nullptr;
    HC(hipMemcpyAsync(h->d_cx_in, in, n_in * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (cxb_mark(m, h->d_cx_in, R, n_list, h->d_cx_out, h->stream, &enq, &err)) return set_err(where, err);
    HC(hipMemcpyAsync(h->hp_cx_out, h->d_cx_out, cxb_out_ints(R) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    enq += 2;
    HC(hipStreamSynchronize(h->stream));  // the only wait before points move
    waits++;
    const CxbOut o = cxb_out(h->hp_cx_out, R);
    const int *found = o.found, *points = o.points, n_found = o.qrank[R], n_pts = o.qpos[R];
    for (int q = 0; q < R; q++) {
        const int s = sequences[order[q]];
        if (found[q] < 0 || points[q] < found[q] || found[q] > st.coff[s + 1] - st.coff[s] ||
            points[q] > st.poff[s + 1] - st.poff[s] || points[q] >= 0x3fffffff)
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

// test tap of the extraction (out[] as loam_livox_hip.h describes it)
extern "C" int ll_history_batch_extract_work(ll_history_batch *h, int64_t out[4])
{
    static const char *where = "ll_history_batch_extract_work";
    if (!h || !out) return set_err(where, "null argument");
    if (!h->cm_on && !h->fm_on) return set_err(where, "neither cell maps nor full maps are enabled");
    for (int i = 0; i < 4; i++) out[i] = h->cx_work[i];
    return 0;
}
