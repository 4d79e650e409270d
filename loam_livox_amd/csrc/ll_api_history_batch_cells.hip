// ll_api_history_batch_cells.hip -- the cell-mode refresh of the batched match buffer (ll_history_batch_refresh_cells,
// ll_cellmatch_batch_kernels.hip).
#include "ll_api_history_batch_internal.h"

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
    return hb_reserve_tmp("ll_history_batch_refresh_cells", h, q.tmp, q.tmp_bytes, cmb_tmp_bytes, n_log);
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
        if (!cmb_leaf_fits(h->st[k].dev.geom, h->res[k]))
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
        run[k] = h->st[k].dev.n_log > 0 && h->st[k].dev.n_cells > 0;
        if (run[k] && hb_cellmatch_reserve(h, h->cq[k], h->st[k].dev.n_log, h->st[k].dev.n_cells)) return -1;
    }
    // ---- per kind: select, candidates, per-cell VoxelGrid, counts; one copy each, one drain for both
    int enq = 0, waits = 0;
    const char *err = nullptr;
    memset(h->hp_cq, 0, 2 * ((size_t)S + 4) * sizeof(int));
    HC(hipMemcpyAsync(h->d_cq_tab, h->hp_cq_tab, (size_t)S * sizeof(CmbSlot), hipMemcpyHostToDevice, h->stream));
    enq++;
    for (int k = 0; k < 2; k++) {
        if (!run[k]) continue;
        if (cmb_query(h->st[k].dev, h->cq[k], h->d_cq_tab, range[k], maximum_in_fov_angle, h->res[k], h->stream, &enq, &err)) return set_err(where, err);
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
        if (down_sample_replace && h->st[k].dev.n_log + n_leaves[k] >= kCbLimit) return set_err(where, "the cell maps would pass 2^31 stored points per kind");
    }
    if (down_sample_replace)
        for (int k = 0; k < 2; k++)
            if (n_leaves[k] > 0 && hb_cells_reserve_log(h, h->st[k].dev, h->st[k].dev.n_log + n_leaves[k])) return -1;
    const int cat_stride[2] = {max_cat[0] > 0 ? max_cat[0] : 1, max_cat[1] > 0 ? max_cat[1] : 1};
    // ---- the leaves into the concatenations (:496-512)
    HC(hipMemcpyAsync(h->d_ref, h->hp_ref, h->ref_seg_off, hipMemcpyHostToDevice, h->stream));
    HC(hipMemcpyAsync(h->d_mm, h->hp_mm_init, (size_t)2 * S * 8 * sizeof(unsigned int), hipMemcpyHostToDevice, h->stream));
    enq += 2;
    for (int k = 0; k < 2; k++)
        if (run[k] && cmb_scatter(h->st[k].dev, h->cq[k], n_leaves[k], h->d_concat + (size_t)k * S * h->cstride, cat_stride[k], h->stream, &enq, &err))
            return set_err(where, err);
    // The stores are still as they were: a second half that fails (an allocation, a size out of range) leaves no replace behind.
    if (hb_refresh_second_half(where, h, maps, max_cat, cat_stride, n_map_corner, n_map_surf)) return -1;
    waits += 2;
    // ---- the replace (:492-495), once the maps are published; the second half uses none of the chain's scratch
    for (int k = 0; k < 2; k++) {
        if (!run[k] || !down_sample_replace || n_leaves[k] <= 0) continue;
        if (cmb_replace(h->st[k].dev, h->cq[k], n_leaves[k], h->stream, &enq, &err)) return set_err(where, err);
        n_live[k] += n_leaves[k] - n_cand[k];
        h->cm_dirty = true;  // (dead entries in the log: a reader puts the stores in order first)
    }
    h->cq_work[0] = enq;
    h->cq_work[1] = waits;
    h->cq_work[7] = n_cand[0] + n_cand[1];
    for (int k = 0; k < 2; k++) {
        h->cq_work[3 + 2 * k] = h->st[k].dev.n_log;
        h->cq_work[4 + 2 * k] = run[k] ? n_live[k] : 0;
    }
    // ---- the handle puts the stores in order by itself once the dead entries outnumber the live ones
    if (h->cm_dirty && ((run[0] && cmb_compact_now(h->st[0].dev.n_log, n_live[0])) || (run[1] && cmb_compact_now(h->st[1].dev.n_log, n_live[1])))) {
        if (hb_cells_materialise(where, h)) return -1;
        h->cq_work[2]++;
        for (int k = 0; k < 2; k++) h->cq_work[3 + 2 * k] = h->cq_work[4 + 2 * k] = h->st[k].dev.n_log;
    }
    return 0;
}

// test tap of the cell-mode refresh (out[] as loam_livox_hip.h describes it, beside ll_history_batch_refresh_cells)
extern "C" int ll_history_batch_cell_match_work(ll_history_batch *h, int64_t out[8])
{
    static const char *where = "ll_history_batch_cell_match_work";
    if (!h || !out) return set_err(where, "null argument");
    if (!h->cm_on) return set_err(where, "cell maps are not enabled (ll_history_batch_enable_cell_maps)");
    for (int i = 0; i < 8; i++) out[i] = h->cq_work[i];
    return 0;
}
