// ll_cellmatch_batch_core.h -- the per-cell and per-point decisions of the cell-mode refresh of the batched match buffer
// (ll_history_batch_refresh_cells): which cells a slot's pose selects, which logged points are candidates of the per-cell VoxelGrid,
// the key that orders them, and what a replace does to a cell's epoch.  Shared by the HIP kernels (ll_cellmatch_batch_kernels.hip)
// and a test-only host build (tests/cellmatch_batch_host.cpp).
//
// Per slot the rules are cellmap_query_filter's (ll_cellmap_kernels.hip; Laser_mapping::update_buff_for_matching with
// m_matching_mode == 1, laser_mapping.hpp:471-513).  What differs is the store they read: the deferred store of
// ll_cellmap_batch_core.h, in which a point counts while its epoch is its cell's, and in which a replaced cell is given a new epoch
// instead of having its points removed.
#pragma once
#include "ll_cellmap_batch_core.h"

namespace ll {

// one slot of a cell-mode refresh
struct CmbSlot {
    double pose[7];  // (x, y, z, w), t: the pose the cells are selected around
    int active;
    int pad;
};

// find_cells_in_radius + if_pt_in_fov on the cell's centre (laser_mapping.hpp:475-486), as cm_select_kernel decides them
LL_HD bool cmb_cell_selected(unsigned long long cell_key, const CellGeom &g, const CmbSlot &slot, float radius, double max_fov_deg)
{
    if (!slot.active) return false;
    int k[3];
    cell_unpack(cell_key, k);
    float ctr[3];
    cell_centre(k, g, ctr);
    const double q[4] = {slot.pose[0], slot.pose[1], slot.pose[2], slot.pose[3]}, t[3] = {slot.pose[4], slot.pose[5], slot.pose[6]};
    const float sp[3] = {(float)t[0], (float)t[1], (float)t[2]};  // eigen_to_pcl_pt<pcl::PointXYZ>( m_t_w_curr )
    return cell_in_radius(ctr, sp, radius) && cell_in_fov(ctr, q, t, max_fov_deg);
}

// The table entry of a logged point's cell when the point is alive, -1 otherwise.  [first, last) is the range of the point's slot in
// the table: the search never leaves it.
LL_HD int cmb_live_cell(unsigned long long point_key, int point_epoch, const unsigned long long *ckey, const int *cep, int first, int last)
{
    if (point_key == LL_CELL_KEY_NONE) return -1;
    const int c = cb_find(ckey, first, last, point_key);
    return (c >= 0 && cb_live(point_epoch, cep[c])) ? c : -1;
}

// Sort key of the per-cell VoxelGrid: (table entry of the cell) << 30 | leaf z << 20 | leaf y << 10 | leaf x.  The table is ordered by
// (slot, cell key), so ascending keys are slot order, then cell order, then PCL's leaf order inside the cell (cm_leaf_key_kernel).
LL_HD unsigned long long cmb_leaf_key(int table_entry, unsigned long long cell_key, float x, float y, float z, const CellGeom &g, float inv_leaf)
{
    int k[3];
    cell_unpack(cell_key, k);
    int l[3] = {cell_leaf_local(x, k[0], g, inv_leaf), cell_leaf_local(y, k[1], g, inv_leaf), cell_leaf_local(z, k[2], g, inv_leaf)};
    for (int d = 0; d < 3; d++) l[d] = l[d] < 0 ? 0 : (l[d] > 1023 ? 1023 : l[d]);
    return ((unsigned long long)(unsigned)table_entry << 30) | ((unsigned long long)l[2] << 20) | ((unsigned long long)l[1] << 10) | (unsigned long long)l[0];
}
LL_HD int cmb_key_cell(unsigned long long leaf_key) { return (int)(leaf_key >> 30); }
// the key that sorts behind the leaves of every cell of a table of n_cells entries (the padding of the sort)
LL_HD unsigned long long cmb_key_none(int n_cells) { return (unsigned long long)(unsigned)n_cells << 30; }
// the leaf is too small for the cell: more than 1020 leaves across one cell do not fit the 10 bits of an axis
LL_HD bool cmb_leaf_fits(const CellGeom &g, float leaf) { return leaf > 0.f && cell_leaf_span(g, 1.0f / leaf) < 1024.0f; }

// down_sample_replace (laser_mapping.hpp:492-495): the points of a selected cell go, its leaves come in -- the cell starts a new
// epoch, exactly as when the revisit rule resets it, and the leaves are logged under that epoch.  The last-update stamp stays.
LL_HD int cmb_epoch_after_replace(int epoch) { return cb_epoch_after_reset(epoch); }

// The handle puts the store in order by itself when the dead entries outnumber the live ones; with `step` entries coming in between
// two decisions this keeps  log <= 2 * live + step.
LL_HD bool cmb_compact_now(long long n_log, long long n_live) { return n_log - n_live > n_live; }

}  // namespace ll
