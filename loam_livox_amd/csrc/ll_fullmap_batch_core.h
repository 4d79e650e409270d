// ll_fullmap_batch_core.h -- the per-point and per-cell decisions of the full-cloud maps of the batched match buffer
// (ll_history_batch_enable_full_maps): which points of a scan reach the store, which of them count for a cell, and how many a cell
// needs to be reported as touched.  Shared by the HIP kernels (ll_fullmap_batch_kernels.hip) and the test-only host builds
// (tests/fullmap_batch_host.cpp), like ll_cellmap_batch_core.h, whose rules the store itself follows.
//
// The touched cells are those of Points_cloud_map::append_cloud( pts, &cell_vec ) (cell_map_keyframe.hpp:596-607, 619-666): on a
// map without cells every cell the cloud opened, afterwards the cells that received at least min_points of THIS cloud's points.
#pragma once
#include "ll_cellmap_batch_core.h"

namespace ll {

// A scan point with a non-finite coordinate never reaches a cell (the single-sequence route drops it on the host before the
// transform): the gather marks it so that cb_point_key refuses it whatever the pose makes of the other coordinates.
LL_HD bool fb_point_ok(float x, float y, float z) { return ll_isfinite(x) && ll_isfinite(y) && ll_isfinite(z); }

// a logged point counts for its cell when the store kept it (a dropped point has no cell); a point that landed in a cell the same
// append reset counts like any other: the count is over the cloud, not over what the cell held before
LL_HD bool fb_point_counts(unsigned long long key) { return key != LL_CELL_KEY_NONE; }

// points of the cloud a cell needs to be listed: one on a map that had no cells at the call (set_point_cloud, CMK:596-607)
LL_HD int fb_need(bool was_empty, int min_points) { return was_empty ? 1 : min_points; }

LL_HD bool fb_touched(int count, int need) { return count >= need; }

// ---- host decisions of an append_full call, shared by the API and the test-only CPU driver
// one slot of an append_full call
struct FbSlot {
    double pose[7];  // {qx, qy, qz, qw, tx, ty, tz} of the scan
    int n;           // points of the slot's full selection (0 for an inactive slot)
    int active;
    int need;        // fb_need: points of this cloud a cell needs to be listed
    int pad;
};

// cb_fill_slots for the full-cloud store, and beside it the gather's and the touched chain's table: the slot's pose and the points a
// cell needs, from the cell counts at the call (coff, S + 1 host entries)
template <typename N>
inline long long fb_fill_slots(CbSlot *ctab, FbSlot *ftab, int S, N n_of, const int *frame, const int *coff, int min_points, const double *poses7,
                               long long n_log, int *max_n)
{
    const long long n_new = cb_fill_slots(ctab, S, n_of, frame, n_log, max_n);
    for (int s = 0; s < S; s++) {
        FbSlot &f = ftab[s];
        f = FbSlot{{0, 0, 0, 0, 0, 0, 0}, 0, 0, 0, 0};
        if (!ctab[s].active) continue;
        f.n = ctab[s].n;
        f.active = 1;
        f.need = fb_need(coff[s + 1] == coff[s], min_points);
        for (int i = 0; i < 7; i++) f.pose[i] = poses7[7 * (size_t)s + i];
    }
    return n_new;
}

}  // namespace ll
