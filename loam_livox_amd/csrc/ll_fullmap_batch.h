// ll_fullmap_batch.h -- device side of the full-cloud maps of the batched match buffer (ll_history_batch_enable_full_maps,
// ll_fullmap_batch_kernels.hip): m_pt_cell_map_full of S lock-step sequences (laser_mapping.hpp:1442, 1527) in a third deferred
// store.  The store is a CbDev and is appended to by cb_append as it stands (ll_cellmap_batch.h); what is added here is
//   the gather   the extractor's full selection of every active slot, moved into the map frame with the slot's pose, as the
//                [S][max_points_per_frame] stack cb_append reads;
//   the touched  the cells that received enough of THIS cloud's points (append_cloud( pts, &cell_vec )), ordered by (slot, cell
//                key), as {i, j, k} triples with per-slot offsets.
// Neither reads, sorts or moves a stored point: the gather works on the scan, the touched chain on the step's new log entries
// (their keys and slots) and on the cell table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ll_cellmap_batch.h"
#include "ll_fullmap_batch_core.h"

namespace ll {

struct FbDev {
    float4 *xf;  // [S][max_points_per_frame] the gathered clouds in the map frame
    FbSlot *tab;  // [S]
    // scratch of the touched chain, one entry per cell-table entry (tcap, kept at the store's ccap)
    int *cnt;
    unsigned int *flag, *rank;
    int *cells;  // [tcap][3] the touched cells of the last call
    size_t tcap;
    int *toff;  // [S + 1] first touched cell of every slot
    void *tmp;
    size_t tmp_bytes;
};

int fb_tmp_bytes(long long n, size_t *bytes, const char **err);
// The full selections of the active slots into t.xf: slot s reads xyzi[s][full_idx[s][i]], i < t.tab[s].n (t.tab is on the device;
// max_n bounds the n).  An index outside [0, stride) or a non-finite point leaves a point the store drops.
int fb_gather(const FbDev &t, const float4 *xyzi, const int *full_idx, int stride, int S, int max_pts, int max_n, hipStream_t s, int *launches,
              const char **err);
// The touched cells of the append that cb_append has just enqueued on m (table swapped; m.tab and t.tab on the device; the step's
// points are the tab[s].n log entries from tab[s].off).  n_upper bounds the table after the merge (cells before + new points) and
// must not exceed t.tcap: the merged cell count itself is read on the device (m.counts[1]), so the host need not wait for it.
int fb_touched_chain(const CbDev &m, FbDev &t, int max_n, int n_upper, hipStream_t s, int *launches, const char **err);

}  // namespace ll
