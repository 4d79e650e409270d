// ll_cellmatch_batch.h -- device side of the cell-mode refresh of the batched match buffer (ll_history_batch_refresh_cells,
// ll_cellmatch_batch_kernels.hip): per kind one chain over the deferred store of ll_cellmap_batch.h that selects the cells around
// every slot's pose, passes each selected cell through the VoxelGrid and, with down_sample_replace, writes the leaves back.  The chain
// reads the log once and sorts the candidates' (key, position) pairs, padded to the log's length; it never moves a stored point.
#pragma once
#include "ll_cellmap_batch.h"
#include "ll_cellmatch_batch_core.h"

namespace ll {

// scratch and results of one kind (ncap entries where a log entry is meant, ccap where a table entry is)
struct CmbDev {
    unsigned int *csel;                   // [ccap] 1: the cell is selected
    unsigned long long *cflag, *crank;    // [ncap] per log entry: candidate (low word) and alive (high word); their exclusive sums
    int *ccell;                           // [ncap] table entry of a candidate's cell
    unsigned long long *key, *key2;       // [ncap] leaf keys of the compacted candidates, padded with cmb_key_none; sorted
    int *val, *val2;                      // [ncap] their log positions
    unsigned int *hflag, *hrank;          // [ncap] first point of a leaf in the sorted order; exclusive sum = the leaf's number
    int *head;                            // [ncap] sorted position of every leaf's first point
    float4 *leaf;                         // [ncap] the leaves, ordered by (slot, cell, leaf)
    int *leaf_cell;                       // [ncap] table entry of every leaf's cell
    int *out;                             // [S + 4] first leaf of every slot, closing entry = leaves; then candidates, live entries
    size_t ncap, ccap;
    void *tmp;
    size_t tmp_bytes;
};

int cmb_tmp_bytes(long long n, size_t *bytes, const char **err);
// Select, candidates, per-cell VoxelGrid and counts of one kind over the n_log logged points of m (needs n_log <= q.ncap,
// n_cells <= q.ccap, 0 < n_log, 0 < n_cells).  d_tab [S]: the slots' poses and activity.  Leaves q.leaf / q.leaf_cell and q.out on
// the device; changes nothing in m.
int cmb_query(const CbDev &m, CmbDev &q, const CmbSlot *d_tab, float radius, float max_fov_deg, float leaf, hipStream_t s, int *launches,
              const char **err);
// the leaves of every slot into the concatenation buffer [S][stride] of the kind
int cmb_scatter(const CbDev &m, const CmbDev &q, int n_leaves, float4 *concat, int stride, hipStream_t s, int *launches, const char **err);
// down_sample_replace: a new epoch for every selected cell, its leaves behind the log under it (needs n_log + n_leaves <= cap)
int cmb_replace(CbDev &m, const CmbDev &q, int n_leaves, hipStream_t s, int *launches, const char **err);

}  // namespace ll
