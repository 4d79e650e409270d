// ll_cellmap_batch_extract_core.h -- the per-thread decisions of the batched cell extraction (ll_history_batch_extract_cells,
// ll_cellmap_batch_extract_kernels.hip): which request a list entry or an output position belongs to, whether a list entry can name
// a cell at all, what a hit writes, and how far behind its wavefront's first cell a lane's cell can lie.  Shared by the HIP kernels
// and the test-only host build (tests/cellmap_batch_extract_host.cpp).
#pragma once
#include "ll_cellmap_batch_core.h"

namespace ll {

// the last r of [lo, hi] with off[r] <= i (off ascending, off[lo] <= i).  With repeated offsets -- an empty list, a request that
// found nothing -- it is the last of the run: the one entry of the run that can hold i.
LL_HD int cxb_last_le(const int *off, int lo, int hi, int i)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// what cell_index refuses, cell_pack cannot represent: such an entry names no cell
LL_HD bool cxb_in_range(const int k[3])
{
    for (int d = 0; d < 3; d++)
        if (k[d] <= -LL_CELL_K_LIMIT || k[d] >= LL_CELL_K_LIMIT) return false;
    return true;
}

// The word a hit stores for its cell: one cell in the high half, its points in the low half.  A cell without points is not
// selected (0): the gather's bound below needs every selected cell to hold a point, and this keeps it from depending on what the
// store's chains promise.
LL_HD unsigned long long cxb_mark_word(int n_points_of_cell)
{
    return n_points_of_cell > 0 ? ((1ull << 32) | (unsigned long long)(unsigned int)n_points_of_cell) : 0ull;
}

LL_HD int cxb_rank(unsigned long long scanned) { return (int)(scanned >> 32); }
LL_HD int cxb_pos(unsigned long long scanned) { return (int)(unsigned int)scanned; }

// Every selected cell holds at least one point, so the cell of position i lies at most i - i0 selected cells behind the cell r0
// of an earlier position i0; n_found - 1 is the last cell there is.
LL_HD int cxb_far(int r0, int i, int i0, int n_found)
{
    const int far = r0 + (i - i0);
    return far < n_found - 1 ? far : n_found - 1;
}

}  // namespace ll
