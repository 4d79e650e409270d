// ll_cellmap_batch_extract_core.h -- the per-thread decisions of the batched cell extraction (ll_history_batch_extract_cells,
// ll_cellmap_batch_extract_kernels.hip): which request a list entry or an output position belongs to, whether a list entry can name
// a cell at all, what a hit writes, and how far behind its wavefront's first cell a lane's cell can lie.  Shared by the HIP kernels
// and the test-only host build (tests/cellmap_batch_extract_host.cpp).
#pragma once
#include <string.h>

#include <algorithm>

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

// ---- the two tables of a call, both ints, and their staging on the host (the API and the test-only CPU driver)
// d_in : list_off [R + 1] and seq [R] in the caller's order | qslot [R], the requested slots ascending | ijk, n_list x {i, j, k}
// d_out: found [R] | points [R] | qrank [R + 1] first global rank | qpos [R + 1] first global output position; ascending slot order
struct CxbIn { const int *list_off, *seq, *qslot, *ijk; };
struct CxbOut { const int *found, *points, *qrank, *qpos; };
inline size_t cxb_in_ints(int R, long long n_list) { return (size_t)3 * R + 1 + (size_t)3 * n_list; }
inline size_t cxb_out_ints(int R) { return (size_t)4 * R + 2; }
inline CxbIn cxb_in(const int *in, int R) { return CxbIn{in, in + R + 1, in + 2 * (size_t)R + 1, in + 3 * (size_t)R + 1}; }
inline CxbOut cxb_out(const int *out, int R) { return CxbOut{out, out + R, out + 2 * (size_t)R, out + 3 * (size_t)R + 1}; }

// Stages R requests into `in` (cxb_in_ints entries): the list offsets made relative to the first, the slots, the slots again in
// ascending order -- the order of the table, and so of the scan -- and the lists.  order[q]: the request that is q-th in that order.
template <typename Off>
static inline void cxb_stage(int *in, int *order, int R, const int *seq, const Off *list_off, const int *ijk)
{
    for (int r = 0; r < R; r++) order[r] = r;
    std::sort(order, order + R, [&](int a, int b) { return seq[a] < seq[b]; });
    const int n_list = (int)(list_off[R] - list_off[0]);
    for (int r = 0; r <= R; r++) in[r] = (int)(list_off[r] - list_off[0]);
    for (int r = 0; r < R; r++) in[R + 1 + r] = seq[r];
    for (int q = 0; q < R; q++) in[2 * R + 1 + q] = seq[order[q]];
    if (n_list > 0) memcpy(in + 3 * R + 1, ijk + 3 * (size_t)list_off[0], (size_t)3 * n_list * sizeof(int));
}

}  // namespace ll
