// ll_cellmap_select_core.h -- device-independent bodies of the feature-cloud selection (ll_cellmap_select_kernels.hip): the word a cell
// contributes to the scan, and the search that finds the cell of a stored point.  Host and device compile the same text
// (tests/cellmap_feature_clouds_host.cpp).
#pragma once
#include "ll_cellmap_core.h"

namespace ll {

#define LL_FEATURE_LINE 1   // Feature_type e_feature_line  (cell_map_keyframe.hpp:46-51)
#define LL_FEATURE_PLANE 2  // Feature_type e_feature_plane

// What a cell of `n_points` points and feature type `type` adds to the two running sums: its points to the low half for a line cell, to
// the high half for a plane cell, nothing for a sphere.  A map holds fewer than 2^30 points, so neither half carries into the other.
LL_HD unsigned long long select_word(int type, int n_points)
{
    if (type == LL_FEATURE_LINE) return (unsigned long long)(unsigned int)n_points;
    if (type == LL_FEATURE_PLANE) return (unsigned long long)(unsigned int)n_points << 32;
    return 0ull;
}

// the last c of [lo, hi] with cstart[c] <= i (cstart ascending, cstart[lo] <= i)
LL_HD int select_last_le(const int *cstart, int lo, int hi, int i)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cstart[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The cell of stored point i.  A cell holds at least one point, so it lies at most i - i0 table entries behind the cell of an earlier
// point i0: the lanes of a wavefront search for the wavefront's first point together (the same addresses in every lane), then each
// lane searches the few entries after it.
LL_HD int select_cell_of(const int *cstart, int n_cells, int i)
{
    const int i0 = i & ~63;
    const int c0 = select_last_le(cstart, 0, n_cells - 1, i0);
    const int far = c0 + (i - i0);
    return select_last_le(cstart, c0, far < n_cells - 1 ? far : n_cells - 1, i);
}

}  // namespace ll
