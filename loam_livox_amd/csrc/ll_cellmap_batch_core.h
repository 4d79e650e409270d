// ll_cellmap_batch_core.h -- the per-point and per-cell decisions of the batched cell maps (ll_history_batch_enable_cell_maps):
// which cell a point falls in, when a hit resets a cell, what a reset does to the cell's epoch, and which logged points are still
// alive.  Shared by the HIP kernels (ll_cellmap_batch_kernels.hip) and a test-only host build (tests/cellmap_batch_host.cpp), so the
// deferred store can be run on the CPU against the oracle's cell map.
//
// Per map the rules are cellmap_append's (ll_cellmap_kernels.hip; Points_cloud_map::append_cloud, cell_map_keyframe.hpp:619-672,
// 716-759).  What differs is WHEN the work is done: the revisit rule needs the map's frame counter, so it is decided when the
// cloud arrives; the order of the store is not needed until somebody reads it.  A reset therefore does not touch the stored
// points: it gives the cell a new epoch, and a logged point counts for as long as the epoch it was inserted under is its cell's.
#pragma once
#include "ll_cellmap_core.h"

namespace ll {

// the packed cell key of a point, LL_CELL_KEY_NONE for a point the map drops (non-finite, or beyond +-2^20 cells)
LL_HD unsigned long long cb_point_key(float x, float y, float z, const CellGeom &g)
{
    int k[3];
    if (!(ll_isfinite(x) && ll_isfinite(y) && ll_isfinite(z)) || !cell_index(x, y, z, g, k)) return LL_CELL_KEY_NONE;
    return cell_pack(k);
}

// CMK:737 fails: the cell was last updated `threshold` or more appends ago
LL_HD bool cb_stale(int frame, int clast, int threshold) { return !(frame - clast < threshold); }

// Every point of a cloud that hits a cell stamps it with the cloud's frame.  The one that finds an older stamp is the cloud's first
// hit on that cell (stamps of earlier clouds are smaller: the counter moves with every append) and decides about the reset.
LL_HD bool cb_first_touch(int clast_before, int frame) { return clast_before != frame; }

// a reset cell starts a new epoch; a new cell starts at 0
LL_HD int cb_epoch_after_reset(int epoch) { return epoch + 1; }

// a logged point is part of the map while its epoch is its cell's
LL_HD bool cb_live(int point_epoch, int cell_epoch) { return point_epoch == cell_epoch; }

// m_current_frame_idx++ (CMK:667), and once more when the map had no cells at the call (set_point_cloud, CMK:615)
LL_HD int cb_frame_step(bool was_empty) { return was_empty ? 2 : 1; }

// order of the cell tables and of the materialised store: by slot, then by cell key
LL_HD bool cb_less(int slot_a, unsigned long long key_a, int slot_b, unsigned long long key_b)
{
    return slot_a < slot_b || (slot_a == slot_b && key_a < key_b);
}

// first position in [lo, hi) of the ascending keys that is not below k
LL_HD int cb_lower_bound(const unsigned long long *keys, int lo, int hi, unsigned long long k)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// the same over [0, n) of a (slot, key) ordered pair of arrays
LL_HD int cb_lower_bound_pair(const int *slots, const unsigned long long *keys, int n, int slot, unsigned long long k)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cb_less(slots[mid], keys[mid], slot, k))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// ... and of the slots alone
LL_HD int cb_lower_bound_slot(const int *slots, int n, int slot)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (slots[mid] < slot)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// the cell of (slot, key) in a table whose slot `slot` owns [first, last), or -1
LL_HD int cb_find(const unsigned long long *ckey, int first, int last, unsigned long long k)
{
    const int p = cb_lower_bound(ckey, first, last, k);
    return (p < last && ckey[p] == k) ? p : -1;
}

// ---- host decisions of an append, shared by the API (ll_api_history_batch_stores.hip) and the test-only CPU drivers (tests/cellmap_batch_rig.h)
// one slot of an append
struct CbSlot {
    long long off;  // first log position of the slot's points
    int n;          // its points in the source stack
    int frame;      // the map's frame counter at the call
    int active;
    int pad;
};

// The slot table of an append: the working slots' clouds behind the n_log logged points, in slot order.  n_of(s): the slot's points,
// negative for a slot that sits the call out.  Returns the new points; *max_n: the largest cloud.
template <typename N>
inline long long cb_fill_slots(CbSlot *tab, int S, N n_of, const int *frame, long long n_log, int *max_n)
{
    long long n_new = 0;
    *max_n = 0;
    for (int s = 0; s < S; s++) {
        tab[s] = CbSlot{0, 0, 0, 0, 0};
        const int n = n_of(s);
        if (n < 0) continue;
        tab[s].off = n_log + n_new;
        tab[s].n = n;
        tab[s].frame = frame[s];
        tab[s].active = 1;
        n_new += n;
        *max_n = n > *max_n ? n : *max_n;
    }
    return n_new;
}

// After an append: the cell counts at the call (coff, S + 1 host entries) decide the step of every working slot's frame counter;
// then coff takes the offsets the chain left (new_coff; null when nothing was appended).
template <typename W>
inline void cb_after_append(int *frame, int *coff, int S, W worked, const int *new_coff)
{
    for (int s = 0; s < S; s++)
        if (worked(s)) frame[s] += cb_frame_step(coff[s + 1] == coff[s]);
    for (int s = 0; new_coff && s <= S; s++) coff[s] = new_coff[s];
}

}  // namespace ll
