// ll_cellmap_batch.h -- device side of the cell maps of the batched match buffer (ll_history_batch_enable_cell_maps,
// ll_cellmap_batch_kernels.hip).  One CbDev per kind (corner, surface) holds the maps of all S slots:
//   the log      points in arrival order: {x, y, z, 0}, cell key, slot, and the epoch of the point's cell when it went in.  Its
//                first n_store entries are the store the last materialisation left, ordered by (slot, cell key, insertion).
//   the table    the occupied cells of all slots, ordered by (slot, cell key): key, slot, last-update stamp, epoch;
//                slot s owns [coff[s], coff[s + 1]).
// An append classifies the new points, stamps and resets the cells they hit, merges the new cells into the table and writes the
// points behind the log: work for the new points and the table, none for the stored points.  A materialisation drops the dead
// points, orders the rest and rebuilds what a reader of one slot needs (poff, cstart).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ll_cellmap_batch_core.h"

namespace ll {

struct CbDev {
    int S;
    CellGeom geom;
    int threshold;
    // log (cap entries each; the *2 arrays are the targets of the next materialisation)
    float4 *pts, *pts2;
    unsigned long long *pkey, *pkey2;
    int *pslot, *pslot2, *pep, *pep2;
    size_t cap;
    long long n_log;
    // cell table (ccap entries each; the *2 arrays are the targets of the next merge)
    unsigned long long *ckey, *ckey2;
    int *cslot, *cslot2, *clast, *clast2, *cep, *cep2;
    size_t ccap;
    int n_cells;
    int *coff, *coff2;  // [S + 1]
    int *poff;          // [S + 1] first point of every slot in the materialised store
    int *cstart;        // [ccap + S + 1]: slot s's n_cells(s) + 1 local first-point indices start at coff[s] + s
    // scratch of an append (acap entries)
    unsigned long long *akey, *akey2;
    int *aslot, *aslot2;
    unsigned int *aflag, *arank;
    size_t acap;
    // scratch of a materialisation (mcap entries)
    unsigned long long *mkey, *mkey2;
    int *mval, *mval2, *mslot, *mslot2;
    size_t mcap;
    void *tmp;
    size_t tmp_bytes;
    int *counts;  // [4]: new cells of the last append, cells after it
    CbSlot *tab;  // [S]
};

// what the host halves of the units built on this store share: *err (which has to be in scope) and -1 on a HIP error; the blocks of
// 256 threads for n items.  ll_history_batch_kernels.hip and ll_cellmap_extract_kernels.hip do not include this header and keep theirs.
#define CBCHK(x)                              \
    do {                                      \
        hipError_t e_ = (x);                  \
        if (e_ != hipSuccess) {               \
            *err = hipGetErrorString(e_);     \
            return -1;                        \
        }                                     \
    } while (0)
static inline unsigned int cb_blocks(long long n) { return (unsigned int)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

// ---- the arrays of a CbDev, named once per capacity group.  f(array, entries, keep) returns non-zero to stop; `keep` marks the
// arrays whose content has to survive a move (the *2 targets and all scratch are rewritten before they are read).  Whoever sizes a
// group sets its capacity after every array of it has gone through.
template <typename F> static inline int cb_each_log(CbDev &m, size_t n, F f)  // cap
{
    return f(m.pts, n, true) || f(m.pkey, n, true) || f(m.pslot, n, true) || f(m.pep, n, true) || f(m.pts2, n, false) || f(m.pkey2, n, false) ||
           f(m.pslot2, n, false) || f(m.pep2, n, false);
}
template <typename F> static inline int cb_each_table(CbDev &m, size_t n, F f)  // ccap
{
    return f(m.ckey, n, true) || f(m.cslot, n, true) || f(m.clast, n, true) || f(m.cep, n, true) || f(m.ckey2, n, false) || f(m.cslot2, n, false) ||
           f(m.clast2, n, false) || f(m.cep2, n, false) || f(m.cstart, n + (size_t)m.S + 1, false);
}
template <typename F> static inline int cb_each_append(CbDev &m, size_t n, F f)  // acap
{
    return f(m.akey, n, false) || f(m.akey2, n, false) || f(m.aslot, n, false) || f(m.aslot2, n, false) || f(m.aflag, n, false) || f(m.arank, n, false);
}
template <typename F> static inline int cb_each_mat(CbDev &m, size_t n, F f)  // mcap
{
    return f(m.mkey, n, false) || f(m.mkey2, n, false) || f(m.mval, n, false) || f(m.mval2, n, false) || f(m.mslot, n, false) || f(m.mslot2, n, false);
}
template <typename F> static inline int cb_each_fixed(CbDev &m, F f)  // sized by S alone
{
    return f(m.coff, (size_t)m.S + 1, false) || f(m.coff2, (size_t)m.S + 1, false) || f(m.poff, (size_t)m.S + 1, false) || f(m.counts, (size_t)4, false) ||
           f(m.tab, (size_t)m.S, false);
}
// temporary storage the hipcub calls of an append of n_new points / a materialisation of n_log points need
int cb_tmp_bytes(long long n, size_t *bytes, const char **err);
// The append chain of one kind: src [S][src_stride] holds the slots' clouds, m.tab (already on the device) their sizes, log offsets
// and frame counters; max_n bounds tab[s].n and n_new is their sum over the active slots.  Needs n_log + n_new <= cap,
// n_cells + n_new <= ccap, n_new <= acap.  Swaps the table arrays; the new cell count is in counts[1], the new coff on the device.
// *launches += kernel launches and library calls enqueued.
int cb_append(CbDev &m, const float4 *src, int src_stride, int max_n, long long n_new, hipStream_t s, int *launches, const char **err);
// The materialise chain of one kind over the n_log logged points (needs n_log <= mcap): swaps the log arrays; the ordered store's
// size is poff[S] on the device.
int cb_materialise(CbDev &m, hipStream_t s, int *launches, const char **err);

// ---- chosen cells of several slots into one cell map each (ll_cellmap_batch_extract_kernels.hip) -------------------------------
// where one request's cells and points go: the live arrays of its destination cell map
struct CxbDst {
    unsigned long long *ckey;
    int *cstart, *clast;
    float4 *pts;
    unsigned long long *pkey;
};
// temporary storage the scan over n_cells + 1 words needs
int cxb_tmp_bytes(int n_cells, size_t *bytes, const char **err);
// First half, over a store in materialised order (m.n_log = its points; needs n_cells + 1 <= mcap and cxb_tmp_bytes <= tmp_bytes).
// d_in and d_out are device ints in the layouts ll_cellmap_batch_extract_core.h names (cxb_stage, cxb_out).  Writes mkey, mkey2, tmp.
int cxb_mark(CbDev &m, const int *d_in, int n_req, int n_list, int *d_out, hipStream_t s, int *launches, const char **err);
// Second half, with d_out read back and every destination large enough: d_dst [n_req] in ascending slot order; n_found and n_points
// are the totals over all requests.  Writes mval, mval2 and the destinations' arrays; nothing of the store.
int cxb_extract(CbDev &m, const int *d_in, int n_req, const int *d_out, const CxbDst *d_dst, int n_found, int n_points, hipStream_t s, int *launches,
                const char **err);

}  // namespace ll
