// ll_cellmap_batch_extract_kernels.hip -- chosen cells of several slots of a deferred store (ll_cellmap_batch.h, in materialised order)
// copied into one destination cell map per request, in one chain for all requests (ll_history_batch_extract_cells): the key frames
// the lock-step sequences close in the same step, each a view of its own slot's full-cloud map.
//
// It is the mark / scan / table / gather chain of ll_cellmap_extract_kernels.hip with R requests in it.  A request names a slot, and a
// slot is named at most once, so the marks of different requests lie in disjoint ranges [coff[s], coff[s + 1]) of the ONE cell table;
// the device table of the requests is kept in ascending slot order, which is the order of the scan, so a request's cells and points
// are a contiguous piece of the scan's ranks and positions.
//   mark     one thread per entry of the concatenated lists: its request from the list offsets, range check, cell_pack, cb_find in
//            the slot's own table range (a cell index another slot holds is not found); a hit stores (1 << 32 | points of the cell).
//            Every writer of a cell stores the same word: no atomics;
//   scan     ONE exclusive sum over the n_cells + 1 words of the whole table (the store stays below 2^31 points and cells: the
//            halves never meet).  Rank and position of a cell are global; a request's are those minus the scanned word at coff[s];
//   totals   R + 1 threads: {cells found, points} per request and the R + 1 (rank, position) offsets -- what the host waits for;
//   table    one thread per table entry: a selected cell writes key, local first position and stamp 0 into its request's
//            destination, and its first SOURCE position (poff[s] + local first point) and first output position into scratch at its
//            global rank; one more thread per request closes the destination's offsets, one the scratch's;
//   gather   one lane per output position of the concatenation of all requests: key frames and cells are both badly skewed, so the
//            work is divided neither by request nor by cell.  A wavefront's first position finds its cell and request by searches
//            on the same addresses in every lane; each lane searches the few entries after it; 16 bytes of point and 8 bytes of
//            key go into the request's live arrays.  The key is copied, never recomputed.
// Nothing is sorted and nothing of the store is written: marks and scanned words live in the materialisation's key scratch (mkey,
// mkey2), the per-rank positions in its value scratch (mval, mval2).  The chain is cut at the host's wait (cxb_mark | totals, grow
// decisions | cxb_extract) so that the test-only host build drives the same launches (tests/cellmap_batch_extract_host.cpp).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "ll_cellmap_batch.h"
#include "ll_cellmap_batch_extract_core.h"

namespace ll {

typedef unsigned long long u64;
typedef unsigned int u32;

__global__ __launch_bounds__(256) void cxb_mark_kernel(const int *ijk, int n_list, const int *list_off, const int *seq, int n_req, const u64 *ckey,
                                                       const int *coff, const int *cstart, u64 *mark)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_list) return;
    const int s = seq[cxb_last_le(list_off, 0, n_req - 1, t)];
    int k[3];
    for (int d = 0; d < 3; d++) k[d] = ijk[3 * (size_t)t + d];
    if (!cxb_in_range(k)) return;
    const int c = cb_find(ckey, coff[s], coff[s + 1], cell_pack(k));
    if (c < 0) return;
    const u64 w = cxb_mark_word(cstart[c + s + 1] - cstart[c + s]);
    if (w) mark[c] = w;  // every writer stores the same word
}

// out: found [n_req], points [n_req], first rank [n_req + 1], first position [n_req + 1], the requests in ascending slot order
__global__ __launch_bounds__(256) void cxb_totals_kernel(const u64 *scanned, const int *coff, const int *qslot, int n_req, int n_cells, int *out)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q > n_req) return;
    int *found = out, *points = out + n_req, *qrank = out + 2 * (size_t)n_req, *qpos = qrank + n_req + 1;
    if (q == n_req) {
        qrank[q] = cxb_rank(scanned[n_cells]);
        qpos[q] = cxb_pos(scanned[n_cells]);
        return;
    }
    const int s = qslot[q];
    const u64 a = scanned[coff[s]], b = scanned[coff[s + 1]];
    found[q] = cxb_rank(b) - cxb_rank(a);
    points[q] = cxb_pos(b) - cxb_pos(a);
    qrank[q] = cxb_rank(a);
    qpos[q] = cxb_pos(a);
}

__global__ __launch_bounds__(256) void cxb_table_kernel(const u64 *mark, const u64 *scanned, const u64 *ckey, const int *cslot, const int *cstart,
                                                        const int *poff, int n_cells, const int *qslot, int n_req, const int *out, const CxbDst *dst,
                                                        int *src_first, int *gstart)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int *found = out, *points = out + n_req, *qrank = out + 2 * (size_t)n_req, *qpos = qrank + n_req + 1;
    if (t >= n_cells) {
        const int q = t - n_cells;
        if (q < n_req) {
            if (points[q] > 0) dst[q].cstart[found[q]] = points[q];  // cstart[n_found] = n_points
        } else if (q == n_req) {
            gstart[qrank[n_req]] = qpos[n_req];
        }
        return;
    }
    if (!mark[t]) return;
    const int s = cslot[t];
    const int q = cb_lower_bound_slot(qslot, n_req, s);  // (a marked cell's slot is a requested one)
    const int r = cxb_rank(scanned[t]), o = cxb_pos(scanned[t]);
    const CxbDst d = dst[q];
    const int lr = r - qrank[q];
    d.ckey[lr] = ckey[t];  // the key is copied, not recomputed from the coordinates
    d.cstart[lr] = o - qpos[q];
    d.clast[lr] = 0;
    src_first[r] = poff[s] + cstart[t + s];
    gstart[r] = o;
}

// gstart[0 .. n_found]: first output position of every selected cell, all requests in one ascending run.  The 64 lanes of a
// wavefront search for the wavefront's first position together, then each lane searches the entries cxb_far allows.
__global__ __launch_bounds__(256) void cxb_gather_kernel(const float4 *spts, const u64 *spkey, const int *src_first, const int *gstart, const int *out,
                                                         int n_req, int n_found, int n_points, const CxbDst *dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points) return;
    const int *qpos = out + 3 * (size_t)n_req + 1;
    const int i0 = i & ~63;
    const int r0 = cxb_last_le(gstart, 0, n_found - 1, i0);
    const int q0 = cxb_last_le(qpos, 0, n_req - 1, i0);
    const int r = cxb_last_le(gstart, r0, cxb_far(r0, i, i0, n_found), i);
    const int q = cxb_last_le(qpos, q0, n_req - 1, i);
    const int j = src_first[r] + (i - gstart[r]);
    const CxbDst d = dst[q];
    const int li = i - qpos[q];
    d.pts[li] = spts[j];
    d.pkey[li] = spkey[j];
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int cxb_tmp_bytes(int n_cells, size_t *bytes, const char **err)
{
    size_t need = 0;
    u64 *w = nullptr;
    CBCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, w, w, n_cells + 1));
    *bytes = need + 16;
    return 0;
}

int cxb_mark(CbDev &m, const int *d_in, int n_req, int n_list, int *d_out, hipStream_t s, int *launches, const char **err)
{
    const int nc = m.n_cells;
    if (n_req < 1 || n_req > m.S || n_list < 0 || (size_t)nc + 1 > m.mcap) {
        *err = "cell-map scratch too small for the extraction";
        return -1;
    }
    const CxbIn t = cxb_in(d_in, n_req);
    CBCHK(hipMemsetAsync(m.mkey, 0, (size_t)(nc + 1) * sizeof(u64), s));
    hipLaunchKernelGGL(cxb_mark_kernel, dim3(cb_blocks(n_list)), dim3(256), 0, s, t.ijk, n_list, t.list_off, t.seq, n_req, m.ckey, m.coff, m.cstart, m.mkey);
    size_t need = 0;
    CBCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, m.mkey, m.mkey2, nc + 1));
    if (need > m.tmp_bytes) {
        *err = "cell-map scratch too small for the scan";
        return -1;
    }
    size_t tb = m.tmp_bytes;
    CBCHK(hipcub::DeviceScan::ExclusiveSum(m.tmp, tb, m.mkey, m.mkey2, nc + 1, s));
    hipLaunchKernelGGL(cxb_totals_kernel, dim3(cb_blocks(n_req + 1)), dim3(256), 0, s, m.mkey2, m.coff, t.qslot, n_req, nc, d_out);
    CBCHK(hipGetLastError());
    *launches += 4;
    return 0;
}

int cxb_extract(CbDev &m, const int *d_in, int n_req, const int *d_out, const CxbDst *d_dst, int n_found, int n_points, hipStream_t s, int *launches,
                const char **err)
{
    if (n_found < 0 || n_found > m.n_cells || n_points < n_found || (long long)n_points > m.n_log) {
        *err = "cell selection out of range";
        return -1;
    }
    const int *qslot = cxb_in(d_in, n_req).qslot;
    hipLaunchKernelGGL(cxb_table_kernel, dim3(cb_blocks((long long)m.n_cells + n_req + 1)), dim3(256), 0, s, m.mkey, m.mkey2, m.ckey, m.cslot, m.cstart,
                       m.poff, m.n_cells, qslot, n_req, d_out, d_dst, m.mval, m.mval2);
    hipLaunchKernelGGL(cxb_gather_kernel, dim3(cb_blocks(n_points)), dim3(256), 0, s, m.pts, m.pkey, m.mval, m.mval2, d_out, n_req, n_found, n_points,
                       d_dst);
    CBCHK(hipGetLastError());
    *launches += 2;
    return 0;
}

}  // namespace ll
