// ll_cellmap_extract_kernels.hip -- a chosen set of cells of one cell map copied into another on the device: a key frame's view of
// the shared cells (Maps_keyframe holds pointers to the map's cells and reads them as they are now,
// source/cell_map_keyframe.hpp:1243-1261).
//
// The source is ordered by (cell key, insertion order) and so is the result: nothing is sorted.
//   mark     one thread per list entry: range check, cell_pack, binary search of the source table; a hit stores the word
//            (1 << 32 | points of the cell) for its cell.  Every writer of a cell stores the same word: a cell named twice is marked
//            once, and no atomics are needed;
//   scan     ONE exclusive sum of those 64-bit words over n_cells + 1 entries: the high half of entry c is the rank of cell c among
//            the selected, the low half its first output position, and entry n_cells holds {cells found, points} -- the 8 bytes the
//            host reads before it sizes the destination (the sums stay below 2^31 each, so the halves never carry into each other);
//   table    one thread per source cell: a selected cell writes its key, first position and stamp 0 into the destination table and
//            the first SOURCE position of its points into a scratch array indexed by rank;
//   gather   one lane per output position, 16 bytes of point and 8 bytes of key each.  Cell sizes are badly skewed (thousands of
//            points in a wall cell, one in a stray cell), so the work is divided by position, not by cell: a lane finds its cell in
//            the destination's offsets, and consecutive lanes read and write consecutive addresses inside a cell run.
// The chain is cut where the host has to wait (cellmap_extract_mark | the totals, the grow decision | cellmap_extract_cells), so
// that the test-only host build drives the same launches (tests/cellmap_extract_host.cpp).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "ll_cellmap.h"

namespace ll {

typedef unsigned long long u64;
typedef unsigned int u32;

#define CXCHK(x)                              \
    do {                                      \
        hipError_t e_ = (x);                  \
        if (e_ != hipSuccess) {               \
            *err = hipGetErrorString(e_);     \
            return -1;                        \
        }                                     \
    } while (0)

static inline unsigned int cx_blocks(int n) { return (unsigned int)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

// position of `k` in the ascending table ckey[0 .. n), or -1
__device__ __forceinline__ int cx_find(const u64 *ckey, int n, u64 k)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ckey[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < n && ckey[lo] == k) ? lo : -1;
}

// the last r of [lo, hi] with off[r] <= i (off ascending, off[lo] <= i)
__device__ __forceinline__ int cx_last_le(const int *off, int lo, int hi, int i)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void cx_mark_kernel(const int *ijk, int n_list, const u64 *ckey, const int *cstart, int n_cells, u64 *mark)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_list) return;
    int k[3];
    for (int d = 0; d < 3; d++) {
        k[d] = ijk[3 * (size_t)t + d];
        if (k[d] <= -LL_CELL_K_LIMIT || k[d] >= LL_CELL_K_LIMIT) return;  // what cell_index refuses: cell_pack cannot represent it
    }
    const int c = cx_find(ckey, n_cells, cell_pack(k));
    if (c >= 0) mark[c] = (1ull << 32) | (u64)(u32)(cstart[c + 1] - cstart[c]);  // every writer stores the same word
}

__global__ __launch_bounds__(256) void cx_table_kernel(const u64 *mark, const u64 *pos, const u64 *ckey, const int *cstart, int n_cells, u64 *dkey,
                                                       int *dstart, int *dlast, int *src_first)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c > n_cells) return;
    const u64 p = pos[c];
    const int r = (int)(p >> 32), o = (int)(u32)p;
    if (c == n_cells) {
        dstart[r] = o;  // cstart[n_found] = n_points
        return;
    }
    if (!mark[c]) return;
    dkey[r] = ckey[c];  // the key is copied, not recomputed from the coordinates
    dstart[r] = o;
    dlast[r] = 0;
    src_first[r] = cstart[c];
}

// dstart[0 .. n_found]: first output position of each selected cell.  A cell of the table holds at least one point, so the cell of
// position i lies at most i - i0 table entries behind the cell of an earlier position i0: the 64 lanes of a wavefront search for
// the wavefront's first position together (the same addresses in every lane), then each lane searches the few entries after it.
__global__ __launch_bounds__(256) void cx_gather_kernel(const float4 *spts, const u64 *spkey, const int *src_first, const int *dstart, int n_found,
                                                        int n_points, float4 *dpts, u64 *dpkey)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points) return;
    const int i0 = i & ~63;
    const int r0 = cx_last_le(dstart, 0, n_found - 1, i0);
    const int far = r0 + (i - i0);
    const int r = cx_last_le(dstart, r0, far < n_found - 1 ? far : n_found - 1, i);
    const int j = src_first[r] + (i - dstart[r]);
    dpts[i] = spts[j];
    dpkey[i] = spkey[j];
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// Marks and the scan.  Uses the source's scratch between queries -- skey (marks), skey2 (scanned), tmp -- and leaves the cells,
// the points, filt and the result of the last query alone.  Afterwards m.skey2[m.n_cells] = (cells found << 32 | points), on the
// device.  d_ijk: n_list x {i, j, k} on the device.
int cellmap_extract_mark(CellMapDev &m, const int *d_ijk, int n_list, hipStream_t s, const char **err)
{
    const int nc = m.n_cells;
    CXCHK(hipMemsetAsync(m.skey, 0, (size_t)(nc + 1) * sizeof(u64), s));
    if (n_list > 0 && nc > 0) hipLaunchKernelGGL(cx_mark_kernel, dim3(cx_blocks(n_list)), dim3(256), 0, s, d_ijk, n_list, m.ckey, m.cstart, nc, m.skey);
    size_t need = 0;
    CXCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, m.skey, m.skey2, nc + 1));
    if (need > m.tmp_bytes) {
        *err = "cell map scratch too small for the scan";
        return -1;
    }
    size_t tb = m.tmp_bytes;
    CXCHK(hipcub::DeviceScan::ExclusiveSum(m.tmp, tb, m.skey, m.skey2, nc + 1, s));
    CXCHK(hipGetLastError());
    return 0;
}

// After cellmap_extract_mark on src, with the totals it left read back: the n_found selected cells and their n_points points into
// dst (which has room for them; its previous content goes).  Uses src.flag for the first source position of every selected cell.
// dst ends as a fresh map after one append of those points would: frame 2, every stamp 0 -- or empty with frame 0.
int cellmap_extract_cells(CellMapDev &src, CellMapDev &dst, int n_found, int n_points, hipStream_t s, const char **err)
{
    if (n_found < 0 || n_points < n_found || n_points > dst.cap || (n_found > 0 && n_found > src.n_cells) || n_points > src.n_pts) {
        *err = "cell selection does not fit the destination";
        return -1;
    }
    if (n_points > 0) {
        int *src_first = (int *)src.flag;
        hipLaunchKernelGGL(cx_table_kernel, dim3(cx_blocks(src.n_cells + 1)), dim3(256), 0, s, src.skey, src.skey2, src.ckey, src.cstart, src.n_cells,
                           dst.ckey, dst.cstart, dst.clast, src_first);
        hipLaunchKernelGGL(cx_gather_kernel, dim3(cx_blocks(n_points)), dim3(256), 0, s, src.pts, src.pkey, src_first, dst.cstart, n_found, n_points,
                           dst.pts, dst.pkey);
        CXCHK(hipGetLastError());
    }
    dst.n_pts = n_points;
    dst.n_cells = n_points > 0 ? n_found : 0;
    dst.frame = n_points > 0 ? 2 : 0;  // the double increment of an append on an empty map (cellmap_append)
    dst.n_filt = dst.n_sel = 0;
    return 0;
}

}  // namespace ll
