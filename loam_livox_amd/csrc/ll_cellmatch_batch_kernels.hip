// ll_cellmatch_batch_kernels.hip -- the cell-mode refresh of the batched match buffer (ll_history_batch_refresh_cells): the read side
// of the deferred store of ll_cellmap_batch_kernels.hip.
//
// cellmap_query_filter (ll_cellmap_kernels.hip) sorts every stored point of one map with 64-bit keys on every refresh, and once more
// when it replaces.  Here one chain per kind serves all S slots: the cells around every slot's pose are selected in the table, the
// log is streamed once for the points that are alive in a selected cell, and only those candidates are compacted and sorted -- by
// (table entry of the cell, leaf), which is (slot, cell, leaf) because the table is ordered by (slot, cell key).  The compaction keeps
// the log order, the sort is stable, and the log order inside a cell is the insertion order, so a leaf's centroid sums in the order
// cm_centroid_kernel sums.  A replace gives the selected cells a new epoch and logs their leaves under it; nothing stored moves.
//
// The sort's size has to be known on the host and the number of candidates is not (it would cost a host wait): the compacted keys
// are padded to the log's length with a key that sorts last, and the sort covers as many bits as the table has entries for.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "ll_cellmatch_batch.h"

namespace ll {

typedef unsigned long long u64;
typedef unsigned int u32;

struct alignas(16) CmbU64x2 {
    u64 a, b;
};
struct alignas(8) CmbI32x2 {
    int a, b;
};

// one thread per table entry of all slots
__global__ __launch_bounds__(256) void cmb_select_kernel(const u64 *ckey, const int *cslot, int n_cells, CellGeom g, const CmbSlot *tab, float radius,
                                                         double max_fov_deg, u32 *csel)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    csel[c] = cmb_cell_selected(ckey[c], g, tab[cslot[c]], radius, max_fov_deg) ? 1u : 0u;
}

__device__ __forceinline__ void cmb_candidate(u64 key, int slot, int ep, int n_slots, const u64 *ckey, const int *cep, const int *coff, const u32 *csel,
                                              u64 *flag, int *cell)
{
    int c = -1;
    if (slot >= 0 && slot < n_slots) c = cmb_live_cell(key, ep, ckey, cep, coff[slot], coff[slot + 1]);
    const bool cand = c >= 0 && csel[c] != 0u;
    *flag = ((u64)(c >= 0 ? 1u : 0u) << 32) | (u64)(cand ? 1u : 0u);
    *cell = cand ? c : -1;
}

// The stream over the log: 16 B of key, slot and epoch per entry, two entries per thread (16 B + 8 B + 8 B loads, two independent
// searches in flight).  The search stays inside the slot's range of the table: some seven steps for a hundred cells.
__global__ __launch_bounds__(256) void cmb_candidates_kernel(const u64 *pkey, const int *pslot, const int *pep, int n, int n_slots, const u64 *ckey,
                                                             const int *cep, const int *coff, const u32 *csel, u64 *cflag, int *ccell)
{
    const int j = 2 * (blockIdx.x * 256 + threadIdx.x);
    if (j >= n) return;
    if (j + 1 < n) {
        const CmbU64x2 k = *reinterpret_cast<const CmbU64x2 *>(pkey + j);
        const CmbI32x2 s = *reinterpret_cast<const CmbI32x2 *>(pslot + j);
        const CmbI32x2 e = *reinterpret_cast<const CmbI32x2 *>(pep + j);
        CmbU64x2 f;
        CmbI32x2 c;
        cmb_candidate(k.a, s.a, e.a, n_slots, ckey, cep, coff, csel, &f.a, &c.a);
        cmb_candidate(k.b, s.b, e.b, n_slots, ckey, cep, coff, csel, &f.b, &c.b);
        *reinterpret_cast<CmbU64x2 *>(cflag + j) = f;
        *reinterpret_cast<CmbI32x2 *>(ccell + j) = c;
    } else {
        cmb_candidate(pkey[j], pslot[j], pep[j], n_slots, ckey, cep, coff, csel, &cflag[j], &ccell[j]);
    }
}

// candidates to the front in log order, with their leaf keys; the others become the padding behind them
__global__ __launch_bounds__(256) void cmb_compact_kernel(const float4 *pts, const u64 *pkey, const u64 *cflag, const u64 *crank, const int *ccell, int n,
                                                          int n_cells, CellGeom g, float inv_leaf, u64 *key, int *val)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const u32 n_cand = (u32)(crank[n - 1] + cflag[n - 1]);
    const u32 r = (u32)crank[j];
    if ((u32)cflag[j]) {
        const float4 p = pts[j];
        key[r] = cmb_leaf_key(ccell[j], pkey[j], p.x, p.y, p.z, g, inv_leaf);
        val[r] = j;
    } else {
        const u32 pos = n_cand + ((u32)j - r);
        key[pos] = cmb_key_none(n_cells);
        val[pos] = -1;
    }
}

// (behind the candidates lies the padding: its flags are cleared for the scan, its keys are not read)
__global__ __launch_bounds__(256) void cmb_head_kernel(const u64 *key_sorted, const u64 *cflag, const u64 *crank, int n, u32 *hflag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int n_cand = (int)(u32)(crank[n - 1] + cflag[n - 1]);
    if (i >= n_cand) {
        hflag[i] = 0u;
        return;
    }
    hflag[i] = (i == 0 || key_sorted[i - 1] != key_sorted[i]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void cmb_head_pos_kernel(const u32 *hflag, const u32 *hrank, const u64 *cflag, const u64 *crank, int n, int *head)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || i >= (int)(u32)(crank[n - 1] + cflag[n - 1])) return;
    if (hflag[i]) head[hrank[i]] = i;
}

// one thread per leaf: pcl::VoxelGrid's centroid, float sums in insertion order; the intensity of a stored point is 0, so is the leaf's
__global__ __launch_bounds__(256) void cmb_centroid_kernel(const float4 *pts, const u64 *key_sorted, const int *val_sorted, const int *head,
                                                           const u32 *hflag, const u32 *hrank, const u64 *cflag, const u64 *crank, int n, float4 *leaf,
                                                           int *leaf_cell)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n_leaves = (int)(hrank[n - 1] + hflag[n - 1]);
    if (t >= n_leaves) return;
    const int n_cand = (int)(u32)(crank[n - 1] + cflag[n - 1]);
    const int first = head[t], last = t + 1 < n_leaves ? head[t + 1] : n_cand;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = first; i < last; i++) {
        const float4 p = pts[val_sorted[i]];
        sx = sx + p.x;
        sy = sy + p.y;
        sz = sz + p.z;
    }
    const float c = (float)(last - first);
    leaf[t] = make_float4(sx / c, sy / c, sz / c, 0.0f / c);
    leaf_cell[t] = cmb_key_cell(key_sorted[first]);
}

// first leaf of every slot (the leaves are ordered by table entry, a slot owns a range of entries), and the totals
__global__ __launch_bounds__(256) void cmb_counts_kernel(const u64 *key_sorted, const u32 *hflag, const u32 *hrank, const u64 *cflag, const u64 *crank,
                                                         int n, const int *coff, int n_slots, int *out)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s > n_slots + 2) return;
    const u64 total = crank[n - 1] + cflag[n - 1];
    if (s == n_slots + 1) {
        out[s] = (int)(u32)total;  // candidates
        return;
    }
    if (s == n_slots + 2) {
        out[s] = (int)(total >> 32);  // live entries
        return;
    }
    const int p = cb_lower_bound(key_sorted, 0, n, cmb_key_none(coff[s]));
    out[s] = p < n ? (int)hrank[p] : (int)(hrank[n - 1] + hflag[n - 1]);
}

__global__ __launch_bounds__(256) void cmb_scatter_kernel(const float4 *leaf, const int *leaf_cell, const int *cslot, const int *loff, int n_leaves,
                                                          float4 *concat, int stride)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_leaves) return;
    const int s = cslot[leaf_cell[t]];
    const int i = t - loff[s];
    if (i < 0 || i >= stride) return;  // (the host sized the stride by the same counts)
    concat[(size_t)s * stride + i] = leaf[t];
}

// the leaves behind the log, under the epoch their cell is about to get
__global__ __launch_bounds__(256) void cmb_append_leaves_kernel(const float4 *leaf, const int *leaf_cell, int n_leaves, const u64 *ckey, const int *cslot,
                                                                const int *cep, long long base, float4 *pts, u64 *pkey, int *pslot, int *pep)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_leaves) return;
    const int c = leaf_cell[t];
    const long long j = base + t;
    pts[j] = leaf[t];
    pkey[j] = ckey[c];
    pslot[j] = cslot[c];
    pep[j] = cmb_epoch_after_replace(cep[c]);
}

__global__ __launch_bounds__(256) void cmb_bump_kernel(const u32 *csel, int n_cells, int *cep)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    if (csel[c]) cep[c] = cmb_epoch_after_replace(cep[c]);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int cmb_tmp_bytes(long long n, size_t *bytes, const char **err)
{
    size_t t1 = 0, t2 = 0, t3 = 0;
    u64 *k = nullptr;
    int *v = nullptr;
    u32 *f = nullptr;
    const int nn = (int)(n > 0 ? n : 1);
    CBCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, k, k, v, v, nn, 0, 64));
    CBCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, k, k, nn));
    CBCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, t3, f, f, nn));
    *bytes = (t1 > t2 ? (t1 > t3 ? t1 : t3) : (t2 > t3 ? t2 : t3)) + 16;
    return 0;
}

int cmb_query(const CbDev &m, CmbDev &q, const CmbSlot *d_tab, float radius, float max_fov_deg, float leaf, hipStream_t s, int *launches,
              const char **err)
{
    if (!cmb_leaf_fits(m.geom, leaf)) {
        *err = "leaf size too small for the cell size (more than 1020 leaves across one cell)";
        return -1;
    }
    if (m.n_log <= 0 || m.n_cells <= 0 || m.n_log > (long long)q.ncap || (size_t)m.n_cells > q.ccap) {
        *err = "cell-match scratch too small for the store";
        return -1;
    }
    const int n = (int)m.n_log, nc = m.n_cells, S = m.S;
    const float inv_leaf = 1.0f / leaf;
    int bits = 30;
    while (bits < 64 && (cmb_key_none(nc) >> bits) != 0ull) bits++;
    hipLaunchKernelGGL(cmb_select_kernel, dim3(cb_blocks(nc)), dim3(256), 0, s, m.ckey, m.cslot, nc, m.geom, d_tab, radius, (double)max_fov_deg, q.csel);
    hipLaunchKernelGGL(cmb_candidates_kernel, dim3(cb_blocks(((long long)n + 1) / 2)), dim3(256), 0, s, m.pkey, m.pslot, m.pep, n, S, m.ckey, m.cep,
                       m.coff, q.csel, q.cflag, q.ccell);
    size_t tb = q.tmp_bytes;
    CBCHK(hipcub::DeviceScan::ExclusiveSum(q.tmp, tb, q.cflag, q.crank, n, s));
    hipLaunchKernelGGL(cmb_compact_kernel, dim3(cb_blocks(n)), dim3(256), 0, s, m.pts, m.pkey, q.cflag, q.crank, q.ccell, n, nc, m.geom, inv_leaf, q.key,
                       q.val);
    tb = q.tmp_bytes;
    CBCHK(hipcub::DeviceRadixSort::SortPairs(q.tmp, tb, q.key, q.key2, q.val, q.val2, n, 0, bits, s));
    hipLaunchKernelGGL(cmb_head_kernel, dim3(cb_blocks(n)), dim3(256), 0, s, q.key2, q.cflag, q.crank, n, q.hflag);
    tb = q.tmp_bytes;
    CBCHK(hipcub::DeviceScan::ExclusiveSum(q.tmp, tb, q.hflag, q.hrank, n, s));
    hipLaunchKernelGGL(cmb_head_pos_kernel, dim3(cb_blocks(n)), dim3(256), 0, s, q.hflag, q.hrank, q.cflag, q.crank, n, q.head);
    hipLaunchKernelGGL(cmb_centroid_kernel, dim3(cb_blocks(n)), dim3(256), 0, s, m.pts, q.key2, q.val2, q.head, q.hflag, q.hrank, q.cflag, q.crank, n,
                       q.leaf, q.leaf_cell);
    hipLaunchKernelGGL(cmb_counts_kernel, dim3(cb_blocks(S + 3)), dim3(256), 0, s, q.key2, q.hflag, q.hrank, q.cflag, q.crank, n, m.coff, S, q.out);
    CBCHK(hipGetLastError());
    *launches += 10;
    return 0;
}

int cmb_scatter(const CbDev &m, const CmbDev &q, int n_leaves, float4 *concat, int stride, hipStream_t s, int *launches, const char **err)
{
    if (n_leaves <= 0) return 0;
    hipLaunchKernelGGL(cmb_scatter_kernel, dim3(cb_blocks(n_leaves)), dim3(256), 0, s, q.leaf, q.leaf_cell, m.cslot, q.out, n_leaves, concat, stride);
    CBCHK(hipGetLastError());
    *launches += 1;
    return 0;
}

int cmb_replace(CbDev &m, const CmbDev &q, int n_leaves, hipStream_t s, int *launches, const char **err)
{
    if (n_leaves <= 0) return 0;  // (no leaf: no cell is selected -- every cell of the table holds a live point)
    if (m.n_log + n_leaves > (long long)m.cap) {
        *err = "cell-map store too small for the replace";
        return -1;
    }
    hipLaunchKernelGGL(cmb_append_leaves_kernel, dim3(cb_blocks(n_leaves)), dim3(256), 0, s, q.leaf, q.leaf_cell, n_leaves, m.ckey, m.cslot, m.cep,
                       m.n_log, m.pts, m.pkey, m.pslot, m.pep);
    hipLaunchKernelGGL(cmb_bump_kernel, dim3(cb_blocks(m.n_cells)), dim3(256), 0, s, q.csel, m.n_cells, m.cep);
    CBCHK(hipGetLastError());
    *launches += 2;
    m.n_log += n_leaves;
    return 0;
}

}  // namespace ll
