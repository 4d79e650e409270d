// ll_cellmap_batch_kernels.hip -- the cell maps of S lock-step sequences in one deferred store (ll_history_batch_enable_cell_maps).
//
// cellmap_append (ll_cellmap_kernels.hip) re-sorts the whole stored map on every cloud.  Here a cloud costs what it brings: its
// points are classified against the slot's cell table, the cells they hit are stamped (and reset by epoch, ll_cellmap_batch_core.h),
// the cells they open are merged into the table, and the points go behind the log.  No kernel of the append reads, sorts or moves
// a stored point.  The order a reader expects -- (slot, cell key, insertion order), dead points gone -- is made by cb_materialise,
// once for all slots, when somebody reads.
//
// The cell key fills 63 bits, so (slot, key) does not fit one radix key: both chains sort by the key first and then, stably, by the
// few bits of the slot.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <utility>

#include "ll_cellmap_batch.h"

namespace ll {

typedef unsigned long long u64;
typedef unsigned int u32;

static inline int cb_slot_bits(int S)  // the slot field holds 0 .. S (S: "no slot", sorts behind every slot)
{
    int b = 1;
    while ((1 << b) <= S) b++;
    return b;
}

// ---- append ------------------------------------------------------------------------------------------------------------------
// grid (chunks of 256 points, slots): the new points behind the log; a hit stamps its cell, the cloud's first hit on a stale cell
// resets it; a point whose cell is not in the table is a candidate for a new cell
__global__ __launch_bounds__(256) void cb_classify_kernel(const float4 *src, int src_stride, const CbSlot *tab, long long base, CellGeom g, int thr,
                                                          const u64 *ckey, int *clast, int *cep, const int *coff, int n_slots, float4 *pts,
                                                          u64 *pkey, int *pslot, u64 *akey, int *aslot)
{
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const CbSlot t = tab[s];
    if (!t.active || i >= t.n) return;
    const float4 p = src[(size_t)s * src_stride + i];
    const long long j = t.off + i;
    const u64 key = cb_point_key(p.x, p.y, p.z, g);
    u64 cand = LL_CELL_KEY_NONE;
    int cand_slot = n_slots;
    if (key != LL_CELL_KEY_NONE) {
        const int c = cb_find(ckey, coff[s], coff[s + 1], key);
        if (c >= 0) {
            const int before = atomicExch(&clast[c], t.frame);
            if (cb_first_touch(before, t.frame) && cb_stale(t.frame, before, thr)) cep[c] = cb_epoch_after_reset(cep[c]);  // (one thread per cell gets here)
        } else {
            cand = key;
            cand_slot = s;
        }
    }
    pts[j] = make_float4(p.x, p.y, p.z, 0.0f);
    pkey[j] = key;
    pslot[j] = s;
    akey[j - base] = cand;
    aslot[j - base] = cand_slot;
}

// the candidates ordered by (slot, key): the first of every run opens a cell
__global__ __launch_bounds__(256) void cb_newcell_flag_kernel(const u64 *akey, const int *aslot, int n, int n_slots, u32 *flag)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    flag[a] = (aslot[a] < n_slots && (a == 0 || aslot[a - 1] != aslot[a] || akey[a - 1] != akey[a])) ? 1u : 0u;
}

// One thread per old cell and per candidate: the merge of the table with the new cells, both ordered by (slot, key) and disjoint.
// An old cell moves up by the new cells below it, a new cell lands at its rank among the new plus the old cells below it.
__global__ __launch_bounds__(256) void cb_merge_kernel(const u64 *ckey, const int *cslot, const int *clast, const int *cep, int n_cells,
                                                       const int *coff, const u64 *akey, const int *aslot, const u32 *flag, const u32 *rank, int n_new,
                                                       int n_slots, const CbSlot *tab, u64 *ckey2, int *cslot2, int *clast2, int *cep2, int *counts)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n_cells) {
        const int s = cslot[t];
        const u64 k = ckey[t];
        const int lb = cb_lower_bound_pair(aslot, akey, n_new, s, k);
        const int below = lb < n_new ? (int)rank[lb] : (int)(rank[n_new - 1] + flag[n_new - 1]);
        const int pos = t + below;
        ckey2[pos] = k;
        cslot2[pos] = s;
        clast2[pos] = clast[t];
        cep2[pos] = cep[t];
        return;
    }
    const int a = t - n_cells;
    if (a >= n_new) return;
    if (flag[a]) {
        const int s = aslot[a];
        const u64 k = akey[a];
        const int pos = (int)rank[a] + cb_lower_bound(ckey, coff[s], coff[s + 1], k);
        ckey2[pos] = k;
        cslot2[pos] = s;
        clast2[pos] = tab[s].frame;  // CMK:700-702
        cep2[pos] = 0;
    }
    if (a == n_new - 1) {
        const int opened = (int)(rank[a] + flag[a]);
        counts[0] = opened;
        counts[1] = n_cells + opened;
    }
}

// first cell of every slot in the merged table
__global__ __launch_bounds__(256) void cb_coff_kernel(const int *cslot, const int *counts, int n_slots, int *coff)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s > n_slots) return;
    coff[s] = cb_lower_bound_slot(cslot, counts[1], s);
}

// the epoch every new point goes in under: its cell's, after the resets and the merge
__global__ __launch_bounds__(256) void cb_epoch_kernel(const CbSlot *tab, const u64 *pkey, const u64 *ckey, const int *cep, const int *coff, int *pep)
{
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const CbSlot t = tab[s];
    if (!t.active || i >= t.n) return;
    const long long j = t.off + i;
    const u64 key = pkey[j];
    int e = 0;
    if (key != LL_CELL_KEY_NONE) {
        const int c = cb_find(ckey, coff[s], coff[s + 1], key);
        if (c >= 0) e = cep[c];
    }
    pep[j] = e;
}

// ---- materialise -------------------------------------------------------------------------------------------------------------
// a dead or dropped point gets the key and the slot that sort behind everything
__global__ __launch_bounds__(256) void cb_live_kernel(const u64 *pkey, const int *pslot, const int *pep, int n, const u64 *ckey, const int *cep,
                                                      const int *coff, int n_slots, u64 *mkey, int *mslot, int *mval)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const u64 key = pkey[j];
    const int s = pslot[j];
    bool live = false;
    if (key != LL_CELL_KEY_NONE && s >= 0 && s < n_slots) {
        const int c = cb_find(ckey, coff[s], coff[s + 1], key);
        live = c >= 0 && cb_live(pep[j], cep[c]);
    }
    mkey[j] = live ? key : LL_CELL_KEY_NONE;
    mslot[j] = live ? s : n_slots;
    mval[j] = j;
}

__global__ __launch_bounds__(256) void cb_gather_slot_kernel(const int *mslot, const int *val_sorted, int n, int *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = mslot[val_sorted[i]];
}

// the ordered store: the live points by (slot, key, log position)
__global__ __launch_bounds__(256) void cb_gather_kernel(const float4 *pts, const u64 *pkey, const int *pep, const int *slot_sorted, const int *val_sorted,
                                                        int n, int n_slots, float4 *pts2, u64 *pkey2, int *pslot2, int *pep2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = slot_sorted[i];
    if (s >= n_slots) return;
    const int v = val_sorted[i];
    pts2[i] = pts[v];
    pkey2[i] = pkey[v];
    pslot2[i] = s;
    pep2[i] = pep[v];
}

__global__ __launch_bounds__(256) void cb_poff_kernel(const int *slot_sorted, int n, int n_slots, int *poff)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s > n_slots) return;
    poff[s] = cb_lower_bound_slot(slot_sorted, n, s);
}

// per cell the first of its points, counted from its slot's first point; per slot the closing entry (its point count)
__global__ __launch_bounds__(256) void cb_cstart_kernel(const u64 *ckey, const int *cslot, int n_cells, const int *coff, const int *poff,
                                                        const u64 *pkey_sorted, int n_slots, int *cstart)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n_cells) {
        const int s = cslot[t];
        cstart[t + s] = cb_lower_bound(pkey_sorted, poff[s], poff[s + 1], ckey[t]) - poff[s];
        return;
    }
    const int s = t - n_cells;
    if (s < n_slots) cstart[coff[s + 1] + s] = poff[s + 1] - poff[s];
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int cb_tmp_bytes(long long n, size_t *bytes, const char **err)
{
    size_t t1 = 0, t2 = 0, t3 = 0;
    u64 *k = nullptr;
    int *v = nullptr;
    u32 *f = nullptr;
    const int nn = (int)(n > 0 ? n : 1);
    CBCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, k, k, v, v, nn, 0, 64));
    CBCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t2, v, v, k, k, nn, 0, 32));
    CBCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, t3, f, f, nn));
    *bytes = (t1 > t2 ? (t1 > t3 ? t1 : t3) : (t2 > t3 ? t2 : t3)) + 16;
    return 0;
}

int cb_append(CbDev &m, const float4 *src, int src_stride, int max_n, long long n_new, hipStream_t s, int *launches, const char **err)
{
    if (n_new <= 0 || max_n <= 0) return 0;  // (no point: no cell is hit or opened; the caller moves the frame counters)
    if (m.n_log + n_new > (long long)m.cap || (long long)m.n_cells + n_new > (long long)m.ccap || n_new > (long long)m.acap) {
        *err = "cell-map store too small for the append";
        return -1;
    }
    const int n = (int)n_new, S = m.S, sbits = cb_slot_bits(S);
    const dim3 per_slot((max_n + 255) / 256, S);
    hipLaunchKernelGGL(cb_classify_kernel, per_slot, dim3(256), 0, s, src, src_stride, m.tab, m.n_log, m.geom, m.threshold, m.ckey, m.clast, m.cep,
                       m.coff, S, m.pts, m.pkey, m.pslot, m.akey, m.aslot);
    size_t tb = m.tmp_bytes;
    CBCHK(hipcub::DeviceRadixSort::SortPairs(m.tmp, tb, m.akey, m.akey2, m.aslot, m.aslot2, n, 0, 64, s));
    tb = m.tmp_bytes;
    CBCHK(hipcub::DeviceRadixSort::SortPairs(m.tmp, tb, m.aslot2, m.aslot, m.akey2, m.akey, n, 0, sbits, s));
    hipLaunchKernelGGL(cb_newcell_flag_kernel, dim3(cb_blocks(n)), dim3(256), 0, s, m.akey, m.aslot, n, S, m.aflag);
    tb = m.tmp_bytes;
    CBCHK(hipcub::DeviceScan::ExclusiveSum(m.tmp, tb, m.aflag, m.arank, n, s));
    hipLaunchKernelGGL(cb_merge_kernel, dim3(cb_blocks((long long)m.n_cells + n)), dim3(256), 0, s, m.ckey, m.cslot, m.clast, m.cep, m.n_cells, m.coff,
                       m.akey, m.aslot, m.aflag, m.arank, n, S, m.tab, m.ckey2, m.cslot2, m.clast2, m.cep2, m.counts);
    hipLaunchKernelGGL(cb_coff_kernel, dim3(cb_blocks(S + 1)), dim3(256), 0, s, m.cslot2, m.counts, S, m.coff2);
    hipLaunchKernelGGL(cb_epoch_kernel, per_slot, dim3(256), 0, s, m.tab, m.pkey, m.ckey2, m.cep2, m.coff2, m.pep);
    CBCHK(hipGetLastError());
    *launches += 8;
    std::swap(m.ckey, m.ckey2);
    std::swap(m.cslot, m.cslot2);
    std::swap(m.clast, m.clast2);
    std::swap(m.cep, m.cep2);
    std::swap(m.coff, m.coff2);
    m.n_log += n_new;
    return 0;
}

int cb_materialise(CbDev &m, hipStream_t s, int *launches, const char **err)
{
    const int S = m.S, sbits = cb_slot_bits(S);
    if (m.n_log <= 0) {
        CBCHK(hipMemsetAsync(m.poff, 0, (size_t)(S + 1) * sizeof(int), s));
        if (m.n_cells == 0) CBCHK(hipMemsetAsync(m.cstart, 0, (size_t)(S + 1) * sizeof(int), s));
        return 0;
    }
    if (m.n_log > (long long)m.mcap) {
        *err = "cell-map scratch too small for the materialisation";
        return -1;
    }
    const int n = (int)m.n_log;
    hipLaunchKernelGGL(cb_live_kernel, dim3(cb_blocks(n)), dim3(256), 0, s, m.pkey, m.pslot, m.pep, n, m.ckey, m.cep, m.coff, S, m.mkey, m.mslot, m.mval);
    size_t tb = m.tmp_bytes;
    CBCHK(hipcub::DeviceRadixSort::SortPairs(m.tmp, tb, m.mkey, m.mkey2, m.mval, m.mval2, n, 0, 64, s));
    hipLaunchKernelGGL(cb_gather_slot_kernel, dim3(cb_blocks(n)), dim3(256), 0, s, m.mslot, m.mval2, n, m.mslot2);
    tb = m.tmp_bytes;
    CBCHK(hipcub::DeviceRadixSort::SortPairs(m.tmp, tb, m.mslot2, m.mslot, m.mval2, m.mval, n, 0, sbits, s));
    hipLaunchKernelGGL(cb_gather_kernel, dim3(cb_blocks(n)), dim3(256), 0, s, m.pts, m.pkey, m.pep, m.mslot, m.mval, n, S, m.pts2, m.pkey2, m.pslot2,
                       m.pep2);
    hipLaunchKernelGGL(cb_poff_kernel, dim3(cb_blocks(S + 1)), dim3(256), 0, s, m.mslot, n, S, m.poff);
    hipLaunchKernelGGL(cb_cstart_kernel, dim3(cb_blocks((long long)m.n_cells + S)), dim3(256), 0, s, m.ckey, m.cslot, m.n_cells, m.coff, m.poff, m.pkey2,
                       S, m.cstart);
    CBCHK(hipGetLastError());
    *launches += 7;
    std::swap(m.pts, m.pts2);
    std::swap(m.pkey, m.pkey2);
    std::swap(m.pslot, m.pslot2);
    std::swap(m.pep, m.pep2);
    return 0;
}

}  // namespace ll
