// ll_fullmap_batch_kernels.hip -- the full-cloud maps of S lock-step sequences (ll_history_batch_enable_full_maps): the gather of
// the extractor's full selections into the map frame, and the touched cells of an append on the deferred store of
// ll_cellmap_batch_kernels.hip, whose cb_append does the append itself.
//
// A full cloud is some 24 k points per scan against the few hundred of a filtered feature frame, so the touched cells are found
// without ordering anything: every new log entry adds one to its cell's counter (integers: the sums do not depend on the order),
// the cell table is flagged against the slot's threshold, scanned and compacted.  The table is ordered by (slot, cell key), so the
// list comes out in that order with no sort.  A scan puts tens of consecutive points into one cell, so the lanes of a wavefront
// that hit the same cell add once for all of them.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "ll_fullmap_batch.h"
#include "ll_reg_core.h"

namespace ll {

typedef unsigned long long u64;
typedef unsigned int u32;

// grid (chunks of 256 points, slots), one lane per point: 16-byte loads and stores, the index gather is the only irregular access.
// The arithmetic is cloud_transform_kernel's and hb_transform_kernel's: point_to_map in double, stored as float.
__global__ __launch_bounds__(256) void fb_gather_kernel(const float4 *xyzi, const int *full_idx, int stride, const FbSlot *tab, int max_pts, float4 *xf)
{
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (!tab[s].active || i >= tab[s].n || i >= max_pts) return;
    const int src = full_idx[(size_t)s * stride + i];
    const float nan = __builtin_nanf("");
    float4 o = make_float4(nan, nan, nan, 0.0f);  // (what cb_point_key refuses)
    if (src >= 0 && src < stride) {
        const float4 v = xyzi[(size_t)s * stride + src];
        if (fb_point_ok(v.x, v.y, v.z)) {
            double p[7];
#pragma unroll
            for (int k = 0; k < 7; k++) p[k] = tab[s].pose[k];
            float m[3];
            point_to_map(p, v.x, v.y, v.z, m);
            o = make_float4(m[0], m[1], m[2], 0.0f);
        }
    }
    xf[(size_t)s * max_pts + i] = o;
}

// cnt[c] += 1 for the lanes with c >= 0; the lanes of a wavefront that name the same cell add their number once
// (-DLL_FB_PLAIN_ATOMICS: one atomic per lane, the A/B build behind the figure in DESIGN.md)
__device__ __forceinline__ void fb_count_add(int *cnt, int c)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(LL_FB_PLAIN_ATOMICS)
    if (c < 0) return;
    for (;;) {
        const int lead = __builtin_amdgcn_readfirstlane(c);  // (of the lanes still in the loop)
        const u64 same = __ballot(c == lead);
        if (c == lead) {
            if ((int)(threadIdx.x & 63) == __builtin_ctzll(same)) atomicAdd(&cnt[lead], (int)__popcll(same));
            break;
        }
    }
#else
    if (c >= 0) atomicAdd(&cnt[c], 1);  // (the host tier runs one thread at a time)
#endif
}

// grid (chunks of 256 points, slots): the step's new log entries against the merged table
__global__ __launch_bounds__(256) void fb_count_kernel(const CbSlot *tab, const u64 *pkey, const u64 *ckey, const int *coff, int *cnt)
{
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const CbSlot t = tab[s];
    int c = -1;
    if (t.active && i < t.n) {
        const u64 key = pkey[t.off + i];
        if (fb_point_counts(key)) c = cb_find(ckey, coff[s], coff[s + 1], key);
    }
    fb_count_add(cnt, c);
}

// one thread per table entry up to the host's bound; the merged cell count is counts[1]
__global__ __launch_bounds__(256) void fb_flag_kernel(const int *cnt, const int *cslot, const int *counts, int n_upper, const FbSlot *tab, int n_slots,
                                                      u32 *flag)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_upper) return;
    u32 f = 0u;
    if (c < counts[1]) {
        const int s = cslot[c];
        if (s >= 0 && s < n_slots && tab[s].active) f = fb_touched(cnt[c], tab[s].need) ? 1u : 0u;
    }
    flag[c] = f;
}

// the flagged cells as {i, j, k}, in table order; behind them one thread per slot boundary: the first listed cell of every slot
__global__ __launch_bounds__(256) void fb_compact_kernel(const u64 *ckey, const int *coff, const u32 *flag, const u32 *rank, int n_upper, int n_slots,
                                                         int *cells, int *toff)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n_upper) {
        if (flag[t]) {
            int k[3];
            cell_unpack(ckey[t], k);
            int *o = cells + 3 * (size_t)rank[t];
            o[0] = k[0];
            o[1] = k[1];
            o[2] = k[2];
        }
        return;
    }
    const int s = t - n_upper;
    if (s > n_slots) return;
    const int c = coff[s];
    toff[s] = c < n_upper ? (int)rank[c] : (int)(rank[n_upper - 1] + flag[n_upper - 1]);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int fb_tmp_bytes(long long n, size_t *bytes, const char **err)
{
    size_t t = 0;
    u32 *f = nullptr;
    CBCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, t, f, f, (int)(n > 0 ? n : 1)));
    *bytes = t + 16;
    return 0;
}

int fb_gather(const FbDev &t, const float4 *xyzi, const int *full_idx, int stride, int S, int max_pts, int max_n, hipStream_t s, int *launches,
              const char **err)
{
    if (max_n <= 0) return 0;
    hipLaunchKernelGGL(fb_gather_kernel, dim3((max_n + 255) / 256, S), dim3(256), 0, s, xyzi, full_idx, stride, t.tab, max_pts, t.xf);
    CBCHK(hipGetLastError());
    *launches += 1;
    return 0;
}

int fb_touched_chain(const CbDev &m, FbDev &t, int max_n, int n_upper, hipStream_t s, int *launches, const char **err)
{
    if (max_n <= 0 || n_upper <= 0) return 0;
    if ((size_t)n_upper > t.tcap) {
        *err = "full-map scratch too small for the cell table";
        return -1;
    }
    const int S = m.S;
    CBCHK(hipMemsetAsync(t.cnt, 0, (size_t)n_upper * sizeof(int), s));
    hipLaunchKernelGGL(fb_count_kernel, dim3((max_n + 255) / 256, S), dim3(256), 0, s, m.tab, m.pkey, m.ckey, m.coff, t.cnt);
    hipLaunchKernelGGL(fb_flag_kernel, dim3(cb_blocks(n_upper)), dim3(256), 0, s, t.cnt, m.cslot, m.counts, n_upper, t.tab, S, t.flag);
    size_t tb = t.tmp_bytes;
    CBCHK(hipcub::DeviceScan::ExclusiveSum(t.tmp, tb, t.flag, t.rank, n_upper, s));
    hipLaunchKernelGGL(fb_compact_kernel, dim3(cb_blocks((long long)n_upper + S + 1)), dim3(256), 0, s, m.ckey, m.coff, t.flag, t.rank, n_upper, S, t.cells,
                       t.toff);
    CBCHK(hipGetLastError());
    *launches += 5;
    return 0;
}

}  // namespace ll
