// ll_scan_log_kernels.hip -- the two kernels of the scan log of the batched match buffer (ll_history_batch_enable_scan_log): the
// log of a step's full clouds into their blocks, and the gather of logged scans into one staging array for the map refinement
// (ll_map_refine_add_logged).  Both are streaming copies of 32 bytes per point (16 read, 16 written), one float4 per lane, coalesced;
// the log's index read through full_idx is its only irregular access.
#include <hip/hip_runtime.h>

#include "ll_scan_log.h"

namespace ll {

// grid (chunks of 256 points, slots), one lane per point
__global__ __launch_bounds__(256) void sl_log_kernel(const SlSlot *tab, const float4 *xf, int max_pts, const float4 *xyzi, const int *full_idx, int stride)
{
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const SlSlot t = tab[s];
    if (!t.dst || i >= t.n || i >= max_pts) return;
    t.dst[i] = sl_logged_point(xf[(size_t)s * max_pts + i], full_idx[(size_t)s * stride + i], stride, xyzi + (size_t)s * stride);
}

// grid (work items), 256 lanes over the item's <= SL_CHUNK points
__global__ __launch_bounds__(256) void sl_gather_kernel(const SlCopy *work, float4 *dst)
{
    const SlCopy w = work[blockIdx.x];
    for (int i = threadIdx.x; i < w.n; i += 256) dst[w.dst + i] = w.src[i];
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int sl_log(const SlSlot *tab, const float4 *xf, int max_pts, const float4 *xyzi, const int *full_idx, int stride, int S, int max_n, hipStream_t s,
           const char **err)
{
    if (max_n <= 0) return 0;
    hipLaunchKernelGGL(sl_log_kernel, dim3((max_n + 255) / 256, S), dim3(256), 0, s, tab, xf, max_pts, xyzi, full_idx, stride);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *err = hipGetErrorString(e);
        return -1;
    }
    return 0;
}

int sl_gather(const SlCopy *work, int n_work, float4 *dst, hipStream_t s, const char **err)
{
    if (n_work <= 0) return 0;
    hipLaunchKernelGGL(sl_gather_kernel, dim3(n_work), dim3(256), 0, s, work, dst);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *err = hipGetErrorString(e);
        return -1;
    }
    return 0;
}

}  // namespace ll
