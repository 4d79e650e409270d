// ll_history_batch_kernels.hip -- the match buffers of S sequences built together (ll_history_batch_*).
//
// Per slot the arithmetic is that of the single-sequence path: point_to_map (ll_reg_core.h) as cloud_transform_kernel applies it,
// the VoxelGrid of ll_voxel_kernels.hip, and for the search grids cell_coord / the finite test / the clamps of cellkey_kernel
// (ll_map_kernels.hip).  What differs is the layout: every launch covers all slots, the (grid, cell) keys of all grids go through ONE
// stable radix sort -- the points of one cell stay in ascending input order, which the k-NN's tie-breaks depend on -- and one scan
// runs over the concatenated cell tables.  The table of grid g ends with an entry that holds MINUS its valid points, so the running
// sum is back at zero where the next table starts and every table comes out with positions local to its own grid.
#include <hip/hip_runtime.h>
#include <string.h>
#include <hipcub/hipcub.hpp>

#include "ll_history_batch.h"
#include "ll_reg_core.h"

namespace ll {

#define HBCHK(x)                              \
    do {                                      \
        hipError_t e_ = (x);                  \
        if (e_ != hipSuccess) {               \
            *err = hipGetErrorString(e_);     \
            return -1;                        \
        }                                     \
    } while (0)

// ---- add ---------------------------------------------------------------------------------------------------------------------
// what the two transform kernels below share: the points this block's (slot, kind) moves -- the cloud's count within the slot's capacity
// and the producer's stride, 0 for a slot that does not work -- which the block's first thread also writes to n_xf[kind][slot]
__device__ __forceinline__ int hb_transform_count(const int *n_c, const int *n_s, int stride, const HbAddSlot *tab, int n_slots, int max_pts, int *n_xf)
{
    const int s = blockIdx.y, kind = blockIdx.z;
    int n = 0;
    if (tab[s].work) {
        n = kind ? n_s[s] : n_c[s];
        n = n < 0 ? 0 : n;
        n = n < max_pts ? n : max_pts;
        n = n < stride ? n : stride;
    }
    if (blockIdx.x * 256 + threadIdx.x == 0) n_xf[kind * n_slots + s] = n;
    return n;
}

// grid (chunks of 256 points, slots, 2 kinds): both clouds of every working slot into the map frame (laser_mapping.hpp:1421-1431)
__global__ __launch_bounds__(256) void hb_transform_kernel(const float4 *src_c, const int *n_c, int stride_c, const float4 *src_s,
                                                           const int *n_s, int stride_s, const HbAddSlot *tab, int n_slots, int max_pts,
                                                           float4 *xf, int *n_xf)
{
    const int s = blockIdx.y, kind = blockIdx.z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int stride = kind ? stride_s : stride_c;
    if (i >= hb_transform_count(n_c, n_s, stride, tab, n_slots, max_pts, n_xf)) return;
    double p[7];
#pragma unroll
    for (int k = 0; k < 7; k++) p[k] = tab[s].pose[k];
    const float4 v = (kind ? src_s : src_c)[(size_t)s * stride + i];
    float o[3];
    point_to_map(p, v.x, v.y, v.z, o);
    xf[((size_t)kind * n_slots + s) * max_pts + i] = make_float4(o[0], o[1], o[2], v.w);
}

// The deskew form (ll_history_batch_set_undistort; g_if_undistore = 1, laser_mapping.hpp:1424,1430): slot s's clouds move with record
// recs[s] of the registration -- every point with the pose interpolated at its time stamp, point_to_map_undistort as
// cloud_undistort_kernel calls it -- instead of tab[s].pose.  The slot is the block's y index, so its record arrives through scalar loads.
__global__ __launch_bounds__(256) void hb_transform_undistort_kernel(const float4 *src_c, const int *n_c, int stride_c, const float4 *src_s,
                                                                     const int *n_s, int stride_s, const HbAddSlot *tab, const UndistortRec *__restrict__ recs,
                                                                     int n_slots, int max_pts, float4 *xf, int *n_xf)
{
    const int s = blockIdx.y, kind = blockIdx.z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int stride = kind ? stride_s : stride_c;
    if (i >= hb_transform_count(n_c, n_s, stride, tab, n_slots, max_pts, n_xf)) return;
    const UndistortRec &c = recs[s];
    const float4 v = (kind ? src_s : src_c)[(size_t)s * stride + i];
    float o[3];
    point_to_map_undistort(c.pose_last, c.pose_curr, c.inc_t, c.theta, c.hat, c.hat_sq, c.deblur, c.min_ts, c.max_ts, v, o);
    xf[((size_t)kind * n_slots + s) * max_pts + i] = make_float4(o[0], o[1], o[2], v.w);
}

// the filtered frames into the ring slots the host chose; cnt[kind][slot] = their sizes
__global__ __launch_bounds__(256) void hb_scatter_kernel(const float4 *out_c, const int *n_out_c, const float4 *out_s, const int *n_out_s,
                                                         int stride, const HbAddSlot *tab, int n_slots, int max_pts, int ring_slots,
                                                         float4 *frames_c, float4 *frames_s, int *cnt)
{
    const int s = blockIdx.y, kind = blockIdx.z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int n = 0;
    if (tab[s].push) {
        n = kind ? n_out_s[s] : n_out_c[s];
        n = n < 0 ? 0 : n;
        n = n < max_pts ? n : max_pts;
    }
    if (i == 0) cnt[kind * n_slots + s] = n;
    if (i >= n) return;
    const int ring = tab[s].ring;
    if (ring < 0 || ring >= ring_slots) return;
    (kind ? frames_s : frames_c)[((size_t)s * ring_slots + ring) * max_pts + i] = (kind ? out_s : out_c)[(size_t)s * stride + i];
}

// ---- refresh -----------------------------------------------------------------------------------------------------------------
// grid (chunks of 256 points, segments): one frame of one kind of one slot per blockIdx.y (laser_mapping.hpp:519-530)
__global__ __launch_bounds__(256) void hb_gather_frames_kernel(const float4 *frames_c, const float4 *frames_s, const HbSeg *segs, float4 *concat)
{
    const HbSeg sg = segs[blockIdx.y];
    const float4 *src = (sg.kind ? frames_s : frames_c) + sg.src;
    float4 *dst = concat + sg.dst;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < sg.n; i += gridDim.x * 256) dst[i] = src[i];
}

__device__ __forceinline__ unsigned int hb_f2ord(float f)
{
    const unsigned int b = (unsigned int)__float_as_int(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// grid (chunks, slots, 2 kinds).  min / max: the result does not depend on the order.
__global__ __launch_bounds__(256) void hb_aabb_kernel(const float4 *out_c, const int *n_out_c, int stride_c, const float4 *out_s,
                                                      const int *n_out_s, int stride_s, const int *active, int n_slots, int map_stride,
                                                      float4 *d_map, unsigned int *mm)
{
    const int s = blockIdx.y, kind = blockIdx.z;
    if (!active[s]) return;
    const int stride = kind ? stride_s : stride_c;
    int n = kind ? n_out_s[s] : n_out_c[s];
    n = n < 0 ? 0 : (n < stride ? n : stride);
    n = n < map_stride ? n : map_stride;
    const float4 *src = (kind ? out_s : out_c) + (size_t)s * stride;
    float4 *dst = d_map + ((size_t)kind * n_slots + s) * map_stride;
    unsigned int *m = mm + ((size_t)kind * n_slots + s) * 8;
    if (blockIdx.x == 0 && threadIdx.x == 0) m[6] = (unsigned int)n;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int cnt = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float4 p = src[i];
        dst[i] = p;
        if (ll_isfinite(p.x) && ll_isfinite(p.y) && ll_isfinite(p.z)) {
            lo[0] = fminf(lo[0], p.x);
            lo[1] = fminf(lo[1], p.y);
            lo[2] = fminf(lo[2], p.z);
            hi[0] = fmaxf(hi[0], p.x);
            hi[1] = fmaxf(hi[1], p.y);
            hi[2] = fmaxf(hi[2], p.z);
            cnt++;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int d = 0; d < 3; d++) {
            lo[d] = fminf(lo[d], __shfl_down(lo[d], off));
            hi[d] = fmaxf(hi[d], __shfl_down(hi[d], off));
        }
        cnt += __shfl_down(cnt, off);
    }
    if ((threadIdx.x & 63) == 0 && cnt > 0) {
        for (int d = 0; d < 3; d++) {
            atomicMin(&m[d], hb_f2ord(lo[d]));
            atomicMax(&m[3 + d], hb_f2ord(hi[d]));
        }
    }
}

// grid (chunks of 256 points, grids): key = grid << cbits | cell (cellkey_kernel's cell); a non-finite point gets cell = ncell, sorts
// to the end of its grid's run and is dropped.  counts[cell_off + cell]++ per valid point, counts[cell_off + ncell] -= valid points.
__global__ __launch_bounds__(256) void hb_cellkey_kernel(const float4 *d_map, int stride, const HbGrid *tab, int cbits, unsigned long long *keys,
                                                         int *vals, int *counts)
{
    const HbGrid &t = tab[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = t.n < stride ? t.n : stride;
    const Grid &g = t.g;
    bool valid = false;
    if (i < n) {
        const float4 p = d_map[(size_t)t.src * stride + i];
        unsigned int key = (unsigned int)t.ncell;
        if (ll_isfinite(p.x) && ll_isfinite(p.y) && ll_isfinite(p.z)) {
            int cx = cell_coord(p.x, g.ox, g.inv_h), cy = cell_coord(p.y, g.oy, g.inv_h), cz = cell_coord(p.z, g.oz, g.inv_h);
            cx = min(max(cx, 0), g.nx - 1);
            cy = min(max(cy, 0), g.ny - 1);
            cz = min(max(cz, 0), g.nz - 1);
            key = (unsigned int)((cz * g.ny + cy) * g.nx + cx);
            atomicAdd(&counts[t.cell_off + key], 1);
            valid = true;
        }
        keys[t.pt_off + i] = ((unsigned long long)blockIdx.y << cbits) | (unsigned long long)key;
        vals[t.pt_off + i] = i;
    }
    const int nv = __popcll(__ballot(valid));
    if ((threadIdx.x & 63) == 0 && nv > 0) atomicSub(&counts[t.cell_off + t.ncell], nv);
}

// one thread per sorted position of all grids: the {x, y, z, original index} record of gather_kernel (ll_map_kernels.hip)
__global__ __launch_bounds__(256) void hb_gather_points_kernel(const float4 *d_map, int stride, const HbGrid *tab, int cbits,
                                                               const unsigned long long *keys_sorted, const int *vals_sorted, long long n_total,
                                                               const int *cell_pool, f4 *pts_pool, int *n_valid)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_total) return;
    const unsigned long long k = keys_sorted[j];
    const int gi = (int)(k >> cbits);
    const unsigned int cell = (unsigned int)(k & ((1ull << cbits) - 1ull));
    const HbGrid &t = tab[gi];
    if (j == t.pt_off) n_valid[gi] = cell_pool[t.cell_off + t.ncell];  // (the scan's total of this grid: its finite points)
    if (cell >= (unsigned int)t.ncell) return;
    const int i = vals_sorted[j];
    const float4 v = d_map[(size_t)t.src * stride + i];
    f4 p;
    p.x = v.x;
    p.y = v.y;
    p.z = v.z;
    p.w = __int_as_float(i);
    pts_pool[j] = p;
}

// ---- launch wrappers -----------------------------------------------------------------------------------------------------------
void launch_hb_transform(const float4 *src_c, const int *n_c, int stride_c, const float4 *src_s, const int *n_s, int stride_s,
                         const HbAddSlot *tab, int n_slots, int max_pts, float4 *xf, int *n_xf, hipStream_t s)
{
    hipLaunchKernelGGL(hb_transform_kernel, dim3((max_pts + 255) / 256, n_slots, 2), dim3(256), 0, s, src_c, n_c, stride_c, src_s, n_s, stride_s,
                       tab, n_slots, max_pts, xf, n_xf);
}

void launch_hb_transform_undistort(const float4 *src_c, const int *n_c, int stride_c, const float4 *src_s, const int *n_s, int stride_s,
                                   const HbAddSlot *tab, const UndistortRec *recs, int n_slots, int max_pts, float4 *xf, int *n_xf, hipStream_t s)
{
    hipLaunchKernelGGL(hb_transform_undistort_kernel, dim3((max_pts + 255) / 256, n_slots, 2), dim3(256), 0, s, src_c, n_c, stride_c, src_s, n_s,
                       stride_s, tab, recs, n_slots, max_pts, xf, n_xf);
}

void launch_hb_scatter(const float4 *out_c, const int *n_out_c, const float4 *out_s, const int *n_out_s, int stride, const HbAddSlot *tab,
                       int n_slots, int max_pts, int ring_slots, float4 *frames_c, float4 *frames_s, int *cnt, hipStream_t s)
{
    hipLaunchKernelGGL(hb_scatter_kernel, dim3((max_pts + 255) / 256, n_slots, 2), dim3(256), 0, s, out_c, n_out_c, out_s, n_out_s, stride, tab,
                       n_slots, max_pts, ring_slots, frames_c, frames_s, cnt);
}

void launch_hb_gather_frames(const float4 *frames_c, const float4 *frames_s, const HbSeg *segs, int n_seg, int max_pts, float4 *concat,
                             hipStream_t s)
{
    if (n_seg <= 0) return;
    int gx = (max_pts + 255) / 256;
    gx = gx < 32 ? gx : 32;
    for (int first = 0; first < n_seg; first += 65535) {  // (one launch up to 65 535 frames: the limit of a grid's y dimension)
        const int m = n_seg - first < 65535 ? n_seg - first : 65535;
        hipLaunchKernelGGL(hb_gather_frames_kernel, dim3(gx, m), dim3(256), 0, s, frames_c, frames_s, segs + first, concat);
    }
}

void launch_hb_aabb(const float4 *out_c, const int *n_out_c, int stride_c, const float4 *out_s, const int *n_out_s, int stride_s,
                    const int *active, int n_slots, int max_n, int map_stride, float4 *d_map, unsigned int *mm, hipStream_t s)
{
    int gx = (max_n + 255) / 256;
    gx = gx < 1 ? 1 : (gx < 32 ? gx : 32);
    hipLaunchKernelGGL(hb_aabb_kernel, dim3(gx, n_slots, 2), dim3(256), 0, s, out_c, n_out_c, stride_c, out_s, n_out_s, stride_s, active, n_slots,
                       map_stride, d_map, mm);
}

void launch_hb_cellkey(const float4 *d_map, int stride, const HbGrid *tab, int n_grids, int max_n, int cbits, unsigned long long *keys,
                       int *vals, int *counts, hipStream_t s)
{
    if (n_grids <= 0 || max_n <= 0) return;
    hipLaunchKernelGGL(hb_cellkey_kernel, dim3((max_n + 255) / 256, n_grids), dim3(256), 0, s, d_map, stride, tab, cbits, keys, vals, counts);
}

void launch_hb_gather_points(const float4 *d_map, int stride, const HbGrid *tab, int cbits, const unsigned long long *keys_sorted,
                             const int *vals_sorted, long long n_total, const int *cell_pool, f4 *pts_pool, int *n_valid, hipStream_t s)
{
    if (n_total <= 0) return;
    hipLaunchKernelGGL(hb_gather_points_kernel, dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, s, d_map, stride, tab, cbits, keys_sorted,
                       vals_sorted, n_total, cell_pool, pts_pool, n_valid);
}

int hb_sort_scan_bytes(long long n_total, long long n_cells, size_t *bytes, const char **err)
{
    size_t t1 = 0, t2 = 0;
    unsigned long long *k = nullptr;
    int *v = nullptr;
    if (n_total > 0) HBCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, k, k, v, v, (int)n_total, 0, 64));
    HBCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, v, v, (int)n_cells));
    *bytes = (t1 > t2 ? t1 : t2) + 16;
    return 0;
}

int hb_sort_scan(void *tmp, size_t tmp_bytes, unsigned long long *keys, unsigned long long *keys2, int *vals, int *vals2, long long n_total,
                 int key_bits, int *counts, int *cell_pool, long long n_cells, hipStream_t s, const char **err)
{
    size_t tb = tmp_bytes;
    HBCHK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, counts, cell_pool, (int)n_cells, s));
    tb = tmp_bytes;
    // stable LSD radix sort by (grid, cell): the points of one cell stay in ascending original-index order
    if (n_total > 0) HBCHK(hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys, keys2, vals, vals2, (int)n_total, 0, key_bits, s));
    return 0;
}

void hb_aabb_identity(unsigned int m[8])
{
    m[0] = m[1] = m[2] = 0xffffffffu;
    m[3] = m[4] = m[5] = 0u;
    m[6] = m[7] = 0u;
}

void hb_aabb_decode(const unsigned int m[8], float mm[6], int *n_out)
{
    for (int d = 0; d < 6; d++) {
        const unsigned int o = m[d];
        const unsigned int b = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
        memcpy(&mm[d], &b, sizeof(float));
    }
    *n_out = (int)m[6];
}

}  // namespace ll
