// ll_map_refine_kernels.hip -- VoxelGrid (PCL 1.9 semantics, ll_voxel_core.h) over a RAGGED set of selections of one float4 array,
// with the move into the corrected frame of Mapping_refine (ll_map_refine_core.h) fused in, before or behind the filter.
//
// A selection is n points at src[src_off ..]; the selections' points are the work indices 0 .. total - 1 in selection order, and only
// those are keyed, sorted and summed -- not n_sel times the largest selection.  The (selection, chunk) work list is the host's.  One
// chain, for any number of selections:
//   mr_init_kernel      identities of min / max, zero counts                                   (one thread per selection)
//   mr_bounds_kernel    finite-point bounding box + count per selection                        (one workgroup per work item)
//   mr_params_kernel    min_b / divb_mul / status per selection                                (one thread per selection)
//   mr_key_kernel       64-bit key = selection << 32 | leaf index, value = work index; non-finite points and the points of
//                       selections that are not filtered get the sentinel, which sorts last     (one workgroup per work item)
//   hipcub radix sort   over the 32 + selection bits in use -- stable, so a voxel's points stay in input order
//   mr_head_kernel      voxel heads -> per-selection voxel counts
//   hipcub scan, mr_headpos_kernel   the v-th head's sorted position
//   mr_offsets_kernel   per-selection voxel and output offsets, status, the voxel total         (one workgroup)
//   mr_centroid_kernel  one thread per voxel: float sums in input order, one division per component, the move behind it in mode 0
//   mr_copy_kernel      pass-through selections: output = the filter's input, moved in mode 0   (one workgroup per work item)
// In mode 1 the bounds, key and centroid passes each recompute the moved point from the stored one (mr_filter_input: contraction off,
// so the three see one float) instead of a 16 B store and two 16 B loads per point.  No float atomics anywhere: a selection's output
// depends on its points, its affine and the leaf alone.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "ll_map_refine.h"
#include "ll_ordered_float.h"

namespace ll {

__global__ void mr_init_kernel(unsigned int *mm, int *n_vox, int n_sel)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_sel) return;
    unsigned int *m = mm + (size_t)b * 8;
    m[0] = m[1] = m[2] = 0xffffffffu;  // identities of min / max in the ordered encoding
    m[3] = m[4] = m[5] = 0u;
    m[6] = m[7] = 0u;
    n_vox[b] = 0;
}

// mm[s][0..2] = min (ordered encoding), [3..5] = max, [6] = finite count
__global__ __launch_bounds__(256) void mr_bounds_kernel(const float4 *src, const MrSel *sel, const MrWork *work, int mode, unsigned int *mm)
{
    const MrWork w = work[blockIdx.x];
    const MrSel &e = sel[w.sel];
    const int end = e.n < w.first + MR_CHUNK ? e.n : w.first + MR_CHUNK;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int cnt = 0;
    for (int i = w.first + threadIdx.x; i < end; i += 256) {
        const float4 p = mr_filter_input(mode, e.aff, src[e.src_off + i]);
        if (mr_finite(p.x, p.y, p.z)) {
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
    if ((threadIdx.x & 63) == 0 && cnt > 0) {  // min / max / integer add: the result does not depend on the order
        unsigned int *m = mm + (size_t)w.sel * 8;
        for (int d = 0; d < 3; d++) {
            atomicMin(&m[d], f2ord(lo[d]));
            atomicMax(&m[3 + d], f2ord(hi[d]));
        }
        atomicAdd(&m[6], (unsigned int)cnt);
    }
}

__global__ void mr_params_kernel(const unsigned int *mm, int n_sel, float inv, VoxelParams *prm)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_sel) return;
    const unsigned int *m = mm + (size_t)b * 8;
    const float mn[3] = {ord2f(m[0]), ord2f(m[1]), ord2f(m[2])}, mx[3] = {ord2f(m[3]), ord2f(m[4]), ord2f(m[5])};
    const float iv[3] = {inv, inv, inv};
    voxel_params(mn, mx, (int)m[6], iv, prm[b]);
}

__global__ __launch_bounds__(256) void mr_key_kernel(const float4 *src, const MrSel *sel, const MrWork *work, int mode, const VoxelParams *prm,
                                                     float inv, unsigned long long *keys, unsigned int *vals)
{
    const MrWork w = work[blockIdx.x];
    const MrSel &e = sel[w.sel];
    const VoxelParams p = prm[w.sel];
    const int end = e.n < w.first + MR_CHUNK ? e.n : w.first + MR_CHUNK;
    const float iv[3] = {inv, inv, inv};
    for (int i = w.first + threadIdx.x; i < end; i += 256) {
        const unsigned int g = (unsigned int)(e.in_off + i);
        // (a selection that is not filtered needs no load: the sentinel whatever the point)
        keys[g] = p.status == VOX_OK ? mr_key(w.sel, mr_filter_input(mode, e.aff, src[e.src_off + i]), iv, p) : MR_SENTINEL;
        vals[g] = g;
    }
}

// The heads of a wavefront nearly always belong to one selection (the sorted keys carry it on top), and a cloud that was filtered
// before has a head at almost every point: one atomic per head is millions of atomics on a few hundred counters (42 ms of a 63 ms run
// over 200 key frames).  The wavefront's first head speaks for every head of its selection; a head of another selection -- a
// wavefront across a selection boundary -- adds itself.  Integer counts: order-independent.
__global__ __launch_bounds__(256) void mr_head_kernel(const unsigned long long *keys, size_t total, int *n_vox, unsigned int *is_head)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < total;
    const unsigned long long k = in ? keys[i] : MR_SENTINEL;
    const bool head = in && k != MR_SENTINEL && (i == 0 || keys[i - 1] != k);
    if (in) is_head[i] = head ? 1u : 0u;
    const int sel = head ? (int)(k >> 32) : -1;
    const unsigned long long heads = __ballot(head);
    if (heads == 0ull) return;  // (uniform over the wavefront)
    const int leader = __ffsll((long long)heads) - 1;
    const int leader_sel = __shfl(sel, leader);
    const unsigned long long same = __ballot(head && sel == leader_sel);
    if ((int)(threadIdx.x & 63) == leader)
        atomicAdd(&n_vox[leader_sel], (int)__popcll(same));
    else if (head && sel != leader_sel)
        atomicAdd(&n_vox[sel], 1);
}

// rank[i] = exclusive prefix of is_head = global voxel id of the head at i
__global__ __launch_bounds__(256) void mr_headpos_kernel(const unsigned int *is_head, const unsigned int *rank, size_t total, unsigned int *head_pos)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total && is_head[i]) head_pos[rank[i]] = (unsigned int)i;
}

// exclusive scans over the selections (one workgroup): voxels before selection s, output points before it; result[0 .. n_sel] = the
// output offsets, result[n_sel + 1 + s] = status of s
__global__ __launch_bounds__(256) void mr_offsets_kernel(const int *n_vox, const MrSel *sel, const VoxelParams *prm, int n_sel, int *vox_off, int *result,
                                                         int *n_vox_total)
{
    __shared__ int s_w[2][4];
    __shared__ int s_carry[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry[0] = s_carry[1] = 0;
    __syncthreads();
    for (int base = 0; base < n_sel; base += 256) {
        const int b = base + tid;
        int st = VOX_EMPTY, c[2] = {0, 0};  // voxels, output points
        if (b < n_sel) {
            st = prm[b].status;
            c[0] = n_vox[b];
            c[1] = st == VOX_PASSTHROUGH ? sel[b].n : c[0];
        }
        int incl[2] = {c[0], c[1]};
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const int y = __shfl_up(incl[q], off);
                if (lane >= off) incl[q] += y;
            }
        }
        if (lane == 63) s_w[0][wave] = incl[0], s_w[1][wave] = incl[1];
        __syncthreads();
        int excl[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            excl[q] = s_carry[q] + incl[q] - c[q];
            for (int w = 0; w < wave; w++) excl[q] += s_w[q][w];
        }
        if (b < n_sel) {
            vox_off[b] = excl[0];
            result[b] = excl[1];
            result[n_sel + 1 + b] = st;
        }
        __syncthreads();
        if (tid == 255) s_carry[0] = excl[0] + c[0], s_carry[1] = excl[1] + c[1];
        __syncthreads();
    }
    if (tid == 0) {
        *n_vox_total = s_carry[0];
        result[n_sel] = s_carry[1];
    }
}

// one thread per VOXEL (dense: thread t takes the t-th head), as vox_centroid_kernel
__global__ __launch_bounds__(256) void mr_centroid_kernel(const float4 *src, const MrSel *sel, int mode, const unsigned long long *keys,
                                                          const unsigned int *vals, const unsigned int *head_pos, const int *vox_off,
                                                          const int *out_off, const int *n_vox_total, size_t total, float4 *out)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)*n_vox_total) return;
    const size_t i = head_pos[t];
    const int b = (int)(keys[i] >> 32);
    const MrSel &e = sel[b];
    const float4 c = mr_centroid(mode, src, e, keys, vals, i, total);
    out[(size_t)out_off[b] + ((int)t - vox_off[b])] = mr_output(mode, e.aff, c);
}

__global__ __launch_bounds__(256) void mr_copy_kernel(const float4 *src, const MrSel *sel, const MrWork *work, int mode, const VoxelParams *prm,
                                                      const int *out_off, float4 *out)
{
    const MrWork w = work[blockIdx.x];
    if (prm[w.sel].status != VOX_PASSTHROUGH) return;
    const MrSel &e = sel[w.sel];
    const int end = e.n < w.first + MR_CHUNK ? e.n : w.first + MR_CHUNK;
    for (int i = w.first + threadIdx.x; i < end; i += 256)
        out[(size_t)out_off[w.sel] + i] = mr_output(mode, e.aff, mr_filter_input(mode, e.aff, src[e.src_off + i]));
}

#define MRCHK(x)                              \
    do {                                      \
        hipError_t e_ = (x);                  \
        if (e_ != hipSuccess) {               \
            *err = hipGetErrorString(e_);     \
            return -1;                        \
        }                                     \
    } while (0)

template <typename T>
static int mr_grow(T *&p, size_t count, const char **err)
{
    if (p) (void)hipFree(p);
    p = nullptr;
    MRCHK(hipMalloc((void **)&p, (count ? count : 1) * sizeof(T)));
    return 0;
}

int map_refine_room(MrDev &d, int64_t points, int64_t n_sel, int64_t n_work, const char **err)
{
    if (points >= 0x7fffffffLL) {
        *err = "a run holds fewer than 2^31 points";
        return -1;
    }
    if (points > d.pt_cap) {
        int64_t cap = d.pt_cap * 2 > points ? d.pt_cap * 2 : points;
        if (cap > 0x7ffffffeLL) cap = 0x7ffffffeLL;
        d.pt_cap = 0;
        if (mr_grow(d.keys, (size_t)cap, err) || mr_grow(d.keys2, (size_t)cap, err) || mr_grow(d.vals, (size_t)cap, err) ||
            mr_grow(d.vals2, (size_t)cap, err) || mr_grow(d.is_head, (size_t)cap, err) || mr_grow(d.rank, (size_t)cap, err) ||
            mr_grow(d.head_pos, (size_t)cap, err))
            return -1;
        size_t t1 = 0, t2 = 0;
        MRCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, d.keys, d.keys2, d.vals, d.vals2, (int)cap, 0, 64));
        MRCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, d.is_head, d.rank, (int)cap));
        d.tmp_bytes = t1 > t2 ? t1 : t2;
        if (d.tmp) (void)hipFree(d.tmp);
        d.tmp = nullptr;
        MRCHK(hipMalloc(&d.tmp, d.tmp_bytes ? d.tmp_bytes : 1));
        d.pt_cap = cap;
    }
    if (n_sel > d.sel_cap) {
        const int64_t cap = d.sel_cap * 2 > n_sel ? d.sel_cap * 2 : n_sel;
        d.sel_cap = 0;
        if (mr_grow(d.sel, (size_t)cap, err) || mr_grow(d.mm, (size_t)cap * 8, err) || mr_grow(d.prm, (size_t)cap, err) ||
            mr_grow(d.n_vox, (size_t)cap, err) || mr_grow(d.vox_off, (size_t)cap, err) || mr_grow(d.result, (size_t)cap * 2 + 1, err))
            return -1;
        if (!d.n_vox_total && mr_grow(d.n_vox_total, 1, err)) return -1;
        d.sel_cap = cap;
    }
    if (n_work > d.work_cap) {
        const int64_t cap = d.work_cap * 2 > n_work ? d.work_cap * 2 : n_work;
        d.work_cap = 0;
        if (mr_grow(d.work, (size_t)cap, err)) return -1;
        d.work_cap = cap;
    }
    return 0;
}

void map_refine_free(MrDev &d)
{
    void *ptrs[] = {d.keys, d.keys2, d.vals, d.vals2, d.is_head, d.rank, d.head_pos, d.tmp, d.sel, d.work, d.mm, d.prm, d.n_vox, d.vox_off, d.result, d.n_vox_total};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    d = MrDev();
}

int map_refine_chain(MrDev &d, const float4 *src, int mode, int n_sel, int n_work, int total, float leaf, float4 *out, hipStream_t s, const char **err)
{
    if (n_sel < 1 || n_sel > d.sel_cap || n_work < 1 || n_work > d.work_cap || total < 1 || total > d.pt_cap) {
        *err = "a chain beyond the room made for it";
        return -1;
    }
    const float inv = 1.0f / leaf;  // inverse_leaf_size_ = 1 / leaf_size_ (float)
    const int gs = (n_sel + 63) / 64, gt = (int)(((size_t)total + 255) / 256);
    int *out_off = d.result;
    hipLaunchKernelGGL(mr_init_kernel, dim3(gs), dim3(64), 0, s, d.mm, d.n_vox, n_sel);
    hipLaunchKernelGGL(mr_bounds_kernel, dim3(n_work), dim3(256), 0, s, src, d.sel, d.work, mode, d.mm);
    hipLaunchKernelGGL(mr_params_kernel, dim3(gs), dim3(64), 0, s, d.mm, n_sel, inv, d.prm);
    hipLaunchKernelGGL(mr_key_kernel, dim3(n_work), dim3(256), 0, s, src, d.sel, d.work, mode, d.prm, inv, d.keys, d.vals);
    int sel_bits = 1;
    while ((1 << sel_bits) < n_sel + 1 && sel_bits < 31) sel_bits++;
    // hipcub's temporary storage was sized for pt_cap items and all 64 key bits (map_refine_room); what THIS call needs is asked for
    // again -- host-only work -- and checked, so that a smaller sort or scan that wanted more could never write past it
    size_t need_sort = 0, need_scan = 0;
    MRCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need_sort, d.keys, d.keys2, d.vals, d.vals2, total, 0, 32 + sel_bits, s));
    MRCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, need_scan, d.is_head, d.rank, total, s));
    if (need_sort > d.tmp_bytes || need_scan > d.tmp_bytes) {
        *err = "the sort's temporary storage is below what this call needs";
        return -1;
    }
    size_t tb = d.tmp_bytes;
    // the leaf index has at most 31 bits, the selection sel_bits: sorting the low 32 + sel_bits bits orders everything, and the
    // sentinel's bits there are all ones (2^sel_bits - 1 >= n_sel is above every selection): it sorts last
    MRCHK(hipcub::DeviceRadixSort::SortPairs(d.tmp, tb, d.keys, d.keys2, d.vals, d.vals2, total, 0, 32 + sel_bits, s));
    hipLaunchKernelGGL(mr_head_kernel, dim3(gt), dim3(256), 0, s, d.keys2, (size_t)total, d.n_vox, d.is_head);
    tb = d.tmp_bytes;
    MRCHK(hipcub::DeviceScan::ExclusiveSum(d.tmp, tb, d.is_head, d.rank, total, s));
    hipLaunchKernelGGL(mr_headpos_kernel, dim3(gt), dim3(256), 0, s, d.is_head, d.rank, (size_t)total, d.head_pos);
    hipLaunchKernelGGL(mr_offsets_kernel, dim3(1), dim3(256), 0, s, d.n_vox, d.sel, d.prm, n_sel, d.vox_off, d.result, d.n_vox_total);
    hipLaunchKernelGGL(mr_centroid_kernel, dim3(gt), dim3(256), 0, s, src, d.sel, mode, d.keys2, d.vals2, d.head_pos, d.vox_off, out_off, d.n_vox_total,
                       (size_t)total, out);
    hipLaunchKernelGGL(mr_copy_kernel, dim3(n_work), dim3(256), 0, s, src, d.sel, d.work, mode, d.prm, out_off, out);
    MRCHK(hipGetLastError());
    return 0;
}

}  // namespace ll
