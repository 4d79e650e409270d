// ll_reg_aux_kernels.hip -- the registrar's kernels that are neither a search nor a solver, each followed by its launch wrapper
// (declared in ll_device.h, called from ll_api_reg.hip and ll_api_history.hip):
//   reg_finalize_kernel    : accept / reject of a finished registration (point_cloud_registration.hpp:559-573)
//   cloud_transform_kernel : a cloud into the map frame with a pose in device memory
//   reg_merge_heads_kernel : Mid-100, the feature clouds of a sweep's heads concatenated on the device
//   history_concat_kernel  : the match buffer's frames into one cloud
//   debug_quintic_kernel   : test tap of the line-search fit (ll_debug_quintic)
//   debug_lm_sequence_kernel : test tap of the LM controller, lane-0 form against wavefront form (ll_debug_lm_sequence)
// A translation unit of its own: nothing here shares device code with the query kernels or the solvers.
#include <hip/hip_runtime.h>

#include "ll_device.h"
#include "ll_reg_solve_common.h"

namespace ll {

__global__ void reg_finalize_kernel(RegDev rd, RegConst rc, int n_scans)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_scans) return;
    RegState *st = rd.state + b;
    st->result = 1;
    st->accepted = 1;
    if (st->gated || st->icp_iters == 0) return;
    st->inlier_thr = st->inlier_thr * st->final_cost / st->initial_cost;  // PCR:559
    const float minimize_cost = (float)st->final_cost;                    // PCR:192,519
    // (an aborted solve, or anything non-finite that reached the pose, is a rejection too: NaN compares false with both limits)
    const bool broken = st->aborted || !((st->angular_diff - st->angular_diff) == 0.0) || !((st->final_cost - st->final_cost) == 0.0);
    if (broken || st->angular_diff > (double)rc.para_max_angular_rate || minimize_cost > rc.max_final_cost) {  // PCR:561
        for (int i = 0; i < 7; i++) st->pose_curr[i] = st->pose_last[i];
        st->result = 0;
        st->accepted = 0;
    }
}
void launch_reg_finalize(const RegDev &rd, const RegConst &rc, int n_scans, hipStream_t s)
{
    hipLaunchKernelGGL(reg_finalize_kernel, dim3((n_scans + 63) / 64), dim3(64), 0, s, rd, rc, n_scans);
}

__global__ void cloud_transform_kernel(const float4 *in, float4 *out, int n, const double *pose)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double p[7];
#pragma unroll
    for (int k = 0; k < 7; k++) p[k] = pose[k];
    const float4 v = in[i];
    float o[3];
    point_to_map(p, v.x, v.y, v.z, o);
    out[i] = make_float4(o[0], o[1], o[2], v.w);  // intensity copied, PCR:659
}
void launch_cloud_transform(const float4 *in, float4 *out, int n, const double *d_pose, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(cloud_transform_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n, d_pose);
}

// Deskewed clouds, step 1: the constants of a collected registration out of the solver states into records the consumer owns
// (the states are overwritten by the next enqueue's upload).  One lane per slot.
__global__ void undistort_snapshot_kernel(const RegState *state, int first, int n, int deblur, float min_ts, float max_ts, const float2 *ts_tab,
                                          UndistortRec *recs)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const RegState *st = state + first + k;
    UndistortRec *o = recs + first + k;
    const bool gated = st->gated != 0;  // PCR:199: no increment was estimated -- identity, I p + 0 is exact
    for (int i = 0; i < 7; i++) {
        o->pose_last[i] = st->pose_last[i];
        o->pose_curr[i] = gated ? st->pose_last[i] : st->pose_curr[i];
    }
    for (int i = 0; i < 3; i++) o->inc_t[i] = gated ? 0.0 : st->inc[4 + i];
    o->theta = gated ? 0.0 : st->interp_theta;
    for (int i = 0; i < 9; i++) {
        o->hat[i] = gated ? 0.0 : st->hat[i];
        o->hat_sq[i] = gated ? 0.0 : st->hat_sq[i];
    }
    o->deblur = deblur;
    o->min_ts = ts_tab ? ts_tab[first + k].x : min_ts;  // (a registration with a time range per scan: ll_reg_set_time_ranges)
    o->max_ts = ts_tab ? ts_tab[first + k].y : max_ts;
    o->pad = 0;
}
void launch_undistort_snapshot(const RegState *state, int first, int n, const RegConst &rc, UndistortRec *recs, hipStream_t s, const float2 *ts_tab)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(undistort_snapshot_kernel, dim3((n + 63) / 64), dim3(64), 0, s, state, first, n, rc.if_motion_deblur, rc.min_ts, rc.max_ts, ts_tab, recs);
}

// Deskewed clouds, step 2: pointcloudAssociateToMap( in, out, if_undistore = 1 ) (PCR:673-685) for the slots of a batch in one launch.
// One lane per point; blockIdx.y = slot.  The slot's job and its record are indexed by the block index alone, so they arrive through
// scalar loads, once per wavefront, ahead of the per-point work.  32 bytes of traffic per point and, in the Rodrigues branch, the fp64
// sin / cos of point_to_map_undistort (the library's: the bits the registrar's searches computed).  Intensity copied (PCR:659).
__global__ __launch_bounds__(256) void cloud_undistort_kernel(const UndistortRec *__restrict__ recs, const UndistortJob *__restrict__ jobs, UndistortJob one,
                                                              const float4 *__restrict__ src, const int *__restrict__ pick, const float *__restrict__ pick_w,
                                                              float4 *__restrict__ dst)
{
    const UndistortJob j = jobs ? jobs[blockIdx.y] : one;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= j.n) return;
    const UndistortRec &c = recs[j.rec];
    float4 v;
    if (pick) {  // a selection by position (the extractor's full cloud): point pick[i] of the slot, its time stamp from the plane beside it
        const int k = pick[j.src_off + i];
        v = src[j.src_off + k];
        v.w = pick_w[j.src_off + k];  // intensity := time stamp, LFE:246,255
    } else {
        v = src[j.src_off + i];
    }
    float o[3];
    point_to_map_undistort(c.pose_last, c.pose_curr, c.inc_t, c.theta, c.hat, c.hat_sq, c.deblur, c.min_ts, c.max_ts, v, o);
    dst[j.dst_off + i] = make_float4(o[0], o[1], o[2], v.w);
}
void launch_cloud_undistort(const UndistortRec *recs, const UndistortJob *d_jobs, const UndistortJob &one, int n_slots, int max_n, const float4 *src,
                            const int *pick, const float *pick_w, float4 *dst, hipStream_t s)
{
    if (n_slots <= 0 || max_n <= 0) return;
    for (int first = 0; first < n_slots; first += 65535) {  // (grid.y is a 16-bit dimension)
        const int ny = n_slots - first < 65535 ? n_slots - first : 65535;
        hipLaunchKernelGGL(cloud_undistort_kernel, dim3((max_n + 255) / 256, ny), dim3(256), 0, s, recs, d_jobs ? d_jobs + first : nullptr, one, src, pick, pick_w, dst);
    }
}

// Mid-100: the selected features of `heads` consecutive extractor slots (the lidars of one sweep) become ONE registrar scan,
// corner clouds and surface clouds each concatenated in head order (laser_feature_extractor.hpp:348-358), device to device.
// grid (chunks of the extractor stride, n_scans * heads, 2 kinds).  Points beyond the registrar's capacity are not written;
// the counts are, so the host sees the overflow.
__global__ void reg_merge_heads_kernel(const float4 *fe_corner, const float4 *fe_surf, const int *fe_nc, const int *fe_ns, int fe_stride,
                                       int heads, float4 *dst_corner, float4 *dst_surf, int *dst_nc, int *dst_ns, int dst_stride)
{
    const int slot = blockIdx.y, kind = blockIdx.z;
    const int b = slot / heads, h = slot - b * heads;
    const int *cnt = kind ? fe_ns : fe_nc;
    int off = 0;
    for (int k = 0; k < h; k++) off += cnt[b * heads + k];
    const int n = cnt[slot];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && off + i < dst_stride) {
        const float4 *src = (kind ? fe_surf : fe_corner) + (size_t)slot * fe_stride;
        float4 *dst = (kind ? dst_surf : dst_corner) + (size_t)b * dst_stride;
        dst[off + i] = src[i];
    }
    if (i == 0 && h == heads - 1) (kind ? dst_ns : dst_nc)[b] = off + n;
}
void launch_reg_merge_heads(const float4 *fe_corner, const float4 *fe_surf, const int *fe_nc, const int *fe_ns, int fe_stride, int heads,
                            float4 *dst_corner, float4 *dst_surf, int *dst_nc, int *dst_ns, int dst_stride, int n_scans, hipStream_t s)
{
    hipLaunchKernelGGL(reg_merge_heads_kernel, dim3((fe_stride + 255) / 256, n_scans * heads, 2), dim3(256), 0, s, fe_corner, fe_surf, fe_nc,
                       fe_ns, fe_stride, heads, dst_corner, dst_surf, dst_nc, dst_ns, dst_stride);
}

// The history's frames, oldest first, into one cloud (laser_mapping.hpp:519-530): segment g of the table is {first point of the frame in
// `frames`, its first position in `out`}, the table ends with {-, total}.  One launch instead of one device-to-device copy per frame
// (20 frames x 2 kinds per refresh of the match buffer: the copies' launch overhead was a third of the refresh).
__global__ __launch_bounds__(256) void history_concat_kernel(const float4 *frames, const int2 *table, int n_seg, float4 *out)
{
    __shared__ int2 s_tab[LL_HIST_CONCAT_MAX + 1];
    for (int e = threadIdx.x; e <= n_seg; e += 256) s_tab[e] = table[e];
    __syncthreads();
    const int total = s_tab[n_seg].y;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        int lo = 0, hi = n_seg - 1;  // the last segment whose first output position is <= i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_tab[mid].y <= i)
                lo = mid;
            else
                hi = mid - 1;
        }
        out[i] = frames[(size_t)s_tab[lo].x + (size_t)(i - s_tab[lo].y)];
    }
}
void launch_history_concat(const float4 *frames, const int2 *d_table, int n_seg, int total, float4 *out, hipStream_t s)
{
    if (n_seg <= 0 || total <= 0) return;
    const int blocks = (total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024;
    hipLaunchKernelGGL(history_concat_kernel, dim3(blocks), dim3(256), 0, s, frames, d_table, n_seg, out);
}

// test tap (ll_debug_quintic): the sequential and the wavefront form of the fit on n argument sets, one wavefront each
__global__ __launch_bounds__(64) void debug_quintic_kernel(const double *args, int n, double *out_seq, double *out_wave)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const double *a = args + 10 * (size_t)i;
    const double w = lm_quintic_min_step_wave(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], lane);
    if (lane == 0) {
        out_wave[i] = w;
        out_seq[i] = lm_quintic_min_step(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]);
    }
}
void launch_debug_quintic(const double *args, int n, double *out_seq, double *out_wave, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(debug_quintic_kernel, dim3(n), dim3(64), 0, s, args, n, out_seq, out_wave);
}

// test tap (ll_debug_lm_sequence): the controller on lane 0 (lm_begin, lm_init, lm_update_lane0) and on the wavefront (ll_lm_wave.h) over
// the same scripted evaluations, one wavefront per sequence.  hdr = {x0[7], bound, max_iter, n_active, calls, -} per sequence; after call k
// the two LmCtl go to img_*[(i * max_calls + k) * sizeof(LmCtl)] and the return values to ret_*[i * max_calls + k].  A sequence ends
// with the first call either form answers with 0.
__global__ __launch_bounds__(64) void debug_lm_sequence_kernel(const double *hdr, const double *evals, int n, int max_calls, unsigned int *img_seq,
                                                               unsigned int *img_wave, int *ret_seq, int *ret_wave)
{
    constexpr int WORDS = (int)(sizeof(LmCtl) / sizeof(unsigned int));
    static_assert(sizeof(LmCtl) % sizeof(unsigned int) == 0, "LmCtl is copied in 32-bit words");
    __shared__ LmCtl cs, cw;
    __shared__ double sum[LL_NACC], fit_s[10], fit_w[10];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const double *h = hdr + 12 * (size_t)i;
    for (int w = lane; w < WORDS; w += 64) ((unsigned int *)&cs)[w] = 0u, ((unsigned int *)&cw)[w] = 0u;
    __syncthreads();
    const int max_iter = (int)h[8], n_active = (int)h[9];
    int calls = (int)h[10];
    calls = calls < max_calls ? calls : max_calls;
    if (lane == 0) {
        double x0[7];
        for (int k = 0; k < 7; k++) x0[k] = h[k];
        lm_begin(cs, x0, max_iter, h[7]);
        lm_begin(cw, x0, max_iter, h[7]);
    }
    for (int k = 0; k < calls; k++) {
        const size_t slot = (size_t)i * max_calls + k;
        __syncthreads();
        if (lane < LL_NACC) sum[lane] = evals[slot * LL_NACC + lane];
        __syncthreads();
        int rs, rw;
        if (k == 0) {
            rs = lane == 0 ? lm_init(cs, sum, n_active) : 0;
            rw = lmw_init(cw, sum, n_active, lane);
        } else {
            rs = lm_update_lane0(cs, sum, fit_s, lane);
            rw = lmw_update(cw, sum, fit_w, lane);
        }
        rs = __shfl(rs, 0);
        rw = __shfl(rw, 0);
        __syncthreads();
        for (int w = lane; w < WORDS; w += 64) {
            img_seq[slot * WORDS + w] = ((const unsigned int *)&cs)[w];
            img_wave[slot * WORDS + w] = ((const unsigned int *)&cw)[w];
        }
        if (lane == 0) ret_seq[slot] = rs, ret_wave[slot] = rw;
        if (!rs || !rw) break;
    }
}
void launch_debug_lm_sequence(const double *hdr, const double *evals, int n, int max_calls, unsigned int *img_seq, unsigned int *img_wave, int *ret_seq,
                              int *ret_wave, hipStream_t s)
{
    if (n > 0 && max_calls > 0)
        hipLaunchKernelGGL(debug_lm_sequence_kernel, dim3(n), dim3(64), 0, s, hdr, evals, n, max_calls, img_seq, img_wave, ret_seq, ret_wave);
}
int debug_lm_ctl_bytes() { return (int)sizeof(LmCtl); }

}  // namespace ll
