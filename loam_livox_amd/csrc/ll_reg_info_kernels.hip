// ll_reg_info_kernels.hip -- reg_information_kernel and its launch wrapper: the Gauss-Newton matrix, gradient and cost of every scan's
// last linearisation (ll_reg_information; definition and the order of the sums: ll_reg_info_core.h).
//
// One workgroup of 256 threads per scan, launched once per registration behind the last ICP iteration.  A thread walks the candidates
// c = tid, tid + 256, ... < n_corner + n_surf: flag -> neighbour positions -> two or three map points and the feature, block constants
// through block_line / block_plane, 28 fp64 accumulators in registers.  The wavefronts reduce by the butterfly of
// ll_reg_solve_common.h, four partial sums meet in LDS.  No traffic between workgroups, no wait on anything; gated, aborted,
// iteration-less and empty scans write their zero record and leave.  A translation unit of its own: no solver kernel shares its code.
#include <hip/hip_runtime.h>

#include "ll_reg_info_core.h"
#include "ll_reg_solve_common.h"

namespace ll {

static_assert(sizeof(InfoRecord) == LL_INFO_RECORD_DOUBLES * sizeof(double) + 4 * sizeof(int32_t), "the record is 43 doubles and four words");
static_assert(LL_INFO_THREADS % 64 == 0, "whole wavefronts");

template <int DEBLUR, bool TABLE>
__global__ __launch_bounds__(LL_INFO_THREADS) void reg_information_kernel(RegDev rd, RegConst rc, Grid gc, Grid gs, const Grid *map_tab, InfoRecord *out,
                                                                          int n_scans, const float2 *ts_tab)
{
    constexpr int W = LL_INFO_THREADS / 64;
    __shared__ double s_red[W][LL_NACC];
    __shared__ double s_sum[LL_NACC];
    __shared__ int s_cnt[W][2];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (b >= n_scans) return;
    const RegState *st = rd.state + b;
    InfoRecord *o = out + b;
    int nC = rd.n_corner[b], nS = rd.n_surf[b];
    nC = nC < 0 ? 0 : (nC > rd.cap_c ? rd.cap_c : nC);  // (the host refused larger scans: the loops below stay inside the scan's slots)
    nS = nS < 0 ? 0 : (nS > rd.cap_s ? rd.cap_s : nS);
    const int status = info_status(st->gated, st->aborted, st->icp_iters, nC + nS);  // (uniform)
    if (status) {
        double *od = reinterpret_cast<double *>(o);
        if (tid < LL_INFO_RECORD_DOUBLES) od[tid] = 0.0;
        if (tid == 0) o->n_line = 0, o->n_plane = 0, o->status = status, o->reserved = 0;
        return;
    }
    if (TABLE) {
        gc = map_tab[2 * b];
        gs = map_tab[2 * b + 1];
    }
    InfoScan s;
    s.flag0 = rd.blk_flag0 + (size_t)b * rd.cap;
    s.nn = reinterpret_cast<const int *>(rd.nn + (size_t)b * rd.cap);
    s.corner = reinterpret_cast<const float *>(rd.corner_feat + (size_t)b * rd.feat_stride_c);
    s.surf = reinterpret_cast<const float *>(rd.surf_feat + (size_t)b * rd.feat_stride_s);
    s.map_c = gc.pts;
    s.map_s = gs.pts;
    // points in a map = the closing entry of its cell table; a map without points or table has none to read
    s.n_map_c = (gc.pts && gc.cell_start) ? gc.cell_start[(size_t)gc.nx * gc.ny * gc.nz] : 0;
    s.n_map_s = (gs.pts && gs.cell_start) ? gs.cell_start[(size_t)gs.nx * gs.ny * gs.nz] : 0;
    s.n_corner = nC;
    s.n_surf = nS;
    s.cap_c = rd.cap_c;
    s.min_ts = rc.min_ts;
    s.max_ts = rc.max_ts;
    if (TABLE && DEBLUR) {  // a time range per scan (ll_reg_set_time_ranges); behind the status test: idle and gated slots have left
        const float2 ts = ts_tab[b];
        s.min_ts = ts.x;
        s.max_ts = ts.y;
    }
    s.huber_a = rc.huber_a;
    double x[7];
#pragma unroll
    for (int i = 0; i < 7; i++) {
        s.pose_last[i] = st->pose_last[i];
        x[i] = st->inc[i];
    }
    InfoCtx c;
    info_context<DEBLUR>(x, c);
    double acc[LL_NACC];
    int n_line, n_plane;
    info_thread<DEBLUR>(s, c, tid, LL_INFO_THREADS, acc, n_line, n_plane);
    wave_sum_acc(acc, s_red[wave], lane);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_line += __shfl_xor(n_line, off);
        n_plane += __shfl_xor(n_plane, off);
    }
    if (lane == 0) s_cnt[wave][0] = n_line, s_cnt[wave][1] = n_plane;
    __syncthreads();
    if (tid < LL_NACC) {
        double v = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < W; w++) v += s_red[w][tid];
        s_sum[tid] = v;
    }
    __syncthreads();
    if (tid < LL_INFO_RECORD_DOUBLES) reinterpret_cast<double *>(o)[tid] = info_record_entry(s_sum, tid);
    if (tid == 64) {
        int nl = 0, np = 0;
#pragma unroll
        for (int w = 0; w < W; w++) nl += s_cnt[w][0], np += s_cnt[w][1];
        o->n_line = nl, o->n_plane = np, o->status = 0, o->reserved = 0;
    }
}

void launch_reg_information(const RegDev &rd, const RegConst &rc, const Grid &gc, const Grid &gs, const Grid *map_tab, InfoRecord *out, int n_scans,
                            hipStream_t s, const float2 *ts_tab)
{
    if (n_scans <= 0) return;
    const dim3 grid(n_scans), block(LL_INFO_THREADS);
    if (map_tab && rc.if_motion_deblur)  // (the caller has a table of ranges: ll_reg_enqueue_fe_maps refuses deblur without one)
        hipLaunchKernelGGL((reg_information_kernel<1, true>), grid, block, 0, s, rd, rc, gc, gs, map_tab, out, n_scans, ts_tab);
    else if (map_tab)
        hipLaunchKernelGGL((reg_information_kernel<0, true>), grid, block, 0, s, rd, rc, gc, gs, map_tab, out, n_scans, ts_tab);
    else if (rc.if_motion_deblur)
        hipLaunchKernelGGL((reg_information_kernel<1, false>), grid, block, 0, s, rd, rc, gc, gs, map_tab, out, n_scans, ts_tab);
    else
        hipLaunchKernelGGL((reg_information_kernel<0, false>), grid, block, 0, s, rd, rc, gc, gs, map_tab, out, n_scans, ts_tab);
}

}  // namespace ll
