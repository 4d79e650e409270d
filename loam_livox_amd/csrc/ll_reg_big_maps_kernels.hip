// ll_reg_big_maps_kernels.hip -- reg_solve_big_maps_kernel and launch_reg_solve_big_maps (declared in ll_device.h, called from
// ll_api_reg.hip): the solver of a motion-deblur registration with a map per slot (ll_reg_set_time_ranges + ll_reg_enqueue_fe_maps).
// It is reg_solve_big_kernel<1>'s plane-table path (solve_big<1>, ll_reg_big_path.h, unchanged) with the surface map of every scan
// taken from the device table (map_tab[2 b + 1]) and the scan's time range from ts_tab[b]; both are uniform per workgroup and are read
// once, through scalar loads, ahead of the work.  solve_general has no form here: the host refuses a scan that scan_is_compact would
// send there before anything is launched.
// A translation unit of its own, for the reason ll_reg_maps_kernels.hip gives: a second kernel in ll_reg_solve_kernels.hip's module
// moves registers and spills of the kernels already there.  Compiled apart, they are the code they were.
#include <hip/hip_runtime.h>

#include "ll_reg_big_path.h"

namespace ll {

__global__ __launch_bounds__(RS_THREADS) void reg_solve_big_maps_kernel(RegDev rd, RegConst rc, const Grid *__restrict__ map_tab, const float2 *__restrict__ ts_tab)
{
    __shared__ SolveShared sh;
    __shared__ uint4 s_raw[PT_LDS_BYTES / 16];
    const int b = blockIdx.x;
    RegState *st = rd.state + b;
    if (st->done) return;  // idle and gated slots: an empty Grid{} in the table, nothing to read in either table
    const f4 *map_surf = map_tab[2 * b + 1].pts;
    const float2 ts = ts_tab[b];
    rc.min_ts = ts.x;  // (rc is this kernel's own copy of the constants: solve_big reads the range nowhere else)
    rc.max_ts = ts.y;
    if (!scan_is_compact(rd, rc, b)) return;  // (refused by the host; a scan that came through anyway is left as it was enqueued)
    if (threadIdx.x == 0) {
        sh.grp_g = 0;
        sh.grp_G = 1;
        sh.grp_seq = 0;
        sh.xch_seq = 0;
        sh.xch_epoch = rc.xch_epoch;
        sh.grp_abort = 0;
    }
    __syncthreads();
    solve_big<1>(rd, rc, map_surf, b, st, sh, s_raw);
}

void launch_reg_solve_big_maps(const RegDev &rd, const RegConst &rc, const Grid *map_tab, const float2 *ts_tab, int n_scans, hipStream_t s)
{
    RegConst one = rc;
    one.solve_group = 1;  // one workgroup per scan
    hipLaunchKernelGGL(reg_solve_big_maps_kernel, dim3(n_scans), dim3(RS_THREADS), 0, s, rd, one, map_tab, ts_tab);
}

}  // namespace ll
