// ll_reg_solve_kernels.hip -- the registrar's single-map solver kernels and the host-side choice between them (launch_reg_solve,
// declared in ll_device.h, called from ll_api_reg.hip once per ICP iteration):
//   small  voxel-filtered scans                               -> reg_solve_small_kernel (ll_reg_small_kernels.hip, a unit of its own)
//   fast   no motion deblur, every scan <= FAST_MAX_BLOCKS    -> reg_solve_kernel: solve_fast3 (ll_reg_solve_fast.h)
//   big    everything else                                    -> reg_solve_big_kernel<DEBLUR> (ll_reg_big_path.h): solve_big per scan, or
//                                                                inside it solve_general (ll_reg_solve_general.h) for a scan beyond
//                                                                LL_TABLE_MAX_BLOCKS and for the force_general test switch
// reg_solve_kernel and reg_solve_big_kernel<0/1> are compiled in ONE module on purpose: they share non-inlined device functions
// (block_sum_int), whose code and the register allocation around their calls depend on the set of callers ("Which
// solvers share a module").  The map-per-slot form of reg_solve_kernel is ll_reg_maps_kernels.hip.
#include <hip/hip_runtime.h>

#include "ll_reg_big_path.h"
#include "ll_reg_solve_fast.h"

namespace ll {

// The Mid-40 batches: no motion deblur, every scan within FAST_MAX_BLOCKS (launch_reg_solve decides per batch from the host's feature
// counts; everything else goes to reg_solve_big_kernel).
__global__ __launch_bounds__(RS_THREADS) void reg_solve_kernel(RegDev rd, RegConst rc, const f4 *map_surf)
{
    __shared__ SolveShared sh;
    // 152 KB: hash table -> plane table + record cache; the inlier phase's tables in between
    __shared__ uint4 s_raw[PT_LDS_BYTES / 16];
    const SolveTicket tk = solve_fast_ticket(rd, rc, sh);
    const int b = tk.b, g = tk.g, G = tk.G;
    RegState *st = rd.state + b;
    if (st->done) return;  // the same answer for every member: the epilogue that sets it runs behind the group's barriers
    const int nS = rd.n_surf[b], nC = rd.n_corner[b];
    if (!solve_fast_check(rd, rc, b, g, nC, nS, st)) return;
    solve_fast_group_fields(rc, g, G, sh);
    if (G > 1)
        solve_fast3<true>(rd, rc, map_surf, b, st, sh, s_raw);
    else
        solve_fast3<false>(rd, rc, map_surf, b, st, sh, s_raw);
}

// batches reg_solve_kernel holds: no motion deblur, the largest scan within FAST_MAX_BLOCKS (planes padded to whole rounds + lines)
bool reg_solve_fast_eligible(const RegConst &rc, int max_nc, int max_ns)
{
    return !rc.if_motion_deblur && !rc.force_general && padded_block_count(max_nc, max_ns) <= FAST_MAX_BLOCKS;
}
void launch_reg_solve(const RegDev &rd, const RegConst &rc, const Grid &gs, int n_scans, int max_nc, int max_ns, int iter, hipStream_t s)
{
    if (reg_solve_small_eligible(rc, max_nc, max_ns))  // voxel-filtered scans: one or four wavefronts per scan (ll_reg_small_kernels.hip)
        launch_reg_solve_small(rd, rc, gs, n_scans, max_nc, max_ns, iter, s);
    else if (reg_solve_fast_eligible(rc, max_nc, max_ns))  // Mid-40 batches: solve_fast3 (one workgroup per scan, or a group of them for small batches)
        hipLaunchKernelGGL(reg_solve_kernel, dim3(n_scans * (rc.solve_group > 1 ? rc.solve_group : 1)), dim3(RS_THREADS), 0, s, rd, rc, gs.pts);
    else if (rc.if_motion_deblur)
        hipLaunchKernelGGL(reg_solve_big_kernel<1>, dim3(n_scans), dim3(RS_THREADS), 0, s, rd, rc, gs.pts);
    else
        hipLaunchKernelGGL(reg_solve_big_kernel<0>, dim3(n_scans), dim3(RS_THREADS), 0, s, rd, rc, gs.pts);
}

}  // namespace ll
