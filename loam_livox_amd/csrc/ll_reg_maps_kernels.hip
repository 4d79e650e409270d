// ll_reg_maps_kernels.hip -- reg_solve_maps_kernel and launch_reg_solve_maps (declared in ll_device.h, called from ll_api_reg.hip): the
// solver of a map per slot (ll_reg_enqueue_fe_maps).  It is reg_solve_kernel (ll_reg_solve_kernels.hip) with the surface map of every
// scan taken from a device table (map_tab[2 b + 1]) and a per-scan choice of form, built on the same solve_fast3 (ll_reg_solve_fast.h).
// A translation unit of its own: a second kernel built on solve_fast3 in reg_solve_kernel's module changes how that kernel is compiled
// (two SGPR and two VGPR spills moved when it was tried); compiled apart, reg_solve_kernel is the code it was.
#include <hip/hip_runtime.h>

#include "ll_reg_solve_fast.h"

namespace ll {

__global__ __launch_bounds__(RS_THREADS) void reg_solve_maps_kernel(RegDev rd, RegConst rc, const Grid *map_tab, int grp_min)
{
    __shared__ SolveShared sh;
    __shared__ uint4 s_raw[PT_LDS_BYTES / 16];
    const SolveTicket tk = solve_fast_ticket(rd, rc, sh);
    const int b = tk.b, g = tk.g, G = tk.G;
    RegState *st = rd.state + b;
    if (st->done) return;  // the same answer for every member: the epilogue that sets it runs behind the group's barriers
    const int nS = rd.n_surf[b], nC = rd.n_corner[b];
    if (reg_maps_class(rc, nC, nS, grp_min) != (G > 1 ? 3 : 2)) return;  // (the small solver's launches, or this kernel's other launch, have it)
    if (!solve_fast_check(rd, rc, b, g, nC, nS, st)) return;
    solve_fast_group_fields(rc, g, G, sh);
    const f4 *map_surf = map_tab[2 * b + 1].pts;
    if (G > 1)
        solve_fast3<true>(rd, rc, map_surf, b, st, sh, s_raw);
    else
        solve_fast3<false>(rd, rc, map_surf, b, st, sh, s_raw);
}

// (the caller has checked that one of the two table forms holds the batch: no motion deblur, nothing beyond reg_solve_kernel's size)
void launch_reg_solve_maps(const RegDev &rd, const RegConst &rc, const Grid *map_tab, int n_scans, const RegMapsClasses &cls, int iter, hipStream_t s)
{
    for (int c = 0; c < 2; c++)
        if (cls.n[c] > 0) launch_reg_solve_small_maps(rd, rc, map_tab, n_scans, c, cls.max_nc[c], cls.max_ns[c], iter, s);
    RegConst one = rc;  // (rc.solve_group is what the kernel reads: one workgroup per scan, or a group of LL_GRP)
    one.solve_group = 1;
    if (cls.n[2] > 0) hipLaunchKernelGGL(reg_solve_maps_kernel, dim3(n_scans), dim3(RS_THREADS), 0, s, rd, one, map_tab, cls.grp_min);
    if (cls.n[3] > 0) {
        one.solve_group = LL_GRP;
        hipLaunchKernelGGL(reg_solve_maps_kernel, dim3(n_scans * LL_GRP), dim3(RS_THREADS), 0, s, rd, one, map_tab, cls.grp_min);
    }
}

}  // namespace ll
