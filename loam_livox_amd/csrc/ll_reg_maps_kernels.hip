// ll_reg_maps_kernels.hip -- reg_solve_maps_kernel: reg_solve_kernel (ll_reg_kernels.hip) with the surface map of every scan taken from
// the map table of a map-per-slot registration (ll_reg_enqueue_fe_maps).  It is built on the same solve_fast3 and therefore compiles
// that file's solver code, but as a module of its own, so that the single-map kernels of ll_reg_kernels.hip stay exactly the code they
// were: under LL_REG_MAPS_TU that file leaves out its kernels and launch wrappers and defines reg_solve_maps_kernel and
// launch_reg_solve_maps instead.
#define LL_REG_MAPS_TU 1
#include "ll_reg_kernels.hip"
