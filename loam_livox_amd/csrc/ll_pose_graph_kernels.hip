// ll_pose_graph_kernels.hip -- the pose-graph optimiser's one kernel: a workgroup per graph runs the whole Levenberg-Marquardt loop of
// ll_pose_graph_core.h.  A graph belongs to one workgroup, so no workgroup waits for another; the loop makes at most
// max_num_iterations passes of a bounded number of barrier-separated phases, every barrier is reached by all work items of the
// workgroup (the branches around them read the shared scalars item 0 wrote before the barrier in front), and nothing spins.
// Workspace lives in global memory (a graph's few hundred kilobytes stay in L2); the vector of the triangular solves is in LDS for
// graphs of up to 342 poses.
#include <hip/hip_runtime.h>

#include "ll_pose_graph.h"

namespace ll {

__global__ __launch_bounds__(LL_PG_THREADS) void pg_solve_kernel(const PgView v, int n_graphs)
{
    __shared__ PgShared sh;
    const int gi = blockIdx.x;
    if (gi >= n_graphs) return;
    pg_solve_graph(v, gi, &sh, (int)threadIdx.x, LL_PG_THREADS);
}

int pose_graph_launch(const PgView &view, int n_graphs, hipStream_t s, const char **err)
{
    if (n_graphs <= 0) return 0;
    hipLaunchKernelGGL(pg_solve_kernel, dim3((unsigned)n_graphs), dim3(LL_PG_THREADS), 0, s, view, n_graphs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (err) *err = hipGetErrorString(e);
        return -1;
    }
    return 0;
}

}  // namespace ll
