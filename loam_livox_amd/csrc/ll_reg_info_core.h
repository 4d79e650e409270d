// ll_reg_info_core.h -- the information matrix of a registration (ll_reg_information): per-candidate arithmetic, the per-thread loop and
// the order of the sums, shared by reg_information_kernel (ll_reg_info_kernels.hip) and the host tier (tests/reg_info_host.cpp compiles
// this text with g++ and walks the kernel's threads serially).
//
// Definition (DESIGN "Registration information").  For a scan in which at least one ICP iteration ran,
//     H = sum rho' J^T J,   g = sum rho' J^T r,   cost = 1/2 sum rho(|r|^2)
// over the candidate blocks of the scan's LAST ICP iteration, evaluated at x = st->inc, the increment that iteration returned, in the
// solver's tangent d = [d_rot(3); d_t(3)] (ll_reg_core.h:11-12: R_inc+ = Exp(2 d_rot) R_inc, t_inc+ = t_inc + d_t).
//   * A candidate counts when its pristine flag blk_flag0 has BLK_ACTIVE; candidates come in the reference's order, corner queries
//     0 .. n_corner-1, then the surface queries.
//   * NOT applied: the sub-sampling drop (a13, PCR:438-458) and the inlier prune (PCR:487-499).  The pruned set lives only in the solver's
//     registers and LDS, its threshold is rescaled by reg_finalize_kernel (PCR:559), and keeping it would change every solver kernel;
//     outliers are down-weighted by the Huber term, as in every cost evaluation.
//   * The block constants are recomputed from what EVERY solver and search form leaves in HBM -- the neighbour positions rd.nn, the
//     feature clouds, the map snapshot's points and st->pose_last -- through block_line / block_plane, the arithmetic of every solver
//     path: a compact scan never writes its plane constants to blk_av, the tile search writes only flag and triple, so one load path
//     serves all forms and a scan's record has the same bits whichever form ran.
//   * Plain scans: block_accumulate.  if_motion_deblur = 1: block_accumulate_mb with the rotation context of the evaluation point
//     (mb_prepare, as reg_solve_big_kernel<1> builds it) and the block's s = refine_blur(feature stamp).
// Determinism: candidate c goes to thread c mod LL_INFO_THREADS, a thread adds its candidates in increasing c, the wavefront's lanes are
// summed by the fixed butterfly of ll_reg_solve_common.h (pairs 32 apart, then 16, 8, 4, 2, 1), the wavefronts in order.  No atomics.
#pragma once
#include <stdint.h>

#include "ll_knn_core.h"
#include "ll_reg_core.h"

namespace ll {

#define LL_INFO_THREADS 256

// one scan's record, the layout of ll_reg_information (include/loam_livox_hip.h)
struct InfoRecord {
    double H[36];  // full symmetric 6 x 6, row-major
    double g[6];
    double cost;
    int32_t n_line, n_plane;  // blocks summed
    int32_t status;           // 0 computed, 1 gated / no ICP iteration / empty scan, 2 aborted solve
    int32_t reserved;
};
#define LL_INFO_RECORD_DOUBLES 43

// what the evaluation of one scan reads
struct InfoScan {
    const unsigned char *flag0;  // [cap] pristine block flags of the scan
    const int *nn;               // [cap][4] neighbour positions {0, 1 | 2, 4, found}
    const float *corner, *surf;  // [n][4] features, sensor frame (w: the point's time stamp)
    const f4 *map_c, *map_s;     // the maps' points in cell order
    int n_map_c, n_map_s;
    int n_corner, n_surf, cap_c;
    float min_ts, max_ts;
    double huber_a;
    double pose_last[7];
};

// the evaluation point: R_inc / t_inc for the plain blocks, axis and angle for the motion-deblur ones
struct InfoCtx {
    double R[9], t[3];
    MbRot mb;
};

template <int DEBLUR>
LL_HD void info_context(const double x[7], InfoCtx &c)
{
    const double q[4] = {x[0], x[1], x[2], x[3]};
    quat_to_mat(q, c.R);
    c.t[0] = x[4];
    c.t[1] = x[5];
    c.t[2] = x[6];
    if (DEBLUR) mb_prepare(q, c.mb);
}

// candidate `cand` of the scan (corner queries first): adds its block to acc and returns BLK_LINE / BLK_PLANE, or 0 when it is no block
template <int DEBLUR>
LL_HD int info_candidate(const InfoScan &s, const InfoCtx &c, int cand, double acc[LL_NACC])
{
    const int kind = cand < s.n_corner ? 0 : 1;
    const int q = kind ? cand - s.n_corner : cand;
    const int slot = kind ? s.cap_c + q : q;
    if (!(s.flag0[slot] & BLK_ACTIVE)) return 0;
    const int *nn = s.nn + 4 * (size_t)slot;
    const f4 *map = kind ? s.map_s : s.map_c;
    const unsigned int nm = (unsigned int)(kind ? s.n_map_s : s.n_map_c);
    const int i0 = nn[0], i1 = nn[1], i2 = kind ? nn[2] : nn[0];
    // (an active block has its neighbours inside the map; a position outside is never dereferenced)
    if (!nn[3] || (unsigned int)i0 >= nm || (unsigned int)i1 >= nm || (unsigned int)i2 >= nm) return 0;
    const f4 p0 = map[i0], p1 = map[i1];
    const double pa[3] = {(double)p0.x, (double)p0.y, (double)p0.z};
    const double pb[3] = {(double)p1.x, (double)p1.y, (double)p1.z};
    double a[3], v[3];
    if (kind == 0) {
        if (!block_line(s.pose_last, pa, pb, a, v)) return 0;
    } else {
        const f4 p2 = map[i2];
        const double pc[3] = {(double)p2.x, (double)p2.y, (double)p2.z};
        if (!block_plane(s.pose_last, pa, pb, pc, a, v)) return 0;
    }
    const float *fp = (kind ? s.surf : s.corner) + 4 * (size_t)q;
    const double f[3] = {(double)fp[0], (double)fp[1], (double)fp[2]};
    const int blk = kind ? BLK_PLANE : BLK_LINE;
    if (DEBLUR) {
        const double sb = (double)refine_blur(1, fp[3], s.min_ts, s.max_ts);
        block_accumulate_mb(blk, c.mb, c.t, sb, f, a, v, s.huber_a, acc);  // ICP:81-233
    } else {
        block_accumulate(blk, c.R, c.t, f, a, v, s.huber_a, acc);  // ICP:238-380
    }
    return blk;
}

// thread `tid` of `nt`: candidates tid, tid + nt, ... in increasing order
template <int DEBLUR>
LL_HD void info_thread(const InfoScan &s, const InfoCtx &c, int tid, int nt, double acc[LL_NACC], int &n_line, int &n_plane)
{
    LL_UNROLL
    for (int i = 0; i < LL_NACC; i++) acc[i] = 0.0;
    n_line = 0;
    n_plane = 0;
    const int ncand = s.n_corner + s.n_surf;
    for (int cand = tid; cand < ncand; cand += nt) {
        const int k = info_candidate<DEBLUR>(s, c, cand, acc);
        n_line += k == BLK_LINE ? 1 : 0;
        n_plane += k == BLK_PLANE ? 1 : 0;
    }
}

// entry e of the record's 43 doubles {H[36], g[6], cost} from the 28 sums
LL_HD double info_record_entry(const double sum[LL_NACC], int e)
{
    if (e < 36) {
        const int i = e / 6, j = e - 6 * i;
        return sum[i <= j ? hidx(i, j) : hidx(j, i)];
    }
    return e < 42 ? sum[21 + (e - 36)] : sum[27];
}

// status of a scan from its solver state: 2 aborted, 1 gated / no ICP iteration / no candidate, 0 computed
LL_HD int info_status(int gated, int aborted, int icp_iters, int n_cand)
{
    if (aborted) return 2;
    return (gated || icp_iters <= 0 || n_cand <= 0) ? 1 : 0;
}

// The kernel's reduction restated serially (host tier): acc[t] are the sums of thread t, t < nt (a multiple of 64).  Per wavefront the
// tree of wave_sum_acc -- lanes 32 apart, then 16, 8, 4, 2, 1 -- then the wavefronts in order.
inline void info_reduce_serial(const double (*acc)[LL_NACC], int nt, double sum[LL_NACC])
{
    for (int i = 0; i < LL_NACC; i++) {
        double total = 0.0;
        for (int w = 0; w * 64 < nt; w++) {
            double v[64];
            for (int l = 0; l < 64; l++) v[l] = acc[w * 64 + l][i];
            for (int d = 32; d >= 1; d >>= 1)
                for (int l = 0; l < d; l++) v[l] = v[l] + v[l + d];
            total = w == 0 ? v[0] : total + v[0];
        }
        sum[i] = total;
    }
}

}  // namespace ll

#if defined(__HIPCC__)
#include "ll_device.h"
namespace ll {
// one workgroup of LL_INFO_THREADS per scan, behind the last ICP iteration and in front of reg_finalize_kernel; out[n_scans] in device
// memory.  map_tab == nullptr: every scan against the grids gc / gs; otherwise scan b against map_tab[2 b] / map_tab[2 b + 1].
// ts_tab (with map_tab and motion deblur only): scan b's time range is ts_tab[b] = {minimum, maximum} instead of rc's pair.
void launch_reg_information(const RegDev &rd, const RegConst &rc, const Grid &gc, const Grid &gs, const Grid *map_tab, InfoRecord *out, int n_scans,
                            hipStream_t s, const float2 *ts_tab = nullptr);
}  // namespace ll
#endif
