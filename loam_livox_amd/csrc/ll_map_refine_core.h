// ll_map_refine_core.h -- the arithmetic of the key-frame map refinement (Mapping_refine, hku-mars/loam_livox
// source/ceres_pose_graph_3d.hpp:368-538): the affine of refine_pts (:444-445) on the host, the move of one point (:449), which
// point the filter of a selection sees, and the sums of one voxel.  Shared by ll_map_refine_kernels.hip, the host side of the C ABI
// and tests/map_refine_host.cpp, which runs the chain on the CPU from this text.  Float throughout, no contraction: the build's
// -ffp-contract=off holds, and the move says so itself because three passes must see the same float.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ll_voxel_core.h"

namespace ll {

// what a chain does with the points of its selections
enum : int {
    MR_FILTER_THEN_MOVE = 0,  // refine_pointcloud( ..., if_save = 0 ), :476-485: VoxelGrid, then the centroids are moved
    MR_MOVE_THEN_FILTER = 1,  // refine_mapping's in-memory overload, :511-533: every point is moved, then VoxelGrid
    MR_FILTER_ONLY = 2        // add_cloud and merge: VoxelGrid alone, the averaged intensity kept
};

#define MR_CHUNK 2048                       // points of one (selection, chunk) work item: 256 threads x 8
#define MR_MAX_SEL (1 << 20)
#define MR_SENTINEL 0xffffffffffffffffull   // key of a point no voxel takes: sorts last

struct MrAffine {
    float R[9];  // R_aff, row-major
    float T[3];  // T_aff
};

// one selection of a chain: n points at src[src_off ..], which are the work indices in_off .. in_off + n
struct MrSel {
    long long src_off;
    int n, in_off;
    MrAffine aff;
};

// opm_pt = R_aff * raw_pt + T_aff (:449): Eigen's lazy 3x3-by-3 product for float, e0 + (e1 + e2) per row, then the sum with T_aff
LL_HD void mr_move(const MrAffine &a, float x, float y, float z, float out[3])
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    for (int i = 0; i < 3; i++) {
        const float e0 = a.R[3 * i] * x, e1 = a.R[3 * i + 1] * y, e2 = a.R[3 * i + 2] * z;
        out[i] = (e0 + (e1 + e2)) + a.T[i];
    }
}

// the point the filter of a chain sees at src[i]: the stored point, or in MR_MOVE_THEN_FILTER its image (eigen_to_pcl_pt leaves the
// intensity at PointXYZI's default, 0).  The bounds, key and centroid passes all come through here, so they see one float.
template <typename P>
LL_HD P mr_filter_input(int mode, const MrAffine &a, const P &p)
{
    if (mode != MR_MOVE_THEN_FILTER) return p;
    float m[3];
    mr_move(a, p.x, p.y, p.z, m);
    P q = p;
    q.x = m[0], q.y = m[1], q.z = m[2], q.w = 0.f;
    return q;
}

// what a chain writes for a centroid c (or, of a pass-through selection, for the filter's input c): MR_FILTER_THEN_MOVE moves it and
// drops the averaged intensity as the reference does; MR_MOVE_THEN_FILTER has moved already (the intensity is 0 by then);
// MR_FILTER_ONLY keeps c
template <typename P>
LL_HD P mr_output(int mode, const MrAffine &a, const P &c)
{
    if (mode != MR_FILTER_THEN_MOVE) return c;
    float m[3];
    mr_move(a, c.x, c.y, c.z, m);
    P q = c;
    q.x = m[0], q.y = m[1], q.z = m[2], q.w = 0.f;
    return q;
}

LL_HD bool mr_finite(float x, float y, float z) { return ll_isfinite(x) && ll_isfinite(y) && ll_isfinite(z); }

// sort key of work index g's point (already through mr_filter_input): selection << 32 | leaf index
template <typename P>
LL_HD unsigned long long mr_key(int sel, const P &p, const float inv[3], const VoxelParams &prm)
{
    if (prm.status != VOX_OK || !mr_finite(p.x, p.y, p.z)) return MR_SENTINEL;
    return ((unsigned long long)(unsigned int)sel << 32) | (unsigned long long)voxel_index(p.x, p.y, p.z, inv, prm);
}

// The centroid of the voxel whose first sorted position is i (CentroidPoint<PointXYZI>: AccumulatorXYZ + AccumulatorIntensity).  The
// additions run in input order -- the sort is stable -- the loads need not: eight keys, the matching eight work indices, then the
// eight points are independent loads, as in vox_centroid_kernel.  src: the chain's source; sel: the voxel's selection (keys[i] >> 32).
template <typename P>
LL_HD P mr_centroid(int mode, const P *src, const MrSel &sel, const unsigned long long *keys, const unsigned int *vals, size_t i, size_t total)
{
    const unsigned long long k = keys[i];
    const P *base = src + sel.src_off - sel.in_off;  // work index g -> src[src_off + (g - in_off)]
    float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
    int cnt = 0;
    bool more = true;
    for (size_t j = i; more && j < total; j += 8) {
        bool ok[8];
        unsigned int v[8];
        P p[8];
        for (int u = 0; u < 8; u++) ok[u] = (j + u < total) && keys[j + u] == k;
        for (int u = 1; u < 8; u++) ok[u] = ok[u] && ok[u - 1];
        for (int u = 0; u < 8; u++) v[u] = ok[u] ? vals[j + u] : vals[i];
        for (int u = 0; u < 8; u++) p[u] = base[v[u]];
        for (int u = 0; u < 8; u++) {
            if (ok[u]) {
                const P q = mr_filter_input(mode, sel.aff, p[u]);
                sx = sx + q.x;
                sy = sy + q.y;
                sz = sz + q.z;
                si = si + q.w;
                cnt++;
            }
        }
        more = ok[7];
    }
    const float c = (float)cnt;
    P out;
    out.x = sx / c, out.y = sy / c, out.z = sz / c, out.w = si / c;
    return out;
}

// Host only.  R_aff and T_aff exactly as refine_pts writes them (:444-445) for T = float, TT = double, poses {qx, qy, qz, qw, tx, ty, tz}:
//   R_aff = ( R_opm * R_ori^T ).cast< float >()                    double lazy product, ( e0 + e1 ) + e2
//   T_aff = ( R_aff.cast< double >() * ( -t_ori ) + t_opm ).cast< float >()
// toRotationMatrix is Eigen's formula as it stands: the quaternion is not renormalised.
inline void mr_rotation(const double q[4], double R[9])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
    R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
    R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
}

inline void mr_affine(const double ori7[7], const double opm7[7], float R_aff[9], float T_aff[3])
{
    double Ro[9], Rp[9];
    mr_rotation(ori7, Ro);
    mr_rotation(opm7, Rp);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {  // ( R_opm * R_ori^T )( r, c ) = sum_k R_opm( r, k ) * R_ori( c, k )
            const double e0 = Rp[3 * r] * Ro[3 * c], e1 = Rp[3 * r + 1] * Ro[3 * c + 1], e2 = Rp[3 * r + 2] * Ro[3 * c + 2];
            R_aff[3 * r + c] = (float)((e0 + e1) + e2);
        }
    const double nt[3] = {-ori7[4], -ori7[5], -ori7[6]};
    for (int r = 0; r < 3; r++) {
        const double e0 = (double)R_aff[3 * r] * nt[0], e1 = (double)R_aff[3 * r + 1] * nt[1], e2 = (double)R_aff[3 * r + 2] * nt[2];
        T_aff[r] = (float)(((e0 + e1) + e2) + opm7[4 + r]);
    }
}

}  // namespace ll
