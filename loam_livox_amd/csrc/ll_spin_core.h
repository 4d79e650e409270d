// ll_spin_core.h -- per-point decisions of the spinning-lidar feature extraction (hku-mars/loam_livox
// source/laser_feature_extractor.hpp:393-597, lidar_type != "livox"), shared by the HIP kernels (ll_spin_kernels.hip)
// and by ll_spin_resolve, which re-decides the flagged points with the host C library.
//
// The reference calls atan / atan2 / sqrt on floats through `using namespace std`: the float overloads (atanf,
// atan2f, sqrtf).  Everything is fp32 with the reference's evaluation order and its double promotions (M_PI, 0.1,
// 0.0002); compile with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ll_fe_core.h"  // LL_HD, ll_isfinite

namespace ll {

enum : int { SPIN_MAX_LINES = 64, SPIN_BAND_ULP = 16 };

// vertical angle in degrees (:426); the libm of whoever compiles this (device: the HIP math library, host: the C library)
LL_HD float spin_angle(float x, float y, float z) { return atanf(z / sqrtf(x * x + y * y)) * 180 / M_PI; }
LL_HD float spin_ori(float x, float y) { return -atan2f(y, x); }

// :427-461 -- scan ID of a point with vertical angle `angle`, or -1 when the rule drops it
LL_HD int spin_scan_id(float angle, int scan_line)
{
    int scanID = 0;
    if (scan_line == 16) {
        scanID = int((angle + 15) / 2 + 0.5);
        if (scanID > (scan_line - 1) || scanID < 0) return -1;
    } else {
        if (angle >= -8.83)
            scanID = int((2 - angle) * 3.0 + 0.5);
        else
            scanID = scan_line / 2 + int((-8.83 - angle) * 2.0 + 0.5);
        if (angle > 2 || angle < -24.33 || scanID > 50 || scanID < 0) return -1;
    }
    return scanID;
}

// :470-484 before the flip.  *flips = 1 when this point sets halfPassed (it is itself still processed here).
LL_HD float spin_unwrap_pre(float ori, float startOri, int *wrap, int *flips)
{
    *wrap = 0;
    if (ori < startOri - M_PI / 2) {
        ori += 2 * M_PI;
        *wrap = 1;
    } else if (ori > startOri + M_PI * 3 / 2) {
        ori -= 2 * M_PI;
        *wrap = 2;
    }
    *flips = (ori - startOri > M_PI) ? 1 : 0;
    return ori;
}

// :485-497 after the flip
LL_HD float spin_unwrap_post(float ori, float endOri, int *wrap)
{
    *wrap = 0;
    ori += 2 * M_PI;
    if (ori < endOri - M_PI * 3 / 2) {
        ori += 2 * M_PI;
        *wrap = 1;
    } else if (ori > endOri + M_PI / 2) {
        ori -= 2 * M_PI;
        *wrap = 2;
    }
    return ori;
}

// :501-502 (m_para_scanPeriod = 0.1, a double)
LL_HD float spin_intensity(int scanID, float ori, float startOri, float endOri)
{
    float relTime = (ori - startOri) / (endOri - startOri);
    return scanID + 0.1 * relTime;
}

// every discrete outcome the orientation of a point drives, packed: pre-flip wrap, flip, post-flip wrap
LL_HD int spin_ori_decisions(float ori, float startOri, float endOri)
{
    int w0, f, w1;
    (void)spin_unwrap_pre(ori, startOri, &w0, &f);
    (void)spin_unwrap_post(ori, endOri, &w1);
    return w0 | (f << 2) | (w1 << 3);
}

LL_HD float spin_step_ulps(float v, int k)
{
    // v moved by k units in the last place (k may be negative), through the ordered integer encoding of floats
    union {
        float f;
        int32_t i;
    } u;
    u.f = v;
    int32_t o = u.i >= 0 ? u.i : (int32_t)(0x80000000u - (uint32_t)u.i);
    o += k;
    u.i = o >= 0 ? o : (int32_t)(0x80000000u - (uint32_t)o);
    return u.f;
}

// 1 when a libm result within SPIN_BAND_ULP ulps of `angle` / `ori` could decide differently: the scan-ID rule and every
// orientation test are monotone step functions of one float, so agreeing at both ends of the band means agreeing inside it
LL_HD int spin_angle_ambiguous(float angle, int scan_line)
{
    const int a = spin_scan_id(spin_step_ulps(angle, -SPIN_BAND_ULP), scan_line);
    const int b = spin_scan_id(spin_step_ulps(angle, SPIN_BAND_ULP), scan_line);
    return a != b;
}
LL_HD int spin_ori_ambiguous(float ori, float startOri, float endOri)
{
    return spin_ori_decisions(spin_step_ulps(ori, -SPIN_BAND_ULP), startOri, endOri) !=
           spin_ori_decisions(spin_step_ulps(ori, SPIN_BAND_ULP), startOri, endOri);
}

// :586-595 parallel-beam test and :548-563 backward occlusion test of position i (5 <= i < n - 5) of the line-ordered
// cloud p (float4 xyz.), from its curvature `diff`.  The forward marks of :566-577 land on i+1..i+6 and are cleared by
// the loop's own `m_pc_neighbor_picked[i] = 0` before selection can read them (selection reads positions <= n - 7).
template <class P>
LL_HD int spin_occlusion_back(const P *p, int i, float diff)
{
    if (!(diff > 0.1)) return 0;
    float depth1 = sqrtf(p[i].x * p[i].x + p[i].y * p[i].y + p[i].z * p[i].z);
    float depth2 = sqrtf(p[i + 1].x * p[i + 1].x + p[i + 1].y * p[i + 1].y + p[i + 1].z * p[i + 1].z);
    if (!(depth1 > depth2)) return 0;
    float diffX = p[i + 1].x - p[i].x * depth2 / depth1;
    float diffY = p[i + 1].y - p[i].y * depth2 / depth1;
    float diffZ = p[i + 1].z - p[i].z * depth2 / depth1;
    return (sqrtf(diffX * diffX + diffY * diffY + diffZ * diffZ) / depth2 < 0.1) ? 1 : 0;
}
template <class P>
LL_HD int spin_parallel(const P *p, int i, float diff)
{
    float diffX2 = p[i].x - p[i - 1].x;
    float diffY2 = p[i].y - p[i - 1].y;
    float diffZ2 = p[i].z - p[i - 1].z;
    float diff2 = diffX2 * diffX2 + diffY2 * diffY2 + diffZ2 * diffZ2;
    float dis = p[i].x * p[i].x + p[i].y * p[i].y + p[i].z * p[i].z;
    return (diff > 0.0002 * dis && diff2 > 0.0002 * dis) ? 1 : 0;
}
template <class P>
LL_HD float spin_curvature(const P *p, int i)
{
    float diffX = p[i - 5].x + p[i - 4].x + p[i - 3].x + p[i - 2].x + p[i - 1].x - 10 * p[i].x + p[i + 1].x + p[i + 2].x + p[i + 3].x + p[i + 4].x + p[i + 5].x;
    float diffY = p[i - 5].y + p[i - 4].y + p[i - 3].y + p[i - 2].y + p[i - 1].y - 10 * p[i].y + p[i + 1].y + p[i + 2].y + p[i + 3].y + p[i + 4].y + p[i + 5].y;
    float diffZ = p[i - 5].z + p[i - 4].z + p[i - 3].z + p[i - 2].z + p[i - 1].z - 10 * p[i].z + p[i + 1].z + p[i + 2].z + p[i + 3].z + p[i + 4].z + p[i + 5].z;
    return diffX * diffX + diffY * diffY + diffZ * diffZ;
}
// squared step between positions a and b (:687-690 / :727-730): compared with 0.05 in double
template <class P>
LL_HD bool spin_walk_breaks(const P *p, int a, int b)
{
    float diffX = p[a].x - p[b].x;
    float diffY = p[a].y - p[b].y;
    float diffZ = p[a].z - p[b].z;
    return diffX * diffX + diffY * diffY + diffZ * diffZ > 0.05;
}

// :636-638 sub-region j of a line starting at `start` = offset + 5 and ending at `end` = offset + size - 6 (C division)
LL_HD void spin_subregion(int start, int end, int j, int *sp, int *ep)
{
    *sp = (start * (6 - j) + end * j) / 6;
    *ep = (start * (5 - j) + end * (j + 1)) / 6 - 1;
}

}  // namespace ll
