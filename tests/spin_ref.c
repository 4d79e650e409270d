/* spin_ref.c -- TEST-ONLY host restatement of the spinning-lidar branch of Laser_feature::laserCloudHandler
 * (hku-mars/loam_livox source/laser_feature_extractor.hpp:393-787, lidar_type != "livox"), with the edges the
 * reference leaves undefined given the definitions of include/loam_livox_hip.h (ll_spin_*):
 *   - startOri / endOri and the orientation loop read the filtered cloud (the reference sizes them before the filters);
 *   - a sharp walk stops at either end of the line-ordered cloud;
 *   - no point gets a curvature when the cloud has 10 points or fewer.
 * The arithmetic is the reference's, operation for operation, with the C library's float atanf / atan2f / sqrtf (the
 * reference's `atan`, `atan2`, `sqrt` on floats resolve to the float overloads through its `using namespace std`).
 * Build with -ffp-contract=off.  The per-line VoxelGrid (:769-776) is applied by tests/spin_ref.py.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define SPIN_MAX_POINTS 400000

static int finite3(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

/* Returns 0; -1 for a scan_line other than 16 / 64 (:160-164); -2 for more than SPIN_MAX_POINTS input points.
 * Outputs (capacity n_in each unless noted):
 *   full[n][4], full_src[n]   laserCloud (/laser_points_2) and the input index of each of its points; *n_full = n
 *   line_n[scan_line]         points per line (laserCloudScans[i].size())
 *   sharp / less_sharp / flat positions in laserCloud, in publish order
 *   less_flat                 positions of the less-flat points before the VoxelGrid, line after line; lf_line_n[scan_line]
 *   curvature[n], picked0[n]  (may be NULL) curvature and the picked flag selection starts from (0 outside 5..n-6) */
int spin_ref(const float *in, int n_in, int stride, int scan_line, double minimum_range, float *full, int *full_src, int *n_full,
             int *line_n, int *sharp, int *n_sharp, int *less_sharp, int *n_less_sharp, int *flat, int *n_flat, int *less_flat,
             int *lf_line_n, int *n_less_flat, float *curvature, int *picked0)
{
    if (scan_line != 16 && scan_line != 64) return -1;
    if (n_in < 0 || n_in > SPIN_MAX_POINTS) return -2;
    *n_full = *n_sharp = *n_less_sharp = *n_flat = *n_less_flat = 0;
    for (int i = 0; i < scan_line; i++) line_n[i] = lf_line_n[i] = 0;

    /* :399-400 removeNaNFromPointCloud + removeClosedPointCloud */
    const float thres = (float)minimum_range;
    int *src = (int *)malloc(sizeof(int) * (n_in + 1));
    int m = 0;
    for (int i = 0; i < n_in; i++) {
        const float *p = in + (size_t)i * stride;
        if (!finite3(p)) continue;
        if (p[0] * p[0] + p[1] * p[1] + p[2] * p[2] < thres * thres) continue;
        src[m++] = i;
    }
    if (m == 0) {
        free(src);
        return 0;
    }
#define PX(k) (in[(size_t)src[k] * stride + 0])
#define PY(k) (in[(size_t)src[k] * stride + 1])
#define PZ(k) (in[(size_t)src[k] * stride + 2])

    /* :403-415 */
    float startOri = -atan2f(PY(0), PX(0));
    float endOri = -atan2f(PY(m - 1), PX(m - 1)) + 2 * M_PI;
    if (endOri - startOri > 3 * M_PI) {
        endOri -= 2 * M_PI;
    } else if (endOri - startOri < M_PI) {
        endOri += 2 * M_PI;
    }

    /* :417-505 */
    int *sid = (int *)malloc(sizeof(int) * m);
    float *inten = (float *)malloc(sizeof(float) * m);
    int halfPassed = 0;
    for (int i = 0; i < m; i++) {
        const float x = PX(i), y = PY(i), z = PZ(i);
        float angle = atanf(z / sqrtf(x * x + y * y)) * 180 / M_PI;
        int scanID = 0;
        sid[i] = -1;
        if (scan_line == 16) {
            scanID = (int)((angle + 15) / 2 + 0.5);
            if (scanID > (scan_line - 1) || scanID < 0) continue;
        } else {
            if (angle >= -8.83)
                scanID = (int)((2 - angle) * 3.0 + 0.5);
            else
                scanID = scan_line / 2 + (int)((-8.83 - angle) * 2.0 + 0.5);
            if (angle > 2 || angle < -24.33 || scanID > 50 || scanID < 0) continue;
        }
        float ori = -atan2f(y, x);
        if (!halfPassed) {
            if (ori < startOri - M_PI / 2)
                ori += 2 * M_PI;
            else if (ori > startOri + M_PI * 3 / 2)
                ori -= 2 * M_PI;
            if (ori - startOri > M_PI) halfPassed = 1;
        } else {
            ori += 2 * M_PI;
            if (ori < endOri - M_PI * 3 / 2)
                ori += 2 * M_PI;
            else if (ori > endOri + M_PI / 2)
                ori -= 2 * M_PI;
        }
        float relTime = (ori - startOri) / (endOri - startOri);
        inten[i] = scanID + 0.1 * relTime; /* m_para_scanPeriod = 0.1 (double) */
        sid[i] = scanID;
        line_n[scanID]++;
    }

    /* :513-521 concatenate the lines (stable: input order inside a line) */
    int *scanStartInd = (int *)malloc(sizeof(int) * scan_line), *scanEndInd = (int *)malloc(sizeof(int) * scan_line);
    int *fill = (int *)malloc(sizeof(int) * scan_line);
    int n = 0;
    for (int l = 0; l < scan_line; l++) {
        scanStartInd[l] = n + 5;
        fill[l] = n;
        n += line_n[l];
        scanEndInd[l] = n - 6;
    }
    for (int i = 0; i < m; i++) {
        if (sid[i] < 0) continue;
        const int k = fill[sid[i]]++;
        full[4 * k + 0] = PX(i);
        full[4 * k + 1] = PY(i);
        full[4 * k + 2] = PZ(i);
        full[4 * k + 3] = inten[i];
        full_src[k] = src[i];
    }
    *n_full = n;
#define X(k) (full[4 * (k) + 0])
#define Y(k) (full[4 * (k) + 1])
#define Z(k) (full[4 * (k) + 2])

    /* :524-597, with the member arrays' per-message state; picked needs room for the forward marks up to i + 6 */
    float *curv = (float *)calloc(n + 8, sizeof(float));
    int *sort_idx = (int *)calloc(n + 8, sizeof(int));
    int *picked = (int *)calloc(n + 8, sizeof(int));
    int *label = (int *)calloc(n + 8, sizeof(int));
    for (int i = 5; n > 10 && i < n - 5; i++) {
        float diffX = X(i - 5) + X(i - 4) + X(i - 3) + X(i - 2) + X(i - 1) - 10 * X(i) + X(i + 1) + X(i + 2) + X(i + 3) + X(i + 4) + X(i + 5);
        float diffY = Y(i - 5) + Y(i - 4) + Y(i - 3) + Y(i - 2) + Y(i - 1) - 10 * Y(i) + Y(i + 1) + Y(i + 2) + Y(i + 3) + Y(i + 4) + Y(i + 5);
        float diffZ = Z(i - 5) + Z(i - 4) + Z(i - 3) + Z(i - 2) + Z(i - 1) - 10 * Z(i) + Z(i + 1) + Z(i + 2) + Z(i + 3) + Z(i + 4) + Z(i + 5);
        float diff = diffX * diffX + diffY * diffY + diffZ * diffZ;
        curv[i] = diff;
        sort_idx[i] = i;
        picked[i] = 0;
        label[i] = 0;
        if (diff > 0.1) {
            float depth1 = sqrtf(X(i) * X(i) + Y(i) * Y(i) + Z(i) * Z(i));
            float depth2 = sqrtf(X(i + 1) * X(i + 1) + Y(i + 1) * Y(i + 1) + Z(i + 1) * Z(i + 1));
            if (depth1 > depth2) {
                diffX = X(i + 1) - X(i) * depth2 / depth1;
                diffY = Y(i + 1) - Y(i) * depth2 / depth1;
                diffZ = Z(i + 1) - Z(i) * depth2 / depth1;
                if (sqrtf(diffX * diffX + diffY * diffY + diffZ * diffZ) / depth2 < 0.1)
                    for (int k = i - 5; k <= i; k++) picked[k] = 1;
            } else {
                diffX = X(i + 1) * depth1 / depth2 - X(i);
                diffY = Y(i + 1) * depth1 / depth2 - Y(i);
                diffZ = Z(i + 1) * depth1 / depth2 - Z(i);
                if (sqrtf(diffX * diffX + diffY * diffY + diffZ * diffZ) / depth1 < 0.1)
                    for (int k = i + 1; k <= i + 6; k++) picked[k] = 1;
            }
        }
        float diffX2 = X(i) - X(i - 1);
        float diffY2 = Y(i) - Y(i - 1);
        float diffZ2 = Z(i) - Z(i - 1);
        float diff2 = diffX2 * diffX2 + diffY2 * diffY2 + diffZ2 * diffZ2;
        float dis = X(i) * X(i) + Y(i) * Y(i) + Z(i) * Z(i);
        if (diff > 0.0002 * dis && diff2 > 0.0002 * dis) picked[i] = 1;
    }
    if (curvature)
        for (int i = 0; i < n; i++) curvature[i] = curv[i];
    if (picked0)
        for (int i = 0; i < n; i++) picked0[i] = (n > 10 && i >= 5 && i < n - 5) ? picked[i] : 0;

    /* :631-777 */
    const float sharp_point_threshold = 0.05;
    for (int i = 0; i < scan_line; i++) {
        for (int j = 0; j < 6; j++) {
            int sp = (scanStartInd[i] * (6 - j) + scanEndInd[i] * j) / 6;
            int ep = (scanStartInd[i] * (5 - j) + scanEndInd[i] * (j + 1)) / 6 - 1;
            for (int k = sp + 1; k <= ep; k++)
                for (int l = k; l >= sp + 1; l--)
                    if (curv[sort_idx[l]] < curv[sort_idx[l - 1]]) {
                        int temp = sort_idx[l - 1];
                        sort_idx[l - 1] = sort_idx[l];
                        sort_idx[l] = temp;
                    }
            int largestPickedNum = 0;
            for (int k = ep; k >= sp; k--) {
                int ind = sort_idx[k];
                if (picked[ind] == 0 && curv[ind] > sharp_point_threshold * 10) {
                    largestPickedNum++;
                    if (largestPickedNum <= 20) {
                        label[ind] = 2;
                        sharp[(*n_sharp)++] = ind;
                        less_sharp[(*n_less_sharp)++] = ind;
                    } else if (largestPickedNum <= 200) {
                        label[ind] = 1;
                        less_sharp[(*n_less_sharp)++] = ind;
                    } else {
                        break;
                    }
                    picked[ind] = 1;
                    float times = 100;
                    for (int l = 1; l <= 5 * times; l++) {
                        if (ind + l > n - 1) break; /* defined edge: the end of the cloud */
                        float diffX = X(ind + l) - X(ind + l - 1);
                        float diffY = Y(ind + l) - Y(ind + l - 1);
                        float diffZ = Z(ind + l) - Z(ind + l - 1);
                        if (diffX * diffX + diffY * diffY + diffZ * diffZ > 0.05) break;
                        picked[ind + l] = 1;
                    }
                    for (int l = -1; l >= -5 * times; l--) {
                        if (ind + l < 0) break; /* defined edge: the start of the cloud */
                        float diffX = X(ind + l) - X(ind + l + 1);
                        float diffY = Y(ind + l) - Y(ind + l + 1);
                        float diffZ = Z(ind + l) - Z(ind + l + 1);
                        if (diffX * diffX + diffY * diffY + diffZ * diffZ > 0.05) break;
                        picked[ind + l] = 1;
                    }
                }
            }
            int smallestPickedNum = 0;
            for (int k = sp; k <= ep; k++) {
                int ind = sort_idx[k];
                if (picked[ind] == 0 && curv[ind] < sharp_point_threshold) {
                    label[ind] = -1;
                    flat[(*n_flat)++] = ind;
                    smallestPickedNum++;
                    if (smallestPickedNum >= 5) break;
                    picked[ind] = 1;
                    for (int l = 1; l <= 5; l++) {
                        float diffX = X(ind + l) - X(ind + l - 1);
                        float diffY = Y(ind + l) - Y(ind + l - 1);
                        float diffZ = Z(ind + l) - Z(ind + l - 1);
                        if (diffX * diffX + diffY * diffY + diffZ * diffZ > 0.05) break;
                        picked[ind + l] = 1;
                    }
                    for (int l = -1; l >= -5; l--) {
                        float diffX = X(ind + l) - X(ind + l + 1);
                        float diffY = Y(ind + l) - Y(ind + l + 1);
                        float diffZ = Z(ind + l) - Z(ind + l + 1);
                        if (diffX * diffX + diffY * diffY + diffZ * diffZ > 0.05) break;
                        picked[ind + l] = 1;
                    }
                }
            }
            for (int k = sp; k <= ep; k++)
                if (label[k] <= 0) {
                    less_flat[(*n_less_flat)++] = k;
                    lf_line_n[i]++;
                }
        }
    }
    free(src);
    free(sid);
    free(inten);
    free(scanStartInd);
    free(scanEndInd);
    free(fill);
    free(curv);
    free(sort_idx);
    free(picked);
    free(label);
    return 0;
}
