// tests/undistort_host.cpp -- TEST-ONLY host build of the deskew arithmetic of loam_livox_amd/csrc/ll_reg_core.h
// (point_to_map_undistort, interp_rodrigues, point_to_map): the text cloud_undistort_kernel and transform_query run, compiled with
// g++ -ffp-contract=off like the device units, one serial loop in place of the kernel's lanes.  tests/test_undistort_host.py drives it.
#include <cmath>
#include <cstdint>

#include "../loam_livox_amd/csrc/ll_fe_core.h"
#include "../loam_livox_amd/csrc/ll_reg_core.h"

using namespace ll;

struct P4 {
    float x, y, z, w;
};

extern "C" {

void uh_undistort(const double *pose_last, const double *pose_curr, const double *inc_t, double theta, const double *hat, const double *hat_sq,
                  int deblur, float min_ts, float max_ts, const float *xyzi, int n, float *out_xyzi)
{
    for (int i = 0; i < n; i++) {
        const P4 p = {xyzi[4 * i], xyzi[4 * i + 1], xyzi[4 * i + 2], xyzi[4 * i + 3]};
        float o[3];
        point_to_map_undistort(pose_last, pose_curr, inc_t, theta, hat, hat_sq, deblur, min_ts, max_ts, p, o);
        out_xyzi[4 * i] = o[0];
        out_xyzi[4 * i + 1] = o[1];
        out_xyzi[4 * i + 2] = o[2];
        out_xyzi[4 * i + 3] = p.w;
    }
}

void uh_point_to_map(const double *pose, const float *xyzi, int n, float *out_xyzi)
{
    for (int i = 0; i < n; i++) {
        float o[3];
        point_to_map(pose, xyzi[4 * i], xyzi[4 * i + 1], xyzi[4 * i + 2], o);
        out_xyzi[4 * i] = o[0];
        out_xyzi[4 * i + 1] = o[1];
        out_xyzi[4 * i + 2] = o[2];
        out_xyzi[4 * i + 3] = xyzi[4 * i + 3];
    }
}

void uh_interp(const double *q, double *theta, double *hat, double *hat_sq) { interp_rodrigues(q, theta, hat, hat_sq); }

}  // extern "C"
