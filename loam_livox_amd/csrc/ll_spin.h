// ll_spin.h -- device buffers and launchers of the spinning-lidar feature extraction (ll_spin_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>

#include "ll_spin_core.h"

namespace ll {

// per-scan counters: cloud sizes, and a status (0 or SPIN_STATUS_*)
enum : int { SPIN_C_FULL = 0, SPIN_C_SHARP, SPIN_C_LESS_SHARP, SPIN_C_FLAT, SPIN_C_LESS_FLAT, SPIN_C_LF_PRE, SPIN_C_STATUS, SPIN_NCNT = 8 };
enum : int { SPIN_STATUS_LINE_OVERFLOW = 2 };

struct SpinDev {
    int stride;       // points per scan slot (max_points)
    int line_cap;     // less-flat points per line handed to the VoxelGrid (max_line_points)
    int ambig_cap;
    float thres;      // (float)minimum_range
    float4 *in;       // [S][stride] input xyzi
    int *n_in;        // [S]
    float2 *ori_se;   // [S] startOri, endOri (host libm, at upload)
    int *raw_sid;     // [S][stride] scan ID or -1 (input order)
    float *raw_ori;   // [S][stride] -atan2f(y, x)
    int *n_ambig;     // [1]
    int2 *ambig;      // [ambig_cap] (scan, input index)
    float4 *ambig_p;  // [ambig_cap] the listed points, and their scan ID / raw orientation (device, then host-decided)
    int *ambig_sid;
    float *ambig_ori;
    int *line_off;    // [S][65]
    float4 *full;     // [S][stride] laserCloud
    int *full_src;    // [S][stride] input index of each laserCloud point
    float *curv;      // [S][stride]
    unsigned char *flags;  // [S][stride] bit 0 backward occlusion, bit 1 parallel beam
    signed char *label;    // [S][stride]
    int *order;       // [S][stride] positions sorted per sub-region
    int *sharp, *less_sharp, *flat, *lf_pos;  // [S][stride] positions in laserCloud
    float4 *vox_in;   // [S][n_vlines][line_cap]
    int *vox_n;       // [S][n_vlines]
    float4 *less_flat;  // [S][stride]
    int *cnt;         // [S][SPIN_NCNT]
};

void spin_launch_assign(const SpinDev &d, int n_scans, int scan_line, int max_n, hipStream_t st);
void spin_launch_lines(const SpinDev &d, int n_scans, int scan_line, hipStream_t st);
void spin_launch_curv(const SpinDev &d, int n_scans, int max_n, hipStream_t st);
void spin_launch_sort(const SpinDev &d, int n_scans, int scan_line, hipStream_t st);
void spin_launch_select(const SpinDev &d, int n_scans, int scan_line, int n_vlines, hipStream_t st);
// ll_spin_resolve: gather the listed points out / scatter the host decisions back (n listed entries)
void spin_launch_ambig(const SpinDev &d, int n, bool patch, hipStream_t st);
void spin_launch_gather(const SpinDev &d, const float4 *vout, const int *vn, int out_stride, int n_scans, int n_vlines, hipStream_t st);
// hand-off: gathers full[list[i]] of slots 0 .. n_scans-1 into out[S][out_stride] (list = sharp / less_sharp / flat, its size in
// cnt[][cnt_slot]) and writes n_out[S]; n_surf (may be null) receives cnt[][SPIN_C_LESS_FLAT]
void spin_launch_pack(const SpinDev &d, const int *list, int cnt_slot, float4 *out, int out_stride, int *n_out, int *n_surf, int n_scans,
                      hipStream_t st);

// What a device consumer (registrar, history, sub-map: ll_api.hip) sees of a spin handle.  The less-sharp cloud is bounded by
// 200 points x 6 sub-regions x scan_line (laser_feature_extractor.hpp:667-676) and by max_points, so the packed clouds are
// [S][min(max_points, 1200 * scan_line)]; they are allocated by the first hand-off.
struct SpinView {
    int device, max_scans, max_points, scan_line;
    int pack_stride;        // points per slot of a packed cloud
    hipStream_t stream;     // the handle's stream: the consumer orders itself after it
    const float4 *corner;   // [S][pack_stride] LL_SPIN_LESS_SHARP, packed by spin_handoff
    const int *n_corner;    // [S]
    const float4 *surf;     // [S][max_points] LL_SPIN_LESS_FLAT
    const int *n_surf;      // [S]
};

}  // namespace ll

struct ll_spin;

namespace ll {
// capacities and the stream only: no device work (argument checks of the consumers)
void spin_view(const ll_spin *h, SpinView *v);
// packs the corner stack of slots 0 .. n_scans-1 on the handle's stream (once per extraction) and fills every field of *v.
// < 0 with the error text set.
int spin_handoff(ll_spin *h, int n_scans, SpinView *v);
// Cloud `which` (LL_SPIN_FULL .. LL_SPIN_LESS_FLAT) of slots 0 .. n_scans-1 as device memory: *src is [S][*stride], counts[S]
// on the host.  SHARP / LESS_SHARP / FLAT are packed into a buffer of their own.  Synchronises the handle's stream.
int spin_device_cloud(ll_spin *h, int n_scans, int which, const float4 **src, int *stride, int *counts);

}  // namespace ll
