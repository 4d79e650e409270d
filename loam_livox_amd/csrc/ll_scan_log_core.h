// ll_scan_log_core.h -- the per-point decision of the scan log of the batched match buffer (ll_history_batch_enable_scan_log) and the
// tables its two kernels read.  Shared by the HIP kernels (ll_scan_log_kernels.hip) and the test-only host build
// (tests/scan_log_host.cpp), like ll_fullmap_batch_core.h, whose gather decides which points of a scan are refused.
//
// The scan log is m_laser_cloud_full_history of S lock-step sequences (laser_mapping.hpp:1456, 1480-1486, 1545-1558): the full cloud
// of every scan the history's add rule let in, in the map frame, with the intensity pointcloudAssociateToMap copies (PCR:659).
#pragma once
#include "ll_fullmap_batch_core.h"

namespace ll {

#ifndef SL_CHUNK
#define SL_CHUNK 2048  // points of one (request, block, chunk) work item of the gather: 256 threads x 8 (the host test builds a smaller one)
#endif

// What the log keeps of point i of a slot's full selection.  xf: what fb_gather_kernel left for it in the map frame -- the very
// floats the full-cloud map received, or the marker of a refused point, which stays (the VoxelGrid behind the log drops it);
// src: full_idx of the point; scan: the slot's scan.  The intensity is the scan's, as cloud_transform_kernel copies it; a refused
// point keeps the marker's 0.
template <typename P>
LL_HD P sl_logged_point(const P &xf, int src, int stride, const P *scan)
{
    P o = xf;
    if (src >= 0 && src < stride) {
        const P v = scan[src];
        if (fb_point_ok(v.x, v.y, v.z)) o.w = v.w;
    }
    return o;
}

// one slot of a log call: the block its scan goes to (null: the slot logs nothing) and the points of its full selection
template <typename P>
struct SlSlotT {
    P *dst;
    int n, pad;
};

// one work item of the gather: n <= SL_CHUNK points of a block, from src to staging index dst
template <typename P>
struct SlCopyT {
    const P *src;
    long long dst;
    int n, req;
};

}  // namespace ll
