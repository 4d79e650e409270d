// ll_history_batch.h -- device side of the batched match buffer (ll_history_batch_*, ll_history_batch_kernels.hip): the tables the
// host fills per call and the launch wrappers.  One handle holds the histories of S sequences; every launch below covers all of
// them, so the number of launches of an add or a refresh does not depend on S.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ll_device.h"

namespace ll {

// one slot of an add: the pose its two clouds are moved with and the ring slot the filtered frame goes to
struct HbAddSlot {
    double pose[7];
    int work;             // 0: the slot is idle, or its frame is neither pushed nor wanted by the cell maps (nothing is read, nothing is written)
    int ring;             // ring slot of the frame (0 .. maximum_history_size)
    int push;             // the filtered frame goes into the ring (without cell maps: wherever work is set)
    int pad;
};

// one frame of one kind of one slot in a refresh's concatenation
struct HbSeg {
    long long src;        // first point in frames[kind]
    long long dst;        // first point in the concatenation buffer (per kind: [S][the longest concatenation of this refresh])
    int n, kind;
};

// one search grid of a refresh (an active slot's corner or surface cloud)
struct HbGrid {
    Grid g;               // geometry (the pointers are not read on the device)
    int src;              // kind * S + slot: the cloud in d_map [2][S][concat_stride]
    int n;                // its points
    int ncell;
    int pad;
    long long pt_off;     // first record of the grid in the pooled point array = first entry of its keys in the sort
    long long cell_off;   // first entry of its cell table (ncell + 1 entries) in the pooled table
};

void launch_hb_transform(const float4 *src_c, const int *n_c, int stride_c, const float4 *src_s, const int *n_s, int stride_s,
                         const HbAddSlot *tab, int n_slots, int max_pts, float4 *xf, int *n_xf, hipStream_t s);
// the same with slot s's clouds moved by recs[s] (a registration's deskew records, ll_device.h) instead of tab[s].pose
void launch_hb_transform_undistort(const float4 *src_c, const int *n_c, int stride_c, const float4 *src_s, const int *n_s, int stride_s,
                                   const HbAddSlot *tab, const UndistortRec *recs, int n_slots, int max_pts, float4 *xf, int *n_xf, hipStream_t s);
void launch_hb_scatter(const float4 *out_c, const int *n_out_c, const float4 *out_s, const int *n_out_s, int stride, const HbAddSlot *tab,
                       int n_slots, int max_pts, int ring_slots, float4 *frames_c, float4 *frames_s, int *cnt, hipStream_t s);
void launch_hb_gather_frames(const float4 *frames_c, const float4 *frames_s, const HbSeg *segs, int n_seg, int max_pts, float4 *concat,
                             hipStream_t s);
// bounding box and size of every active slot's filtered cloud (mm[(kind * S + slot) * 8 ..]: min, max, n_out), and its copy from the
// filters' outputs ([S][stride_c] / [S][stride_s]) into d_map [2][S][map_stride]
void launch_hb_aabb(const float4 *out_c, const int *n_out_c, int stride_c, const float4 *out_s, const int *n_out_s, int stride_s,
                    const int *active, int n_slots, int max_n, int map_stride, float4 *d_map, unsigned int *mm, hipStream_t s);
void launch_hb_cellkey(const float4 *d_map, int stride, const HbGrid *tab, int n_grids, int max_n, int cbits, unsigned long long *keys,
                       int *vals, int *counts, hipStream_t s);
void launch_hb_gather_points(const float4 *d_map, int stride, const HbGrid *tab, int cbits, const unsigned long long *keys_sorted,
                             const int *vals_sorted, long long n_total, const int *cell_pool, f4 *pts_pool, int *n_valid, hipStream_t s);
// the two hipcub steps: temporary-storage size for n_total keys of key_bits bits and n_cells table entries, and the run
int hb_sort_scan_bytes(long long n_total, long long n_cells, size_t *bytes, const char **err);
int hb_sort_scan(void *tmp, size_t tmp_bytes, unsigned long long *keys, unsigned long long *keys2, int *vals, int *vals2, long long n_total,
                 int key_bits, int *counts, int *cell_pool, long long n_cells, hipStream_t s, const char **err);
// identities of min / max in the ordered encoding of hb_aabb's box, and the decoding (host)
void hb_aabb_identity(unsigned int m[8]);
void hb_aabb_decode(const unsigned int m[8], float mm[6], int *n_out);

}  // namespace ll
