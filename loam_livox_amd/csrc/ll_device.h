// ll_device.h -- device-side data layout shared by the kernel files and the C-ABI host code (ll_api.hip).
// All buffers are HBM-resident SoA planes; [scan][point] with a fixed per-scan stride so one launch covers a
// whole batch of scans.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ll_fe_core.h"
#include "ll_knn_core.h"

namespace ll {

#define LL_MAX_PIECES 8
#define LL_GRP 8             // workgroups per scan of the grouped solver
#define LL_GRP_MIN_BLOCKS 6000  // ... whose largest scan has at least this many features (below, one CU's LDS cache holds most of a scan)
#define LL_GRP_MAX_SCANS 16  // batches up to this size use it (LL_GRP * LL_GRP_MAX_SCANS workgroups stay below the CU count)
// One wavefront per query (ll_knn_coop.h) where a launch is bound by its longest single-lane search chain:
#define LL_KNN_COOP_MAX_QUERIES 8192  // ll_map_knn5 batches up to this size; corner searches of a late ICP iteration's work lists
#define LL_KNN_COOP_MAX_SCANS 16      // all corner queries of ICP iterations 0 / 1 for batches up to this size ...
#define LL_KNN_COOP_MAX_SURF 2048     // ... and the surface queries of scans with up to this many (voxel-filtered clouds)
// Tile search of the surface queries (ll_knn_tile.h, ll_knn_kernels.hip): queries sorted by map cell once per registration, one
// wavefront per 64 of them against the LDS-staged points of their cells' common neighbourhood
#define LL_KNN_TILE_MIN_SURF 1024   // batches whose largest scan has at least this many surface queries (below: the wavefront-per-query search)
#define LL_KNN_TILE_SEG 24576       // queries one sorting workgroup orders (1024 threads x 24); a multiple of the tile kernel's workgroup
#define LL_KNN_TILE_MAX_SURF (4 * LL_KNN_TILE_SEG)  // ... and at most this many: larger scans are sorted in segments (Mid-100: three heads)
#define LL_KNN_SPARSE_FROM 4        // first ICP iteration whose tile search takes only the queries that left their list's order budget
                                    // (RegConst::knn_sparse_from; profiles/knn_sparse_gate.json: the unsettled share per iteration; measured at B = 256
                                    //  with three batches in flight: from 5 -> 54.5 / 55.3 k scans/s, from 4 -> 55.8 / 55.9 k, from 3 -> 55.4 / 55.6 k,
                                    //  every query in every iteration 52.9 / 53.3 k)

// Small scans (voxel-filtered feature clouds: a few hundred residual blocks) have a solver of their own (ll_reg_small_kernels.hip)
#define LL_SMALL_MAX_BLOCKS 2048     // batches whose largest scan has at most this many corner + surface queries (more than 1024: eight wavefronts per scan)
#define LL_SMALL_W1_MIN_SCANS 512    // ... one or two wavefronts per scan from this batch size on (many scans per CU), four wavefronts below
#define LL_SMALL_ORDER_MIN_SCANS 512  // batches of this many scans or more start their longest scans first (reg_solve_order_kernel) ...
#define LL_SMALL_ORDER_MAX_SCANS 8192 // ... up to this many (one ordering workgroup)

struct FeScanInfo {
    int n_split;         // entries in split_idx (incl. the closing n-1)
    int clutter_size;    // return value of projection_scan_3d_2d (LFE:606; 0 when fewer than 6 entries)
    int n_petal_clouds;  // laserCloudScans.size() after split_laser_scan (LFE:718)
    int pad;
    float piece_start[LL_MAX_PIECES], piece_end[LL_MAX_PIECES];  // LFX:321-322
};

struct FeDev {
    // inputs
    const float4 *xyzi;   // [B][stride] raw points (x,y,z,intensity)
    const int *npts;      // [B]
    const double *time0;  // [B] m_current_time of each scan
    int stride;           // points per scan slot
    // per-point planes [B][stride]
    int *type, *label;
    float *depth2, *polar2, *curv, *view, *tstamp, *polar_angle;
    float2 *img;
    signed char *flags;   // bit0: defines own polar/img values, bit1: reached the split logic
    int *cand;            // split candidates scratch
    // per-scan split bookkeeping [B][split_cap]
    int split_cap;
    int *split_idx, *petal_first, *petal_last;
    float *run_angle;
    FeScanInfo *info;     // [B]
    // selection [B][stride]
    int *corner_idx, *surf_idx, *full_idx;
    float4 *corner_feat, *surf_feat;
    int *n_corner, *n_surf, *n_full;  // [B]
    // view-angle ambiguity list
    int *n_ambig;
    int2 *ambig_list;
    int ambig_cap;
};

void launch_fe_point(const FeDev &fb, const FeConst &fc, int n_scans, int max_n, hipStream_t s);
void launch_fe_split(const FeDev &fb, int pieces, int n_scans, hipStream_t s);
void launch_fe_select(const FeDev &fb, int n_scans, int piece, float min_blur, float max_blur, hipStream_t s);
// d_last[b] = the last entry of slot b's selection of kind (0 corner, 1 surface, 2 full: fb.full_idx must exist), -1 where it is empty
void launch_fe_selection_last(const FeDev &fb, int n_scans, int kind, int *d_last, hipStream_t s);

// ------------------------------------------------------------------------------------------------ map grid

struct MapKind {
    f4 *pts = nullptr;          // sorted by cell, w = original index bits (nullptr for an fp16-point map)
    int *cell_start = nullptr;  // [ncell + 1]
    unsigned long long *pts16 = nullptr;  // fp16-point records (ll_knn_core.h, Grid::pts16), same order as pts
    int *perm = nullptr;        // original index of every fp16 record
    int64_t n = 0;              // points given
    int64_t n_valid = 0;        // finite points stored in the grid
    Grid grid{};                // device pointers + geometry
    size_t ncell = 0;
    // Buffers are kept between builds and only grow: the mapping loop rebuilds its match buffer every frame
    // (laser_mapping.hpp:539-546), and a hipMalloc / hipFree pair per temporary costs more than the build itself.
    size_t cap_pts = 0, cap_cells = 0;       // capacity of pts / cell_start (elements)
    size_t cap_n = 0, cap_tmp = 0;           // capacity of the per-point scratch (elements) and of b_tmp (bytes)
    unsigned int *b_keys = nullptr, *b_keys2 = nullptr;
    int *b_vals = nullptr, *b_vals2 = nullptr, *b_counts = nullptr;   // b_counts shares cap_cells
    void *b_tmp = nullptr;
    float *b_mm = nullptr;
};

// builds the grid for `n` device-resident raw points (stride floats apart); fills mk. Returns 0 or a HIP error.
int map_build(MapKind &mk, const float *d_raw, int stride, int64_t n, float cell, hipStream_t s, const char **err);
// map_build in two halves for a caller that reads the bounding box back in a wait of its own: the box of the first *d_n (<= n_max)
// points into d_mm[6] (enqueued); then the grid from the box on -- wait = false only enqueues and leaves mk.n_valid 0
int map_bbox_enqueue(const float *d_raw, int stride, const int *d_n, int64_t n_max, float *d_mm, hipStream_t s, const char **err);
int map_build_boxed(MapKind &mk, const float *d_raw, int stride, int64_t n, float cell, const float mm[6], bool wait, hipStream_t s, const char **err);
void map_free(MapKind &mk);
// dimensions, origin, cell size and slack of the grid over a bounding box (host arithmetic; fills the geometry fields of g only)
void map_grid_geometry(const float mm[6], float cell, Grid &g);
// replaces the fp32 records of a built map by fp16-point records (BASELINE config C5); returns 0 or -1 with *err set
int map_to_f16(MapKind &mk, hipStream_t s, const char **err);
// dequantised coordinates of an fp16-point map in ORIGINAL index order (d_out: n_valid... n points x 3 floats, NaN where dropped)
int map_f16_dequant(const MapKind &mk, float *d_out_xyz, hipStream_t s, const char **err);
void launch_knn5(const Grid &g, const float *d_q, int nq, float max_d2, int *d_idx, float *d_d2, hipStream_t s);

// ------------------------------------------------------------------------------------------------ registrar

// Per-scan solver state, resident in HBM between the kernels of one registration.
struct RegState {
    double pose_last[7], pose_curr[7], inc[7];
    double prev_q[4], prev_t[3];          // q_last_optimize / t_last_optimize (PCR:204-205,529-530)
    double interp_theta, hat[9], hat_sq[9];  // m_interpolatation_* (PCR:58,66-68)
    double inlier_thr, final_cost, initial_cost, angular_diff, t_diff;
    int icp_iters, n_blocks_last, corner_avail, surf_avail, lm_total;
    int done, accepted, gated, result;
    int last_work;  // small solver: cost evaluations of this scan's last solver launch (the next launch starts the longest scans first)
    int aborted;  // the grouped solver gave up on a barrier (bounded spin): the scan is rejected and ll_reg_collect reports it
    long long dbg_cycles[16];  // LL_SOLVE_TIMING builds (shader clocks): eval, LM controller, L1, dedupe, select, total, census (+ triple inserts), prune,
                               // epilogue (plane-table path: table build), [9] = exchanges / L1 shortcuts taken; plane-table path: [10] census load waits,
                               // [11] inserts, [12] block sums, [13] id compaction, [14] plane constants, [15] id pass + LDS fill
};

struct RegConst {
    int if_motion_deblur, icp_max_iterations, ceres_max_iterations, ceres_prerun_times;
    int icp_line, icp_plane, force_all_iterations, debug_knn;
    int debug_knn_iter;  // the ICP iteration whose neighbour lists the debug taps record (ll_reg_set_debug_knn_iteration; default 0)
    int force_general;   // test switch: run the HBM-resident solver path even for small scans
    int knn_reuse;       // exact neighbour reuse across ICP iterations (ll_knn_core.h)
    int knn_reuse_from;  // first ICP iteration that tries it (iteration 1 usually moves the queries too far)
    int check_line_pca, check_plane_pca;  // K7 (PCR:46,48)
    int solve_group;     // workgroups per scan of the compact solver (1, or LL_GRP for small batches: ll_reg_solve_fast.h, group_*)
    int xch_epoch;       // ... number of this solver launch within its registration, from 1 (tags of the exchange granules, group_reduce)
    int test_group_abort; // test switch: the grouped solver behaves as if its first barrier had timed out
    int knn_coop;        // corner searches by whole wavefronts where a launch has few of them (ll_knn_coop.h); 0 = A/B switch off
    int knn_tile_last_sort;  // the tile search re-sorts a scan's queries by map cell in ICP iterations 0 .. this one (1: after the first pose update too)
    int no_solve_order;  // A/B switch: the small solver's workgroups in scan order, not longest first (ll_reg_set_debug bit 18)
    int no_small_solver; // A/B switch: small scans take the 512-thread solver too (ll_reg_set_debug bit 15)
    int small_waves;     // test switch: wavefronts per scan of the small solver whatever the batch size (0 = by batch size; bits 16 / 17: 1 / 4)
    int no_line_cache;   // A/B switch: the solver reads line blocks from HBM in every evaluation (no LDS copy)
    int knn_tile;        // surface searches by the tile kernel (ll_knn_tile.h): 0 = off (A/B), 1 = wherever the per-lane search of ALL surface
                         // queries would run (ICP iterations before knn_reuse_from, or every iteration without reuse), 2 = every ICP iteration
                         // (the reuse machinery is then off: a tile search of everything costs less than classifying + searching the lists)
    int knn_sparse_from; // knn_tile == 2 only: from this ICP iteration on the tile search takes only the surface queries that have moved
                         // out of their list's order budget (reg_knn_classify_kernel, ll_knn_kernels.hip); 0 = every query in every iteration
    unsigned int subsample_seed;  // a13 (0 = off)
    int max_blocks;               // maximum_allow_residual_block
    float max_d2_line, max_d2_plane;      // compared against fp32 squared distances (PCR:254,353)
    double max_d2_line_d, max_d2_plane_d;
    double huber_a, inliner_dis, inlier_ratio, minimum_icp_R_diff, minimum_icp_T_diff;
    double bound;                          // m_para_max_speed (PCR:143-151)
    float para_max_angular_rate, max_final_cost, min_ts, max_ts;
};

struct RegDev {
    RegState *state;              // [B]
    const float4 *corner_feat;    // [B][feat_stride_c]
    const float4 *surf_feat;      // [B][feat_stride_s]
    const int *n_corner, *n_surf; // [B]
    int feat_stride_c, feat_stride_s;
    // residual blocks, slot layout per scan: [0, cap_c) corner queries, [cap_c, cap_c + cap_s) surface queries
    int cap_c, cap_s, cap;        // cap = cap_c + cap_s
    float4 *blk_f;                // [B][cap]  f.xyz (sensor frame), w = motion-blur ratio s
    double *blk_av;               // [B][6 * cap] per scan {a0, v0}[cap], {v1, v2}[cap], {a1, a2}[cap] (16-byte pairs; ll_reg_query.h av_load), frame of pose_last
    // round-3 compact path (solve_fast3): the plane constants {n', c} are stored once per DISTINCT neighbour triple of a scan
    // (a scan's ~17 k plane blocks share 2.4 - 4.6 k triples), built by the solver itself at the start of every launch
    unsigned short *blk_id;       // [B][cap_s] plane id of every surface block (relative to its solver workgroup's table region)
    int4 *pl_tab;                 // [B][tab_cap][2] plane table: {n'.x, n'.y}, {n'.z, c = n'.a'} (fp64), frame of pose_last
    int tab_cap;                  // entries per scan: min(cap_s, 61440) rounded up to 4096 (LL_GRP regions of whole 512-thread rounds)
    float4 *qw;                   // [B][cap]  queries transformed into the map frame (K6t -> K6a)
    float4 *ref_q;                // [B][cap]  query position where the neighbour list was established, w = m_strong
    int4 *ref_p;                  // [B][cap]  its neighbours 0..3 (positions in the cell-sorted array)
    float2 *ref_s;                // [B][cap]  x = bits(neighbour 4, -1 when fewer than 5 inside the radius), y = m_set
    int *solve_order;             // [B] small solver: the scans in the order their workgroups start (reg_solve_order_kernel)
    int *grp_ctl;                 // [1 + 2 B] grouped solver: [0] ticket counter, [1 + 2 b] arrival counter of scan b's group barrier, [2 + 2 b] its abort word (zeroed per launch)
    double *grp_part;             // [B][2][LL_GRP][28] grouped solver: the workgroups' partial sums of the evaluation that also publishes the L1 values
    unsigned long long *grp_xch;  // [B][2][LL_GRP][56] ... of every other evaluation, as self-validating 8-byte granules {32-bit half, tag}; zeroed per registration
    unsigned char *blk_flag0;     // [B][cap]  block flag as built; the solver prunes a copy (LDS, or blk_flag in the general path)
    int *work_search;             // [B][cap]  slots that need a full search this iteration
    int *work_build;              // [B][cap]  slots that were re-sorted (block must be rebuilt)
    int *work_off;                // [3][2 B + 1] exclusive prefix sums of work_cnt per list (reg_list_offsets_kernel): searches, re-sorts, and
                                  // the searches of the corner segments alone (their surface segments counted as empty)
    int *work_cnt;                // [B][2 kinds][2] lengths of this ICP iteration's work lists (search, re-sorted) per scan and kind:
                                  // work_search / work_build hold (scan * cap + slot) entries, dense inside the scan-and-kind's own
                                  // segment [scan * cap + kind * cap_c, ...); one atomic per re-query workgroup and list reserves a range
                                  // (a registration that takes the tile search in every ICP iteration, ll_knn_kernels.hip: [b][0][0] = length of
                                  // the scan's list of unsettled surface positions in work_build, [b][0][1] = sum of those lengths over the
                                  // iterations so far, [b][1][iter & 1] = length of the lane kernel's list in work_search)
    int n_chunks;                 // chunks of 256 queries (RQ_THREADS) per (scan, kind): the re-query kernel's grid
    int4 *nn;                     // [B][cap]  neighbour positions (cell-sorted order) + found flag (K6a -> K6b)
    unsigned short *qperm;        // [B][cap_s] surface queries of a scan ordered by the map cell they fall into at ICP iteration 0 (reg_qsort_kernel)
    unsigned short *qperm_c;      // [B][LL_QSORT_CORNER_MAX] a scan's corner queries in the order of the corner map's cells (scans with more corner
                                  // queries than that keep the feature order)
    float4 *qsorted;              // [B][cap_s] the surface FEATURES (sensor frame) in that order, written with qperm when the tile kernel transforms
                                  // the queries itself (no motion deblur): its loads are then coalesced and independent of each other
    unsigned char *blk_flag;      // [B][cap]  BLK_* bits
    double *blk_l1;               // [B][cap]  scratch for the inlier threshold
    unsigned long long *hash;     // [B][hash_cap] dedup table for the std::set semantics of PCR:155-160
    int hash_cap;
    // debug taps (first ICP iteration)
    int *dbg_idx;                 // [B][cap][5]
    float *dbg_d2;                // [B][cap][5]
};

void launch_reg_knn_build(const RegDev &rd, const RegConst &rc, const Grid &gc, const Grid &gs, int n_scans, int iter,
                          int max_nc, int max_ns, hipStream_t s);
#define LL_QSORT_CORNER_MAX 2048
void launch_reg_qsort(const RegDev &rd, const RegConst &rc, const Grid &gc, const Grid &gs, int n_scans, int max_nc, int max_ns, bool fused, hipStream_t s);
void launch_debug_quintic(const double *args, int n, double *out_seq, double *out_wave, hipStream_t s);
void launch_debug_lm_sequence(const double *hdr, const double *evals, int n, int max_calls, unsigned int *img_seq, unsigned int *img_wave, int *ret_seq,
                              int *ret_wave, hipStream_t s);
int debug_lm_ctl_bytes();  // sizeof(LmCtl)
void launch_reg_knn_tile(const RegDev &rd, const RegConst &rc, const Grid &gc, const Grid &gs, int n_scans, int iter, int max_nc, int max_ns,
                         bool fused, hipStream_t s);
void launch_reg_solve(const RegDev &rd, const RegConst &rc, const Grid &gs, int n_scans, int max_nc, int max_ns, int iter, hipStream_t s);
bool reg_solve_small_eligible(const RegConst &rc, int max_nc, int max_ns);
bool reg_solve_fast_eligible(const RegConst &rc, int max_nc, int max_ns);
void launch_reg_solve_small(const RegDev &rd, const RegConst &rc, const Grid &gs, int n_scans, int max_nc, int max_ns, int iter, hipStream_t s);
int reg_solve_small_waves(const RegConst &rc, int n_scans, int max_nc, int max_ns);
// A map per slot (ll_reg_enqueue_fe_maps): map_tab[2 b] / map_tab[2 b + 1] are the corner / surface grid of scan b, in device memory.
// Per-lane or per-wavefront searches of every query in every ICP iteration (no tile search, no reuse lists), the small solver or
// reg_solve_kernel's table form; the caller refuses motion deblur and batches beyond reg_solve_fast_eligible.
// ts_tab (ll_reg_set_time_ranges; motion deblur with a map per slot): {minimum, maximum time stamp} of scan b at ts_tab[b], in device
// memory; the transform and the block constants of scan b then read its pair where the single-map kernels read rc.min_ts / rc.max_ts.
// nullptr: the launches of a map per slot without motion deblur, unchanged.
void launch_reg_knn_build_maps(const RegDev &rd, const RegConst &rc, const Grid *map_tab, int n_scans, int iter, int max_nc, int max_ns, hipStream_t s,
                               const float2 *ts_tab = nullptr);
// The solver form is chosen PER SLOT, as the single-map entry points would choose it for that scan alone (the forms group their sums
// differently and agree to rounding only; a slot must give the bits of its own registration): class 0 = the small solver's
// four-wavefront form (up to 1024 blocks; whatever the batch size: the one- and two-wavefront forms of large single-map batches are
// not used), 1 = its eight-wavefront form (up to LL_SMALL_MAX_BLOCKS), 2 = reg_solve_kernel's table form on one
// workgroup, 3 = the same spread over a group of LL_GRP workgroups (grp_min features or more: LL_GRP_MIN_BLOCKS, or INT_MAX with the groups off).
// One launch per class that has a scan; a workgroup whose scan belongs to another class leaves at once.
__host__ __device__ inline int reg_maps_class(const RegConst &rc, int nc, int ns, int grp_min)
{
    const bool small = !rc.force_general && !rc.no_small_solver && nc + ns > 0 && nc + ns <= LL_SMALL_MAX_BLOCKS && nc <= 1024;  // reg_solve_small_eligible for the scan alone
    return small ? (nc + ns <= 1024 ? 0 : 1) : (nc + ns < grp_min ? 2 : 3);
}
struct RegMapsClasses {
    int n[4], max_nc[4], max_ns[4];  // running scans of each class and their largest feature counts
    int grp_min;
};
void launch_reg_solve_maps(const RegDev &rd, const RegConst &rc, const Grid *map_tab, int n_scans, const RegMapsClasses &cls, int iter, hipStream_t s);
// Motion deblur with a map per slot: reg_solve_big_kernel<1>'s plane-table path (solve_big<1>) for every running scan, one workgroup each,
// the surface map from map_tab[2 b + 1] and the time range from ts_tab[b] (ll_reg_big_maps_kernels.hip).  The caller has refused scans
// that scan_is_compact would send to solve_general.
void launch_reg_solve_big_maps(const RegDev &rd, const RegConst &rc, const Grid *map_tab, const float2 *ts_tab, int n_scans, hipStream_t s);
void launch_reg_solve_small_maps(const RegDev &rd, const RegConst &rc, const Grid *map_tab, int n_scans, int cls, int max_nc, int max_ns, int iter, hipStream_t s);
void launch_reg_finalize(const RegDev &rd, const RegConst &rc, int n_scans, hipStream_t s);
void launch_cloud_transform(const float4 *in, float4 *out, int n, const double *d_pose, hipStream_t s);
// Deskewed clouds (pointAssociateToMap with g_if_undistore = 1, PCR:622-661).  What one slot of a COLLECTED registration left for it,
// copied out of RegState into a record its consumer owns (the next enqueue overwrites the states): 304 bytes per slot.
struct UndistortRec {
    double pose_last[7], pose_curr[7], inc_t[3];
    double theta, hat[9], hat_sq[9];  // m_interpolatation_* (PCR:58,66-68)
    int deblur;                       // if_motion_deblur of the registration
    float min_ts, max_ts;             // its time range (PCR:53-54)
    int pad;
};
struct UndistortJob {  // one slot of a cloud_undistort_kernel launch
    int rec, n;                  // its record, its points
    long long src_off, dst_off;  // first point in src / dst
};
// recs[first + k] <- state[first + k], k < n.  A gated slot gets the identity increment: both poses = pose_last, theta 0, zero matrices.
// ts_tab != nullptr: record k takes its time range from ts_tab[first + k] (a registration with a range per scan) instead of rc's.
void launch_undistort_snapshot(const RegState *state, int first, int n, const RegConst &rc, UndistortRec *recs, hipStream_t s, const float2 *ts_tab = nullptr);
// grid (ceil(max_n / 256), n_slots): slot b moves jobs[b].n points with recs[jobs[b].rec].  d_jobs == nullptr: the one slot `one`.
// pick != nullptr: point i of a slot is src[src_off + pick[src_off + i]] with intensity pick_w[same] (the extractor's full selection).
void launch_cloud_undistort(const UndistortRec *recs, const UndistortJob *d_jobs, const UndistortJob &one, int n_slots, int max_n, const float4 *src,
                            const int *pick, const float *pick_w, float4 *dst, hipStream_t s);
#define LL_HIST_CONCAT_MAX 1023  // frames one history_concat_kernel launch gathers (longer histories: the per-frame copies)
void launch_history_concat(const float4 *frames, const int2 *d_table, int n_seg, int total, float4 *out, hipStream_t s);
void launch_reg_merge_heads(const float4 *fe_corner, const float4 *fe_surf, const int *fe_nc, const int *fe_ns, int fe_stride, int heads,
                            float4 *dst_corner, float4 *dst_surf, int *dst_nc, int *dst_ns, int dst_stride, int n_scans, hipStream_t s);

}  // namespace ll
