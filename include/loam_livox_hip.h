/*
 * loam_livox_hip.h -- C ABI of libloamlivox_hip.so: MI355X (gfx950) scan-to-map registration core for
 * Loam-Livox.  This is the drop-in boundary for the hot path of hku-mars/loam_livox; every entry point
 * cites the reference interface it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain C types only; the caller owns every host buffer, the library owns all device memory;
 *   - pose[7] = {qx,qy,qz,qw,tx,ty,tz}: the storage order of m_para_buffer_RT / m_para_buffer_incremental
 *     (source/point_cloud_registration.hpp:51-56, source/laser_mapping.hpp:206-213);
 *   - clouds are AoS float xyzi (4 floats per point) like pcl::PointXYZI payloads; feature clouds carry the
 *     per-point time stamp in the intensity slot (source/livox_feature_extractor.hpp:246,255);
 *   - return value: >= 0 success (meaning per function), < 0 library error (text via ll_last_error()).
 *     No exceptions, no abort.  There is NO CPU fallback: without a HIP device every *_create fails.
 *   - handles are not thread-safe individually (the reference serialises the extractor with a mutex,
 *     laser_feature_extractor.hpp:244); different handles may be used from different threads, and one
 *     ll_map may be shared read-only by several ll_reg (laser_mapping.hpp:1737-1742 runs several
 *     process_new_scan concurrently against one map snapshot).
 */
#ifndef LOAM_LIVOX_HIP_H
#define LOAM_LIVOX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ll_fe ll_fe;   /* replaces class Livox_laser                (livox_feature_extractor.hpp:77)  */
typedef struct ll_map ll_map; /* replaces the map clouds + KdTreeFLANN pair (point_cloud_registration.hpp:72-73,
                                 laser_mapping.hpp:539-546)                                               */
typedef struct ll_reg ll_reg; /* replaces class Point_cloud_registration    (point_cloud_registration.hpp:38) */

/* Point-type bit masks (livox_feature_extractor.hpp:82-92) and feature labels (:94-103). */
enum { LL_PT_NORMAL = 0, LL_PT_000 = 1, LL_PT_TOO_NEAR = 2, LL_PT_REFL_LOW = 4, LL_PT_REFL_HIGH = 8,
       LL_PT_CIRCLE_EDGE = 16, LL_PT_NAN = 32, LL_PT_SMALL_VIEW_ANGLE = 64 };
enum { LL_LABEL_INVALID = -1, LL_LABEL_UNLABELED = 0, LL_LABEL_CORNER = 1, LL_LABEL_SURFACE = 2,
       LL_LABEL_NEAR_NAN = 4, LL_LABEL_NEAR_ZERO = 8, LL_LABEL_HIGH_INTENSITY = 16 };

/* ------------------------------------------------------------------------------------------------ extractor */

/* Public tunables of Livox_laser (livox_feature_extractor.hpp:143-167) as the node sets them
 * (laser_feature_extractor.hpp:146-154,854,859), plus capacities. */
typedef struct {
    float thr_corner_curvature;  /* :153, ROS feature_extraction/corner_curvature   */
    float thr_surface_curvature; /* :154, ROS feature_extraction/surface_curvature  */
    float minimum_view_angle;    /* :155, ROS feature_extraction/minimum_view_angle */
    float livox_min_allow_dis;   /* :166, ROS feature_extraction/livox_min_dis      */
    float livox_min_sigma;       /* :167, ROS feature_extraction/livox_min_sigma    */
    float max_fov;               /* :143 (17 deg) */
    float time_internal_pts;     /* :145 (1e-5 s) */
    int32_t device;              /* HIP device ordinal */
    int32_t max_points;          /* capacity: points per scan */
    int32_t max_scans;           /* capacity: scans resident at once (1 for the per-message node path) */
    int32_t piecewise_number;    /* ROS common/piecewise_number (laser_feature_extractor.hpp:142); 1 when deblur */
} ll_fe_params;

void ll_fe_default_params(ll_fe_params *p); /* node defaults, max_points 24000, max_scans 1 */
int ll_fe_create(const ll_fe_params *p, ll_fe **out);
void ll_fe_destroy(ll_fe *h);

/* Livox_laser::extract_laser_features(cloud, time_stamp) (livox_feature_extractor.hpp:722-766) for ONE scan
 * given on the host: projection_scan_3d_2d (:458), eval_point (:343), add_mask_of_point (:322),
 * compute_features (:361), petal split + split_laser_scan (:657).  Keeps the sequential time base of the
 * class (:150-152,724-736).  Synchronous.  *n_petal_clouds = laserCloudScans.size() of the reference
 * (the caller drops the scan when it is <= 5, laser_feature_extractor.hpp:287).  Returns 0. */
int ll_fe_extract(ll_fe *h, const float *xyzi, int32_t n, double time_stamp, int32_t *n_petal_clouds);

/* m_pts_info_vec fields of scan slot `scan` (livox_feature_extractor.hpp:118-133). Any pointer may be NULL. */
int ll_fe_labels(ll_fe *h, int32_t scan, int32_t *pt_type, int32_t *pt_label, float *depth_sq2,
                 float *polar_dis_sq2, float *curvature, float *view_angle, float *time_stamp, float *polar_angle);

/* split bookkeeping of scan slot `scan`: split_idx (livox_feature_extractor.hpp:465-565; capacity
 * max_points/50+8), the return value of projection_scan_3d_2d (:606), and for every surviving petal cloud the
 * index of its first/last point, plus the piece-wise windows of laser_feature_extractor.hpp:305-323
 * (piecewise_number entries; boundary points go through find_pt_info's first-occurrence lookup, :321-322). */
int ll_fe_splits(ll_fe *h, int32_t scan, int32_t *split_idx, int32_t *n_split, int32_t *clutter_size,
                 int32_t *n_petal_clouds, int32_t *first_idx, int32_t *last_idx, float *piece_start, float *piece_end);

/* Livox_laser::get_features(corners, surface, full, minimum_blur, maximum_blur)
 * (livox_feature_extractor.hpp:219-272) on scan slot 0: ascending index lists (the integer parity artefact)
 * and, optionally, the packed clouds (xyz + time stamp).  Output buffers sized max_points; NULL to skip. */
int ll_fe_select(ll_fe *h, float minimum_blur, float maximum_blur, int32_t *corner_idx, int32_t *n_corner,
                 int32_t *surf_idx, int32_t *n_surf, int32_t *full_idx, int32_t *n_full, float *corner_xyzi,
                 float *surf_xyzi);

/* Batched, device-resident form (offline map building / throughput): scans are independent, so the time base
 * is given explicitly per scan (current_time = m_current_time of livox_feature_extractor.hpp:727-731). */
int ll_fe_upload(ll_fe *h, int32_t first_scan, int32_t n_scans, const float *xyzi, int32_t n_points,
                 const double *current_time);
/* The same without the final wait: the copies are queued on the handle's stream and the call returns; xyzi and
 * current_time must stay valid (and should be page-locked host memory for a true asynchronous copy) until ll_fe_sync or
 * a later synchronous call on this handle.  Lets the next batch cross PCIe while the previous one is being processed
 * on another handle (bench.py "streamed" figure). */
int ll_fe_upload_async(ll_fe *h, int32_t first_scan, int32_t n_scans, const float *xyzi, int32_t n_points,
                       const double *current_time);
int ll_fe_extract_batch(ll_fe *h, int32_t n_scans); /* asynchronous on the handle's stream */
/* piece >= 0: use the device-computed piece-wise window `piece`; piece < 0: explicit [minimum,maximum]_blur */
int ll_fe_select_batch(ll_fe *h, int32_t n_scans, int32_t piece, float minimum_blur, float maximum_blur);
/* last_position[b], b < n_scans: the last (largest: a selection is ascending) position of slot b's selection of `kind` (0 corner,
 * 1 surface, 2 full) after ll_fe_select_batch, -1 where the selection is empty.  One small launch and one copy of n_scans ints: what a
 * motion-deblur frame's time range needs of the full selection (laser_mapping.hpp:1336) without downloading it. */
int ll_fe_selection_last(ll_fe *h, int32_t n_scans, int32_t kind, int32_t *last_position);
/* The selection ll_fe_select_batch left in slot `scan`: what ll_fe_select returns for slot 0 (get_features' outputs,
 * livox_feature_extractor.hpp:219-272), for any slot of a batch.  Output buffers sized max_points; NULL to skip.  Synchronises. */
int ll_fe_selection(ll_fe *h, int32_t scan, int32_t *corner_idx, int32_t *n_corner, int32_t *surf_idx, int32_t *n_surf,
                    int32_t *full_idx, int32_t *n_full, float *corner_xyzi, float *surf_xyzi);
int ll_fe_counts(ll_fe *h, int32_t n_scans, int32_t *n_corner, int32_t *n_surf, int32_t *n_full,
                 int32_t *n_ambiguous); /* synchronises */
int ll_fe_sync(ll_fe *h);
/* Labels depend on `view_angle > minimum_view_angle` where view_angle comes from the C library's acosf
 * (tools_eigen_math.hpp:38).  Device and host acosf can differ in the last ulp, so the kernels flag the (very
 * rare) points whose angle falls inside a few-ulp band around the threshold; this call re-derives those labels
 * with the host libm (what the reference executable itself would have computed on this machine) and patches
 * them on the device.  Synchronises; returns the number of flagged points.  ll_fe_extract calls it itself;
 * batch users call it between ll_fe_extract_batch and ll_fe_select_batch. */
int ll_fe_resolve(ll_fe *h);

/* ------------------------------------------------------------------------------------------------ map */

enum { LL_MAP_CORNER = 0, LL_MAP_SURF = 1 };

int ll_map_create(int32_t device, ll_map **out);
void ll_map_destroy(ll_map *m);
/* Replaces pcl::KdTreeFLANN::setInputCloud for the match buffers (laser_mapping.hpp:544-545,
 * point_cloud_registration.hpp:596-597): uploads the cloud and builds the device search grid.
 * xyz: m points, stride_floats apart (3 = xyz, 4 = xyzi).  cell_size <= 0 selects the default
 * (1.45 m corner: the sparse edge map is searched out to the sqrt(2) m line radius, one cell ring covers it;
 * 0.6 m surface: about 1.5x the 0.4 m surface-map leaf).  The results do not depend on it, the speed does: a search reads
 * every point of the query's own cells before it can prune, so a cloud that was voxel-filtered at leaf l wants cells of
 * about 3-4 l (ll_history_refresh picks that itself); a 1.45 m cell on an edge map with 0.1 m spacing costs 10x.
 * Point indices reported by the library refer to this input order. */
int ll_map_upload(ll_map *m, int32_t kind, const float *xyz, int32_t stride_floats, int64_t n, float cell_size);
int64_t ll_map_size(const ll_map *m, int32_t kind);

/* Number of search structures published for `kind` so far (by ll_map_upload, ll_map_to_f16, ll_history_refresh*).  A host-side
 * cache of "what did I upload last" (include/loam_livox_adapter.hpp keys the map clouds of find_out_incremental_transfrom,
 * point_cloud_registration.hpp:163-168, by their contents) stays valid only while this number is the one it saw after its own
 * upload; -1 for a bad argument. */
int64_t ll_map_generation(const ll_map *m, int32_t kind);
/* cells of the published grid of `kind` (the cell table is 4 bytes per cell): with ll_map_size() the map's footprint in HBM */
int64_t ll_map_cells(const ll_map *m, int32_t kind);
/* ll_map_upload that also reports the generation number ITS publication got (taken under the map's lock): a cache keyed by
 * "generation after my upload" must use this one -- reading ll_map_generation after ll_map_upload returns would pick up a
 * publication another thread (ll_history_refresh*) made in between and later skip a required re-upload. */
int ll_map_upload_gen(ll_map *m, int32_t kind, const float *xyz, int32_t stride_floats, int64_t n, float cell_size, int64_t *generation);
/* BASELINE config C5 ("fp16 points / fp32 accumulate k-NN"): replaces the 16-byte fp32 records of an uploaded map kind by
 * 8-byte records -- the point's position inside its grid cell in binary16 (<= 2^-11 cell sizes off) + the cell index
 * bits -- and ll_map_knn5 then returns the exact 5-NN of that dequantised cloud, distances accumulated in fp32.  The
 * registrar refuses such a map (its parity contract is fp32 points, like pcl::KdTreeFLANN<PointXYZI>).
 * ll_map_dequantized: the cloud the fp16 records stand for, in upload order (NaN rows for dropped points). */
int ll_map_to_f16(ll_map *m, int32_t kind);
int ll_map_dequantized(ll_map *m, int32_t kind, float *xyz, int64_t capacity_points);

/* pcl::KdTreeFLANN::nearestKSearch(pt, 5, idx, sq_dis) (point_cloud_registration.hpp:249,351) for a batch of
 * host query points: exact 5-NN among map points with squared distance < max_sq_dis, ascending (d2, idx);
 * missing entries are idx -1 / d2 +inf.  Returns 0. */
int ll_map_knn5(ll_map *m, int32_t kind, const float *queries_xyz, int32_t n_queries, float max_sq_dis,
                int32_t *idx5, float *sq_dis5);
/* The same search with the queries and both result arrays resident on the device (hipMalloc'd / a framework tensor's pointer): nothing
 * crosses PCIe.  *kernel_ms (may be NULL): duration of the search kernel from HIP events on the map's stream.  Synchronous. */
int ll_map_knn5_device(ll_map *m, int32_t kind, const float *dev_queries_xyz, int64_t n_queries, float max_sq_dis, int32_t *dev_idx5,
                       float *dev_sq_dis5, float *kernel_ms);

/* ------------------------------------------------------------------------------------------------ registrar */

/* Public configuration fields of Point_cloud_registration set by Laser_mapping::init_pointcloud_registration
 * (laser_mapping.hpp:1266-1297) and class defaults (point_cloud_registration.hpp:45-103). */
typedef struct {
    int32_t if_motion_deblur;               /* :60  */
    int32_t icp_max_iterations;             /* :89  m_para_icp_max_iterations   */
    int32_t ceres_max_iterations;           /* :90  m_para_cere_max_iterations  */
    int32_t ceres_prerun_times;             /* :91  (2) */
    int32_t icp_line;                       /* :50  ICP_LINE  */
    int32_t icp_plane;                      /* :49  ICP_PLANE */
    int32_t current_frame_index;            /* :83  */
    int32_t mapping_init_accumulate_frames; /* :84  */
    int32_t maximum_allow_residual_block;   /* :103; random sub-sampling (:232-238,339-345,438-458) is only
                                               engaged when feature counts exceed it; must be >= feature count
                                               for deterministic parity runs */
    int32_t force_all_iterations;           /* harness switch: ignore the :521-526 convergence break */
    double maximum_dis_line_for_match;      /* :65 (2.0)  squared distance */
    double maximum_dis_plane_for_match;     /* :64 (50.0) squared distance */
    double huber_a;                         /* :220 ceres::HuberLoss(0.1) */
    double inliner_dis;                     /* :97  */
    double inlier_ratio;                    /* :98  */
    double minimum_icp_R_diff;              /* :94  */
    double minimum_icp_T_diff;              /* :95  */
    float para_max_angular_rate;            /* :86  (ROS optimization/max_allow_incre_R) */
    float para_max_speed;                   /* :87  (ROS optimization/max_allow_incre_T): box bound on t_incre */
    float max_final_cost;                   /* :88  (ROS optimization/max_allow_final_cost) */
    float minimum_pt_time_stamp;            /* :92  */
    float maximum_pt_time_stamp;            /* :93  */
    int32_t if_line_feature_check;          /* :46  IF_LINE_FEATURE_CHECK  (0): PCA test of the 5 line neighbours, :259-292  */
    int32_t if_plane_feature_check;         /* :48  IF_PLANE_FEATURE_CHECK (0): PCA test of the 5 plane neighbours, :357-389;
                                               uses the SURFACE cloud (the reference indexes the corner cloud, a bug) */
    int32_t subsample_seed;                 /* a13: 0 = refuse scans with more features than maximum_allow_residual_block (strict
                                               parity mode); otherwise the reference's random sub-sampling (:232-238,339-345,
                                               438-458) with a reproducible counter-based stream seeded by this value          */
} ll_reg_params;

void ll_reg_default_params(ll_reg_params *p);

/* What callers read back from the object after the call (point_cloud_registration.hpp:62-63,100-102,555-559). */
typedef struct {
    double final_cost, initial_cost;  /* summary of the last ceres::Solve */
    double inlier_threshold;          /* m_inlier_threshold (:100,:559) */
    double angular_diff_deg, t_diff;  /* m_angular_diff, m_t_diff (:517-518) */
    int32_t icp_iterations;
    int32_t n_blocks_last;            /* summary.num_residual_blocks */
    int32_t corner_avail, surf_avail; /* :325,:425 */
    int32_t lm_iterations_total;
    int32_t accepted;                 /* return value of find_out_incremental_transfrom */
    int32_t gated;                    /* :199 gate skipped the optimisation */
    int32_t aborted;                  /* the small-batch solver gave up on this scan (a barrier between its workgroups timed out):
                                         the scan is rejected (accepted 0) and its pose restored */
} ll_reg_report;

int ll_reg_create(int32_t device, int32_t max_scans, int32_t max_features_per_scan, ll_reg **out);
void ll_reg_destroy(ll_reg *r);

/* int Point_cloud_registration::find_out_incremental_transfrom(map_corner, map_surf, kd_corner, kd_surf,
 * scan_corner, scan_surf) (point_cloud_registration.hpp:163-583; the 4-argument overload :585-605 is the same
 * call after ll_map_upload).  pose_last = m_q_w_last/m_t_w_last, pose_curr in = initial guess
 * (m_q_w_curr/m_t_w_curr) / out = result, pose_incre in/out = m_para_buffer_incremental (identity for a fresh
 * object, laser_mapping.hpp:1348).  Returns 1 (accepted, or skipped by the :199 gate), 0 (rejected: pose_curr
 * restored to pose_last, :561-573), < 0 library error. */
int ll_reg_solve(ll_reg *r, const ll_map *map, const float *scan_corner_xyzi, int32_t n_corner,
                 const float *scan_surf_xyzi, int32_t n_surf, const ll_reg_params *prm, const double pose_last[7],
                 double pose_curr[7], double pose_incre[7], ll_reg_report *rep);

/* Batched form: n_scans independent registrations against the same map snapshot (the reference's
 * maximum_parallel_thread model, laser_mapping.hpp:1737-1742).  Features are taken from the extractor's
 * device-resident selection (ll_fe_select_batch) without a host round trip.  poses_* are [n_scans][7],
 * reports [n_scans], results[n_scans] = per-scan return value.  Returns 0. */
int ll_reg_solve_batch_fe(ll_reg *r, const ll_map *map, ll_fe *fe, int32_t n_scans, const ll_reg_params *prm,
                          const double *poses_last, double *poses_curr, double *poses_incre, ll_reg_report *reports,
                          int32_t *results);
/* The two halves of ll_reg_solve_batch for callers that register the same host-provided feature clouds more than once
 * (or want the upload outside a timed region): upload the per-scan corner / surface clouds into the registrar's own
 * HBM buffers, then enqueue registrations of the first n_scans of them (collect with ll_reg_collect). */
int ll_reg_upload_features(ll_reg *r, int32_t n_scans, const float *corner_xyzi, const int32_t *n_corner, int32_t stride_corner,
                           const float *surf_xyzi, const int32_t *n_surf, int32_t stride_surf);
int ll_reg_enqueue_uploaded(ll_reg *r, const ll_map *map, int32_t n_scans, const ll_reg_params *prm, const double *poses_last,
                            const double *poses_curr, const double *poses_incre);

/* Same with host feature clouds: corner_xyzi [n_scans][stride_c][4] with counts n_corner[n_scans], etc. */
int ll_reg_solve_batch(ll_reg *r, const ll_map *map, int32_t n_scans, const float *corner_xyzi,
                       const int32_t *n_corner, int32_t stride_corner, const float *surf_xyzi, const int32_t *n_surf,
                       int32_t stride_surf, const ll_reg_params *prm, const double *poses_last, double *poses_curr,
                       double *poses_incre, ll_reg_report *reports, int32_t *results);

/* Asynchronous halves of ll_reg_solve_batch_fe for benchmarking with inputs resident in HBM:
 * _enqueue uploads only the poses (n_scans*7 doubles) and launches; _collect synchronises and downloads. */
/* Mid-100 / multi-lidar form (laser_feature_extractor.hpp:348-358: the clouds of all lidars are concatenated before they are
 * published): registrar scan b is the concatenation, in head order, of the selected features of extractor slots
 * b * heads ... b * heads + heads - 1 (corner clouds together, surface clouds together), merged device to device.  Every
 * head keeps its own time base (its slot's stamp); n_scans * heads <= the extractor's max_scans, the merged counts must fit
 * the registrar's max_features.  Followed by ll_reg_collect like the other _enqueue forms. */
int ll_reg_enqueue_fe_merged(ll_reg *r, const ll_map *map, ll_fe *fe, int32_t n_scans, int32_t heads, const ll_reg_params *prm,
                             const double *poses_last, const double *poses_curr, const double *poses_incre);
int ll_reg_enqueue_fe(ll_reg *r, const ll_map *map, ll_fe *fe, int32_t n_scans, const ll_reg_params *prm,
                      const double *poses_last, const double *poses_curr, const double *poses_incre);
/* Returns 0; a negative value on an error of the call; or the number (> 0) of scans whose registration was aborted on the device
 * (ll_reg_report.aborted) -- not an error: all outputs are filled in, the aborted scans are rejected with their pose restored, the
 * results of the other scans of the batch are valid, and ll_last_error() carries the reason. */
/* RETURN VALUE of ll_reg_collect and of the calls that end in it (ll_reg_solve, ll_reg_solve_batch, ll_reg_solve_fe ...; the adapter's
 * find_out_incremental_transfrom): < 0 an error; 0 every scan solved; > 0 the NUMBER OF SCANS whose solve was abandoned (a bounded
 * wait of the small-batch grouped solver ran out, or a launch that could not hold the scan): those scans come back rejected -- result 0,
 * report.aborted 1, pose restored -- the others are valid, and ll_last_error() says why.  Callers that treat any non-zero status as
 * failure should test `< 0`. */
int ll_reg_collect(ll_reg *r, int32_t n_scans, double *poses_curr, double *poses_incre, ll_reg_report *reports,
                   int32_t *results);

/* Test tap: the three-sample line-search fit (ll_reg_core.h lm_quintic_min_step: Ceres' InterpolatingPolynomialMinimizingStepSize with
 * three samples, restated) in its sequential form and in the wavefront form the solver kernel runs, on n argument sets
 * {f0, g0, x1, f1, g1, x2, f2, g2, lo, hi}: the two must agree to the bit. */
int ll_debug_quintic(int32_t device, const double *args10, int32_t n, double *out_sequential, double *out_wavefront);

/* Test tap: the Levenberg-Marquardt controller of the solver kernels on lane 0 (ll_reg_core.h lm_init / lm_update, the specification) and
 * spread over its wavefront (ll_lm_wave.h, what the kernels run), on n scripted sequences of at most max_calls evaluations.  hdr12 holds
 * per sequence {x0[7], bound, max_iter, n_active, calls, 0}, evals28 the 28 sums of evaluation k of sequence i at [(i * max_calls + k) * 28];
 * call 0 is lm_init, the others lm_update, and a sequence ends with the first call that answers 0.  After call k the controller's state
 * (*ctl_bytes bytes each) is written to out_*[(i * max_calls + k) * *ctl_bytes] and the answer to ret_*[i * max_calls + k] (-1: not
 * called); the two forms must agree to the byte.  n = 0 returns *ctl_bytes alone. */
int ll_debug_lm_sequence(int32_t device, const double *hdr12, const double *evals28, int32_t n, int32_t max_calls, void *out_lane0,
                         void *out_wavefront, int32_t *ret_lane0, int32_t *ret_wavefront, int32_t *ctl_bytes);

/* Debug/parity taps of the first ICP iteration of scan slot `scan` after a solve: 5-NN indices/sq-distances
 * per corner / surface query (row = query, -1/inf when not found within the match radius). NULL to skip. */
int ll_reg_debug_knn(ll_reg *r, int32_t scan, int32_t *corner_idx5, float *corner_d25, int32_t *surf_idx5,
                     float *surf_d25);
/* enable: bit 0 = record the k-NN taps; bit 1 = force the general (HBM-resident) solver path that scans with
 * more than 24576 residual blocks use, for testing it on small inputs; bit 2 = disable the exact neighbour reuse
 * across ICP iterations (every iteration runs the full 5-NN search); bit 3 = try the reuse from ICP iteration 1
 * already (default: from iteration 2, the first pose update usually moves the queries too far); bit 4 = run the
 * round-1 solver fast path (49-byte fp64 plane blocks re-read on every evaluation) instead of the packed 48-byte
 * records with the LDS record cache -- an A/B switch, results agree to rounding; bit 5 = one workgroup per scan whatever
 * the batch size (by default batches of up to 16 scans give every scan a group of 8 workgroups whose cost evaluations
 * each cover an eighth of the blocks, resident in LDS; the sums are then grouped differently, so results agree with the
 * one-workgroup form to rounding, not bit for bit). */
int ll_reg_set_debug(ll_reg *r, int32_t enable);
/* Test tap: the ICP iteration (0-based, point_cloud_registration.hpp:211 `iterCount`) whose 5-NN lists ll_reg_debug_knn returns;
 * default 0.  A scan that has converged before that iteration keeps the lists of an earlier registration (or zeros). */
int ll_reg_set_debug_knn_iteration(ll_reg *r, int32_t icp_iteration);
/* Further A/B switches of ll_reg_set_debug (measurement and tests only): bit 8 = searches one per lane everywhere (no
 * wavefront-per-query search where the work is small).  Environment switches read by the library, same purpose:
 * LL_LIST_NO_LOCAL_OFFSETS (small batches launch the work-list offsets kernel like large ones), LL_VOXEL_GENERAL_PATH (read
 * when a voxel filter is created: every cloud through the multi-kernel pipeline instead of one workgroup per small cloud).
 * None of them changes a result bit.
 * Small scans (at most 1024 corner + surface queries in the largest scan of a batch: voxel-filtered clouds, laser_mapping.hpp:1367-1373)
 * take a solver of their own, one wavefront per scan in batches of 512 scans or more and four below (ll_reg_small_kernels.hip):
 * bit 15 = off (such scans on the 512-thread solver: A/B; results agree to rounding, counts exactly); bit 16 / bit 17 = one / four
 * wavefronts per scan whatever the batch size, both = two (tests); bit 18 = its workgroups in scan order instead of longest first (A/B).
 * Batches whose surface queries take the tile search in every ICP iteration search, from iteration 4 on, only the queries that have
 * moved out of the order budget of their last search (the others provably keep their list): bit 19 = every query in every iteration
 * (A/B, tests; the environment switch LL_KNN_SPARSE_FROM moves the first such iteration).  Same result bits either way; the
 * iteration whose lists ll_reg_debug_knn records (bit 0) searches every query, so that every list is written. */
/* Test tap: what the solver reads of scan slot `scan` after a registration -- per corner / surface query the neighbour record
 * {three positions in the cell-sorted map, "five found inside the radius"} (4 ints) and the block flag as built (1 byte).  Unlike the
 * lists of ll_reg_debug_knn, which only searched queries write, these are the values of the last ICP iteration whichever iteration
 * established them.  NULL to skip. */
int ll_reg_debug_blocks(ll_reg *r, int32_t scan, int32_t *corner_nn4, uint8_t *corner_flag, int32_t *surf_nn4, uint8_t *surf_flag);

/* ------------------------------------------------------------------------------------------------------------
 * VoxelGrid  (SURVEY 8(f) row 1).  pcl::VoxelGrid<pcl::PointXYZI> as hku-mars/loam_livox uses it:
 *   m_voxel_filter_for_surface / _corner     laser_feature_extractor.hpp:192-193, 372-381
 *   m_down_sample_filter_corner / _surface   laser_mapping.hpp:742-743, 1367-1373, 1434-1437, 533-537
 * i.e. setLeafSize(l, l, l); setInputCloud(c); filter(out).  Semantics: PCL 1.9 VoxelGrid::applyFilter with its
 * defaults (centroid of x, y, z and intensity per leaf, float sums, output in ascending leaf index), made
 * deterministic: the points of a leaf are summed in input order (PCL's std::sort leaves that order open), and
 * non-finite points are always skipped.  One call filters n_clouds independent clouds.
 * status[b]: 0 = filtered; 1 = "leaf size is too small for the input dataset" -> the output is a copy of the input,
 * like PCL; 2 = no finite point -> empty output. */
typedef struct ll_voxel ll_voxel;
int ll_voxel_create(int32_t device, int32_t max_clouds, int32_t max_points_per_cloud, ll_voxel **out);
void ll_voxel_destroy(ll_voxel *v);
/* xyzi / out_xyzi: [n_clouds][stride_points][4] floats on the host; n_points / n_out / status: [n_clouds]. */
int ll_voxel_filter(ll_voxel *v, int32_t n_clouds, const float *xyzi, const int32_t *n_points, int32_t stride_points,
                    const float leaf[3], float *out_xyzi, int32_t *n_out, int32_t *status);

/* m_if_input_downsample_mode (laser_mapping.hpp:1367-1373): the corner / surface clouds selected by the extractor are
 * voxel-filtered on the device (leaf line_res / plane_res, laser_mapping.hpp:742-743) and registered, without leaving
 * HBM.  vox_corner / vox_surf need max_clouds >= n_scans and max_points_per_cloud >= the extractor's max_points.
 * Collect with ll_reg_collect. */
int ll_reg_enqueue_fe_downsampled(ll_reg *r, const ll_map *map, ll_fe *fe, ll_voxel *vox_corner, ll_voxel *vox_surf,
                                  float line_res, float plane_res, int32_t n_scans, const ll_reg_params *prm,
                                  const double *poses_last, const double *poses_curr, const double *poses_incre);
/* A MAP PER SLOT: ll_reg_enqueue_fe / ll_reg_enqueue_fe_downsampled with scan b registered against maps[b] -- S independent sequences
 * that advance in lock step, frame k of all of them one batch, each against the match buffer its own earlier frames built.  Collect
 * with ll_reg_collect.
 *   maps[b] == NULL          an idle slot: comes back as a gated scan does (report.gated 1, result 1, pose untouched), whatever the
 *                            extractor slot holds.  The same handle may appear in several slots.
 *   frame_index              [n_scans], or NULL = prm->current_frame_index for every slot.
 *   gate                     the start-up gate (map sizes, frame index > mapping_init_accumulate_frames) is decided PER SLOT: a gated
 *                            slot comes back gated while its neighbours register.
 *   snapshots                both snapshots of every distinct map are pinned from the enqueue to ll_reg_collect.
 *   results                  slot b's pose, increment, result and report are those of ll_reg_enqueue_fe[_downsampled] for that scan
 *                            alone (n_scans = 1) against maps[b] with that frame index, bit for bit, whatever n_scans is: the solver form
 *                            is chosen per slot as for the scan alone.
 * Refused: null arguments, a map on another device, n_scans out of range, prm->if_motion_deblur != 0 without a time range per scan
 * (below; all before anything is launched), and a batch with a running scan beyond the compact solver's size (Mid-100 sweeps).
 *
 * MOTION DEBLUR WITH A MAP PER SLOT needs ll_reg_set_time_ranges in front of the enqueue: lock-step sequences run from their own
 * previous frame's last stamp to this frame's (laser_mapping.hpp:1336-1347), so the params' one pair per batch cannot serve them.
 *   ll_reg_set_time_ranges   one-shot, like ll_history_set_gate_pose: the next ll_reg_enqueue_fe_maps / _downsampled_maps takes the
 *                            table, whether it succeeds or is refused.  Slot b of that enqueue uses (minimum[b], maximum[b])
 *                            wherever a registration reads the params' minimum_pt_time_stamp / maximum_pt_time_stamp -- searches,
 *                            residual blocks, the *_mb solver, the information record, the deskew records (ll_reg_interpolation,
 *                            ll_cloud_undistort*, ll_history[_batch]_set_undistort) -- and the params' own pair is not read.  A
 *                            running slot gives the bits of ll_reg_enqueue_fe[_downsampled] for that scan alone with its range in
 *                            the params.  With if_motion_deblur == 0 the table is taken and not used.
 *   refused                  null arrays, n_scans < 1 or > max_scans; the next _maps enqueue when its n_scans differs; ANY single-map
 *                            enqueue while a table is pending (the table is dropped, not silently ignored); a running scan that the
 *                            single-map entry points would hand to the general solver (beyond 61 440 padded blocks, or the
 *                            force-general debug switch): the "compact solver" refusal above, before a kernel is launched.
 * The pairs wait in pinned host memory and go up with the enqueue's other per-scan data on the registrar's stream: no host wait is
 * added.  Nothing is allocated before the first call. */
int ll_reg_set_time_ranges(ll_reg *r, const float *minimum_pt_time_stamp, const float *maximum_pt_time_stamp, int32_t n_scans);
int ll_reg_enqueue_fe_maps(ll_reg *r, const ll_map *const *maps, ll_fe *fe, int32_t n_scans, const ll_reg_params *prm,
                           const int32_t *frame_index, const double *poses_last, const double *poses_curr, const double *poses_incre);
int ll_reg_enqueue_fe_downsampled_maps(ll_reg *r, const ll_map *const *maps, ll_fe *fe, ll_voxel *vox_corner, ll_voxel *vox_surf,
                                       float line_res, float plane_res, int32_t n_scans, const ll_reg_params *prm,
                                       const int32_t *frame_index, const double *poses_last, const double *poses_curr,
                                       const double *poses_incre);
/* the filtered feature counts of the last ll_reg_enqueue_fe_downsampled (after ll_reg_collect) */
int ll_voxel_counts(ll_voxel *v, int32_t n_clouds, int32_t *n_out, int32_t *status);

/* ------------------------------------------------------------------------------------------------------------
 * Match buffer, history mode  (m_matching_mode == 0).  Device-resident stand-in for
 *   m_laser_cloud_corner_history / m_laser_cloud_surface_history      laser_mapping.hpp:1443-1478
 *   update_buff_for_matching(), history branch                        laser_mapping.hpp:517-546
 * ll_history_add = "Add new frame" (laser_mapping.hpp:1417-1478): the scan's corner / surface features (sensor frame)
 * are moved to the map frame with `pose` (pointAssociateToMap without undistortion, g_if_undistore = 0), voxel-filtered
 * (leaf line_res / plane_res) and pushed onto the two FIFO histories when
 *     history.size() < maximum_history_size  ||  t_diff > history_add_t_step  ||  r_diff > history_add_angle_step * 57.3
 * with t_diff / r_diff measured from the pose of the last frame that was pushed; the oldest frame is dropped when the
 * history is longer than maximum_history_size.  *added = 1 when the frame was pushed.
 * ll_history_refresh = update_buff_for_matching: concatenation of the history frames (oldest first) -> VoxelGrid
 * (line_res / plane_res) -> the two search structures of `map` (device grids instead of two k-d tree builds).
 * Everything stays in HBM; only the counts come back. */
typedef struct ll_history ll_history;
int ll_history_create(int32_t device, int32_t maximum_history_size, int32_t max_points_per_frame, float line_res, float plane_res,
                      ll_history **out);
void ll_history_destroy(ll_history *h);
int ll_history_add(ll_history *h, const float *corner_xyzi, int32_t n_corner, const float *surf_xyzi, int32_t n_surf,
                   const double pose[7], double history_add_t_step, double history_add_angle_step, int32_t *added);
/* same, taking the clouds selected by the extractor for scan slot `scan` (device to device) */
int ll_history_add_fe(ll_history *h, ll_fe *fe, int32_t scan, const double pose[7], double history_add_t_step,
                      double history_add_angle_step, int32_t *added);
/* same, taking cloud `cloud` of the last ll_reg_enqueue_fe_downsampled (the down-sampled stacks the reference pushes,
 * laser_mapping.hpp:1367-1373,1421-1431) */
int ll_history_add_voxel(ll_history *h, ll_voxel *vox_corner, ll_voxel *vox_surf, int32_t cloud, const double pose[7],
                         double history_add_t_step, double history_add_angle_step, int32_t *added);
/* The add-frame rule of laser_mapping.hpp:1439-1451 compares, and on a push records, the node's m_q_w_curr / m_t_w_curr,
 * which at that point is still the pose BEFORE the registration just done (the new pose is copied back at :1496-1500),
 * while the clouds are moved with the registered pose.  Hand that pre-registration pose over here before an
 * ll_history_add* call (it applies to the next add only); without it the registered pose gates as well, which gives the
 * same pushes as long as both steps are 0.0 (the reference's fixed values). */
int ll_history_set_gate_pose(ll_history *h, const double pose[7]);
/* g_if_undistore = 1 for the next ll_history_add / _add_fe / _add_voxel only (laser_mapping.hpp:1424,1430:
 * pointAssociateToMap( ..., refine_blur( intensity ), g_if_undistore ) on both down-sampled clouds): that add moves its two clouds with
 * the state slot `slot` of r's last collected registration left (see "Deskewed clouds" below) instead of with `pose`; `pose` still
 * serves the add-frame rule and the cell maps' bookkeeping.  The state is copied on the device into memory of this handle when this
 * is called, so r may be enqueued again at once; the host waits for nothing.  ll_history_add_spin refuses an add after it (and
 * drops it): the spinning extractor's intensity is no time stamp (laser_feature_extractor.hpp:502). */
int ll_history_set_undistort(ll_history *h, ll_reg *r, int32_t slot);
int ll_history_refresh(ll_history *h, ll_map *map, int64_t *n_map_corner, int64_t *n_map_surf);
int32_t ll_history_size(const ll_history *h);
/* the match buffer clouds of the last refresh (host copy, for inspection / tests): returns the number of points written */
int64_t ll_history_map_cloud(ll_history *h, int32_t kind, float *xyzi, int64_t capacity_points);
/* The same clouds where they lie: a BORROWED device pointer (float4 x,y,z,intensity per point, on the history's device)
 * and the point count.  Valid until the next ll_history_refresh* on this handle; the handle's stream has been drained
 * when the call returns, so any stream of the caller may read it.  This is what the multi-GPU sub-map gather sends over
 * RCCL without a host hop. */
int ll_history_map_cloud_device(ll_history *h, int32_t kind, const float **dev_xyzi, int64_t *n_points);

/* ------------------------------------------------------------------------------------------------------------
 * Match buffers of S sequences in one handle (the lock-step mapping loop: one registration serves S sequences, slot s against
 * maps[s]).  Per slot the semantics are exactly those of ll_history_add_voxel / ll_history_add_fe with
 * ll_history_set_gate_pose, and of ll_history_refresh: the add-frame rule with the gate pose, the FIFO of
 * maximum_history_size frames, the oldest-first concatenation, VoxelGrid at line_res / plane_res, and a new snapshot of both
 * kinds published into maps[s] (ll_map_generation + 1 per kind).  What differs is the cost: an add and a refresh are each ONE
 * fixed chain of launches and host waits over all slots, whatever S is.
 *   active      [S] or NULL (= all slots).  An inactive slot is not read and not changed: its frames, its last-push pose, its
 *               match-buffer clouds and its map stay as they were, and added[s] comes back 0.
 *   poses7      [S][7] the registered poses the clouds are moved with; gate_poses7 [S][7] the poses BEFORE the registration
 *               (NULL: poses7 gates, as without ll_history_set_gate_pose)
 *   maps        [S]; maps[s] may be NULL only for an inactive slot, and no map may appear in two active slots
 * Slot s takes cloud s of the two filters (what ll_reg_enqueue_fe_downsampled_maps left there) or scan s of the extractor.
 * Refused before anything is enqueued, with the handle still usable: null handles or poses, handles on different devices,
 * filters / an extractor with fewer slots than n_sequences, a frame larger than max_points_per_frame, a map twice; at create,
 * n_sequences * maximum_history_size * max_points_per_frame >= 2^31 (the sorts index with 32 bits).
 * The search grids of one refresh share pooled storage that lives as long as any snapshot built in it is published or pinned
 * by a registration in flight: a registration enqueued before a refresh and collected after it reads the old snapshots.
 * ll_map_to_f16 refuses such a snapshot.  Cell maps per slot: ll_history_batch_enable_cell_maps below. */
typedef struct ll_history_batch ll_history_batch;
int ll_history_batch_create(int32_t device, int32_t n_sequences, int32_t maximum_history_size, int32_t max_points_per_frame,
                            float line_res, float plane_res, ll_history_batch **out);
void ll_history_batch_destroy(ll_history_batch *h);
int ll_history_batch_add_voxel(ll_history_batch *h, ll_voxel *vox_corner, ll_voxel *vox_surf, const int32_t *active,
                               const double *poses7, const double *gate_poses7, double history_add_t_step,
                               double history_add_angle_step, int32_t *added);
int ll_history_batch_add_fe(ll_history_batch *h, ll_fe *fe, const int32_t *active, const double *poses7, const double *gate_poses7,
                            double history_add_t_step, double history_add_angle_step, int32_t *added);
/* g_if_undistore = 1 for the next ll_history_batch_add_voxel / _add_fe only, the batch form of ll_history_set_undistort: that add
 * moves active slot s's two clouds with the state slot s of r's last collected registration left ("Deskewed clouds" below) instead of
 * with poses7[s], all slots in one launch; poses7 / gate_poses7 still serve the add-frame rule and the cell maps.  The S records are
 * copied on the device into memory of this handle when this is called, so r may be enqueued again at once; the host waits for nothing.
 * Refused before a first ll_reg_collect, while an enqueue is uncollected, and when r's last registration had fewer than n_sequences scans. */
int ll_history_batch_set_undistort(ll_history_batch *h, ll_reg *r);
int ll_history_batch_refresh(ll_history_batch *h, ll_map *const *maps, const int32_t *active, int64_t *n_map_corner,
                             int64_t *n_map_surf);
int32_t ll_history_batch_size(const ll_history_batch *h, int32_t sequence);
int64_t ll_history_batch_map_cloud(ll_history_batch *h, int32_t sequence, int32_t kind, float *xyzi, int64_t capacity_points);
/* The two cell maps of every slot (the sub-map a sequence hands over at its end, laser_mapping.hpp:274-275, 1492-1493).  Per slot the
 * semantics are those of ll_history_enable_cell_map: once enabled, every ACTIVE slot of ll_history_batch_add_voxel / _add_fe appends its
 * map-frame, voxel-filtered frame to that slot's corner and surface cell map, whether or not the add-frame rule pushes the frame; an
 * inactive slot's maps and their frame counters stay as they were.  Per map the rules are ll_cellmap_append's: cell index and key,
 * non-finite or out-of-range points dropped, a hit on a cell that was not updated for threshold_cell_revisit appends drops the cell's
 * stored points first, the frame counter moves by 1 per append (by 2 while the map has no cells), also for an empty cloud.
 * The cost differs: an add appends through one fixed chain of launches over all slots whose work is that of the NEW points and of the
 * cell tables -- no kernel of an add reads, sorts or moves the stored points.  The stored points are put in order, (cell key, insertion
 * order) per slot with the points of reset cells gone, when somebody reads: ll_history_batch_cell_map_stats / _dump / _device_view or
 * ll_history_batch_sync_cell_maps materialise all slots at once if an add came since the last time, and cost nothing otherwise.
 * The stores grow geometrically from n_sequences * initial_points_per_map points per kind.
 * Outputs have the layouts of ll_cellmap_stats / ll_cellmap_dump / ll_cellmap_device_view; a device view is valid until the next add.
 * Refused before anything is enqueued, with the handle still usable: a null handle, a second enable, cell_resolution <= 0,
 * initial_points_per_map < max_points_per_frame, a read before the enable, a sequence or kind out of range, buffers too small, and a
 * store that would pass 2^31 points per kind (at the enable, and at an add by the sizes of the incoming frames).
 * ll_history_batch_cell_map_work is a test tap: out[0] points appended since the enable; out[1] points that went through a sort or a
 * gather INSIDE add calls; out[2] materialisations run; out[3] kernel launches and library calls of the cell-map part of the last add. */
int ll_history_batch_enable_cell_maps(ll_history_batch *h, int64_t initial_points_per_map, float cell_resolution,
                                      int32_t threshold_cell_revisit);
int ll_history_batch_sync_cell_maps(ll_history_batch *h);
int ll_history_batch_cell_map_stats(ll_history_batch *h, int32_t sequence, int32_t kind, int64_t *n_cells, int64_t *n_points,
                                    int32_t *frame_idx);
int ll_history_batch_cell_map_dump(ll_history_batch *h, int32_t sequence, int32_t kind, float *xyzi, int64_t capacity_points,
                                   int32_t *cell_ijk, int32_t *cell_start, int32_t *cell_last_update, int64_t capacity_cells);
int ll_history_batch_cell_map_device_view(ll_history_batch *h, int32_t sequence, int32_t kind, const float **dev_xyz0,
                                          const uint64_t **dev_point_keys, int64_t *n_points, int64_t *n_cells);
int ll_history_batch_cell_map_work(ll_history_batch *h, int64_t out[4]);
/* The cell ("cube") matching mode for all slots: update_buff_for_matching with m_matching_mode == 1 (laser_mapping.hpp:471-513,
 * 533-546), per slot what ll_history_refresh_cells does for one sequence.  Needs ll_history_batch_enable_cell_maps.  For every ACTIVE
 * slot s: the cells of its two cell maps whose centre lies within maximum_search_range_corner / _surface of the translation of
 * poses7[s] and inside maximum_in_fov_angle (>= 360: no field-of-view test) of its rotation are selected; every selected cell goes
 * through the VoxelGrid (leaf line_res / plane_res) on its own; the leaves are concatenated in cell-key order, filtered once more
 * and published as the search grids of maps[s], as ll_history_batch_refresh publishes its concatenations.  With down_sample_replace
 * != 0 the leaves replace the points of their cell (the last-update stamps stay).  ll_history_batch_map_cloud then returns the
 * cell-mode buffer; an inactive slot keeps its maps, its buffer and its stored points.
 * Cost: per kind one chain of launches over all slots that selects in the cell tables, streams the log once for the live points of
 * the selected cells, moves those candidates' (key, position) pairs to the front and sorts them -- padded to the log's length, as
 * the sort's size must be known on the host without a wait, so the sort is as long as the log; no stored point is read or moved by
 * it.  A replace gives the selected cells a new epoch and writes their leaves behind the log, after the new maps are published, so
 * dead entries accumulate: the handle materialises by itself after a refresh that leaves more dead entries than live
 * ones, which keeps  log entries <= 2 * live entries + the entries of one step.  Host waits per refresh: one for the leaf counts of
 * both kinds and the two of ll_history_batch_refresh's second half (plus one when it compacts, and one per growth of a store).
 * Refused before anything is changed, with the handle still usable: null handle, maps or poses7, cell maps not enabled, a negative
 * range, a leaf so small that a cell spans more than 1020 leaves, a null map in an active slot, a map on another device or twice,
 * and a slot whose selected cells hold more leaves than its match buffer (maximum_history_size * max_points_per_frame points): the
 * error names slot, size and capacity.  Any later failure up to the publication of the maps (an allocation, a device error) also
 * leaves the stored points and epochs as they were: the replace is enqueued only after the maps are published.  A failure after
 * the publication (the launch of the replace, a compaction) returns -1 with the new maps in place; the replace is then applied for
 * none, one or both kinds, each kind whole, and the stores stay readable.
 * ll_history_batch_cell_match_work is a test tap: out[0] enqueues (launches, library calls, copies) of the cell-mode part of the last
 * refresh, the replace included, out[1] the host waits of the refresh proper including the second half's (a compaction or a growth
 * of a store waits on top and is not counted), out[2] compactions so far, out[3] / out[4] log entries and live entries
 * of the corner stores after the last refresh, out[5] / out[6] of the surface stores, out[7] candidates of the last refresh. */
int ll_history_batch_refresh_cells(ll_history_batch *h, ll_map *const *maps, const int32_t *active, const double *poses7,
                                   float maximum_search_range_corner, float maximum_search_range_surface,
                                   float maximum_in_fov_angle, int32_t down_sample_replace,
                                   int64_t *n_map_corner, int64_t *n_map_surf);
int ll_history_batch_cell_match_work(ll_history_batch *h, int64_t out[8]);
/* The full-cloud map of every slot: m_pt_cell_map_full (laser_mapping.hpp:1442, 1527), the un-filtered cloud of every accepted scan
 * in the map frame, which the key frames and the loop detector are built on (:1524-1562).  Independent of
 * ll_history_batch_enable_cell_maps: either, both or neither may be on.  Once enabled, kind 2 is valid for
 * ll_history_batch_cell_map_stats / _dump / _device_view: a read of kind 2 materialises the full store only, reads of kinds 0 and 1 and
 * the cell-mode refresh (its compaction included) never touch it, and ll_history_batch_sync_cell_maps orders whatever is enabled.
 * ll_history_batch_append_full_fe is ll_cellmap_append_touched for all ACTIVE slots at once: slot s takes the extractor's full
 * selection of scan s (ll_fe_select_batch), moves it with poses7[s] (pointAssociateToMap: double arithmetic, float store), appends
 * it under ll_cellmap_append's rules -- a point with a non-finite coordinate is dropped, the frame counter moves by 1 (by 2 while
 * the map has no cells), also for an empty selection -- and lists the cells that received at least min_points of THIS scan's stored
 * points (every cell that received one when the map had no cells at the call; points in a cell the same append reset count), in
 * ascending cell order.  n_touched[s] is the length of slot s's list; the lists stay on the handle until the next such call, and an
 * inactive slot keeps its map, its counter and its list.  ll_history_batch_full_touched reads one: *n cells, and with cell_ijk their
 * {i, j, k} (capacity_cells >= *n).
 * Cost: one gather launch, the append chain of the cell maps and five enqueues for the touched cells -- a counter per table entry
 * over the step's new log entries, a flag against the slot's threshold, a scan, a compaction; no kernel of the call reads, sorts or
 * moves a stored point.  The host waits three times (selection sizes, tables, lists); enqueues and waits do not depend on
 * n_sequences or on the number of active slots.  A growth of the store waits on top.
 * Refused before anything is enqueued, with the handle still usable: a null handle, extractor, poses7 or n_touched, a call before the
 * enable, a second enable, an extractor on another device or with fewer slots than n_sequences, a full selection larger than
 * max_points_per_frame, min_points < 1, and a store that would pass 2^31 points.
 * ll_history_batch_full_map_work is a test tap: out[0] enqueues (launches, library calls, copies) of the last append call, out[1] its
 * host waits, out[2] stored points that went through a sort or a gather inside append calls (nothing adds to it), out[3]
 * materialisations of the full store. */
int ll_history_batch_enable_full_maps(ll_history_batch *h, int64_t initial_points_per_map, float cell_resolution,
                                      int32_t threshold_cell_revisit);
int ll_history_batch_append_full_fe(ll_history_batch *h, ll_fe *fe, const int32_t *active, const double *poses7, int32_t min_points,
                                    int64_t *n_touched);
int ll_history_batch_full_touched(ll_history_batch *h, int32_t sequence, int32_t *cell_ijk, int64_t capacity_cells, int64_t *n);
int ll_history_batch_full_map_work(ll_history_batch *h, int64_t out[4]);
/* The scan log: m_laser_cloud_full_history of every slot kept on the device (laser_mapping.hpp:1456, 1480-1486, 1545-1558) -- the full
 * cloud, in the map frame, of every scan the history's add rule let in, which the key frames accumulate and the map refinement
 * filters (ll_map_refine_add_logged).  It needs the full maps.
 *   storage     a pool of blocks, one scan per block (max_points_per_frame float4, 384 KB at 24 000 points), allocated in chunks of
 *               initial_scans blocks that never move: the pool grows by another chunk and nothing is copied.  The free list, the
 *               slots' FIFOs and the groups are host bookkeeping.
 *   log_full_fe follows the append_full_fe of the same step, whose slots and selection sizes the handle remembers: every slot that
 *               is named (active NULL: all) and was active in that append gets a block; ONE launch for all slots copies x, y, z
 *               from the gathered clouds -- the very floats the full map received -- and the intensity from the scan through the
 *               extractor's full selection, which is what pointcloudAssociateToMap leaves in column 3; the block joins the slot's
 *               FIFO (:1456); then the FIFO of every slot of the append, named or not, is trimmed to maximum_history_size
 *               (:1480-1486).  No host wait; four enqueue calls whatever n_sequences is (none when every selection is empty); the
 *               extractor's stream is made to wait for the launch, so the next upload cannot replace a scan being read.
 *               The marker the append's gather writes for a refused point (non-finite coordinates, intensity 0) stays in the block:
 *               the VoxelGrid of ll_map_refine_add_logged drops it, so a filtered cloud is that of the host route, which removes
 *               such points first -- except for a pass-through selection (status 1), whose output is its input, markers included.
 *   hand_over   the slot's whole FIFO becomes a group -- an ordered list of scans under a 64-bit id that is never reused -- and the
 *               FIFO is empty afterwards (:1550-1553, 1558).  Host work only; an empty FIFO gives an empty group.
 *   drop        the groups' blocks go back to the free list (a key frame pushed out of the waiting list; close).
 *   read        test tap and debug read: the group's points in order; xyzi NULL: their number alone.
 *   work        out[0] enqueue calls and out[1] host waits of the last log call, out[2] blocks in use, out[3] blocks allocated.
 * Refused with the log untouched: null arguments, a call before the enable, a second enable, the enable before the full maps, a log
 * without an append or a second log for one append, another extractor than the append's, a sequence out of range, an unknown,
 * dropped or consumed group, a group named twice in one drop, a capacity below the group's size. */
int ll_history_batch_enable_scan_log(ll_history_batch *h, int32_t maximum_history_size, int64_t initial_scans);
int ll_history_batch_log_full_fe(ll_history_batch *h, ll_fe *fe, const int32_t *active);
int ll_history_batch_scan_log_hand_over(ll_history_batch *h, int32_t sequence, int64_t *group_id);
int ll_history_batch_scan_log_drop(ll_history_batch *h, int64_t n, const int64_t *group_ids);
int ll_history_batch_scan_log_read(ll_history_batch *h, int64_t group_id, float *xyzi, int64_t capacity_points, int64_t *n);
int ll_history_batch_scan_log_work(ll_history_batch *h, int64_t out[4]);
/* Host arithmetic only (no device needed): the geometry ll_map_upload and both refreshes give the search grid over the bounding
 * box {min x, y, z, max x, y, z} of a cloud's finite points (min > max: no finite point) with cells of cell_size metres.  The
 * cell grows by 1.5 x until the dense table has at most 2^27 cells. */
int ll_map_grid_geometry(const float bbox_min_max[6], float cell_size, int32_t dims[3], float *cell, float *slack);

/* ------------------------------------------------------------------------------------------------------------
 * Match buffer, cell ("cube") mode  (m_matching_mode == 1, the default in code,
 * laser_mapping.hpp:689).  Device-resident stand-in for
 *   Points_cloud_map<float> m_pt_cell_map_corners / m_pt_cell_map_planes   laser_mapping.hpp:274-275, 617-624
 *   Points_cloud_map::append_cloud / find_cell / find_cell_center          cell_map_keyframe.hpp:619-672, 716-759, 556-571
 *   Points_cloud_map::find_cells_in_radius                                 cell_map_keyframe.hpp:761-788
 *   Laser_mapping::if_pt_in_fov                                            laser_mapping.hpp:310-324
 *   update_buff_for_matching(), cell branch                                laser_mapping.hpp:471-513
 * A cell map bins xyz points (intensity is not kept, cell_map_keyframe.hpp:82) into cubes of edge resolution / 2
 * (set_resolution halves it, cell_map_keyframe.hpp:675-680); a cell that is hit again after not being updated for
 * minimum_revisit_threshold appended clouds starts over empty (cell_map_keyframe.hpp:735-756).
 * ll_cellmap_query_filter: the cells whose centre lies within `radius` of the pose's translation and within
 * maximum_in_fov_angle degrees of its x axis, each passed through pcl::VoxelGrid(leaf) on its own, concatenated;
 * down_sample_replace != 0 stores the filtered points back into the cells (laser_mapping.hpp:492-495).
 * maximum_in_fov_angle >= 360 switches the field-of-view test off: find_cells_in_radius on its own, as service_pub_surround_pts
 * uses it for /laser_cloud_surround (laser_mapping.hpp:1172-1187).
 * Order of the result: cells ascending by (ix, iy, iz) -- the reference's order is that of a PCL octree traversal and
 * is not reproducible; within a cell, PCL's leaf order.  Non-finite points and points beyond +-2^20 cells are dropped. */
typedef struct ll_cellmap ll_cellmap;
int ll_cellmap_create(int32_t device, int64_t max_points, float resolution, int32_t minimum_revisit_threshold, ll_cellmap **out);
void ll_cellmap_destroy(ll_cellmap *c);
/* raises the capacity to max_points (no-op when not larger); stored points, cells, revisit stamps and the frame counter are kept.  The
 * reference's Points_cloud_map grows on the heap without bound (cell_map_keyframe.hpp:619-672). */
int ll_cellmap_reserve(ll_cellmap *c, int64_t max_points);
int ll_cellmap_append(ll_cellmap *c, const float *xyzi, int32_t n);
/* append_cloud( pts, &cell_vec ) (cell_map_keyframe.hpp:619-672, the form the mapping node calls when loop closure is on,
 * laser_mapping.hpp:1527): the append, plus the cells that received at least min_points of this cloud's points (3 in the
 * reference, :646; on an empty map every cell that received a point, set_point_cloud :596-607), as cell indices [n][3] in
 * ascending cell order.  cell_ijk == NULL only counts. */
/* (ll_cellmap_append_touched never fails after the cloud has been stored: *n_touched is always the full number of touched cells; when it
 * exceeds capacity_cells the list was cut to capacity_cells entries -- call again with nothing to append is NOT a retry, the cloud is in.) */
int ll_cellmap_append_touched(ll_cellmap *c, const float *xyzi, int32_t n, int32_t min_points, int32_t *cell_ijk, int64_t capacity_cells,
                              int64_t *n_touched);
int ll_cellmap_query_filter(ll_cellmap *c, const double pose[7], float radius, float maximum_in_fov_angle, float leaf,
                            int32_t down_sample_replace, int64_t *n_cells_selected, int64_t *n_out);
/* the concatenated cloud of the last query (host copy); xyzi == NULL returns its size */
int64_t ll_cellmap_result(ll_cellmap *c, float *xyzi, int64_t capacity_points);
int ll_cellmap_stats(const ll_cellmap *c, int64_t *n_cells, int64_t *n_points, int32_t *frame_idx);
/* the whole map for inspection / tests: points in (cell, insertion) order, cell indices [n_cells][3], first point of
 * each cell [n_cells + 1], m_last_update_frame_idx [n_cells]; any output may be NULL */
int ll_cellmap_dump(ll_cellmap *c, float *xyzi, int64_t capacity_points, int32_t *cell_ijk, int32_t *cell_start,
                    int32_t *cell_last_update, int64_t capacity_cells);
/* The map where it lies: device pointers to the stored points ({x, y, z, 0} float4, ordered by (cell key, insertion order)) and to the
 * 64-bit cell key of every point.  Valid until the next call that changes this map.  Input of the multi-GPU gather of cell maps
 * (BASELINE config C4; laser_mapping.hpp:274-275, 1492-1493). */
int ll_cellmap_device_view(ll_cellmap *c, const float **dev_xyz0, const uint64_t **dev_point_keys, int64_t *n_points, int64_t *n_cells);
/* The cells of `src` named in cell_ijk[n_list][3], copied into `dst` on the device (Maps_keyframe's view of the shared cells,
 * cell_map_keyframe.hpp:1243-1261: a key frame holds pointers to the map's cells and reads them as they are now).
 *   The list is a SET: its order does not matter and a cell named twice is copied once.  A cell that src does not hold is skipped
 *   and not counted in *n_cells_found; so is an index outside +-2^20 on any axis (the packed cell key cannot represent it).
 *   n_list == 0 is legal, cell_ijk may then be NULL.
 *   dst ends with exactly the selected cells in ascending cell order, each cell's points in src's stored (insertion) order, and
 *   every point under the cell key it had in src: the key is copied, not recomputed from the coordinates.  That is the order in
 *   which an append of the selected points to an empty map stores them, the order determine_feature's float sums run in.
 *   When at least one point is copied, dst's bookkeeping is that of a freshly created map after one ll_cellmap_append of those
 *   points: frame index 2 (the reference's double increment on an empty map), every cell_last_update 0,
 *   cell_start[n_cells] == n_points.  When nothing is copied dst is empty with frame index 0.  The previous content of dst and
 *   the result of its last query are discarded in both cases; its revisit threshold stays its own.
 *   dst's capacity is raised (as by ll_cellmap_reserve) when the selection does not fit, before anything in dst is overwritten.
 *   The call fails, with ll_last_error() set and dst left as it was, when src == dst, when the two are on different devices or
 *   have different resolutions (the keys would mean different cubes), for a NULL handle (or a NULL list with n_list > 0), a
 *   negative n_list, and when dst is a history-owned handle (ll_history_cell_map).  src may be one: the call then waits for the
 *   frames handed over so far, like every ll_cellmap_* call on such a handle.
 *   src is not modified.  The call uses src's scratch between queries -- the sort-key arrays of the per-cell VoxelGrid, the head
 *   flags and the scan's temporary storage -- and not the filtered cloud: a following ll_cellmap_result still returns the last
 *   query's cloud.
 *   A map whose cells were replaced by ll_cellmap_query_filter(..., down_sample_replace = 1) stores centroids, each under its
 *   cell's key.  Extraction keeps them in that cell, where appending their coordinates again could bin a centroid that sits on
 *   a face into the neighbour.  A key frame is a set of cells, so extraction is the faithful form.
 * Either count may be NULL. */
int ll_cellmap_extract_cells(ll_cellmap *src, const int32_t *cell_ijk, int64_t n_list, ll_cellmap *dst, int64_t *n_cells_found,
                             int64_t *n_points);
/* The same out of the batched store, for several slots in one call: the key frames that lock-step sequences close in the same
 * step.  Request r (0 <= r < n_requests, 1 <= n_requests <= n_sequences) names slot sequences[r], the cells
 * cell_ijk[list_offsets[r] .. list_offsets[r + 1]) ({i, j, k} triples, counted in cells) and the destination dst[r]; a slot and a
 * destination appear at most once per call.  kind 0 / 1 read the feature cell maps (ll_history_batch_enable_cell_maps), kind 2
 * the full-cloud maps (ll_history_batch_enable_full_maps).
 *   Every dst[r] ends as ll_cellmap_extract_cells( the slot's map, its list, dst[r] ) would leave it: the selected cells in key
 *   order, every point in stored order under the key it had, frame index 2 and every stamp 0 -- or empty with frame index 0 --
 *   and no query result.  A list is a set: order and repeats do not matter, cells the SLOT does not hold (other slots may) and
 *   indices beyond +-2^20 are skipped and not counted.  n_cells_found[r] / n_points[r] are the request's totals.
 *   Cost: the store is first put in order as by every reader (at most one materialisation, with its own wait); then one copy of
 *   the requests and lists, a memset, a mark launch over the list entries, ONE scan over the cell table, a totals launch and one
 *   copy back, on which the host waits; one copy of the destinations' addresses, a table launch and a gather launch with one
 *   lane per copied point, and a final wait: nine enqueues and two waits whatever n_requests is.  Nothing is sorted and nothing
 *   of the store is written; the store, its host mirrors, the touched lists and the frame counters are unchanged.
 *   Every destination that needs room is grown (as by ll_cellmap_reserve, content kept) before any destination is overwritten:
 *   when a growth fails no destination has changed.
 *   Refused before anything is enqueued, all destinations as they were: a null handle, sequences, list_offsets, dst, dst[r] or
 *   count array (or a null cell_ijk with a non-empty list), n_requests outside 1 .. n_sequences, a sequence out of range or named
 *   twice, a destination named twice, owned by a history, on another device or of another resolution than the kind was enabled
 *   with, list_offsets that are negative or descend, lists of 2^30 / 3 cells or more in all, a kind that is not enabled.
 * ll_history_batch_extract_work is a test tap: out[0] enqueues and out[1] host waits of the last call behind the store's being put
 * in order, out[2] stored points sorted or moved by such calls (nothing adds to it), out[3] materialisations such calls caused. */
int ll_history_batch_extract_cells(ll_history_batch *h, int32_t kind, int32_t n_requests, const int32_t *sequences,
                                   const int64_t *list_offsets, const int32_t *cell_ijk, ll_cellmap *const *dst, int64_t *n_cells_found,
                                   int64_t *n_points);
int ll_history_batch_extract_work(ll_history_batch *h, int64_t out[4]);

/* Points_cloud_cell::determine_feature( if_recompute = 1 ) for every cell (cell_map_keyframe.hpp:436-473 with get_mean
 * :225-237, get_covmat :280-315, covmat_eig_decompose :239-249; SURVEY 8(f) row 4, first half): float sums and second
 * moments over the cell's points in insertion order (COMP_TYPE = float, :41), cov = (sum p p^T - n mean mean^T) / (n - 1),
 * eigen decomposition, then  < 5 points or |centre - mean| > 0.75 cell edge -> sphere;  l1 / 3 > l0 -> plane, vector =
 * eigenvector of l0;  l2 / 3 > l1 -> line, vector = eigenvector of l2;  otherwise sphere (vector reported as zero).
 * feature_type: 0 sphere, 1 line, 2 plane (Feature_type, :46-51).  Outputs in the cell order of ll_cellmap_dump:
 * feature_vector / mean / eigen_val [n_cells][3] (eigenvalues ascending), cov [n_cells][6] (xx xy xz yy yz zz); any may
 * be NULL.  The eigen decomposition is a double-precision Jacobi iteration of the float covariance; eigenvectors are
 * reported with their first non-zero component positive (Eigen's signs are arbitrary). */
int ll_cellmap_features(ll_cellmap *c, int32_t *feature_type, float *feature_vector, float *mean, float *cov, float *eigen_val,
                        int64_t capacity_cells);

/* Key-frame descriptors over the cells of a cell map: Maps_keyframe::analyze ->
 * extract_feature_mapping_new -> generate_feature_img (cell_map_keyframe.hpp:1486-1493, 1429-1484, 1385-1427) with the map
 * standing for the key frame's cell set.  Every line / plane cell contributes its feature vector, rotated into the
 * principal axes of the plane normals (eigen_decompose_of_featurevector, :1554-1567; largest eigenvalue first, third axis =
 * first x second), to a 60 x 60 (phi, theta) direction histogram (feature_direction, :1071-1089), which is then blurred
 * with a 9 x 9, sigma 4 Gaussian on the wrap-padded image (apply_guassian_blur, :1360-1372).
 *   images[4][60*60]   m_feature_img_line, m_feature_img_plane, then the same two over the cells closer to the key-frame
 *                      centre than m_roi_range (row = phi index, column = theta index)
 *   ratio_nonzero[4]   ratio_of_nonzero_in_img of the four histograms before the blur (:1142-1152)
 *   eigen_R[2][9]      the two rotations, row-major          n_vectors[4]   feature vectors per image
 *   centre_and_range   get_center() (:1291-1301) and m_roi_range = element ceil((k - 1) * roi_ratio) of the k distinct
 *                      centre distances (get_ratio_range_of_cell, :1303-1319; roi_ratio 0.9 in the reference, :1438);
 *                      roi_ratio = 0 skips the two ROI images
 * The reference iterates a std::set of cell pointers (address order) and takes Eigen's eigenvector signs; here cells come
 * in cell-index order and eigenvectors have their first non-zero component positive.  OpenCV's float summation order in
 * cv::GaussianBlur is not reproduced (kernel coefficients are cv::getGaussianKernel's). */
int ll_cellmap_keyframe_images(ll_cellmap *c, float roi_ratio, float *images, float *ratio_nonzero, float *eigen_R, int32_t *n_vectors,
                               float *centre_and_range);
/* Maps_keyframe::max_similiarity_of_two_image (cell_map_keyframe.hpp:1155-1224, minimum_zero_ratio = 0): the maximum of
 * cv::matchTemplate( wrap-padded img_b, img_a, CV_TM_CCORR_NORMED ), i.e. of the normalised correlation over circular
 * shifts of -30 .. +30 bins along both axes.  img_a, img_b: 60 x 60 host images. */
int ll_keyframe_similarity(int32_t device, const float *img_a, const float *img_b, float *similarity);

/* ------------------------------------------------------------------------------------------------------------
 * Scene alignment of two key frames (the last link of service_loop_detection, laser_mapping.hpp:1034-1036).
 * ll_cellmap_feature_clouds: extract_specify_points( e_feature_line ), ( e_feature_plane ) and get_center()
 * (cell_map_keyframe.hpp:1263-1301) of a key frame held as a cell map: the points of the cells ll_cellmap_features labels 1 (line) and
 * 2 (plane), cells in ascending cell order (the reference walks a std::set of cell pointers: address order), every cell's points in
 * stored order, every point {x, y, z, 0}; centre = ll_cellmap_keyframe_images' centre (zeros for a map without cells).  The selection
 * runs on the device (flag, one scan, one gather with a lane per stored point); this call is its host read-back.  Either buffer may be
 * NULL with its capacity 0: only the count comes back.  A buffer that is too small is an error, and nothing is written; so is a NULL
 * handle or count pointer.  centre may be NULL. */
int ll_cellmap_feature_clouds(ll_cellmap *c, float *line_xyzi, int64_t capacity_line, int64_t *n_line, float *plane_xyzi, int64_t capacity_plane,
                              int64_t *n_plane, float centre[3]);
/* Scene_alignment (scene_alignment.hpp:18-41, 233-391) with the clouds staying on the device.  ll_scene_align_run is
 * find_tranfrom_of_two_mappings( keyframe_a, keyframe_b ): key frame b (the scan) is registered against key frame a (the map), coarse to
 * fine.
 *   registrar   with registrar_init != 0 the settings of Scene_alignment::init (:233-243: ICP_LINE 0, m_max_final_cost 20000,
 *               m_para_max_speed 1000, m_para_max_angular_rate 360 * 57.3, m_inliner_dis 0.2), otherwise the registrar's class defaults;
 *               always current_frame_index 10000000, ceres_max_iterations 50, ceres_prerun_times 2 (:296-303);
 *   start       identity rotation and centre_a - centre_b (float) as translation, in m_q/t_w_curr and in the increment, set on every
 *               call: nothing of the previous pair is kept (the reference's object keeps m_q_w_incre);
 *   scales      8, 4, 0 times line_res / plane_res, clamped from below to them; ICP iterations doubled at the finest (:313-327);
 *   per scale   the four clouds through the VoxelGrid (an empty cloud is passed on empty); a's filtered line / plane clouds become the
 *               map's corner / surface kind, b's the scan's corner / surface stack; the registration is skipped when either of a's is
 *               empty (point_cloud_registration.hpp:595-602); stop when inlier_threshold > 2 * accepted_threshold (:350-351);
 *   outputs     pose = m_q_w_curr, m_t_w_curr; *inlier_threshold (0.0 when nothing was registered); reports[0 .. *n_reports) of the
 *               registrations run (<= 3).
 * The results are those of the host route (ll_cellmap_dump + ll_cellmap_features, ll_voxel_filter, ll_map_upload, ll_reg_solve) bit for
 * bit: the same kernels run on the same values in the same order.
 * The handle owns one registrar, one map, one voxel filter, the four selected clouds and their filtered forms at the three scales;
 * they start at initial_points, grow geometrically (every cloud of a run is bounded by its map's point count, known on the host) and
 * are reused across calls.  No point of either key frame crosses to the host.  The three scales' filters do not depend on the
 * registrations, so all twelve filtered clouds are enqueued behind the selection and the host waits ONCE for everything it has to
 * know -- the filtered sizes, the two centres, the bounding boxes of the six clouds that become search grids -- and then once per
 * registration, to collect it (the early stop needs that scale's report).
 * Refused before anything is launched, every handle still usable: null arguments, a cell map on another device than the handle,
 * keyframe_a == keyframe_b, non-positive resolutions or maximum_icp_iteration, a cell map of a history whose feeder has failed.
 * ll_scene_align_work is a test tap on the last run: out[0] bytes of point data copied between host and device (0: there is no such
 * copy), out[1] host waits (stream synchronisations, those inside the library calls included) = 1 + out[2], out[2] registrations run,
 * out[3] kernel launches and library calls of the selection step (both key frames: cell labels, centre, flag, scan, gather each). */
typedef struct ll_scene_align ll_scene_align;
typedef struct {
    float line_res, plane_res;      /* m_line_res, m_plane_res (scene_alignment.hpp:27-28) */
    int32_t maximum_icp_iteration;  /* :35 */
    float accepted_threshold;       /* :36 */
    int32_t maximum_residual_block; /* m_para_scene_alignments_maximum_residual_block (:34) */
    int32_t registrar_init;         /* Scene_alignment::init (:233-243) applied */
    int32_t subsample_seed;         /* ll_reg_params.subsample_seed */
} ll_scene_align_params;
void ll_scene_align_default_params(ll_scene_align_params *p); /* 0.4, 0.4, 10, 0.2, 5000, 1, 1 */
int ll_scene_align_create(int32_t device, int64_t initial_points, ll_scene_align **out);
void ll_scene_align_destroy(ll_scene_align *h);
int ll_scene_align_run(ll_scene_align *h, ll_cellmap *keyframe_a, ll_cellmap *keyframe_b, const ll_scene_align_params *p, double pose[7],
                       double *inlier_threshold, ll_reg_report reports[3], int32_t *n_reports);
int ll_scene_align_work(ll_scene_align *h, int64_t out[4]);

/* ------------------------------------------------------------------------------------------------------------
 * Key-frame descriptor bank: the line and the plane direction image of every processed key frame stay on the device, and "this key
 * frame against these earlier ones" (service_loop_detection's walk, laser_mapping.hpp:988-1057, the two max_similiarity_of_two_image
 * calls of :1009-1010) is ONE call for any number of pairs.  Every similarity is ll_keyframe_similarity( image of a, image of b ) bit
 * for bit: the same sums in the same order (one accumulator per shift, rows outer, columns inner), the norms in that kernel's own
 * summation order -- taken once, when an entry is added -- and its quotient.  A pair is ordered: a is the new key frame, b the old one.
 *   layout      entry id: [2][60 * 60] floats, line image then plane image (28 800 bytes, a multiple of 16), and two doubles (the
 *               norms).  ids count from 0 in the order of the adds and never change; the capacity doubles on demand.
 *   add_cellmap ll_cellmap_keyframe_images with the same host outputs (any may be NULL); behind it, on the cell map's stream, images 0
 *               and 1 are copied device to device into the new entry and their norms are taken: the descriptors are computed once.
 *   add_images  the two images from the host (tests; callers that already hold descriptors).
 *   images      an entry's two images back on the host.
 *   match       sim_line[p], sim_plane[p] of ( ids_a[p], ids_b[p] ), p < n_pairs: the pairs are staged in one copy, then the
 *               correlation launch (a workgroup per tile of 60 x 20 shifts, kind and pair), the finish launch and one copy back; ONE
 *               host wait whatever n_pairs is; n_pairs == 0 returns at once.
 *   debug_surface  test tap: all 3600 sums num( Y, X ), Y, X < 60 (shift index 60 repeats shift index 0), of one pair and kind (0 line,
 *               1 plane) into out[Y * 60 + X].
 *   work        test tap on the last match: out[0] enqueues (4), out[1] host waits (1), out[2] image bytes copied between host and
 *               device (0: there is no such copy), out[3] pairs.
 * Refused before anything is enqueued, the handle and its entries as they were: null arguments, ids out of range, negative counts (or
 * more than 2^24 pairs), a cell map on another device than the bank, roi_ratio outside [0, 1], a cell map of a history whose feeder has
 * failed, a bank that would pass 2^31 image floats (298 261 entries). */
typedef struct ll_keyframe_bank ll_keyframe_bank;
int ll_keyframe_bank_create(int32_t device, int64_t initial_entries, ll_keyframe_bank **out);
void ll_keyframe_bank_destroy(ll_keyframe_bank *b);
int ll_keyframe_bank_add_cellmap(ll_keyframe_bank *b, ll_cellmap *c, float roi_ratio, float *images, float *ratio_nonzero, float *eigen_R,
                                 int32_t *n_vectors, float *centre_and_range, int64_t *id);
int ll_keyframe_bank_add_images(ll_keyframe_bank *b, const float *img_line, const float *img_plane, int64_t *id);
int ll_keyframe_bank_images(ll_keyframe_bank *b, int64_t id, float *img_line, float *img_plane);
int64_t ll_keyframe_bank_size(const ll_keyframe_bank *b);
int ll_keyframe_bank_match(ll_keyframe_bank *b, int64_t n_pairs, const int64_t *ids_a, const int64_t *ids_b, float *sim_line,
                           float *sim_plane);
int ll_keyframe_bank_debug_surface(ll_keyframe_bank *b, int64_t id_a, int64_t id_b, int32_t kind, double *out);
int ll_keyframe_bank_work(ll_keyframe_bank *b, int64_t out[4]);

/* ------------------------------------------------------------------------------------------------------------
 * Pose graph: what the detector does with an accepted loop (laser_mapping.hpp:948-960, 1058-1089; ceres_pose_graph_3d.hpp:198-352;
 * scene_alignment.hpp:97-129).  G independent graphs are optimised by ONE launch (a workgroup per graph runs the whole
 * Levenberg-Marquardt loop on the device) and ONE host wait.  The map refinement behind it is ll_map_refine_*; the file dumps are not here.
 *   problem     a graph has N poses and E edges (a, b, measurement {q_m, p_m}, information 6 x 6); pose 0 is constant; any a != b.
 *               error  e = [ conj(q_a) . (p_b - p_a) - p_m ; 2 vec( q_m (x) conj( conj(q_a) (x) q_b ) ) ],  residual L e with
 *               information = L L' (factored on the host in fp64; an identity matrix skips the product).  Translation moves
 *               additively, a quaternion by Plus(q, d) = ( sin|d| / |d| d, cos|d| ) (x) q without renormalisation; analytic Jacobian; fp64.
 *   minimiser   Ceres' trust-region Levenberg-Marquardt with ll_pose_graph_params (no loss, no bounds): Jacobi scaling from the
 *               first Jacobian, damping diag(J'J) clamped and divided by the radius, the normal equations solved exactly by a
 *               Cholesky factorisation of their block envelope (poses in index order: a chain is block-tridiagonal, a loop edge
 *               a -> b lengthens the row of max(a, b) back to min(a, b); about 2 N + sum |a - b| blocks of 6 x 6), the radius and
 *               tolerance rules of Ceres 1.14's TrustRegionMinimizer.
 *   determinism no atomics; every sum runs in an order fixed by the edge list; a graph's result does not depend on n_graphs, on its
 *               place in the call, or on the run.
 *   layout      poses7 [P][7] {qx, qy, qz, qw, tx, ty, tz} of all graphs one after the other, in and out; pose_offsets[G + 1] and
 *               edge_offsets[G + 1] delimit the graphs; edge_ab[2 E] pose ids within the edge's graph; edge_meas7 [E][7] in the pose
 *               layout; edge_information [E][36] row-major, or NULL for identities.  p may be NULL (the defaults).
 *   summary     per graph.  A graph of one pose or without edges comes back unchanged with LL_POSE_GRAPH_NOTHING_TO_OPTIMISE.
 *   work        test tap on the last solve: out[0] enqueues, out[1] host waits (1), out[2] envelope blocks, out[3] graphs.
 * Refused before anything is enqueued, the poses untouched: null arguments, offsets that do not ascend from 0, ids out of range,
 * a == b, a non-finite input, an information matrix that is not positive definite (its lower triangle is read, as Eigen's llt
 * does), more graphs / poses / edges / envelope
 * blocks than the handle was created for (the text names the size needed). */
typedef struct ll_pose_graph ll_pose_graph;
typedef struct {
    int32_t max_num_iterations;                 /* 200 (ceres_pose_graph_3d.hpp:343) */
    int32_t max_num_consecutive_invalid_steps;  /* 5 */
    double initial_trust_region_radius;         /* 1e4 */
    double max_trust_region_radius;             /* 1e16 */
    double min_trust_region_radius;             /* 1e-32 */
    double min_relative_decrease;               /* 1e-3 */
    double min_lm_diagonal, max_lm_diagonal;    /* 1e-6, 1e32 */
    double function_tolerance;                  /* 1e-6 */
    double gradient_tolerance;                  /* 1e-10 */
    double parameter_tolerance;                 /* 1e-8 */
} ll_pose_graph_params;
#define LL_POSE_GRAPH_MAX_ITERATIONS 0
#define LL_POSE_GRAPH_GRADIENT 1
#define LL_POSE_GRAPH_PARAMETER 2
#define LL_POSE_GRAPH_FUNCTION 3
#define LL_POSE_GRAPH_RADIUS 4
#define LL_POSE_GRAPH_INVALID_STEPS 5
#define LL_POSE_GRAPH_NOTHING_TO_OPTIMISE 6
typedef struct {
    int32_t iterations, successful_steps, unsuccessful_steps, termination;
    double initial_cost, final_cost;
} ll_pose_graph_summary;
void ll_pose_graph_default_params(ll_pose_graph_params *p);
int ll_pose_graph_create(int32_t device, int64_t max_graphs, int64_t max_poses_total, int64_t max_edges_total, int64_t max_envelope_blocks,
                         ll_pose_graph **out);
void ll_pose_graph_destroy(ll_pose_graph *h);
int ll_pose_graph_solve(ll_pose_graph *h, const ll_pose_graph_params *p, int64_t n_graphs, const int64_t *pose_offsets, double *poses7,
                        const int64_t *edge_offsets, const int32_t *edge_ab, const double *edge_meas7, const double *edge_information,
                        ll_pose_graph_summary *summary);
int ll_pose_graph_work(ll_pose_graph *h, int64_t out[4]);

/* ------------------------------------------------------------------------------------------------------------
 * Map refinement: the corrected clouds behind a closed loop (Mapping_refine, ceres_pose_graph_3d.hpp:368-538; the node's call
 * site, laser_mapping.hpp:943-946 and 1091-1100).  The key frames' accumulated clouds stay on the device in one ragged store;
 * n_sel of them are filtered and moved into their corrected frames by ONE launch chain over the SUM of their points and ONE
 * host wait, whatever n_sel is (a fixed number of enqueue calls: see work).
 *   store       one float4 {x, y, z, intensity} array and host-known offsets; a cloud's id is its position in the order of the
 *               adds (map_id_pc.size(), :944) and never changes; the capacity doubles by a device-to-device copy.
 *   add_cloud   one upload, pcl::VoxelGrid with leaf `leaf` (surround_pointcloud_resolution, :943-946) -- ll_voxel_filter's
 *               arithmetic bit for bit, intensity averaged -- appended to the store; one host wait, for the count.
 *   affine      refine_pts' R_aff and T_aff (:444-445) from two poses {qx, qy, qz, qw, tx, ty, tz}, on the host in fp64:
 *               toRotationMatrix as Eigen writes it (no renormalisation), R_aff = float( R_opm R_ori^T ) with every double
 *               product reduced ( e0 + e1 ) + e2, T_aff = float( double( R_aff ) ( -t_ori ) + t_opm ).  Row-major R9.
 *   move        out_i = ( R_i0 x + ( R_i1 y + R_i2 z ) ) + T_i in float, not contracted (:449: Eigen's lazy product for float);
 *               the output intensity is 0 (eigen_to_pcl_pt leaves PointXYZI's default).
 *   run         selection s is cloud ids[s] (any order, duplicates and empty clouds allowed) with poses_ori7[s], poses_opm7[s].
 *               mode 0 = refine_pointcloud( ..., if_save = 0 ) (:476-485): VoxelGrid with `leaf`, then the centroids are moved
 *               (what the node runs).  mode 1 = refine_mapping's in-memory overload (:511-533): every point is moved, then
 *               VoxelGrid.  The outputs are packed in selection order and stay on the device: selection s is points
 *               offsets_out[s] .. offsets_out[s + 1] of what ll_map_refine_fetch copies out (one more copy, one more wait).
 *   status      ll_voxel_filter's: 0 filtered; 1 leaf too small for the (mode 1: moved) cloud's extent, the output is the input,
 *               moved (a non-finite point is carried along, its image whatever the float operations give); 2 no finite point.
 *   merge       VoxelGrid with `leaf` over the last run's outputs taken as one cloud (:577-578): the single corrected map.
 *   determinism no float atomics; a voxel's sums run in input order; a selection's result does not depend on n_sel, on its
 *               slot or on the run.
 *   work        test tap on the last add / run / merge and the fetches behind it: out[0] enqueue calls of the host (copies, kernel
 *               launches, the sort and the scan counted as one call each: 14 per chain whatever n_sel is -- the number of kernels
 *               inside the sort grows with the key bits in use, 32 + ceil( log2( n_sel + 1 ) )), out[1] host waits, out[2] bytes
 *               copied between host and device, out[3] points of the chain.
 * Limits: n_sel <= 2^20; fewer than 2^31 points per run and in the store.  Refused before anything is enqueued, with the
 * store and the last outputs untouched: null arguments, a mode other than 0 / 1, ids out of range, negative counts, a leaf that
 * is not positive and finite, non-finite poses, a run or a store beyond its limit, a capacity below what is to be copied out. */
typedef struct ll_map_refine ll_map_refine;
int ll_map_refine_create(int32_t device, int64_t initial_points, ll_map_refine **out);
void ll_map_refine_destroy(ll_map_refine *h);
int ll_map_refine_add_cloud(ll_map_refine *h, const float *xyzi, int64_t n, float leaf, int64_t *id, int64_t *n_kept, int32_t *status);
/* add_cloud for several key frames at once, device to device, out of the scan log of a batched match buffer
 * (ll_history_batch_enable_scan_log): request r is the concatenation, in order, of the scans of the groups
 * group_ids[group_off[r] .. group_off[r + 1]] (m_accumulated_point_cloud, laser_mapping.hpp:943-946).  One gather launch puts all
 * requests into the staging array, one filter chain over n_req selections puts them into the store under consecutive ids; ONE host
 * wait and a number of enqueue calls that does not depend on n_req; the two handles' streams are ordered with an event.  ids, n_kept,
 * status and the stored clouds are bit for bit what add_cloud gives for the same points.  The groups are consumed: their blocks are
 * free afterwards.  Refused before anything is enqueued, store and log untouched: null arguments, a scan log that is not enabled or
 * lives on another device, an unknown or consumed group, a group named twice, and add_cloud's limits. */
int ll_map_refine_add_logged(ll_map_refine *h, ll_history_batch *hb, int64_t n_req, const int64_t *group_off, const int64_t *group_ids,
                             float leaf, int64_t *ids, int64_t *n_kept, int32_t *status);
/* a cloud that is filtered already (a host-side map_id_pc entry, the adapter's Mapping_refine): stored as it is, one upload, one wait */
int ll_map_refine_add_stored(ll_map_refine *h, const float *xyzi, int64_t n, int64_t *id);
/* clouds held (the next id) */
int64_t ll_map_refine_size(const ll_map_refine *h);
/* a stored cloud back; xyzi_out NULL: its size alone */
int ll_map_refine_cloud(ll_map_refine *h, int64_t id, float *xyzi_out, int64_t capacity_points, int64_t *n);
/* host only: no device is touched */
int ll_map_refine_affine(const double *ori7, const double *opm7, float *R9_out, float *T3_out);
int ll_map_refine_run(ll_map_refine *h, int32_t mode, int64_t n_sel, const int64_t *ids, const double *poses_ori7, const double *poses_opm7,
                      float leaf, int64_t *offsets_out, int32_t *status_out);
int ll_map_refine_fetch(ll_map_refine *h, float *xyzi_out, int64_t capacity_points);
int ll_map_refine_merge(ll_map_refine *h, float leaf, int64_t *n_out, int32_t *status);
int ll_map_refine_fetch_merged(ll_map_refine *h, float *xyzi_out, int64_t capacity_points);
int ll_map_refine_work(ll_map_refine *h, int64_t out[4]);

/* The two cell maps of the mapping node, fed by every frame ll_history_add* receives (laser_mapping.hpp:1492-1493: the
 * voxel-filtered map-frame features, whether or not the frame enters the history), and the cell branch of
 * update_buff_for_matching: query + per-cell VoxelGrid (leaf line_res / plane_res) -> VoxelGrid of the concatenation ->
 * the two search structures of `map`.  ll_history_cell_map returns a borrowed handle (stats / dump). */
int ll_history_enable_cell_map(ll_history *h, int64_t max_points, float cell_resolution, int32_t threshold_cell_revisit);
ll_cellmap *ll_history_cell_map(ll_history *h, int32_t kind);
/* enable != 0: frames handed to ll_history_add* reach the two cell maps through a service thread of the handle, in order, beside the
 * caller -- in matching mode 0 nothing reads them between frames (laser_mapping.hpp:1492-1493 only appends; the reference runs its map
 * services on threads as well, :568-594), and an append re-sorts the stored map.  Every entry point that reads the cell maps
 * (ll_history_cell_map, ll_history_refresh_cells) waits for the frames handed over so far, as does ll_history_sync_cell_maps; a failure
 * of the thread is reported by the next of those calls.  The history-owned cell maps double their capacity when a frame would not fit. */
int ll_history_set_cell_map_async(ll_history *h, int32_t enable);
int ll_history_sync_cell_maps(ll_history *h);
int ll_history_refresh_cells(ll_history *h, ll_map *map, const double pose[7], float maximum_search_range_corner,
                             float maximum_search_range_surface, float maximum_in_fov_angle, int32_t down_sample_replace,
                             int64_t *n_map_corner, int64_t *n_map_surf);

/* unsigned int Point_cloud_registration::pointcloudAssociateToMap(pc_in, pc_out, if_undistore = 0)
 * (point_cloud_registration.hpp:673-685, no-deblur branch :629): p_w = q*p + t in double, stored float. */
int ll_cloud_transform(ll_reg *r, const float *in_xyzi, float *out_xyzi, int32_t n, const double pose[7]);
/* Device-resident form over an extractor's batch (the sub-map of a batched offline run): for every scan
 * b < n_scans with accept[b] != 0, the selected features of `kind` (0 corner, 1 surface; the last ll_fe_select* of slot b)
 * are moved to the map frame with poses[b] (pointAssociateToMap, no deblur) and appended, in scan order, to the
 * caller's DEVICE buffer dev_out_xyzi (float4 per point, capacity_points points) starting at point *n_points, which is
 * advanced.  Nothing crosses PCIe but the per-scan counts.  Fails, leaving *n_points untouched, if the capacity would
 * be exceeded. */
int ll_cloud_transform_fe_device(ll_reg *r, ll_fe *fe, int32_t n_scans, int32_t kind, const int32_t *accept, const double *poses7,
                                 float *dev_out_xyzi, int64_t capacity_points, int64_t *n_points);

/* ------------------------------------------------------------------------------------------------------------
 * Deskewed clouds: pointAssociateToMap / pointcloudAssociateToMap with if_undistore = 1
 * (point_cloud_registration.hpp:622-661, 673-685; the node's g_if_undistore = 1, laser_mapping.hpp:1424,1430,1442,1582,1587).
 * Every point (x, y, z, time stamp) moves with the pose interpolated at its time stamp: s = refine_blur (:128-141, float),
 * s == 1 or if_motion_deblur == 0 -> q_curr p + t_curr (:627-630); otherwise (:641-646)
 *     p_w = q_last ( (I + sin(s theta) hat + (1 - cos(s theta)) hat^2) p + s t_incre ) + t_last,   double math, float store,
 * with theta / hat from compute_interpolatation_rodrigue (:607-620) of the registration's increment.  A time stamp below
 * minimum_pt_time_stamp gives s < 0, which is not clamped (the reference extrapolates); a non-finite s counts as 1 (:137).
 * The intensity is copied (:659).  These are the numbers the registrar's own searches moved the features with (:247-248),
 * operation for operation.
 *
 * All of them use the state the last COLLECTED registration on r left in slot `slot` (scan b of the batch), and are refused
 * before a first ll_reg_collect, while an enqueue is uncollected, and for slots beyond that registration's n_scans.
 *   the time range is the registration's: the params' pair, or slot b's own pair after ll_reg_set_time_ranges (a map per slot).
 *   if_motion_deblur == 0 in that registration: the plain transform with the slot's pose_curr, bit for bit (:627).
 *   a gated slot (report.gated: :199, nothing was estimated): identity increment, theta 0, zero matrices -- the plain
 *     transform with pose_last, bit for bit.
 *   a rejected slot (result 0, :561-573): pose_curr = pose_last, and the increment of its last ICP iteration stays in place, as
 *     in the reference object.  The node never reaches its "Add new frame" for such a scan (laser_mapping.hpp:1405-1411).
 *
 * ll_reg_interpolation: m_interpolatation_theta, m_interpolatation_omega_hat (row-major 3x3), m_q_w_last / m_t_w_last and
 * m_q_w_incre / m_t_w_incre (x y z w, t) of slots 0 .. n_scans-1; any output may be NULL.  No device work.
 * ll_cloud_undistort: pointcloudAssociateToMap( in, out, 1 ) (:673-685) for a host cloud. */
int ll_reg_interpolation(ll_reg *r, int32_t n_scans, double *theta, double *omega_hat9, double *pose_last7, double *pose_incre7);
int ll_cloud_undistort(ll_reg *r, int32_t slot, const float *in_xyzi, float *out_xyzi, int32_t n);
/* ll_cloud_transform_fe_device with if_undistore = 1: slot b's selection of `kind` (0 corner, 1 surface, 2 the full selection,
 * laser_feature_extractor.hpp:246,255: intensity = time stamp) moves with slot b's state -- there is no poses7 -- and is appended
 * to dev_out_xyzi from *n_points on, in one launch for the batch.  Fails, leaving *n_points and the buffer untouched, if the
 * capacity would be exceeded. */
int ll_cloud_undistort_fe_device(ll_reg *r, ll_fe *fe, int32_t n_scans, int32_t kind, const int32_t *accept, float *dev_out_xyzi,
                                 int64_t capacity_points, int64_t *n_points);

/* HIP-event timing of the kernels launched by the last enqueue/solve on this handle (milliseconds, summed
 * over launches) and launch counts: [0] knn+block-build, [1] solver, [2] finalize. Enabled by
 * ll_reg_set_profiling(r, 1). */
int ll_reg_set_profiling(ll_reg *r, int32_t enable);
int ll_reg_kernel_times(ll_reg *r, float ms[3], int32_t launches[3]);

/* Information matrix of a registration, per scan: how well the answer is constrained.  The reference has no such output; the
 * definition is this project's (DESIGN "Registration information").  For a scan in which at least one ICP iteration ran,
 *     H = sum rho' J^T J,   g = sum rho' J^T r,   cost = 1/2 sum rho(|r|^2)
 * over the candidate blocks of the scan's LAST ICP iteration (every candidate the block build left active, corner queries then surface
 * queries), evaluated at the increment that iteration returned, in the solver's tangent d = [d_rot(3); d_t(3)]:
 * R_inc+ = Exp(2 d_rot) R_inc, t_inc+ = t_inc + d_t.  The sub-sampling drop and the inlier prune of the solve are NOT applied (the
 * pruned set never leaves the solver's registers; outliers are down-weighted by the Huber term as in every evaluation).  A scan's
 * record does not depend on its slot, the batch size, the solver or search form, or the single-map against the map-per-slot form.
 *   H       full symmetric 6 x 6, row-major;  g, cost: the gradient and the cost of the same evaluation
 *   n_line, n_plane   blocks summed
 *   status  0 computed (a rejected scan too: the caller has the accept flag); 1 not computed -- the scan was gated (PCR:199), no ICP
 *           iteration ran, or the scan had no feature -- H, g, cost zero; 2 the solve was aborted (ll_reg_report.aborted), all zero
 * (The record type cannot share the name of the entry point that fills it, so it carries the suffix _record.)
 * ll_reg_set_information(r, 1) holds from the next enqueue on (default 0: nothing is launched, allocated or copied).  With it on,
 * every enqueue launches one more kernel behind the last ICP iteration and ll_reg_collect brings the records back in the copy and the
 * one wait it makes anyway.  ll_reg_information copies the records of the last collected enqueue to out[n_scans]; it refuses -- and
 * leaves the handle usable -- a null handle or output, n_scans other than the last enqueue's, a call before ll_reg_collect, and a
 * call after an enqueue made with the switch off.  ll_reg_information_time: with ll_reg_set_profiling, the kernel's time in the last
 * collected enqueue (milliseconds; 0 when it did not run). */
typedef struct {
    double H[36];
    double g[6];
    double cost;
    int32_t n_line, n_plane, status, reserved;
} ll_reg_information_record;
int ll_reg_set_information(ll_reg *r, int32_t enable);
int ll_reg_information(ll_reg *r, int32_t n_scans, ll_reg_information_record *out);
int ll_reg_information_time(ll_reg *r, float *ms);

/* Builds compiled with -DLL_SOLVE_TIMING accumulate shader-clock counts per solver phase of scan slot `scan`:
 * [0] cost evaluations, [1] LM controller, [2] L1 pass, [3] de-duplication, [4] rank select, [5] total, [6] flag census,
 * [7] prune, [8] epilogue (plane-table path: table build); [9] counts how often the L1 pass took the values its last prerun
 * evaluation had left behind; plane-table path: [10] census load waits, [11] triple inserts, [12] block sums, [13] id compaction,
 * [14] plane constants, [15] id pass + LDS fill.  Zeros in normal builds. */
int ll_reg_debug_cycles(ll_reg *r, int32_t scan, long long out[16]);

/* Lengths of the neighbour-reuse work lists left by the last ICP iteration of the last solve, summed over the first
 * n_scans slots: out[0] / out[1] = corner queries that needed a full search / whose five neighbours were re-sorted,
 * out[2] / out[3] = the same for surface queries. */
int ll_reg_debug_worklists(ll_reg *r, int32_t n_scans, int64_t out[4]);

/* ------------------------------------------------------------------------------------------------------------
 * Spinning-lidar feature extraction: the branch of Laser_feature::laserCloudHandler the reference runs when
 * common/lidar_type is not "livox" or is missing (laser_feature_extractor.hpp:393-787, m_lidar_type = 0 at :831-851):
 * classic LOAM features of a VLP-16 / HDL-64 scan.  One message in, five clouds out:
 *   LL_SPIN_FULL        laserCloud, the kept points line after line (:513-521), published on /laser_points_2;
 *                       intensity = scanID + 0.1 * relTime (:501-502)
 *   LL_SPIN_SHARP       /laser_cloud_sharp       (:657-714, label 2)
 *   LL_SPIN_LESS_SHARP  /laser_cloud_less_sharp  (label 2 and 1)
 *   LL_SPIN_FLAT        /laser_cloud_flat        (:716-757, label -1)
 *   LL_SPIN_LESS_FLAT   /laser_cloud_less_flat   (:760-776: label <= 0, per-line VoxelGrid of leaf plane_resolution / 2,
 *                       PCL 1.9 semantics as ll_voxel_filter)
 *   LL_SPIN_LESS_FLAT_PRE  the less-flat points before the VoxelGrid (positions only; not published by the reference)
 * Every cloud is in the reference's order.  Index sets, x, y, z and the less-flat centroids are bit-exact with the host C
 * library; the intensity of laserCloud comes from the device atan2f and may differ from the host's in the last bits
 * (discrete outcomes never do: see ll_spin_resolve).
 *
 * Edges the reference leaves undefined, defined here:
 *   - startOri / endOri and the orientation loop use the first / last point of the FILTERED cloud (the reference takes
 *     cloudSize before the filters of :399-400); identical whenever nothing is filtered;
 *   - a sharp-point walk (+-500, :687-710) stops at either end of laserCloud;
 *   - no point gets a curvature (none is selected) when laserCloud has 10 points or fewer (`cloudSize - 5` is a size_t);
 *   - non-finite points are always removed (removeNaNFromPointCloud skips clouds marked is_dense);
 *   - more than max_points (<= 400 000, the size of the reference's member arrays) points is an error, not a crash;
 *   - a line with more less-flat points than max_line_points is reported as status LL_SPIN_STATUS_LINE_OVERFLOW. */
typedef struct ll_spin ll_spin; /* replaces the lidar_type = velodyne branch of Laser_feature (laser_feature_extractor.hpp:393-787) */

enum { LL_SPIN_FULL = 0, LL_SPIN_SHARP = 1, LL_SPIN_LESS_SHARP = 2, LL_SPIN_FLAT = 3, LL_SPIN_LESS_FLAT = 4, LL_SPIN_LESS_FLAT_PRE = 5 };
enum { LL_SPIN_STATUS_OK = 0, LL_SPIN_STATUS_LINE_OVERFLOW = 2 };
#define LL_SPIN_MAX_POINTS 400000

typedef struct {
    int32_t scan_line;       /* ROS feature_extraction/scan_line (:137, default 16); 16 or 64 (:160-164) */
    float minimum_range;     /* ROS feature_extraction/minimum_range (:140, default 0.1; used as float, :399) */
    float plane_resolution;  /* ROS feature_extraction/mapping_plane_resolution (:138, default 0.8); leaf = value / 2 */
    int32_t device;          /* HIP device ordinal */
    int32_t max_points;      /* capacity: input points per scan, <= LL_SPIN_MAX_POINTS */
    int32_t max_scans;       /* capacity: scans resident at once */
    int32_t max_line_points; /* capacity: less-flat points of one line handed to the VoxelGrid */
} ll_spin_params;

void ll_spin_default_params(ll_spin_params *p); /* node defaults; max_points 32768, max_scans 1, max_line_points 8192 */
/* Fails for a scan_line other than 16 / 64 (the reference refuses them at :160-164) and for bad capacities. */
int ll_spin_create(const ll_spin_params *p, ll_spin **out);
void ll_spin_destroy(ll_spin *h);
/* Uploads n_scans scans into slots first_scan ..: scan b has n_points[b] points at xyzi + b * stride_points * 4 (pcl::PointXYZI
 * payloads, as pcl::fromROSMsg gives them at :396).  Also computes startOri / endOri of each scan with the host C library
 * (:403-415).  A scan of more than max_points points fails the call before anything is changed.  Synchronous. */
int ll_spin_upload(ll_spin *h, int32_t first_scan, int32_t n_scans, const float *xyzi, const int32_t *n_points, int32_t stride_points);
/* Extracts the features of slots 0 .. n_scans-1 (:397-776).  Asynchronous on the handle's stream. */
int ll_spin_extract_batch(ll_spin *h, int32_t n_scans);
/* The scan-ID bins, the range tests, the +-2 pi unwrap tests and the halfPassed flip are decided from atanf / atan2f.  The
 * kernels list every point whose result lies within a few ulps of such a decision; this call re-decides them with the host
 * C library (what the reference executable computes on this machine), patches them and, when a decision changed, runs the
 * extraction of the last ll_spin_extract_batch again.  Synchronises.  Returns the number of listed points. */
int ll_spin_resolve(ll_spin *h);
int ll_spin_sync(ll_spin *h);
/* counts: [n_scans][5] sizes of LL_SPIN_FULL .. LL_SPIN_LESS_FLAT; status (may be NULL): [n_scans] LL_SPIN_STATUS_*.  Synchronises. */
int ll_spin_counts(ll_spin *h, int32_t n_scans, int32_t *counts, int32_t *status);
/* Cloud `which` of slot `scan`: xyzi [*n][4] and idx [*n] (either may be NULL).  idx: for LL_SPIN_FULL the index of each point
 * in the uploaded scan; for SHARP, LESS_SHARP, FLAT, LESS_FLAT_PRE the position in the LL_SPIN_FULL cloud; LL_SPIN_LESS_FLAT
 * (voxel centroids) has no index and requires idx == NULL.  Buffers hold max_points entries.  Synchronises. */
int ll_spin_cloud(ll_spin *h, int32_t scan, int32_t which, float *xyzi, int32_t *idx, int32_t *n);
/* laserCloudScans of slot `scan` as ranges of the LL_SPIN_FULL cloud: line i is [line_start[i], line_start[i] + line_n[i])
 * (scan_line entries each).  The per-line clouds of m_if_pub_each_line (/laser_scanid_<i>, :804-812).  Synchronises. */
int ll_spin_lines(ll_spin *h, int32_t scan, int32_t *line_start, int32_t *line_n);
/* One message (laserCloudHandler body :393-787 without the publishes): upload into slot 0, extract, resolve.  Synchronous.
 * Returns the scan's status (0, or LL_SPIN_STATUS_LINE_OVERFLOW), < 0 on error. */
int ll_spin_extract(ll_spin *h, const float *xyzi, int32_t n);
/* Milliseconds of the phases of the last ll_spin_extract_batch from HIP events (after a synchronising call): [0] assign,
 * [1] lines, [2] curvature, [3] sort, [4] select, [5] VoxelGrid + gather. */
int ll_spin_kernel_times(ll_spin *h, float ms[6]);

/* Hand-off of a spin handle's clouds to the registrar, the history and a device sub-map without leaving the device: the _spin forms of
 * ll_reg_enqueue_fe, ll_reg_enqueue_fe_downsampled, ll_history_add_fe and ll_cloud_transform_fe_device, with the same semantics
 * (collect with ll_reg_collect; ll_history_add_voxel serves the down-sampled stacks).
 *
 * The reference's mapping node subscribes to none of the spinning branch's topics (laser_mapping.hpp:596-598 reads /pc2_corners,
 * /pc2_surface, /pc2_full), so which clouds feed find_out_incremental_transfrom is this project's decision, the LOAM mapping convention:
 *   corner stack = LL_SPIN_LESS_SHARP, surface stack = LL_SPIN_LESS_FLAT, full cloud = LL_SPIN_FULL.
 * The results are bit for bit those of the host round trip (ll_spin_cloud -> ll_reg_upload_features / ll_history_add / ll_cloud_transform).
 *
 *   - The hand-off takes the handle's CURRENT outputs, ordered after everything queued on the handle's stream; it does not wait for the
 *     host.  Callers that want the host-libm-exact discrete decisions call ll_spin_resolve first, as for a download.
 *   - if_motion_deblur must be 0.  The spinning extractor writes intensity = scanID + scanPeriod * relTime
 *     (laser_feature_extractor.hpp:502), not a time stamp in [minimum_pt_time_stamp, maximum_pt_time_stamp]; refine_blur
 *     (point_cloud_registration.hpp:128-141) would misread it.  A non-zero flag is refused with an error, never ignored.
 *   - A scan whose status is LL_SPIN_STATUS_LINE_OVERFLOW is handed over with the clouds a download returns for it; the status stays
 *     readable through ll_spin_counts.
 *   - The less-sharp cloud holds at most 200 points x 6 sub-regions x scan_line (laser_feature_extractor.hpp:667-676): the packed corner
 *     clouds are [max_scans][min(max_points, 1200 * scan_line)] points, allocated by the first hand-off (ll_spin_create does not grow).
 *   - Until it has been collected, the registration reads the handle's buffers: extract the next batch on another handle meanwhile.
 * Errors (non-zero, text in ll_last_error; the handles stay usable): null handle, handles on different devices, n_scans above the
 * extractor's or the registrar's capacity, registrar feature capacity below the extractor's max_points, voxel filter capacity too small
 * (corner: n_scans clouds of min(max_points, 1200 * scan_line) points; surface: n_scans clouds of max_points points),
 * if_motion_deblur != 0, `which` out of range or LL_SPIN_LESS_FLAT_PRE. */
int ll_reg_enqueue_spin(ll_reg *r, const ll_map *map, ll_spin *spin, int32_t n_scans, const ll_reg_params *prm,
                        const double *poses_last, const double *poses_curr, const double *poses_incre);
int ll_reg_enqueue_spin_downsampled(ll_reg *r, const ll_map *map, ll_spin *spin, ll_voxel *vox_corner, ll_voxel *vox_surf, float line_res,
                                    float plane_res, int32_t n_scans, const ll_reg_params *prm, const double *poses_last,
                                    const double *poses_curr, const double *poses_incre);
/* Slot `scan` of the handle: its less-sharp and less-flat clouds, as ll_history_add_fe takes a Livox scan's features.  Synchronises. */
int ll_history_add_spin(ll_history *h, ll_spin *spin, int32_t scan, const double pose[7], double history_add_t_step,
                        double history_add_angle_step, int32_t *added);
/* Cloud `which` (LL_SPIN_FULL .. LL_SPIN_LESS_FLAT) of every accepted scan of slots 0 .. n_scans-1, moved with its pose and appended to
 * dev_out_xyzi from point *n_points on, as ll_cloud_transform_fe_device.  *n_points is left untouched when the buffer is too small. */
int ll_cloud_transform_spin_device(ll_reg *r, ll_spin *spin, int32_t n_scans, int32_t which, const int32_t *accept, const double *poses7,
                                   float *dev_out_xyzi, int64_t capacity_points, int64_t *n_points);
/* Milliseconds of the kernel that packed the corner stack for the last hand-off, from HIP events on the handle's stream.  Waits for it. */
int ll_spin_handoff_time(ll_spin *h, float *ms);

/* The HIP stream the handle launches on (hipStream_t), for callers that want their own events on it. */
void *ll_reg_stream(ll_reg *r);
void *ll_fe_stream(ll_fe *h);

/* Process-wide runtime hint.  The ROCm runtime multiplexes a process's HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4);
 * every handle launches on its own stream, so a host that keeps several registrations in flight (the reference runs up to
 * maximum_parallel_thread process_new_scan tasks at once, laser_mapping.hpp:1737-1742) gets two of them on one queue, where their
 * kernels serialise (measured on MI355X: 44.0 k -> 46.5 k scans/s with three 256-scan batches in flight, profiles/README.md).
 * ll_runtime_hint_hw_queues(n) sets GPU_MAX_HW_QUEUES=n for this process when the caller's environment does not set it.
 * It only takes effect when called before the process's FIRST HIP call (any library's); it never overrides the environment.
 * Returns 1 if it set the variable, 0 if the environment already had it (nothing changed), < 0 on a bad argument.
 * The library never calls it on its own: loam_livox_adapter.hpp does (once, before its first *_create) unless
 * LOAM_LIVOX_HIP_NO_RUNTIME_HINTS is defined; the Python package leaves it to the application (bench.py sets the variable itself). */
int ll_runtime_hint_hw_queues(int32_t n);

const char *ll_last_error(void);
const char *ll_version(void);

#ifdef __cplusplus
}
#endif
#endif
