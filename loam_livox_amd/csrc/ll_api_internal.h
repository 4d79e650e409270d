// ll_api_internal.h -- what the host translation units of the C ABI (ll_api_*.hip, ll_spin_api.hip) share: the error and
// allocation helpers, the handle structs that more than one file touches, the few functions that cross files, and the one view
// through which a device consumer sees a feature producer.  Host code only: never included by a *_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/loam_livox_hip.h"
#include "ll_device.h"
#include "ll_reg_core.h"
#include "ll_reg_info_core.h"
#include "ll_cellmap.h"
#include "ll_voxel.h"
#include "ll_spin.h"
#include "ll_history_batch.h"
#include "ll_cellmap_batch.h"

using namespace ll;

namespace ll {
extern thread_local std::string g_err;  // the text behind ll_last_error: one object, defined in ll_api_common.hip
int set_err(const char *where, const char *what);  // g_err = "where: what"; returns -1
int check_device(int device);
}  // namespace ll
#define HC(call)                                                        \
    do {                                                                \
        hipError_t e_ = (call);                                         \
        if (e_ != hipSuccess) return set_err(#call, hipGetErrorString(e_)); \
    } while (0)

template <typename T>
static int dmalloc(T **p, size_t count)
{
    HC(hipMalloc((void **)p, (count > 0 ? count : 1) * sizeof(T)));
    return 0;
}
#define DM(p, count)                        \
    do {                                    \
        if (dmalloc(&(p), (count)) != 0) return -1; \
    } while (0)

#define D2H_OPT(dst, src, count, type)                                                              \
    do {                                                                                            \
        if (dst) HC(hipMemcpy(dst, src, (size_t)(count) * sizeof(type), hipMemcpyDeviceToHost));    \
    } while (0)

// ============================================================================================== extractor

struct ll_fe {
    ll_fe_params prm;
    FeConst fc;
    FeDev dev;
    hipStream_t stream = nullptr;
    hipEvent_t ev_done = nullptr;
    hipEvent_t ev_staged = nullptr;  // behind the last copies out of hp_npts / hp_time0 (the next upload may rewrite the slots after it)
    bool staged_pending = false;
    int max_n_uploaded = 0;
    // sequential time base of Livox_laser (LFE:150-152)
    double first_receive_time = -1.0, last_maximum_time_stamp = 0.0;
    // mutable device arrays (non-const views of dev.*)
    float4 *d_xyzi = nullptr;
    int *d_npts = nullptr;
    double *d_time0 = nullptr;
    std::vector<int> h_npts;
    // page-locked staging of the per-scan point counts and time bases: an asynchronous copy from pageable memory makes the host
    // wait for everything queued on the stream before it -- behind the 98 MB scan upload that was 1.5 ms per step during which no
    // kernel of the batch in flight could be enqueued
    int *hp_npts = nullptr;
    double *hp_time0 = nullptr;
    int *d_last = nullptr;  // [max_scans] ll_fe_selection_last: the last position of every slot's selection (allocated by the first call)
};

// ============================================================================================== map

// A search structure is an IMMUTABLE snapshot once published (the match buffer is refreshed on one thread,
// laser_mapping.hpp:568, while process_new_scan threads register against it, :1737-1742): ll_map_upload /
// ll_history_refresh* build the next grid in buffers nobody else sees and swap the published pointer under the mutex;
// every solve pins the snapshots it was launched with until it has been collected.  A snapshot that only the pool still
// references is recycled for the next build (its buffers keep their capacity).
struct MapSnap {
    MapKind mk;
    int device = 0;
    // A snapshot of a batched refresh (ll_history_batch_refresh) has its records and its cell table in an arena it shares with the
    // other snapshots of that refresh; holding it here keeps the arena alive for as long as this snapshot is published or pinned.
    std::shared_ptr<void> arena;
    ~MapSnap()
    {
        (void)hipSetDevice(device);
        if (arena) mk.pts = nullptr, mk.cell_start = nullptr;  // (the arena's, not this snapshot's)
        map_free(mk);
    }
};
struct ll_map {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::shared_ptr<MapSnap> cur[2];
    std::vector<std::shared_ptr<MapSnap>> pool[2];
    int64_t generation[2] = {0, 0};  // snapshots published so far per kind (ll_map_generation)
};

// ============================================================================================== registrar

struct ll_reg {
    int device = 0;
    int max_scans = 0, max_feat = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_wait = nullptr;
    RegDev dev;
    RegConst rc;
    // own feature storage (host-provided features)
    float4 *d_corner = nullptr, *d_surf = nullptr;
    int *d_nc = nullptr, *d_ns = nullptr;
    std::vector<RegState> h_state;
    std::vector<int> h_nc, h_ns;
    std::shared_ptr<MapSnap> pinned[2];  // map snapshots of the solve in flight (released once it has been collected)
    // a map per slot (ll_reg_enqueue_fe_maps): both snapshots of every distinct map of the solve in flight, and the grid table
    std::vector<std::shared_ptr<MapSnap>> pinned_maps;
    Grid *d_map_tab = nullptr;     // [2 * max_scans] corner, surface grid of slot b at 2 b, 2 b + 1
    std::vector<Grid> h_map_tab;
    int debug = 0, profiling = 0;
    int debug_knn_iter = 0;  // ll_reg_set_debug_knn_iteration
    int last_n_scans = 0, last_gated = 0;
    // profiling
    std::vector<hipEvent_t> ev;   // pairs
    std::vector<int> ev_class;
    float prof_ms[4] = {0, 0, 0, 0};  // k-NN + build, solver, finalize, information (class 3: ll_reg_information_time)
    int prof_launches[4] = {0, 0, 0, 0};
    double *d_pose_tmp = nullptr;
    int uploaded_scans = 0;  // scans covered by the last ll_reg_upload_features
    // information matrix per scan (ll_reg_set_information): nothing is allocated, launched or copied while the switch is off
    int info_enable = 0;
    int info_enqueued = 0;   // the last enqueue launched reg_information_kernel
    int info_collected = 0;  // ll_reg_collect has run since the last enqueue
    InfoRecord *d_info = nullptr;     // [max_scans]
    std::vector<InfoRecord> h_info;   // the last collect's records
    // deskewed clouds (ll_cloud_undistort*, ll_history_set_undistort): nothing is allocated, launched or copied before the first of them
    int collected_scans = 0;          // slots the last ll_reg_collect brought back (0: an enqueue is uncollected, or none was made)
    UndistortRec *d_und = nullptr;    // [max_scans] the collected registration's records (reg_undistort_records)
    UndistortJob *d_und_jobs = nullptr;  // [max_scans] job table of a batched launch
    int und_valid = 0;                // d_und holds the records of the registration collected last
    // a time range per scan (ll_reg_set_time_ranges): nothing is allocated, launched or copied before the first call
    float2 *hp_ts = nullptr, *d_ts = nullptr;  // [max_scans] {minimum, maximum time stamp}: pinned host staging, device table
    int ts_pending = 0;               // n_scans of the table waiting for the next enqueue (one-shot; 0: none)
    int ts_last = 0;                  // the last enqueue ran with motion deblur on d_ts (its deskew records take their ranges from it)
};

// ---------------------------------------------------------------------------------------------------- voxel grid
struct ll_voxel {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t last_stream = nullptr;  // the stream the current contents of dev.out were produced on
    hipEvent_t ev = nullptr;
    VoxelDev dev{};
};

// ---------------------------------------------------------------------------------------------------- cell map
struct ll_history;
struct ll_cellmap {
    ll_history *owner = nullptr;  // a history's own cell map (ll_history_enable_cell_map): fed by the history, possibly on its service thread
    int device = 0;
    hipStream_t stream = nullptr;
    CellMapDev dev{};
    float4 *d_in = nullptr;   // staging of host clouds (max_points)
    double *d_pose = nullptr;
    CellStats *d_stats = nullptr;  // allocated by the first ll_cellmap_features / ll_cellmap_keyframe_images
    KfOut *d_kf = nullptr;
    int *d_list = nullptr;    // staging of a cell list (ll_cellmap_extract_cells), list_cap x {i, j, k}
    int64_t list_cap = 0;
};

// ---------------------------------------------------------------------------------------------------- scene alignment
// Scene_alignment (scene_alignment.hpp:18-41) with everything it runs on kept between calls: the registrar m_pc_reg, the map the
// source key frame's filtered clouds are built into, one voxel filter, the four selected clouds and their filtered forms at the
// three scales (ll_api_scene_align.hip).
struct ll_scene_align {
    int device = 0;
    ll_reg *reg = nullptr;
    int64_t reg_cap = 0;            // max_features_per_scan of reg
    ll_map *map = nullptr;
    ll_voxel *vox = nullptr;        // its scratch serves all twelve filter calls of a run, one after the other on one stream
    int64_t vox_cap = 0;            // its max_points_per_cloud
    float4 *sel[4] = {nullptr, nullptr, nullptr, nullptr};    // the selected clouds: a's line, a's plane, b's line, b's plane
    float4 *filt[3][4] = {};        // the same four through the VoxelGrid at each of the three scales
    int64_t sel_cap[2] = {0, 0};    // points each cloud of key frame a / b has room for, selected or filtered
    int *d_ints = nullptr;          // [4] selected sizes, [12] filtered sizes (scale-major), [12] filter status
    float *d_mm = nullptr;          // [3][2][6] bounding boxes of a's filtered clouds (the grids' geometry)
    int64_t initial_points = 0;
    int64_t work[4] = {0, 0, 0, 0}; // ll_scene_align_work
};

// ---------------------------------------------------------------------------------------------------- history
struct ll_history {
    int device = 0;
    hipStream_t stream = nullptr;
    int max_hist = 0, max_pts = 0;
    float res[2] = {0.1f, 0.4f};       // line_res, plane_res
    float4 *frames[2] = {nullptr, nullptr};  // [max_hist + 1][max_pts] ring per kind
    std::vector<int> count[2];         // points per ring slot
    int head = 0, size = 0;            // FIFO window over the ring slots
    float4 *d_in = nullptr, *d_xf = nullptr, *d_concat = nullptr;
    int *d_n = nullptr;
    double *d_pose = nullptr;
    int2 *hp_table = nullptr, *d_table = nullptr;  // [2 kinds][LL_HIST_CONCAT_MAX + 1] segment tables of the concatenation (pinned host / device)
    VoxelDev vox_frame{}, vox_map{};
    double last_q[4] = {0, 0, 0, 1}, last_t[3] = {0, 0, 0};  // m_last_his_add_q / m_last_his_add_t
    double gate[7] = {0, 0, 0, 1, 0, 0, 0};                   // ll_history_set_gate_pose: the node's pose BEFORE the registration
    bool has_gate = false;
    // ll_history_set_undistort: the next add moves its clouds with this record (a copy this handle owns, made on the registrar's stream;
    // ev_und orders this handle's stream behind the copy).  Both allocated by the first call.
    UndistortRec *d_und = nullptr;
    hipEvent_t ev_und = nullptr;
    bool has_und = false;
    bool use_und = false;  // the add in progress was preceded by the setter
    int64_t n_map[2] = {0, 0};
    float4 *d_map[2] = {nullptr, nullptr};   // filtered match buffer of the last refresh
    // m_pt_cell_map_corners / m_pt_cell_map_planes (laser_mapping.hpp:274-275), ll_history_enable_cell_map
    ll_cellmap *cells[2] = {nullptr, nullptr};
    VoxelDev vox_cells{};
    float4 *d_cmap[2] = {nullptr, nullptr};  // match buffer of the last ll_history_refresh_cells
    const float4 *map_src[2] = {nullptr, nullptr};
    // The cell maps fed BESIDE the mapping loop (ll_history_set_cell_map_async): in matching mode 0 nothing reads them between frames
    // (laser_mapping.hpp:1492-1493 only appends), and an append re-sorts the whole stored map -- 0.4 ms per frame once the map holds a
    // couple of million points.  A service thread (the reference runs its map services on threads too, laser_mapping.hpp:568-594) takes the
    // filtered frames from a ring of staging buffers and appends them in order on the cell maps' own streams; every reader drains it first.
    bool cells_async = false;
    std::thread feeder;
    std::mutex mu;
    std::condition_variable cv_job, cv_idle;
    struct FeedJob {
        int kind, slot, n;
        hipEvent_t ready;  // recorded on h->stream behind the copy into the staging slot
    };
    std::deque<FeedJob> jobs;
    int in_flight = 0;        // jobs queued or being appended
    bool stop = false;
    std::string feed_error;   // first failure of the thread (reported by the next drain)
    static constexpr int kStage = 16;
    float4 *stage[2][16] = {};
    int stage_next[2] = {0, 0};
};

// ============================================================================================== feature view
namespace ll {

// What a device consumer (registrar, history) sees of a feature producer: a corner and a surface stack, [S][stride] points with
// [S] device counts.  `producer` names the streams a consumer must order itself after; a slot may be null.
struct FeatView {
    const float4 *corner, *surf;
    const int *n_corner, *n_surf;
    int stride_c, stride_s;
    hipStream_t producer[2];
};
// the extractor's selection (ll_fe_select_batch)
inline FeatView feat_view(const ll_fe *fe) { return {fe->dev.corner_feat, fe->dev.surf_feat, fe->dev.n_corner, fe->dev.n_surf, fe->dev.stride, fe->dev.stride, {fe->stream, nullptr}}; }
// a pair of voxel filters: the streams their current contents were produced on
inline FeatView feat_view(const ll_voxel *vc, const ll_voxel *vs) { return {vc->dev.out, vs->dev.out, vc->dev.n_out, vs->dev.n_out, vc->dev.out_stride, vs->dev.out_stride, {vc->last_stream, vs->last_stream}}; }
// a spin handle after spin_handoff: corner stack = LL_SPIN_LESS_SHARP (packed by spin_pack_kernel), surface stack = LL_SPIN_LESS_FLAT
inline FeatView feat_view(const SpinView &v) { return {v.corner, v.surf, v.n_corner, v.n_surf, v.pack_stride, v.max_points, {v.stream, nullptr}}; }
// the registrar's own storage (ll_reg_upload_features, ll_reg_enqueue_fe_merged), written on its own stream
inline FeatView feat_view(const ll_reg *r) { return {r->d_corner, r->d_surf, r->d_nc, r->d_ns, r->max_feat, r->max_feat, {nullptr, nullptr}}; }
// the host waits for the view's producers only (a device-wide barrier would serialise independent sequences sharing the GPU)
inline int feat_sync(const FeatView &v)
{
    if (v.producer[0]) HC(hipStreamSynchronize(v.producer[0]));
    if (v.producer[1] && v.producer[1] != v.producer[0]) HC(hipStreamSynchronize(v.producer[1]));
    return 0;
}

// ---- the functions that cross files (documented where they are defined; the spin view functions are declared in ll_spin.h)
// ll_api_map.hip
std::shared_ptr<MapSnap> map_pin(const ll_map *cm, int kind);
std::shared_ptr<MapSnap> map_build_target(ll_map *m, int kind);
int64_t map_publish(ll_map *m, int kind, const std::shared_ptr<MapSnap> &s);
int map_rebuild(ll_map *m, int kind, const float *d_raw, int stride, int64_t n, float cell, hipStream_t s, const char **err,
                int64_t *generation = nullptr);
int map_rebuild_boxed(ll_map *m, int kind, const float *d_raw, int stride, int64_t n, float cell, const float mm[6], hipStream_t s, const char **err);
// ll_api_reg.hip
int reg_enqueue_device_clouds(const char *where, ll_reg *r, const ll_map *map, const float4 *d_corner, const int *d_n_corner, int n_corner,
                              const float4 *d_surf, const int *d_n_surf, int n_surf, const ll_reg_params *prm, const double pose_last[7],
                              const double pose_curr[7], const double pose_incre[7]);
int reg_undistort_records(const char *where, ll_reg *r, int n_slots);
// ll_api_cellmap.hip
void cellmap_release(ll_cellmap *c);
int cellmap_make_room(ll_cellmap *c, int64_t max_points, const char *where);
int cellmap_settle(const ll_cellmap *c);
// ll_api_scene_align.hip
int cellmap_feature_clouds_enqueue(ll_cellmap *c, float4 *d_line, float4 *d_plane, int *d_n_line, int *d_n_plane, hipStream_t s, const char *where);
// ll_api_history.hip
int history_cells_drain(ll_history *h);
float match_cell_size(int kind, float leaf);
bool history_add_frame(const double gate_pose[7], const double last_q[4], const double last_t[3], int size, int capacity, double t_step,
                       double angle_step);

}  // namespace ll
