// A recording stand-in for libloamlivox_hip.so, for the CPU tier of include/loam_livox_adapter.hpp (adapter_lifetime_host.cpp,
// adapter_calls_host.cpp, which #include this file): the ll_* functions those two drivers reach, written by hand.  Each one appends a
// line to standin::log() -- its name, its scalar arguments, the identity of its handles as kind#ordinal, and for an array its
// length with its values (up to 8 elements) or a hash of its bytes -- and answers 0.  *_create hands out fresh non-null handles and
// counts them, *_destroy counts them back; a null handle is refused with the library's "null handle".  What a function answers as a
// count comes from standin::size(), which the driver sets (default 0; a negative value makes the function fail).  Clouds handed
// back are base + 0.25 * i in float i, so that what a method returns can be compared too.  No device and no library are needed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "loam_livox_hip.h"

namespace standin {

struct Book {
    std::string name;  // kind#ordinal
    int created = 0, destroyed = 0;
};
static std::vector<std::string> &log()
{
    static std::vector<std::string> l;
    return l;
}
static std::map<std::string, int64_t> &size()
{
    static std::map<std::string, int64_t> s;
    return s;
}
static std::map<const void *, Book> &handles()
{
    static std::map<const void *, Book> h;
    return h;
}
static std::map<std::string, int> &made()  // handles created per kind
{
    static std::map<std::string, int> m;
    return m;
}
static std::string &error()
{
    static std::string e;
    return e;
}
static int64_t size_of(const char *name, int64_t otherwise = 0) { return size().count(name) ? size()[name] : otherwise; }

static std::string num(double v)
{
    char b[40];
    std::snprintf(b, sizeof(b), "%.9g", v);
    return b;
}
static std::string hnd(const void *p)
{
    if (!p) return "null";
    return handles().count(p) ? handles()[p].name : "unknown";
}
template <class T>
static std::string arr(const char *tag, const T *p, int64_t n)
{
    if (!p) return "null";
    std::ostringstream s;
    s << tag << "[" << n << "]";
    if (n <= 0) return s.str();
    if (n <= 8) {
        s << "{";
        for (int64_t i = 0; i < n; i++) s << (i ? " " : "") << num((double)p[i]);
        s << "}";
    } else {
        uint64_t h = 1469598103934665603ull;  // FNV-1a over the bytes
        const unsigned char *b = (const unsigned char *)p;
        for (size_t i = 0; i < (size_t)n * sizeof(T); i++) h = (h ^ b[i]) * 1099511628211ull;
        char x[24];
        std::snprintf(x, sizeof(x), ":%016llx", (unsigned long long)h);
        s << x;
    }
    return s.str();
}
static std::string out(const void *p) { return p ? "out" : "null"; }

struct Line {  // one log line: name( argument, argument, ... )
    std::ostringstream s;
    bool first = true;
    explicit Line(const char *fn) { s << fn << "("; }
    Line &operator<<(const std::string &v)
    {
        s << (first ? "" : ", ") << v;
        first = false;
        return *this;
    }
    Line &operator<<(const char *v) { return *this << std::string(v); }
    Line &operator<<(double v) { return *this << num(v); }
    Line &operator<<(float v) { return *this << num(v); }
    Line &operator<<(int v) { return *this << std::to_string(v); }
    Line &operator<<(long v) { return *this << std::to_string(v); }
    Line &operator<<(long long v) { return *this << std::to_string(v); }
    ~Line() { log().push_back(s.str() + ")"); }
};

template <class T>
static int create(const char *kind, T **o)
{
    const int k = made()[kind]++;
    T *h = (T *)(uintptr_t)(0x1000 + 0x10 * handles().size());  // never dereferenced
    handles()[h].name = std::string(kind) + "#" + std::to_string(k);
    handles()[h].created++;
    *o = h;
    return 0;
}
static void destroy(const char *fn, const void *h)
{
    Line(fn) << hnd(h);
    if (h) handles()[h].destroyed++;
}
static int fail(const char *fn, const char *why)
{
    error() = std::string(fn) + ": " + why;
    return -1;
}
static void fill(float *p, int64_t n_points, float base)
{
    for (int64_t i = 0; i < 4 * n_points; i++) p[i] = base + 0.25f * (float)i;
}
// size-then-fill with the count returned
static int64_t counted(const char *fn, float *xyzi, int64_t capacity, float base)
{
    const int64_t n = size_of(fn);
    if (n < 0) return fail(fn, "the stand-in was told to fail");
    if (xyzi) fill(xyzi, n < capacity ? n : capacity, base);
    return n;
}
// handles that were not destroyed exactly once (the registrars and maps of Handle_pool live as long as the process, by design)
static int leaked(std::string *which = nullptr)
{
    int bad = 0;
    for (const auto &kv : handles()) {
        const std::string &n = kv.second.name;
        if (n.compare(0, 4, "reg#") == 0 || n.compare(0, 4, "map#") == 0) continue;
        if (kv.second.created != 1 || kv.second.destroyed != 1) {
            bad++;
            if (which) *which += n + " destroyed " + std::to_string(kv.second.destroyed) + " times; ";
        }
    }
    return bad;
}
static int64_t map_generation[2] = {0, 0};
static int64_t next_stored_id = 0, last_run_points = 0;

}  // namespace standin

#define NEED(h) \
    if (!(h)) return standin::fail(fn, "null handle")

extern "C" {
using namespace standin;

const char *ll_last_error(void) { return error().c_str(); }
int ll_runtime_hint_hw_queues(int32_t n)
{
    Line("ll_runtime_hint_hw_queues") << n;
    return 0;
}

// ---- extractor
void ll_fe_default_params(ll_fe_params *p)
{
    std::memset(p, 0, sizeof(*p));
    p->max_points = 24000, p->max_scans = 1;
}
int ll_fe_create(const ll_fe_params *p, ll_fe **o)
{
    Line("ll_fe_create") << p->thr_corner_curvature << p->thr_surface_curvature << p->minimum_view_angle << p->livox_min_allow_dis << p->livox_min_sigma
                         << p->max_fov << p->time_internal_pts << p->device << p->max_points << p->max_scans << p->piecewise_number;
    return create("fe", o);
}
void ll_fe_destroy(ll_fe *h) { destroy("ll_fe_destroy", h); }
int ll_fe_extract(ll_fe *h, const float *xyzi, int32_t n, double time_stamp, int32_t *n_petal_clouds)
{
    const char *fn = "ll_fe_extract";
    NEED(h);
    Line(fn) << hnd(h) << arr("f32", xyzi, 4 * (int64_t)n) << n << time_stamp;
    *n_petal_clouds = 0;
    return 0;
}
int ll_fe_labels(ll_fe *h, int32_t scan, int32_t *, int32_t *, float *, float *, float *, float *, float *, float *)
{
    const char *fn = "ll_fe_labels";
    NEED(h);
    Line(fn) << hnd(h) << scan;
    return 0;  // (the caller's arrays are zero already)
}
int ll_fe_splits(ll_fe *h, int32_t scan, int32_t *, int32_t *n_split, int32_t *clutter_size, int32_t *n_petal_clouds, int32_t *, int32_t *, float *, float *)
{
    const char *fn = "ll_fe_splits";
    NEED(h);
    Line(fn) << hnd(h) << scan;
    *n_split = *clutter_size = *n_petal_clouds = 0;
    return 0;
}
int ll_fe_select(ll_fe *h, float, float, int32_t *, int32_t *, int32_t *, int32_t *, int32_t *, int32_t *, float *, float *)
{
    const char *fn = "ll_fe_select";
    NEED(h);
    return 0;
}

// ---- spinning extractor
void ll_spin_default_params(ll_spin_params *p)
{
    std::memset(p, 0, sizeof(*p));
    p->scan_line = 16, p->minimum_range = 0.1f, p->plane_resolution = 0.8f, p->max_scans = 1, p->max_line_points = 8192;
    p->max_points = (int32_t)size_of("ll_spin_default_params", 32768);
}
int ll_spin_create(const ll_spin_params *p, ll_spin **o)
{
    Line("ll_spin_create") << p->scan_line << p->minimum_range << p->plane_resolution << p->device << p->max_points << p->max_scans << p->max_line_points;
    return create("spin", o);
}
void ll_spin_destroy(ll_spin *h) { destroy("ll_spin_destroy", h); }
int ll_spin_extract(ll_spin *h, const float *xyzi, int32_t n)
{
    const char *fn = "ll_spin_extract";
    NEED(h);
    Line(fn) << hnd(h) << arr("f32", xyzi, 4 * (int64_t)n) << n;
    return (int)size_of(fn);  // the scan's status
}
int ll_spin_cloud(ll_spin *h, int32_t scan, int32_t which, float *xyzi, int32_t *idx, int32_t *n)
{
    const char *fn = "ll_spin_cloud";
    NEED(h);
    Line(fn) << hnd(h) << scan << which << out(xyzi) << out(idx);
    *n = (int32_t)size_of(fn);
    fill(xyzi, *n, (float)which);
    return 0;
}

// ---- voxel filter
int ll_voxel_create(int32_t device, int32_t max_clouds, int32_t max_points_per_cloud, ll_voxel **o)
{
    Line("ll_voxel_create") << device << max_clouds << max_points_per_cloud;
    return create("voxel", o);
}
void ll_voxel_destroy(ll_voxel *v) { destroy("ll_voxel_destroy", v); }
int ll_voxel_filter(ll_voxel *v, int32_t n_clouds, const float *xyzi, const int32_t *n_points, int32_t stride_points, const float leaf[3], float *o,
                    int32_t *n_out, int32_t *status)
{
    const char *fn = "ll_voxel_filter";
    NEED(v);
    Line(fn) << hnd(v) << n_clouds << arr("f32", xyzi, 4 * (int64_t)n_points[0]) << n_points[0] << stride_points << arr("f32", leaf, 3);
    std::memcpy(o, xyzi, sizeof(float) * 4 * (size_t)n_points[0]);  // every point its own voxel
    *n_out = n_points[0], *status = 0;
    return 0;
}

// ---- history buffers
int ll_history_create(int32_t device, int32_t maximum_history_size, int32_t max_points_per_frame, float line_res, float plane_res, ll_history **o)
{
    Line("ll_history_create") << device << maximum_history_size << max_points_per_frame << line_res << plane_res;
    return create("history", o);
}
void ll_history_destroy(ll_history *h) { destroy("ll_history_destroy", h); }
int32_t ll_history_size(const ll_history *h)
{
    Line("ll_history_size") << hnd(h);
    return 0;
}
int64_t ll_history_map_cloud(ll_history *h, int32_t kind, float *xyzi, int64_t capacity_points)
{
    const char *fn = "ll_history_map_cloud";
    NEED(h);
    Line(fn) << hnd(h) << kind << out(xyzi) << (long long)capacity_points;
    return counted(fn, xyzi, capacity_points, (float)kind);
}
int ll_history_batch_create(int32_t device, int32_t n_sequences, int32_t maximum_history_size, int32_t max_points_per_frame, float line_res,
                            float plane_res, ll_history_batch **o)
{
    Line("ll_history_batch_create") << device << n_sequences << maximum_history_size << max_points_per_frame << line_res << plane_res;
    return create("history_batch", o);
}
void ll_history_batch_destroy(ll_history_batch *h) { destroy("ll_history_batch_destroy", h); }
int32_t ll_history_batch_size(const ll_history_batch *h, int32_t sequence)
{
    Line("ll_history_batch_size") << hnd(h) << sequence;
    return 0;
}
int64_t ll_history_batch_map_cloud(ll_history_batch *h, int32_t sequence, int32_t kind, float *xyzi, int64_t capacity_points)
{
    const char *fn = "ll_history_batch_map_cloud";
    NEED(h);
    Line(fn) << hnd(h) << sequence << kind << out(xyzi) << (long long)capacity_points;
    return counted(fn, xyzi, capacity_points, (float)(10 * sequence + kind));
}
int ll_history_batch_scan_log_read(ll_history_batch *h, int64_t group_id, float *xyzi, int64_t capacity_points, int64_t *n)
{
    const char *fn = "ll_history_batch_scan_log_read";
    NEED(h);
    Line(fn) << hnd(h) << (long long)group_id << out(xyzi) << (long long)capacity_points;
    const int64_t c = counted(fn, xyzi, capacity_points, (float)group_id);
    if (c >= 0) *n = c;
    return c < 0 ? -1 : 0;
}
int ll_history_batch_extract_cells(ll_history_batch *h, int32_t kind, int32_t n_requests, const int32_t *sequences, const int64_t *list_offsets,
                                   const int32_t *cell_ijk, ll_cellmap *const *dst, int64_t *n_cells_found, int64_t *n_points)
{
    const char *fn = "ll_history_batch_extract_cells";
    NEED(h);
    std::string maps;
    for (int32_t r = 0; r < n_requests; r++) maps += (r ? " " : "") + hnd(dst[r]);
    Line(fn) << hnd(h) << kind << n_requests << arr("i32", sequences, n_requests) << arr("i64", list_offsets, (int64_t)n_requests + 1)
             << arr("i32", cell_ijk, 3 * list_offsets[n_requests]) << ("dst{" + maps + "}");
    for (int32_t r = 0; r < n_requests; r++) n_cells_found[r] = list_offsets[r + 1] - list_offsets[r], n_points[r] = 10 * (r + 1);
    return 0;
}

// ---- cell maps
int ll_cellmap_create(int32_t device, int64_t max_points, float resolution, int32_t minimum_revisit_threshold, ll_cellmap **o)
{
    Line("ll_cellmap_create") << device << (long long)max_points << resolution << minimum_revisit_threshold;
    return create("cellmap", o);
}
void ll_cellmap_destroy(ll_cellmap *c) { destroy("ll_cellmap_destroy", c); }
int ll_cellmap_stats(const ll_cellmap *c, int64_t *n_cells, int64_t *n_points, int32_t *frame_idx)
{
    const char *fn = "ll_cellmap_stats";
    NEED(c);
    Line(fn) << hnd(c) << out(n_cells) << out(n_points) << out(frame_idx);
    if (n_cells) *n_cells = size_of(fn);
    if (n_points) *n_points = size_of(fn);
    if (frame_idx) *frame_idx = 0;
    return 0;
}
int ll_cellmap_extract_cells(ll_cellmap *src, const int32_t *cell_ijk, int64_t n_list, ll_cellmap *dst, int64_t *n_cells_found, int64_t *n_points)
{
    const char *fn = "ll_cellmap_extract_cells";
    NEED(src);
    Line(fn) << hnd(src) << arr("i32", cell_ijk, 3 * n_list) << (long long)n_list << hnd(dst);
    *n_cells_found = n_list, *n_points = 3 * n_list;
    return 0;
}
int ll_cellmap_feature_clouds(ll_cellmap *c, float *line_xyzi, int64_t capacity_line, int64_t *n_line, float *plane_xyzi, int64_t capacity_plane,
                              int64_t *n_plane, float centre[3])
{
    const char *fn = "ll_cellmap_feature_clouds";
    NEED(c);
    Line(fn) << hnd(c) << out(line_xyzi) << (long long)capacity_line << out(plane_xyzi) << (long long)capacity_plane << out(centre);
    *n_line = size_of("n_line"), *n_plane = size_of("n_plane");
    if (line_xyzi) fill(line_xyzi, *n_line < capacity_line ? *n_line : capacity_line, 1.0f);
    if (plane_xyzi) fill(plane_xyzi, *n_plane < capacity_plane ? *n_plane : capacity_plane, 2.0f);
    return 0;
}
int ll_cellmap_query_filter(ll_cellmap *c, const double pose[7], float radius, float maximum_in_fov_angle, float leaf, int32_t down_sample_replace,
                            int64_t *n_cells_selected, int64_t *n_out)
{
    const char *fn = "ll_cellmap_query_filter";
    NEED(c);
    Line(fn) << hnd(c) << arr("f64", pose, 7) << radius << maximum_in_fov_angle << leaf << down_sample_replace;
    *n_cells_selected = 1, *n_out = size_of("ll_cellmap_result");
    return 0;
}
int64_t ll_cellmap_result(ll_cellmap *c, float *xyzi, int64_t capacity_points)
{
    const char *fn = "ll_cellmap_result";
    NEED(c);
    Line(fn) << hnd(c) << out(xyzi) << (long long)capacity_points;
    return counted(fn, xyzi, capacity_points, 3.0f);
}

// ---- registrar and map
int ll_map_create(int32_t device, ll_map **o)
{
    Line("ll_map_create") << device;
    return create("map", o);
}
int64_t ll_map_generation(const ll_map *m, int32_t kind)
{
    Line("ll_map_generation") << hnd(m) << kind;
    return map_generation[kind];
}
int ll_map_upload_gen(ll_map *m, int32_t kind, const float *xyz, int32_t stride_floats, int64_t n, float cell_size, int64_t *generation)
{
    const char *fn = "ll_map_upload_gen";
    NEED(m);
    std::vector<float> pts;  // the coordinates as the library reads them, at the caller's stride
    for (int64_t i = 0; i < n; i++) pts.insert(pts.end(), xyz + i * stride_floats, xyz + i * stride_floats + 3);
    Line(fn) << hnd(m) << kind << (xyz ? arr("xyz", pts.data(), (int64_t)pts.size()) : "null") << stride_floats << (long long)n << cell_size;
    *generation = ++map_generation[kind];
    return 0;
}
void ll_reg_default_params(ll_reg_params *p) { std::memset(p, 0, sizeof(*p)); }
int ll_reg_create(int32_t device, int32_t max_scans, int32_t max_features_per_scan, ll_reg **o)
{
    Line("ll_reg_create") << device << max_scans << max_features_per_scan;
    return create("reg", o);
}
static std::string params(const ll_reg_params *p)
{
    return "prm{" + num(p->if_motion_deblur) + " " + num(p->icp_max_iterations) + " " + num(p->icp_line) + " " + num(p->current_frame_index) + " " +
           num(p->maximum_allow_residual_block) + " " + num(p->inliner_dis) + " " + num(p->max_final_cost) + " " + num(p->subsample_seed) + "}";
}
int ll_reg_upload_features(ll_reg *r, int32_t n_scans, const float *corner_xyzi, const int32_t *n_corner, int32_t stride_corner, const float *surf_xyzi,
                           const int32_t *n_surf, int32_t stride_surf)
{
    const char *fn = "ll_reg_upload_features";
    NEED(r);
    Line(fn) << hnd(r) << n_scans << arr("f32", corner_xyzi, 4 * (int64_t)n_corner[0]) << n_corner[0] << stride_corner
             << arr("f32", surf_xyzi, 4 * (int64_t)n_surf[0]) << n_surf[0] << stride_surf;
    return 0;
}
int ll_reg_enqueue_uploaded(ll_reg *r, const ll_map *map, int32_t n_scans, const ll_reg_params *prm, const double *poses_last, const double *poses_curr,
                            const double *poses_incre)
{
    const char *fn = "ll_reg_enqueue_uploaded";
    NEED(r);
    Line(fn) << hnd(r) << hnd(map) << n_scans << params(prm) << arr("f64", poses_last, 7) << arr("f64", poses_curr, 7) << arr("f64", poses_incre, 7);
    return 0;
}
int ll_reg_enqueue_spin(ll_reg *r, const ll_map *map, ll_spin *spin, int32_t n_scans, const ll_reg_params *prm, const double *poses_last,
                        const double *poses_curr, const double *poses_incre)
{
    const char *fn = "ll_reg_enqueue_spin";
    NEED(r);
    Line(fn) << hnd(r) << hnd(map) << hnd(spin) << n_scans << params(prm) << arr("f64", poses_last, 7) << arr("f64", poses_curr, 7)
             << arr("f64", poses_incre, 7);
    return 0;
}
int ll_reg_collect(ll_reg *r, int32_t n_scans, double *poses_curr, double *poses_incre, ll_reg_report *reports, int32_t *results)
{
    const char *fn = "ll_reg_collect";
    NEED(r);
    Line(fn) << hnd(r) << n_scans;
    for (int i = 0; i < 3; i++) poses_curr[4 + i] += 1.0 + i, poses_incre[4 + i] = 0.5 * (i + 1);
    std::memset(reports, 0, sizeof(*reports));
    reports->final_cost = 0.25, reports->initial_cost = 4.0, reports->inlier_threshold = 0.125, reports->angular_diff_deg = 0.5, reports->t_diff = 0.75;
    reports->icp_iterations = 3, reports->n_blocks_last = 11, reports->lm_iterations_total = 17, reports->accepted = 1;
    *results = 1;
    return 0;
}
int ll_cloud_transform(ll_reg *r, const float *in_xyzi, float *out_xyzi, int32_t n, const double pose[7])
{
    const char *fn = "ll_cloud_transform";
    NEED(r);
    Line(fn) << hnd(r) << arr("f32", in_xyzi, 4 * (int64_t)n) << n << arr("f64", pose, 7);
    for (int64_t i = 0; i < 4 * (int64_t)n; i++) out_xyzi[i] = in_xyzi[i] + 1.0f;
    return 0;
}

// ---- pose graph, scene alignment, key-frame bank
int ll_pose_graph_create(int32_t device, int64_t max_graphs, int64_t max_poses_total, int64_t max_edges_total, int64_t max_envelope_blocks,
                         ll_pose_graph **o)
{
    Line("ll_pose_graph_create") << device << (long long)max_graphs << (long long)max_poses_total << (long long)max_edges_total
                                 << (long long)max_envelope_blocks;
    return create("pose_graph", o);
}
void ll_pose_graph_destroy(ll_pose_graph *h) { destroy("ll_pose_graph_destroy", h); }
int ll_pose_graph_solve(ll_pose_graph *h, const ll_pose_graph_params *p, int64_t n_graphs, const int64_t *pose_offsets, double *poses7,
                        const int64_t *edge_offsets, const int32_t *edge_ab, const double *edge_meas7, const double *edge_information,
                        ll_pose_graph_summary *summary)
{
    const char *fn = "ll_pose_graph_solve";
    NEED(h);
    const int64_t n = pose_offsets[n_graphs], e = edge_offsets[n_graphs];
    Line(fn) << hnd(h) << out(p) << (long long)n_graphs << arr("i64", pose_offsets, n_graphs + 1) << arr("f64", poses7, 7 * n)
             << arr("i64", edge_offsets, n_graphs + 1) << arr("i32", edge_ab, 2 * e) << arr("f64", edge_meas7, 7 * e) << arr("f64", edge_information, 36 * e);
    if (size_of(fn) < 0) return fail(fn, "the stand-in was told to fail");
    for (int64_t k = 0; k < n; k++) poses7[7 * k + 4] += 1.0;
    summary->iterations = 5, summary->successful_steps = 4, summary->unsuccessful_steps = 1, summary->termination = LL_POSE_GRAPH_FUNCTION;
    summary->initial_cost = 8.0, summary->final_cost = 0.5;
    return 0;
}
void ll_scene_align_default_params(ll_scene_align_params *p)
{
    std::memset(p, 0, sizeof(*p));
    p->line_res = p->plane_res = 0.4f, p->maximum_icp_iteration = 10, p->accepted_threshold = 0.2f, p->maximum_residual_block = 5000;
    p->registrar_init = p->subsample_seed = 1;
}
int ll_scene_align_create(int32_t device, int64_t initial_points, ll_scene_align **o)
{
    Line("ll_scene_align_create") << device << (long long)initial_points;
    return create("scene_align", o);
}
void ll_scene_align_destroy(ll_scene_align *h) { destroy("ll_scene_align_destroy", h); }
int ll_scene_align_run(ll_scene_align *h, ll_cellmap *keyframe_a, ll_cellmap *keyframe_b, const ll_scene_align_params *p, double pose[7],
                       double *inlier_threshold, ll_reg_report reports[3], int32_t *n_reports)
{
    const char *fn = "ll_scene_align_run";
    NEED(h);
    Line(fn) << hnd(h) << hnd(keyframe_a) << hnd(keyframe_b) << p->line_res << p->plane_res << p->maximum_icp_iteration << p->accepted_threshold
             << p->maximum_residual_block << p->registrar_init << p->subsample_seed;
    const double answer[7] = {0.5, -0.5, 0.5, 0.5, 1, 2, 3};
    std::memcpy(pose, answer, sizeof(answer));
    *inlier_threshold = 0.125;
    *n_reports = 2;
    std::memset(reports, 0, 3 * sizeof(*reports));
    reports[0].n_blocks_last = 7, reports[0].final_cost = 2.0;
    reports[1].n_blocks_last = 9, reports[1].final_cost = 1.0;
    return 0;
}
int ll_scene_align_work(ll_scene_align *h, int64_t *)
{
    const char *fn = "ll_scene_align_work";
    NEED(h);
    return 0;
}
int ll_keyframe_bank_create(int32_t device, int64_t initial_entries, ll_keyframe_bank **o)
{
    Line("ll_keyframe_bank_create") << device << (long long)initial_entries;
    return create("keyframe_bank", o);
}
void ll_keyframe_bank_destroy(ll_keyframe_bank *b) { destroy("ll_keyframe_bank_destroy", b); }
int ll_keyframe_bank_work(ll_keyframe_bank *b, int64_t *)
{
    const char *fn = "ll_keyframe_bank_work";
    NEED(b);
    Line(fn) << hnd(b);
    return 0;
}

// ---- map refinement
int ll_map_refine_create(int32_t device, int64_t initial_points, ll_map_refine **o)
{
    Line("ll_map_refine_create") << device << (long long)initial_points;
    return create("map_refine", o);
}
void ll_map_refine_destroy(ll_map_refine *h) { destroy("ll_map_refine_destroy", h); }
int ll_map_refine_work(ll_map_refine *h, int64_t *)
{
    const char *fn = "ll_map_refine_work";
    NEED(h);
    return 0;
}
int ll_map_refine_add_logged(ll_map_refine *h, ll_history_batch *hb, int64_t n_req, const int64_t *group_off, const int64_t *group_ids, float leaf,
                             int64_t *ids, int64_t *n_kept, int32_t *status)
{
    const char *fn = "ll_map_refine_add_logged";
    NEED(h);
    Line(fn) << hnd(h) << hnd(hb) << (long long)n_req << arr("i64", group_off, n_req + 1) << arr("i64", group_ids, group_off[n_req]) << leaf;
    for (int64_t r = 0; r < n_req; r++) ids[r] = 100 + r, n_kept[r] = r + 1, status[r] = 0;
    return 0;
}
int ll_map_refine_add_stored(ll_map_refine *h, const float *xyzi, int64_t n, int64_t *id)
{
    const char *fn = "ll_map_refine_add_stored";
    NEED(h);
    Line(fn) << hnd(h) << arr("f32", xyzi, 4 * n) << (long long)n;
    *id = next_stored_id++;
    return 0;
}
int ll_map_refine_run(ll_map_refine *h, int32_t mode, int64_t n_sel, const int64_t *ids, const double *poses_ori7, const double *poses_opm7, float leaf,
                      int64_t *offsets_out, int32_t *status_out)
{
    const char *fn = "ll_map_refine_run";
    NEED(h);
    Line(fn) << hnd(h) << mode << (long long)n_sel << arr("i64", ids, n_sel) << arr("f64", poses_ori7, 7 * n_sel) << arr("f64", poses_opm7, 7 * n_sel) << leaf;
    for (int64_t k = 0; k <= n_sel; k++) offsets_out[k] = k * size_of(fn), status_out[k] = 0;  // every output of the same size
    last_run_points = offsets_out[n_sel];
    return 0;
}
int ll_map_refine_fetch(ll_map_refine *h, float *xyzi_out, int64_t capacity_points)
{
    const char *fn = "ll_map_refine_fetch";
    NEED(h);
    Line(fn) << hnd(h) << out(xyzi_out) << (long long)capacity_points;
    if (capacity_points < last_run_points) return fail(fn, "capacity below the outputs' size");
    fill(xyzi_out, last_run_points, 4.0f);
    return 0;
}
int ll_map_refine_merge(ll_map_refine *h, float leaf, int64_t *n_out, int32_t *status)
{
    const char *fn = "ll_map_refine_merge";
    NEED(h);
    Line(fn) << hnd(h) << leaf << out(status);
    *n_out = size_of(fn);
    return 0;
}
int ll_map_refine_fetch_merged(ll_map_refine *h, float *xyzi_out, int64_t capacity_points)
{
    const char *fn = "ll_map_refine_fetch_merged";
    NEED(h);
    Line(fn) << hnd(h) << out(xyzi_out) << (long long)capacity_points;
    if (capacity_points < size_of("ll_map_refine_merge")) return fail(fn, "capacity below the merged cloud's size");
    fill(xyzi_out, size_of("ll_map_refine_merge"), 5.0f);
    return 0;
}
}  // extern "C"
