// loam_livox_adapter.hpp -- header-only C++ adapter that gives the reference's node shells the call surface they
// already use (hku-mars/loam_livox), backed by the C ABI of libloamlivox_hip.so:
//
//   loam_livox_hip::Livox_laser               <->  class Livox_laser               source/livox_feature_extractor.hpp:77
//   loam_livox_hip::Point_cloud_registration  <->  class Point_cloud_registration  source/point_cloud_registration.hpp:38
//
// The adapter is templated on the cloud type so that it compiles with or without PCL: any type with a
// `points` std::vector whose elements have float members x, y, z, intensity works (pcl::PointCloud<pcl::PointXYZI>
// does).  Poses are the reference's own members (m_q_w_curr, m_t_w_curr, m_q_w_last, m_t_w_last, m_q_w_incre, m_t_w_incre;
// Eigen objects when Eigen is on the include path) next to the raw buffers in the reference's storage order
// {qx,qy,qz,qw,tx,ty,tz} (m_para_buffer_RT, point_cloud_registration.hpp:51-56).
//
// See INTEGRATION.md for the two-line change in laser_feature_extractor.hpp / laser_mapping.hpp.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "loam_livox_hip.h"

// The two entry points behind Point_cloud_registration::m_if_compute_information are referenced weakly: the header's registration path
// names them, and a program that never sets the member must keep linking against whatever it linked against before (an older build of
// the library, a test stand-in of the C ABI).  Setting the member without them throws.
extern "C" {
int ll_reg_set_information(ll_reg *r, int32_t enable) __attribute__((weak));
int ll_reg_information(ll_reg *r, int32_t n_scans, ll_reg_information_record *out) __attribute__((weak));
// ... and the deskewed clouds (if_undistore = 1): used only by callers that ask for them
int ll_reg_interpolation(ll_reg *r, int32_t n_scans, double *theta, double *omega_hat9, double *pose_last7, double *pose_incre7) __attribute__((weak));
int ll_cloud_undistort(ll_reg *r, int32_t slot, const float *in_xyzi, float *out_xyzi, int32_t n) __attribute__((weak));
int ll_history_set_undistort(ll_history *h, ll_reg *r, int32_t slot) __attribute__((weak));
// ... and motion deblur with a map per slot
int ll_reg_set_time_ranges(ll_reg *r, const float *minimum_pt_time_stamp, const float *maximum_pt_time_stamp, int32_t n_scans) __attribute__((weak));
int ll_history_batch_set_undistort(ll_history_batch *h, ll_reg *r) __attribute__((weak));
}

// The registrar's pose members (m_q_w_curr, m_t_w_curr, m_q_w_last, m_t_w_last, m_q_w_incre, m_t_w_incre,
// point_cloud_registration.hpp:53-56,75-76) are Eigen objects in the reference and the node assigns Eigen objects to them
// (laser_mapping.hpp:1290-1294, 1498-1499).  With Eigen on the include path they ARE Eigen objects here; without it
// (no-dependency builds, the C++ smoke test) they are the small look-alikes below.
#if defined(__has_include)
#if __has_include(<Eigen/Geometry>) && !defined(LOAM_LIVOX_ADAPTER_NO_EIGEN)
#include <Eigen/Core>
#include <Eigen/Geometry>
#define LOAM_LIVOX_ADAPTER_EIGEN 1
#endif
#endif

namespace loam_livox_hip {

#if defined(LOAM_LIVOX_ADAPTER_EIGEN)
typedef Eigen::Quaterniond Quaterniond;
typedef Eigen::Vector3d Vector3d;
typedef Eigen::Map<Eigen::Quaterniond> Quaterniond_map;
typedef Eigen::Map<Eigen::Vector3d> Vector3d_map;
#else
struct Quaterniond {  // storage x, y, z, w like Eigen
    double c[4] = {0, 0, 0, 1};
    double &x() { return c[0]; }
    double &y() { return c[1]; }
    double &z() { return c[2]; }
    double &w() { return c[3]; }
    double x() const { return c[0]; }
    double y() const { return c[1]; }
    double z() const { return c[2]; }
    double w() const { return c[3]; }
    void setIdentity() { c[0] = c[1] = c[2] = 0, c[3] = 1; }
};
struct Vector3d {
    double c[3] = {0, 0, 0};
    double &operator()(int i) { return c[i]; }
    double operator()(int i) const { return c[i]; }
    double &x() { return c[0]; }
    double &y() { return c[1]; }
    double &z() { return c[2]; }
    double x() const { return c[0]; }
    double y() const { return c[1]; }
    double z() const { return c[2]; }
    void setZero() { c[0] = c[1] = c[2] = 0; }
};
struct Quaterniond_map {
    double *p;
    explicit Quaterniond_map(double *q) : p(q) {}
    double &x() { return p[0]; }
    double &y() { return p[1]; }
    double &z() { return p[2]; }
    double &w() { return p[3]; }
    double x() const { return p[0]; }
    double y() const { return p[1]; }
    double z() const { return p[2]; }
    double w() const { return p[3]; }
    Quaterniond_map &operator=(const Quaterniond &q)
    {
        for (int i = 0; i < 4; i++) p[i] = q.c[i];
        return *this;
    }
    operator Quaterniond() const
    {
        Quaterniond q;
        for (int i = 0; i < 4; i++) q.c[i] = p[i];
        return q;
    }
};
struct Vector3d_map {
    double *p;
    explicit Vector3d_map(double *q) : p(q) {}
    double &operator()(int i) { return p[i]; }
    double operator()(int i) const { return p[i]; }
    Vector3d_map &operator=(const Vector3d &v)
    {
        for (int i = 0; i < 3; i++) p[i] = v.c[i];
        return *this;
    }
    operator Vector3d() const
    {
        Vector3d v;
        for (int i = 0; i < 3; i++) v.c[i] = p[i];
        return v;
    }
};
#endif

// Pointer members the node sets but the device path has no use for (m_logger_common, m_logger_pcd, m_logger_timer,
// m_timer: point_cloud_registration.hpp:78-82, set at laser_mapping.hpp:1271-1274, scene_alignment.hpp:234-236): any
// pointer can be assigned, it is kept as-is.
struct Any_ptr {
    const void *p = nullptr;
    template <class T>
    Any_ptr &operator=(T *q)
    {
        p = (const void *)q;
        return *this;
    }
};
// m_kdtree_corner_from_map / m_kdtree_surf_from_map (point_cloud_registration.hpp:72-73): the device grid replaces the
// k-d trees, assignments are accepted and dropped.
struct Any_sink {
    template <class T>
    Any_sink &operator=(const T &)
    {
        return *this;
    }
};

inline void check(int rc, const char *what)
{
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + ll_last_error());
}

// Runtime hints of the process, applied once before the adapter's first *_create (= before its first HIP call): 16 hardware queues
// instead of the runtime's default of 4, so that registrations in flight on different handles do not share a queue
// (ll_runtime_hint_hw_queues in loam_livox_hip.h).  The caller's environment always wins; a host that
// initialises HIP before constructing any adapter object must export GPU_MAX_HW_QUEUES itself.  -DLOAM_LIVOX_HIP_NO_RUNTIME_HINTS
// leaves the process environment alone.
inline void runtime_hints()
{
#ifndef LOAM_LIVOX_HIP_NO_RUNTIME_HINTS
    static std::once_flag once;
    std::call_once(once, [] { (void)ll_runtime_hint_hw_queues(16); });
#endif
}

template <class Cloud>
inline std::vector<float> cloud_to_xyzi(const Cloud &c)
{
    std::vector<float> v(c.points.size() * 4);
    for (size_t i = 0; i < c.points.size(); i++) {
        v[4 * i + 0] = c.points[i].x;
        v[4 * i + 1] = c.points[i].y;
        v[4 * i + 2] = c.points[i].z;
        v[4 * i + 3] = c.points[i].intensity;
    }
    return v;
}

template <class Cloud>
inline void xyzi_to_cloud(const float *v, int n, Cloud &c)
{
    c.points.resize(n);
    for (int i = 0; i < n; i++) {
        c.points[i].x = v[4 * i + 0];
        c.points[i].y = v[4 * i + 1];
        c.points[i].z = v[4 * i + 2];
        c.points[i].intensity = v[4 * i + 3];
    }
}

// ------------------------------------------------------------------------------------------------------------
// What the classes below share.
//
// Ownership: a class that owns an ll_* handle holds it in a Handle, which destroys it exactly once.  A Handle moves and does not
// copy, and so does its class; a moved-from object holds null, and the library refuses its calls ("null handle", thrown by check).
template <class T, void (*Destroy)(T *)>
struct Destroyer {
    void operator()(T *h) const { Destroy(h); }
};
template <class T, void (*Destroy)(T *)>
using Handle = std::unique_ptr<T, Destroyer<T, Destroy>>;

// The one way a handle is made, in a constructor, on first use, or larger than the one before (which is destroyed first):
// create( &raw ) wraps the ll_*_create call.  The process' runtime hints come first, so no call site applies them.
template <class H, class Create>
inline void make_handle(H &h, const char *what, Create create)
{
    h.reset();
    runtime_hints();
    typename H::pointer raw = nullptr;
    check(create(&raw), what);
    h.reset(raw);
}

// The one way a cloud is read back, size then fill: call( buffer, capacity in points ) wraps the C call and answers the number of
// points; it is asked with ( nullptr, 0 ) first and, unless the cloud is empty, with a buffer of that size.  A negative answer throws
// through check with the entry point's name.
template <class Call>
inline std::vector<float> read_xyzi(const char *what, Call call)
{
    const int64_t n = call((float *)nullptr, (int64_t)0);
    if (n < 0) check(-1, what);
    std::vector<float> v((size_t)n * 4);
    if (n > 0 && call(v.data(), n) < 0) check(-1, what);
    return v;
}
template <class Cloud, class Call>
inline void read_cloud(const char *what, Cloud &out, Call call)
{
    const std::vector<float> v = read_xyzi(what, call);
    xyzi_to_cloud(v.data(), (int)(v.size() / 4), out);
}

// A pose in the C ABI's order {qx,qy,qz,qw,tx,ty,tz}, from and to a quaternion read as q.x() and a vector read as t( i ): the
// look-alikes above, their _map views and Eigen's types.
template <class Q, class V>
inline void to_pose7(const Q &q, const V &t, double out[7])
{
    out[0] = q.x(), out[1] = q.y(), out[2] = q.z(), out[3] = q.w();
    for (int i = 0; i < 3; i++) out[4 + i] = t(i);
}
template <class Q, class V>
inline void from_pose7(const double in[7], Q &q, V &t)
{
    q.x() = in[0], q.y() = in[1], q.z() = in[2], q.w() = in[3];
    for (int i = 0; i < 3; i++) t(i) = in[4 + i];
}

// cell indices as the int32 {i, j, k} triples of the C ABI, appended to ijk
inline void pack_cells(const std::vector<std::array<int, 3>> &cells, std::vector<int32_t> &ijk)
{
    for (const std::array<int, 3> &c : cells)
        for (size_t d = 0; d < 3; d++) ijk.push_back((int32_t)c[d]);
}
// lists laid end to end: list r is [ off[r], off[r + 1] )
template <class T>
inline std::vector<int64_t> csr_offsets(const std::vector<std::vector<T>> &lists)
{
    std::vector<int64_t> off(lists.size() + 1, 0);
    for (size_t r = 0; r < lists.size(); r++) off[r + 1] = off[r] + (int64_t)lists[r].size();
    return off;
}
// the points of a cloud argument; the C ABI wants a readable pointer for an empty one too
inline const float *xyzi_or_dummy(const std::vector<float> &v)
{
    static const float dummy[4] = {0, 0, 0, 0};
    return v.empty() ? dummy : v.data();
}

// ------------------------------------------------------------------------------------------------------------
class Livox_laser {
   public:
    // public tunables of the reference class (livox_feature_extractor.hpp:143-167); set them before the first
    // extract_laser_features() call, exactly where laser_feature_extractor.hpp:152-154,854,859 sets them
    float max_fov = 17;
    float m_time_internal_pts = 1.0e-5f;
    float thr_corner_curvature = 0.05f;
    float thr_surface_curvature = 0.01f;
    float minimum_view_angle = 10;
    float m_livox_min_allow_dis = 1.0f;
    float m_livox_min_sigma = 7e-3f;
    int m_input_points_size = 0;
    int piecewise_number = 3;  // common/piecewise_number (laser_feature_extractor.hpp:142)
    int device = 0;
    int max_points = 100000;

    struct Pt_infos {  // the fields callers read (livox_feature_extractor.hpp:118-133)
        int pt_type, pt_label, idx;
        float time_stamp, depth_sq2, curvature, view_angle;
    };
    std::vector<Pt_infos> m_pts_info_vec;

    // std::vector<pcl::PointCloud<PointXYZI>> extract_laser_features(cloud, time_stamp), LFE:722: the petal clouds of
    // split_laser_scan (LFE:657-719) -- a new cloud whenever the petal angle changes, the last petal dropped (:681), points
    // masked 000 / too-near / nan removed, intensity = idx / N (set_intensity(e_I_motion_blur), :283-286), empty petals
    // removed -- rebuilt on the host from the device's per-point planes.
    template <class Cloud>
    std::vector<Cloud> extract_laser_features(Cloud &laserCloudIn, double time_stamp = -1)
    {
        ensure_handle();
        raw_ = cloud_to_xyzi(laserCloudIn);
        const int n = (int)laserCloudIn.points.size();
        m_input_points_size = n;
        first_of_.clear();
        int32_t n_clouds = 0;
        check(ll_fe_extract(h_.get(), raw_.data(), n, time_stamp, &n_clouds), "ll_fe_extract");
        std::vector<int32_t> type(n), label(n);
        std::vector<float> depth(n), curv(n), view(n), ts(n), pang(n);
        check(ll_fe_labels(h_.get(), 0, type.data(), label.data(), depth.data(), nullptr, curv.data(), view.data(), ts.data(), pang.data()),
              "ll_fe_labels");
        m_pts_info_vec.resize(n);
        for (int i = 0; i < n; i++) m_pts_info_vec[i] = Pt_infos{type[i], label[i], i, ts[i], depth[i], curv[i], view[i]};
        int32_t ns = 0, cl = 0, npc = 0;
        check(ll_fe_splits(h_.get(), 0, nullptr, &ns, &cl, &npc, nullptr, nullptr, nullptr, nullptr), "ll_fe_splits");
        std::vector<Cloud> out;
        if (cl == 0) return out;  // fewer than 6 split entries (LFE:572, 759-762)
        int scan_idx = 0;
        std::vector<Cloud> petals((size_t)cl);
        for (int i = 0; i < n; i++) {
            if (i > 0 && pang[i] != pang[i - 1]) scan_idx++;
            if (scan_idx >= cl) break;  // cannot happen: clutter_size counts the angle changes + 1
            if (type[i] & (1 | 2 | 32)) continue;  // e_pt_000 | e_pt_too_near | e_pt_nan, LFE:684-688
            auto pt = laserCloudIn.points[i];
            // set_intensity(e_I_motion_blur) reads find_pt_info(pt)->idx (LFE:278-286, 706): the index of the FIRST inserted point
            // with these coordinates (the unordered_map keeps the first of equal keys, LFE:478)
            pt.intensity = (float)find_pt_info(pt)->idx / (float)n;
            petals[scan_idx].points.push_back(pt);
        }
        for (int s = 0; s < scan_idx && s < cl; s++)  // resize(scan_idx): the last petal is dropped, LFE:681
            if (!petals[s].points.empty()) out.push_back(petals[s]);
        if ((int)out.size() != npc) throw std::runtime_error("extract_laser_features: petal count differs from the device's");
        return out;
    }

    // Pt_infos *find_pt_info(const T &pt), LFE:206-217: the first inserted point with the same xyz (the unordered_map keeps
    // the first of equal keys, LFE:478).  A hash index over the scan is built at the first look-up after an extraction.
    template <class P>
    Pt_infos *find_pt_info(const P &pt)
    {
        if (first_of_.empty() && !m_pts_info_vec.empty()) {
            size_t cap = 16;
            while (cap < 2 * m_pts_info_vec.size()) cap <<= 1;
            first_of_.assign(cap, -1);
            for (size_t i = 0; i < m_pts_info_vec.size(); i++) {
                size_t h = hash_xyz(raw_[4 * i], raw_[4 * i + 1], raw_[4 * i + 2]) & (cap - 1);
                for (;; h = (h + 1) & (cap - 1)) {
                    const int j = first_of_[h];
                    if (j < 0) {
                        first_of_[h] = (int)i;
                        break;
                    }
                    if (raw_[4 * j] == raw_[4 * i] && raw_[4 * j + 1] == raw_[4 * i + 1] && raw_[4 * j + 2] == raw_[4 * i + 2]) break;
                }
            }
        }
        if (!first_of_.empty()) {
            const size_t cap = first_of_.size();
            for (size_t h = hash_xyz(pt.x, pt.y, pt.z) & (cap - 1);; h = (h + 1) & (cap - 1)) {
                const int j = first_of_[h];
                if (j < 0) break;
                if (raw_[4 * j] == pt.x && raw_[4 * j + 1] == pt.y && raw_[4 * j + 2] == pt.z) return &m_pts_info_vec[j];
            }
        }
        throw std::runtime_error("find_pt_info: point not in the current scan (assert at livox_feature_extractor.hpp:214)");
    }

    // void get_features(pc_corners, pc_surface, pc_full_res, minimum_blur, maximum_blur), LFE:219
    template <class Cloud>
    void get_features(Cloud &pc_corners, Cloud &pc_surface, Cloud &pc_full_res, float minimum_blur = 0.0f, float maximum_blur = 0.3f)
    {
        const int n = m_input_points_size;
        std::vector<int32_t> ci(n), si(n), fi(n);
        std::vector<float> cc((size_t)n * 4), sc((size_t)n * 4);
        int32_t nc = 0, ns = 0, nf = 0;
        check(ll_fe_select(h_.get(), minimum_blur, maximum_blur, ci.data(), &nc, si.data(), &ns, fi.data(), &nf, cc.data(), sc.data()),
              "ll_fe_select");
        xyzi_to_cloud(cc.data(), nc, pc_corners);
        xyzi_to_cloud(sc.data(), ns, pc_surface);
        pc_full_res.points.resize(nf);
        for (int k = 0; k < nf; k++) {  // pc_full keeps every in-window point, intensity := time stamp (LFE:263-265)
            const int i = fi[k];
            pc_full_res.points[k].x = raw_[4 * i];
            pc_full_res.points[k].y = raw_[4 * i + 1];
            pc_full_res.points[k].z = raw_[4 * i + 2];
            pc_full_res.points[k].intensity = m_pts_info_vec[i].time_stamp;
        }
    }

   private:
    void ensure_handle()
    {
        if (h_) return;
        ll_fe_params p;
        ll_fe_default_params(&p);
        p.thr_corner_curvature = thr_corner_curvature;
        p.thr_surface_curvature = thr_surface_curvature;
        p.minimum_view_angle = minimum_view_angle;
        p.livox_min_allow_dis = m_livox_min_allow_dis;
        p.livox_min_sigma = m_livox_min_sigma;
        p.max_fov = max_fov;
        p.time_internal_pts = m_time_internal_pts;
        p.device = device;
        p.max_points = max_points;
        p.max_scans = 1;
        p.piecewise_number = piecewise_number;
        make_handle(h_, "ll_fe_create", [&](ll_fe **out) { return ll_fe_create(&p, out); });
    }
    static size_t hash_xyz(float x, float y, float z)
    {
        uint32_t a, b, c;
        x = x + 0.0f;  // -0.0f == 0.0f must hash alike (the reference compares with ==, pcl_tools.hpp:32-36)
        y = y + 0.0f;
        z = z + 0.0f;
        std::memcpy(&a, &x, 4);
        std::memcpy(&b, &y, 4);
        std::memcpy(&c, &z, 4);
        uint64_t h = (uint64_t)a * 0x9E3779B97F4A7C15ull ^ ((uint64_t)b << 21) * 0xC2B2AE3D27D4EB4Full ^ (uint64_t)c * 0x165667B19E3779F9ull;
        return (size_t)(h ^ (h >> 29));
    }
    Handle<ll_fe, ll_fe_destroy> h_;
    std::vector<float> raw_;
    std::vector<int> first_of_;
};

// ------------------------------------------------------------------------------------------------------------
// The spinning-lidar branch of Laser_feature::laserCloudHandler (lidar_type != "livox", laser_feature_extractor.hpp:393-787):
// the reference has no class for it; extract() replaces the body between the start-up gate and the publishes and fills the five
// clouds the node publishes (/laser_points_2, /laser_cloud_sharp, /laser_cloud_less_sharp, /laser_cloud_flat,
// /laser_cloud_less_flat).  Cloud is pcl::PointCloud<pcl::PointXYZI> or anything with
// points[i].x / y / z / intensity.  Set the parameters before the first call (ROS feature_extraction/*, :137-140).
class Spinning_laser {
   public:
    int scan_line = 16;             // feature_extraction/scan_line; 16 or 64 (:160-164)
    float minimum_range = 0.1f;     // feature_extraction/minimum_range
    float plane_resolution = 0.8f;  // feature_extraction/mapping_plane_resolution
    int device = 0;
    int max_points = 0;             // 0: sized for the first scan seen (grown on demand)
    int max_line_points = 8192;

    template <class Cloud>
    void extract(const Cloud &in, Cloud &full, Cloud &sharp, Cloud &less_sharp, Cloud &flat, Cloud &less_flat)
    {
        const int st = extract_device(in);
        if (st != LL_SPIN_STATUS_OK) throw std::runtime_error("ll_spin_extract: a line holds more less-flat points than max_line_points");
        Cloud *outs[5] = {&full, &sharp, &less_sharp, &flat, &less_flat};
        for (int which = 0; which < 5; which++) {
            int32_t m = 0;
            check(ll_spin_cloud(h_.get(), 0, which, buf_.data(), nullptr, &m), "ll_spin_cloud");
            xyzi_to_cloud(buf_.data(), m, *outs[which]);
        }
    }

    // The same extraction with nothing downloaded: the clouds stay on the device for
    // Point_cloud_registration::find_out_incremental_transfrom( spin ) and History_buffer::add( spin, pose ) (corner stack =
    // /laser_cloud_less_sharp, surface stack = /laser_cloud_less_flat).  Returns the scan's status
    // (LL_SPIN_STATUS_OK or LL_SPIN_STATUS_LINE_OVERFLOW: the hand-off takes the clouds a download would return either way).
    template <class Cloud>
    int extract_device(const Cloud &in)
    {
        const std::vector<float> raw = cloud_to_xyzi(in);
        const int n = (int)in.points.size();
        ensure_handle(n);
        const int st = ll_spin_extract(h_.get(), xyzi_or_dummy(raw), n);
        check(st, "ll_spin_extract");
        return st;
    }
    ll_spin *handle() { return h_.get(); }  // null before the first extraction
    int capacity() const { return cap_; }

   private:
    void ensure_handle(int n)
    {
        if (h_ && n <= cap_) return;
        ll_spin_params p;
        ll_spin_default_params(&p);
        p.scan_line = scan_line;
        p.minimum_range = minimum_range;
        p.plane_resolution = plane_resolution;
        p.device = device;
        cap_ = max_points > 0 ? max_points : (n > p.max_points ? n : p.max_points);
        p.max_points = cap_;
        p.max_scans = 1;
        p.max_line_points = max_line_points;
        make_handle(h_, "ll_spin_create", [&](ll_spin **out) { return ll_spin_create(&p, out); });
        buf_.assign((size_t)cap_ * 4, 0.f);
    }
    Handle<ll_spin, ll_spin_destroy> h_;
    int cap_ = 0;
    std::vector<float> buf_;
};

// ------------------------------------------------------------------------------------------------------------
// pcl::VoxelGrid<PointType> as the node shells use it: setLeafSize / setInputCloud / filter
// (laser_feature_extractor.hpp:192-193,372-381; laser_mapping.hpp:742-743,1367-1373,1434-1437,533-537).
// CloudPtr is anything that dereferences to a cloud (std::shared_ptr, boost::shared_ptr, raw pointer).
template <class Cloud>
class VoxelGrid {
   public:
    int device = 0;
    int max_points = 0;  // 0: sized for the first cloud seen (grown on demand)
    int status = 0;      // of the last filter(): 0 filtered, 1 leaf too small (copy of the input, like PCL), 2 no finite point

    VoxelGrid() {}
    // The node copies its filters by value into every call (laser_mapping.hpp:465-466, 1325-1326): a copy takes the configuration
    // and creates its own device handle on first use.
    VoxelGrid(const VoxelGrid &o) : device(o.device), max_points(o.max_points), status(0)
    {
        leaf_[0] = o.leaf_[0];
        leaf_[1] = o.leaf_[1];
        leaf_[2] = o.leaf_[2];
    }
    VoxelGrid &operator=(const VoxelGrid &o)
    {
        if (this != &o) {
            device = o.device;
            max_points = o.max_points;
            leaf_[0] = o.leaf_[0];
            leaf_[1] = o.leaf_[1];
            leaf_[2] = o.leaf_[2];
            in_.clear();
        }
        return *this;
    }
    void setLeafSize(float lx, float ly, float lz)
    {
        leaf_[0] = lx;
        leaf_[1] = ly;
        leaf_[2] = lz;
    }
    template <class CloudPtr>
    void setInputCloud(const CloudPtr &cloud)
    {
        in_ = cloud_to_xyzi(*cloud);
    }
    void filter(Cloud &output)  // `output` may be the input cloud itself (the reference filters in place)
    {
        const int32_t n = (int32_t)(in_.size() / 4);
        if (n == 0) {
            output.points.clear();
            status = 2;
            return;
        }
        if (!h_ || n > cap_) {
            cap_ = n > max_points ? n : max_points;
            make_handle(h_, "ll_voxel_create", [&](ll_voxel **out) { return ll_voxel_create(device, 1, cap_, out); });
        }
        std::vector<float> out(in_.size());
        int32_t n_out = 0, st = 0;
        check(ll_voxel_filter(h_.get(), 1, in_.data(), &n, n, leaf_, out.data(), &n_out, &st), "ll_voxel_filter");
        status = st;
        xyzi_to_cloud(out.data(), n_out, output);
    }

   private:
    Handle<ll_voxel, ll_voxel_destroy> h_;
    int cap_ = 0;
    float leaf_[3] = {0.4f, 0.4f, 0.4f};
    std::vector<float> in_;
};

// ------------------------------------------------------------------------------------------------------------
// The history match buffer of Laser_mapping (m_matching_mode == 0): m_laser_cloud_corner_history /
// m_laser_cloud_surface_history with the add-frame rule and FIFO of laser_mapping.hpp:1417-1478, and
// update_buff_for_matching's history branch (laser_mapping.hpp:517-546), resident on the device.  refresh() rebuilds the
// search grids of the ll_map the registrar uses, so the two KdTreeFLANN::setInputCloud calls (:544-545) disappear.
class History_buffer {
   public:
    History_buffer(int maximum_history_size, int max_points_per_frame, float line_res, float plane_res, int device = 0)
    {
        make_handle(h_, "ll_history_create", [&](ll_history **out) {
            return ll_history_create(device, maximum_history_size, max_points_per_frame, line_res, plane_res, out);
        });
    }

    // "Add new frame" (laser_mapping.hpp:1417-1478): features in the sensor frame, pose = {qx,qy,qz,qw,tx,ty,tz} of the
    // accepted registration.  Returns true when the frame was pushed (false: "Reject add history").
    template <class Cloud>
    bool add(const Cloud &corner_stack, const Cloud &surf_stack, const double pose[7], double history_add_t_step = 0.0,
             double history_add_angle_step = 0.0)
    {
        const std::vector<float> c = cloud_to_xyzi(corner_stack), s = cloud_to_xyzi(surf_stack);
        int32_t added = 0;
        check(ll_history_add(h_.get(), c.data(), (int32_t)(c.size() / 4), s.data(), (int32_t)(s.size() / 4), pose, history_add_t_step,
                             history_add_angle_step, &added),
              "ll_history_add");
        return added != 0;
    }
    // the same for the scan a Spinning_laser holds (extract_device), device to device: its less-sharp and less-flat clouds
    bool add(Spinning_laser &spin, const double pose[7], double history_add_t_step = 0.0, double history_add_angle_step = 0.0)
    {
        if (!spin.handle()) throw std::runtime_error("History_buffer::add: the Spinning_laser has not extracted a scan");
        int32_t added = 0;
        check(ll_history_add_spin(h_.get(), spin.handle(), 0, pose, history_add_t_step, history_add_angle_step, &added), "ll_history_add_spin");
        return added != 0;
    }
    // The add-frame rule (laser_mapping.hpp:1439-1451) reads the node's m_q_w_curr / m_t_w_curr, which is still the pose
    // BEFORE the registration whose result add() receives: hand it over first (applies to the next add only).
    void set_gate_pose(const double pose_before_registration[7]) { check(ll_history_set_gate_pose(h_.get(), pose_before_registration), "ll_history_set_gate_pose"); }
    // g_if_undistore = 1 for the next add() of clouds (laser_mapping.hpp:1424,1430): it moves them with the pose interpolated at every
    // point's time stamp, from the registration `reg` (Point_cloud_registration::handle()) collected last; `pose` keeps gating.
    void set_undistort(ll_reg *reg, int slot = 0)
    {
        if (!&ll_history_set_undistort) throw std::runtime_error("set_undistort: this program is linked against a library without ll_history_set_undistort");
        check(ll_history_set_undistort(h_.get(), reg, slot), "ll_history_set_undistort");
    }
    // update_buff_for_matching(): concatenation of the history -> VoxelGrid -> search grids of `map`
    void refresh(ll_map *map, int64_t *n_corner = nullptr, int64_t *n_surf = nullptr)
    {
        check(ll_history_refresh(h_.get(), map, n_corner, n_surf), "ll_history_refresh");
    }
    // m_laser_cloud_corner_from_map_last / m_laser_cloud_surf_from_map_last of the last refresh (for publishing / saving)
    template <class Cloud>
    void map_cloud(int kind, Cloud &out)
    {
        read_cloud("ll_history_map_cloud", out, [&](float *xyzi, int64_t capacity) { return ll_history_map_cloud(h_.get(), kind, xyzi, capacity); });
    }
    int size() const { return ll_history_size(h_.get()); }

    // m_pt_cell_map_corners / m_pt_cell_map_planes (laser_mapping.hpp:274-275, 617-624) for m_matching_mode == 1: once
    // enabled, every add() also appends the frame to the two cell maps (laser_mapping.hpp:1492-1493)
    void enable_cell_map(int64_t max_points, float m_pt_cell_resolution = 1.0f, int m_para_threshold_cell_revisit = 5000)
    {
        check(ll_history_enable_cell_map(h_.get(), max_points, m_pt_cell_resolution, m_para_threshold_cell_revisit), "ll_history_enable_cell_map");
    }
    // m_matching_mode == 0 never reads the cell maps between frames (laser_mapping.hpp:1492-1493 only appends): feed them beside the mapping
    // loop, on a service thread of the handle, as the reference runs its own map services on threads (:568-594).  Every reader
    // (refresh_cells, cell_map_size, cell_map) waits for the frames handed over so far; sync_cell_maps() does only that.
    void set_cell_map_async(bool enable = true) { check(ll_history_set_cell_map_async(h_.get(), enable ? 1 : 0), "ll_history_set_cell_map_async"); }
    void sync_cell_maps() { check(ll_history_sync_cell_maps(h_.get()), "ll_history_sync_cell_maps"); }
    // the cell map of one feature kind (borrowed: valid as long as this object), e.g. for ll_cellmap_device_view -- the input of a multi-GPU
    // gather of cell maps
    ll_cellmap *cell_map(int kind)
    {
        ll_cellmap *c = ll_history_cell_map(h_.get(), kind);
        if (!c) check(-1, "ll_history_cell_map");
        return c;
    }
    // update_buff_for_matching(), cell branch (laser_mapping.hpp:471-546): pose = m_q_w_curr / m_t_w_curr
    void refresh_cells(ll_map *map, const double pose[7], float m_maximum_search_range_corner = 100.0f,
                       float m_maximum_search_range_surface = 100.0f, float m_maximum_in_fov_angle = 30.0f, int m_down_sample_replace = 1,
                       int64_t *n_corner = nullptr, int64_t *n_surf = nullptr)
    {
        check(ll_history_refresh_cells(h_.get(), map, pose, m_maximum_search_range_corner, m_maximum_search_range_surface, m_maximum_in_fov_angle,
                                       m_down_sample_replace, n_corner, n_surf),
              "ll_history_refresh_cells");
    }
    // Points_cloud_map::get_cells_size() and the number of points held, per feature kind (0 corner, 1 surface)
    void cell_map_size(int kind, int64_t *n_cells, int64_t *n_points)
    {
        ll_cellmap *c = ll_history_cell_map(h_.get(), kind);
        if (!c) check(-1, "ll_history_cell_map");
        check(ll_cellmap_stats(c, n_cells, n_points, nullptr), "ll_cellmap_stats");
    }

   private:
    Handle<ll_history, ll_history_destroy> h_;
};

// ------------------------------------------------------------------------------------------------------------
// The history match buffers of n_sequences Laser_mapping instances advanced in lock step, in one handle (ll_history_batch_*):
// slot s behaves as a History_buffer of its own -- add-frame rule with the gate pose, FIFO, refresh into maps[s] -- while one
// add() and one refresh() serve all slots with a fixed number of launches and host waits.  active: n_sequences flags or nullptr
// (all); an inactive slot is neither read nor changed.  poses / gate_poses: n_sequences x {qx,qy,qz,qw,tx,ty,tz}, the registered
// poses and the poses before the registration (nullptr: the registered poses gate).
class History_batch {
   public:
    History_batch(int n_sequences, int maximum_history_size, int max_points_per_frame, float line_res, float plane_res, int device = 0)
        : n_(n_sequences)
    {
        make_handle(h_, "ll_history_batch_create", [&](ll_history_batch **out) {
            return ll_history_batch_create(device, n_sequences, maximum_history_size, max_points_per_frame, line_res, plane_res, out);
        });
    }

    // slot s takes scan s of the extractor; added (optional): n_sequences flags, 1 where the frame was pushed
    void add(ll_fe *fe, const double *poses, const double *gate_poses = nullptr, const int32_t *active = nullptr,
             double history_add_t_step = 0.0, double history_add_angle_step = 0.0, int32_t *added = nullptr)
    {
        check(ll_history_batch_add_fe(h_.get(), fe, active, poses, gate_poses, history_add_t_step, history_add_angle_step, added), "ll_history_batch_add_fe");
    }
    // slot s takes cloud s of the two filters (the down-sampled stacks of the last enqueue_fe_maps with filters)
    void add(ll_voxel *vox_corner, ll_voxel *vox_surf, const double *poses, const double *gate_poses = nullptr, const int32_t *active = nullptr,
             double history_add_t_step = 0.0, double history_add_angle_step = 0.0, int32_t *added = nullptr)
    {
        check(ll_history_batch_add_voxel(h_.get(), vox_corner, vox_surf, active, poses, gate_poses, history_add_t_step, history_add_angle_step, added),
              "ll_history_batch_add_voxel");
    }
    // g_if_undistore = 1 for the next add() (laser_mapping.hpp:1424,1430), History_buffer::set_undistort for all slots: active slot s moves
    // its clouds with the state slot s of the registration `reg` collected last left; poses / gate_poses keep serving the add-frame rule.
    void set_undistort(ll_reg *reg)
    {
        if (!&ll_history_batch_set_undistort)
            throw std::runtime_error("set_undistort: this program is linked against a library without ll_history_batch_set_undistort");
        check(ll_history_batch_set_undistort(h_.get(), reg), "ll_history_batch_set_undistort");
    }
    // update_buff_for_matching() of every active slot: new search grids of both kinds in maps[s]
    void refresh(ll_map *const *maps, const int32_t *active = nullptr, int64_t *n_corner = nullptr, int64_t *n_surf = nullptr)
    {
        check(ll_history_batch_refresh(h_.get(), maps, active, n_corner, n_surf), "ll_history_batch_refresh");
    }
    // update_buff_for_matching() with m_matching_mode == 1 for every active slot, at poses [n_sequences][7]: the cells of the slot's cell
    // maps in range and in the field of view, each through the VoxelGrid (and replaced by its leaves with m_down_sample_replace),
    // concatenated, filtered, published into maps[s].  Needs enable_cell_maps().
    void refresh_cells(ll_map *const *maps, const double *poses, const int32_t *active = nullptr, float m_maximum_search_range_corner = 100.0f,
                       float m_maximum_search_range_surface = 100.0f, float m_maximum_in_fov_angle = 30.0f, int m_down_sample_replace = 1,
                       int64_t *n_corner = nullptr, int64_t *n_surf = nullptr)
    {
        check(ll_history_batch_refresh_cells(h_.get(), maps, active, poses, m_maximum_search_range_corner, m_maximum_search_range_surface,
                                             m_maximum_in_fov_angle, m_down_sample_replace, n_corner, n_surf),
              "ll_history_batch_refresh_cells");
    }
    void cell_match_work(int64_t out[8]) { check(ll_history_batch_cell_match_work(h_.get(), out), "ll_history_batch_cell_match_work"); }
    template <class Cloud>
    void map_cloud(int sequence, int kind, Cloud &out)
    {
        read_cloud("ll_history_batch_map_cloud", out,
                   [&](float *xyzi, int64_t capacity) { return ll_history_batch_map_cloud(h_.get(), sequence, kind, xyzi, capacity); });
    }
    int size(int sequence) const { return ll_history_batch_size(h_.get(), sequence); }
    int n_sequences() const { return n_; }
    ll_history_batch *handle() { return h_.get(); }

    // m_pt_cell_map_corners / m_pt_cell_map_planes of every slot (laser_mapping.hpp:274-275, 617-624): from here on every active slot
    // of add() appends its filtered frame to its two cell maps, pushed or not.  An add costs the new points; the stored points are put
    // in order by the first read after it (cell_map_stats / cell_map_dump / cell_map_device_view, or sync_cell_maps()).
    void enable_cell_maps(int64_t initial_points_per_map, float cell_resolution = 1.0f, int threshold_cell_revisit = 5000)
    {
        check(ll_history_batch_enable_cell_maps(h_.get(), initial_points_per_map, cell_resolution, threshold_cell_revisit), "ll_history_batch_enable_cell_maps");
    }
    void sync_cell_maps() { check(ll_history_batch_sync_cell_maps(h_.get()), "ll_history_batch_sync_cell_maps"); }
    void cell_map_stats(int sequence, int kind, int64_t *n_cells, int64_t *n_points, int32_t *frame_idx = nullptr)
    {
        check(ll_history_batch_cell_map_stats(h_.get(), sequence, kind, n_cells, n_points, frame_idx), "ll_history_batch_cell_map_stats");
    }
    // the layouts of ll_cellmap_dump: xyzi [n_points][4], cell_ijk [n_cells][3], cell_start [n_cells + 1], cell_last_update [n_cells]
    void cell_map_dump(int sequence, int kind, std::vector<float> &xyzi, std::vector<int32_t> &cell_ijk, std::vector<int32_t> &cell_start,
                       std::vector<int32_t> &cell_last_update)
    {
        int64_t nc = 0, np = 0;
        cell_map_stats(sequence, kind, &nc, &np);
        xyzi.assign((size_t)(np > 0 ? np : 1) * 4, 0.0f);
        cell_ijk.assign((size_t)(nc > 0 ? nc : 1) * 3, 0);
        cell_start.assign((size_t)nc + 1, 0);
        cell_last_update.assign((size_t)(nc > 0 ? nc : 1), 0);
        check(ll_history_batch_cell_map_dump(h_.get(), sequence, kind, xyzi.data(), np > 0 ? np : 1, cell_ijk.data(), cell_start.data(),
                                             cell_last_update.data(), nc > 0 ? nc : 1),
              "ll_history_batch_cell_map_dump");
        xyzi.resize((size_t)np * 4);
        cell_ijk.resize((size_t)nc * 3);
        cell_last_update.resize((size_t)nc);
    }
    // device pointers to the slot's stored points ({x, y, z, 0}) and their 64-bit cell keys: valid until the next add()
    void cell_map_device_view(int sequence, int kind, const float **dev_xyz0, const uint64_t **dev_point_keys, int64_t *n_points,
                              int64_t *n_cells = nullptr)
    {
        check(ll_history_batch_cell_map_device_view(h_.get(), sequence, kind, dev_xyz0, dev_point_keys, n_points, n_cells),
              "ll_history_batch_cell_map_device_view");
    }
    // Maps_keyframe's view of the shared cells (cell_map_keyframe.hpp:1243-1261) for several slots in one call: request r copies the
    // cells of slot sequences[r]'s map of `kind` (0 corner, 1 surface; 2 the full-cloud map of ll_history_batch_enable_full_maps) named
    // in cells[r] into *dst[r], on the device, as Points_cloud_map::extract_cells does out of a map of the slot's own.  A slot and a
    // destination appear at most once per call; enqueues and host waits do not depend on the number of requests.  Returns, per
    // request, the cells found; n_points (when given): the points copied.
    // Map: Points_cloud_map (defined below).
    template <class Map>
    std::vector<int64_t> extract_cells(int kind, const std::vector<int> &sequences, const std::vector<std::vector<std::array<int, 3>>> &cells,
                                       const std::vector<Map *> &dst, std::vector<int64_t> *n_points = nullptr)
    {
        const size_t R = sequences.size();
        if (cells.size() != R || dst.size() != R) throw std::invalid_argument("History_batch::extract_cells: one cell list and one destination per sequence");
        std::vector<int32_t> seq(sequences.begin(), sequences.end()), ijk;
        const std::vector<int64_t> off = csr_offsets(cells);
        std::vector<int64_t> n_found(R > 0 ? R : 1, 0), n_pts(R > 0 ? R : 1, 0);
        std::vector<ll_cellmap *> maps(R > 0 ? R : 1, nullptr);
        for (size_t r = 0; r < R; r++) {
            pack_cells(cells[r], ijk);
            maps[r] = dst[r] ? dst[r]->handle() : nullptr;
        }
        check(ll_history_batch_extract_cells(h_.get(), kind, (int32_t)R, seq.data(), off.data(), ijk.empty() ? nullptr : ijk.data(), maps.data(), n_found.data(),
                                             n_pts.data()),
              "ll_history_batch_extract_cells");
        for (size_t r = 0; r < R; r++) dst[r]->holds_at_least(n_pts[r]);
        n_found.resize(R);
        n_pts.resize(R);
        if (n_points) *n_points = n_pts;
        return n_found;
    }
    // The scan log: m_laser_cloud_full_history of every slot on the device (laser_mapping.hpp:1456, 1480-1486, 1545-1558).  It needs
    // the full maps (ll_history_batch_enable_full_maps); log_full follows the ll_history_batch_append_full_fe of the same step with
    // that call's extractor.  Thin wrappers of the C ABI, which documents them.
    void enable_scan_log(int maximum_history_size, int64_t initial_scans)
    {
        check(ll_history_batch_enable_scan_log(h_.get(), maximum_history_size, initial_scans), "ll_history_batch_enable_scan_log");
    }
    void log_full(ll_fe *fe, const int32_t *active = nullptr) { check(ll_history_batch_log_full_fe(h_.get(), fe, active), "ll_history_batch_log_full_fe"); }
    int64_t hand_over(int sequence)
    {
        int64_t id = 0;
        check(ll_history_batch_scan_log_hand_over(h_.get(), sequence, &id), "ll_history_batch_scan_log_hand_over");
        return id;
    }
    void drop_groups(const std::vector<int64_t> &group_ids)
    {
        check(ll_history_batch_scan_log_drop(h_.get(), (int64_t)group_ids.size(), group_ids.empty() ? nullptr : group_ids.data()), "ll_history_batch_scan_log_drop");
    }
    // the group's points {x, y, z, intensity}, scan after scan
    std::vector<float> read_group(int64_t group_id)
    {
        return read_xyzi("ll_history_batch_scan_log_read", [&](float *xyzi, int64_t capacity) {
            int64_t n = 0;
            const int rc = ll_history_batch_scan_log_read(h_.get(), group_id, xyzi, capacity, &n);
            return rc < 0 ? (int64_t)rc : n;
        });
    }
    void scan_log_work(int64_t out[4]) { check(ll_history_batch_scan_log_work(h_.get(), out), "ll_history_batch_scan_log_work"); }

   private:
    Handle<ll_history_batch, ll_history_batch_destroy> h_;
    int n_ = 0;
};

// ------------------------------------------------------------------------------------------------------------
// Points_cloud_map<float> (cell_map_keyframe.hpp:477-790) with the cell statistics and key-frame descriptors the loop
// detection reads (determine_feature :436-473, Maps_keyframe::analyze :1385-1493), resident on the device.
class Points_cloud_map {
   public:
    enum Feature_type { e_feature_sphere = 0, e_feature_line = 1, e_feature_plane = 2 };  // cell_map_keyframe.hpp:46-51

    explicit Points_cloud_map(int64_t max_points, float resolution = 1.0f, int m_minimum_revisit_threshold = 2147483647, int device = 0)
        : capacity_(max_points)
    {
        make_handle(h_, "ll_cellmap_create",
                    [&](ll_cellmap **out) { return ll_cellmap_create(device, max_points, resolution, m_minimum_revisit_threshold, out); });
    }

    template <class Cloud>
    void append_cloud(const Cloud &cloud)  // :619-672 (intensity is not kept, :82)
    {
        const std::vector<float> v = cloud_to_xyzi(cloud);
        check(ll_cellmap_append(h_.get(), v.data(), (int32_t)(v.size() / 4)), "ll_cellmap_append");
    }
    // append_cloud( pts, &cell_vec ) (:619-672, what the mapping node calls when loop closure is on, laser_mapping.hpp:1442): the
    // reference's cell_vec is a set of cell POINTERS; the cells live on the device here, so the set holds their integer cell
    // indices {ix, iy, iz} (centre = index * box + box / 2, :559-568) -- every cell of the first cloud, afterwards the cells that
    // received at least three points of this cloud (:640-662).  Set arithmetic of Maps_keyframe::add_cells (:1243-1261) works on
    // these as it does on the pointers.
    typedef std::array<int32_t, 3> Cell_index;
    template <class Cloud>
    void append_cloud(const Cloud &cloud, std::set<Cell_index> *cell_vec)
    {
        if (!cell_vec) return append_cloud(cloud);
        const std::vector<float> v = cloud_to_xyzi(cloud);
        const int32_t n = (int32_t)(v.size() / 4);
        std::vector<int32_t> ijk((size_t)(n > 0 ? n : 1) * 3);  // a cloud of n points touches at most n cells
        int64_t n_touched = 0;
        check(ll_cellmap_append_touched(h_.get(), v.data(), n, 3, ijk.data(), (int64_t)(ijk.size() / 3), &n_touched), "ll_cellmap_append_touched");
        cell_vec->clear();
        const int64_t n_listed = n_touched < (int64_t)(ijk.size() / 3) ? n_touched : (int64_t)(ijk.size() / 3);  // (a short buffer truncates; this one never is)
        for (int64_t i = 0; i < n_listed; i++) cell_vec->insert(Cell_index{ijk[3 * i], ijk[3 * i + 1], ijk[3 * i + 2]});
    }
    // The reference's cells live on the heap and the map grows without bound (:619-672); the device map has a capacity: raise it, content,
    // revisit stamps and frame counter kept (no-op when not larger).
    void reserve(int64_t max_points)
    {
        check(ll_cellmap_reserve(h_.get(), max_points), "ll_cellmap_reserve");
        if (max_points > capacity_) capacity_ = max_points;  // (reserve_for doubles from the capacity the map really has)
    }
    // Maps_keyframe's view of the shared cells (:1243-1261: a key frame holds pointers to the map's cells and reads them as they are
    // now): the cells of this map named in `cells` -- a set: order and repeats do not matter, cells the map does not hold are skipped --
    // copied on the device into dst, a map of the same resolution on the same device.  dst's previous content goes and its capacity
    // grows when the selection does not fit; it ends as a fresh map after one append_cloud of the selected points, every point in
    // the cell it had here.  Returns the cells found; *n_points: the points copied.
    int64_t extract_cells(const std::vector<std::array<int, 3>> &cells, Points_cloud_map &dst, int64_t *n_points = nullptr)
    {
        std::vector<int32_t> ijk;
        pack_cells(cells, ijk);
        int64_t n_found = 0, n_pts = 0;
        check(ll_cellmap_extract_cells(h_.get(), ijk.empty() ? nullptr : ijk.data(), (int64_t)cells.size(), dst.h_.get(), &n_found, &n_pts),
              "ll_cellmap_extract_cells");
        if (n_pts > dst.capacity_) dst.capacity_ = n_pts;
        if (n_points) *n_points = n_pts;
        return n_found;
    }
    // Maps_keyframe::extract_specify_points( Feature_type ) (:1263-1281) with the map standing for the key frame's cell set: the points
    // of the line cells or of the plane cells, selected on the device (ll_cellmap_feature_clouds), cells in ascending cell order (the
    // reference walks a std::set of cell pointers: address order), every cell's points in stored order, intensity 0.  The sphere
    // cells are not selected by the scene alignment and have no device selection: asking for them throws.
    template <class Cloud>
    Cloud extract_specify_points(Feature_type select_type)
    {
        if (select_type != e_feature_line && select_type != e_feature_plane) check(-1, "extract_specify_points: only e_feature_line and e_feature_plane are selected on the device");
        const bool line = select_type == e_feature_line;
        Cloud out;
        read_cloud("ll_cellmap_feature_clouds", out, [&](float *xyzi, int64_t capacity) {
            int64_t n_line = 0, n_plane = 0;
            const int rc = ll_cellmap_feature_clouds(h_.get(), line ? xyzi : nullptr, line ? capacity : 0, &n_line, line ? nullptr : xyzi,
                                                     line ? 0 : capacity, &n_plane, nullptr);
            return rc < 0 ? (int64_t)rc : line ? n_line : n_plane;
        });
        return out;
    }
    // Maps_keyframe::get_center (:1291-1301): the float mean of the cell centres, cells in ascending cell order
    void get_center(float centre[3])
    {
        int64_t n_line = 0, n_plane = 0;
        check(ll_cellmap_feature_clouds(h_.get(), nullptr, 0, &n_line, nullptr, 0, &n_plane, centre), "ll_cellmap_feature_clouds");
    }
    // the stored points ({x, y, z, 0}, ordered by (cell, insertion)) and the 64-bit cell key of every point where they lie on the device;
    // valid until the next call that changes the map
    void device_view(const float **dev_xyz0, const uint64_t **dev_point_keys, int64_t *n_points, int64_t *n_cells = nullptr)
    {
        check(ll_cellmap_device_view(h_.get(), dev_xyz0, dev_point_keys, n_points, n_cells), "ll_cellmap_device_view");
    }
    // grows the capacity (doubling) so that n_more points fit: the reference's map grows on the heap without bound
    void reserve_for(size_t n_more)
    {
        int64_t n_pts = 0, cap = capacity_;
        check(ll_cellmap_stats(h_.get(), nullptr, &n_pts, nullptr), "ll_cellmap_stats");
        if (cap <= 0) cap = 1;
        while (cap < n_pts + (int64_t)n_more) cap *= 2;
        if (cap != capacity_) reserve(cap);
    }
    // find_cells_in_radius( centre, radius ) (:761-788) followed by what service_pub_surround_pts does with the cells
    // (laser_mapping.hpp:1172-1187): every cell's cloud through pcl::VoxelGrid( leaf ) on its own, concatenated in ascending cell order;
    // nothing is stored back.  pose[4..6] is the centre (no field-of-view test: maximum_in_fov_angle >= 360 switches it off).
    template <class Cloud>
    void find_cells_in_radius_filtered(const double pose[7], float radius, float leaf, Cloud &out)
    {
        int64_t n_sel = 0, n_out = 0;
        check(ll_cellmap_query_filter(h_.get(), pose, radius, 360.0f, leaf, 0, &n_sel, &n_out), "ll_cellmap_query_filter");
        read_cloud("ll_cellmap_result", out, [&](float *xyzi, int64_t capacity) { return xyzi ? ll_cellmap_result(h_.get(), xyzi, capacity) : n_out; });
    }
    int64_t get_cells_size() const  // :551-554
    {
        int64_t n = 0;
        check(ll_cellmap_stats(h_.get(), &n, nullptr, nullptr), "ll_cellmap_stats");
        return n;
    }
    // m_feature_type / m_feature_vector of every cell, in ascending cell-index order
    void determine_features(std::vector<int32_t> &feature_type, std::vector<float> &feature_vector)
    {
        const int64_t n = get_cells_size();
        feature_type.assign((size_t)n, 0);
        feature_vector.assign((size_t)n * 3, 0.f);
        check(ll_cellmap_features(h_.get(), feature_type.data(), feature_vector.data(), nullptr, nullptr, nullptr, n), "ll_cellmap_features");
    }
    // m_feature_img_line, m_feature_img_plane, m_feature_img_line_roi, m_feature_img_plane_roi (60 x 60 each, row = phi bin)
    // and m_ratio_nonzero_line / _plane of the four histograms; the map stands for the key frame's cell set
    void analyze(std::vector<float> &images, float ratio_nonzero[4], float roi_ratio = 0.9f)
    {
        images.assign((size_t)4 * 60 * 60, 0.f);
        check(ll_cellmap_keyframe_images(h_.get(), roi_ratio, images.data(), ratio_nonzero, nullptr, nullptr, nullptr), "ll_cellmap_keyframe_images");
    }
    // Maps_keyframe::max_similiarity_of_two_image (:1155-1196) of two 60 x 60 images
    static float max_similiarity_of_two_image(const float *img_a, const float *img_b, int device = 0)
    {
        float s = 0.f;
        check(ll_keyframe_similarity(device, img_a, img_b, &s), "ll_keyframe_similarity");
        return s;
    }
    ll_cellmap *handle() { return h_.get(); }
    // the library raised the capacity itself (History_batch::extract_cells into this map): reserve_for doubles from what the map has
    void holds_at_least(int64_t n_points)
    {
        if (n_points > capacity_) capacity_ = n_points;
    }

   private:
    Handle<ll_cellmap, ll_cellmap_destroy> h_;
    int64_t capacity_ = 0;
};

// ------------------------------------------------------------------------------------------------------------
// Device handles are expensive to create (hipMalloc of the per-scan scratch) and the node constructs a fresh
// Point_cloud_registration for every scan (laser_mapping.hpp:1348), up to maximum_parallel_thread of them at once
// (:1737-1742).  Objects therefore borrow their ll_reg from a process-wide pool and give it back in the destructor; the
// match-buffer ll_map is shared by all of them (an immutable snapshot is pinned by each solve, see ll_map_upload).
class Handle_pool {
   public:
    static Handle_pool &instance()
    {
        static Handle_pool p;
        return p;
    }
    ll_reg *acquire(int device, int max_features)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (size_t i = 0; i < free_.size(); i++)
                if (free_[i].device == device && free_[i].max_features >= max_features) {
                    ll_reg *r = free_[i].reg;
                    free_.erase(free_.begin() + (long)i);
                    return r;
                }
        }
        ll_reg *r = nullptr;
        runtime_hints();
        check(ll_reg_create(device, 1, max_features, &r), "ll_reg_create");
        std::lock_guard<std::mutex> lk(mu_);
        feat_.push_back(std::make_pair(r, Entry{r, device, max_features}));
        return r;
    }
    void release(ll_reg *r)
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto &kv : feat_)
            if (kv.first == r) {
                free_.push_back(kv.second);
                return;
            }
    }
    // What the shared match-buffer map of a device holds, as far as this process uploaded it: size and a hash of EVERY point of
    // the cloud (the node allocates new clouds for each scan and deep-copies the match buffer into them, laser_mapping.hpp:1391-1392,
    // 1396-1401: an address says nothing, and an allocator may hand the same address out again for other contents), plus the map's
    // generation right after that upload -- anything else that publishes a structure (History_buffer::refresh) voids the key.
    struct Key {
        size_t n = (size_t)-1;
        uint64_t hash = 0;
        int64_t generation = -1;
    };
    struct Shared_map {
        int device = 0;
        ll_map *map = nullptr;
        Key key[2];
        std::mutex upload_mu;  // upload + pin of one registration are atomic against another thread's upload
    };
    Shared_map &shared(int device)
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto &m : maps_)
            if (m->device == device) return *m;
        ll_map *m = nullptr;
        runtime_hints();
        check(ll_map_create(device, &m), "ll_map_create");
        maps_.push_back(std::unique_ptr<Shared_map>(new Shared_map()));
        maps_.back()->device = device;
        maps_.back()->map = m;
        return *maps_.back();
    }
    ll_map *shared_map(int device) { return shared(device).map; }

   private:
    struct Entry {
        ll_reg *reg;
        int device, max_features;
    };
    Handle_pool() {}
    // No HIP calls at static destruction: the runtime may already be gone by then (the handles die with the process).
    ~Handle_pool() {}
    std::mutex mu_;
    std::vector<Entry> free_;
    std::vector<std::pair<ll_reg *, Entry>> feat_;
    std::vector<std::unique_ptr<Shared_map>> maps_;
};

// ------------------------------------------------------------------------------------------------------------
// Registration information (ll_reg_information, DESIGN "Registration information"): host arithmetic on the 36 numbers of a scan's
// Gauss-Newton matrix.  The adapter has no Eigen of its own, so the eigen decomposition is a cyclic Jacobi.

// Eigenvalues (ascending, w[6]) and eigenvectors (the COLUMNS of V, row-major: V[i * 6 + k] = component i of vector k) of the symmetric
// 6 x 6 matrix H (row-major; the upper triangle is read).  Cyclic Jacobi: every sweep annihilates the 15 off-diagonal entries in turn by
// plane rotations, until the off-diagonal norm is below 2^-52 of the diagonal's (a handful of sweeps; convergence is quadratic).
// Returns the sweeps taken.
inline int symmetric_eigen6(const double H[36], double w[6], double V[36])
{
    double a[36];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            a[i * 6 + j] = i <= j ? H[i * 6 + j] : H[j * 6 + i];
            V[i * 6 + j] = i == j ? 1.0 : 0.0;
        }
    int sweep = 0;
    for (; sweep < 60; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < 6; i++) {
            diag += a[i * 6 + i] * a[i * 6 + i];
            for (int j = i + 1; j < 6; j++) off += a[i * 6 + j] * a[i * 6 + j];
        }
        if (off == 0.0 || off <= 4.9303806576313238e-32 * diag) break;  // 2^-104: |off| <= 2^-52 |diag|
        for (int p = 0; p < 5; p++)
            for (int q = p + 1; q < 6; q++) {
                const double apq = a[p * 6 + q];
                if (apq == 0.0) continue;
                const double theta = (a[q * 6 + q] - a[p * 6 + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < 6; k++) {  // A <- A J
                    const double akp = a[k * 6 + p], akq = a[k * 6 + q];
                    a[k * 6 + p] = c * akp - sn * akq;
                    a[k * 6 + q] = sn * akp + c * akq;
                }
                for (int k = 0; k < 6; k++) {  // A <- J^T A
                    const double apk = a[p * 6 + k], aqk = a[q * 6 + k];
                    a[p * 6 + k] = c * apk - sn * aqk;
                    a[q * 6 + k] = sn * apk + c * aqk;
                }
                a[p * 6 + q] = a[q * 6 + p] = 0.0;  // (what the rotation was chosen for)
                for (int k = 0; k < 6; k++) {  // V <- V J
                    const double vkp = V[k * 6 + p], vkq = V[k * 6 + q];
                    V[k * 6 + p] = c * vkp - sn * vkq;
                    V[k * 6 + q] = sn * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < 6; i++) w[i] = a[i * 6 + i];
    for (int i = 0; i < 5; i++) {  // ascending, the vectors with their values
        int m = i;
        for (int j = i + 1; j < 6; j++)
            if (w[j] < w[m]) m = j;
        if (m != i) {
            std::swap(w[i], w[m]);
            for (int k = 0; k < 6; k++) std::swap(V[k * 6 + i], V[k * 6 + m]);
        }
    }
    return sweep;
}

// H of the solver's tangent d = [d_rot; d_t] of the increment as the information of the scan's pose in the map frame, ordered
// translation then rotation vector (radians) like the pose graph's residual: with R = R(pose_last) a step d moves the pose by
// xi = T d, T = [[0, R], [2 R, 0]], hence H_pose = T^-T H T^-1 with T^-1 = [[0, R^T / 2], [R^T, 0]].  pose_last = (qx, qy, qz, qw, t).
inline void information_in_pose_frame(const double H[36], const double pose_last[7], double H_pose[36])
{
    const double x = pose_last[0], y = pose_last[1], z = pose_last[2], w = pose_last[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w),     2 * (x * z + y * w),
                         2 * (x * y + z * w),     1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w),     2 * (y * z + x * w),     1 - 2 * (x * x + y * y)};
    double Ti[36] = {0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            Ti[i * 6 + 3 + j] = 0.5 * R[j * 3 + i];  // d_rot = R^T theta / 2
            Ti[(3 + i) * 6 + j] = R[j * 3 + i];      // d_t = R^T dt
        }
    double HT[36];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            double v = 0.0;
            for (int k = 0; k < 6; k++) v += H[i * 6 + k] * Ti[k * 6 + j];
            HT[i * 6 + j] = v;
        }
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            double v = 0.0;
            for (int k = 0; k < 6; k++) v += Ti[k * 6 + i] * HT[k * 6 + j];
            H_pose[i * 6 + j] = v;
        }
}

// what Point_cloud_registration::information() returns
struct Registration_information {
    double H[36], g[6], cost;           // ll_reg_information_record: solver tangent [d_rot; d_t]
    int n_line, n_plane, status;        // blocks summed; 0 computed, 1 gated / no iteration / empty scan, 2 aborted solve
    double eigenvalues[6];              // of H, ascending
    double eigenvectors[36];            // columns, row-major (symmetric_eigen6)
    double H_pose[36];                  // information_in_pose_frame( H, the pose the registration started from )
};

// ------------------------------------------------------------------------------------------------------------
// The part of Point_cloud_registration that copies as plain values: the class copies it as a whole, so a field added here is copied
// without being named anywhere.
struct Point_cloud_registration_fields {
    // configuration fields with the reference names and defaults (point_cloud_registration.hpp:45-103)
    int ICP_PLANE = 1, ICP_LINE = 1;
    int IF_LINE_FEATURE_CHECK = 0, IF_PLANE_FEATURE_CHECK = 0;  // PCR:46,48
    int line_search_num = 5, plane_search_num = 5;              // PCR:45,47 (the device search is fixed at k = 5)
    int m_if_motion_deblur = 0;
    int m_if_compute_information = 0;  // 1: every registration also leaves information() (not in the reference; off: no call more)
    int m_current_frame_index = 0;
    int m_mapping_init_accumulate_frames = 100;
    float m_last_time_stamp = 0;
    float m_para_max_angular_rate = 200.0f / 50.0f;
    float m_para_max_speed = 100.0f / 50.0f;
    float m_max_final_cost = 100.0f;
    int m_para_icp_max_iterations = 20;
    int m_para_cere_max_iterations = 100;
    int m_para_cere_prerun_times = 2;
    float m_minimum_pt_time_stamp = 0, m_maximum_pt_time_stamp = 1.0f;
    double m_minimum_icp_R_diff = 0.01, m_minimum_icp_T_diff = 0.01;
    double m_inliner_dis = 0.02, m_inlier_ratio = 0.80;
    double m_maximum_dis_plane_for_match = 50.0, m_maximum_dis_line_for_match = 2.0;
    int m_maximum_allow_residual_block = 100000;
    int m_subsample_seed = 1;  // seed of the reproducible stand-in for m_rand_float (PCR:104); 0 = refuse to sub-sample
    int m_if_verbose_screen_printf = 1;  // ADD_SCREEN_PRINTF_OUT_METHOD (PCR:119); nothing is printed here
    // what the node points at its loggers / timer (PCR:78-82, LM:1271-1274, SA:234-236) and the k-d tree members (PCR:72-73)
    Any_ptr m_logger_common, m_logger_pcd, m_logger_timer, m_timer;
    Any_sink m_kdtree_corner_from_map, m_kdtree_surf_from_map;
    // state, with the reference's member names and types (PCR:51-56, 75-76)
    double m_para_buffer_RT[7] = {0, 0, 0, 1, 0, 0, 0};
    double m_para_buffer_RT_last[7] = {0, 0, 0, 1, 0, 0, 0};
    double m_para_buffer_incremental[7] = {0, 0, 0, 1, 0, 0, 0};
    Quaterniond m_q_w_curr, m_q_w_last;
    Vector3d m_t_w_curr, m_t_w_last;
    double m_inlier_threshold = 0, m_angular_diff = 0, m_t_diff = 0;
    // ceres::Solver::Summary look-alike: the fields and reports the node reads (LM:1041, 1511-1512; PCR:555-559)
    struct Opt_summary : ll_reg_report {
        int num_residual_blocks = 0;
        Opt_summary() : ll_reg_report() {}
        static Opt_summary from(const ll_reg_report &rep)
        {
            Opt_summary s;
            static_cast<ll_reg_report &>(s) = rep;
            s.num_residual_blocks = rep.n_blocks_last;
            return s;
        }
        std::string BriefReport() const
        {
            char b[256];
            std::snprintf(b, sizeof(b), "loam_livox_hip: ICP iterations %d, LM iterations %d, initial_cost %.6e, final_cost %.6e, blocks %d",
                          icp_iterations, lm_iterations_total, initial_cost, final_cost, n_blocks_last);
            return b;
        }
        std::string FullReport() const { return BriefReport(); }
    };
    Opt_summary summary, m_final_opt_summary;
    ll_reg_information_record m_information_record = {};  // of the last registration made with m_if_compute_information
    int m_information_valid = 0;
    int device = 0;
    int max_features = 100000;
};

class Point_cloud_registration : public Point_cloud_registration_fields {
   public:
    // views of this object's own m_para_buffer_incremental (PCR:55-56): a copy keeps its own
    Quaterniond_map m_q_w_incre = Quaterniond_map(m_para_buffer_incremental);
    Vector3d_map m_t_w_incre = Vector3d_map(m_para_buffer_incremental + 4);

    Point_cloud_registration()
    {
        m_q_w_last.setIdentity();
        m_t_w_last.setZero();
        m_q_w_curr.setIdentity();
        m_t_w_curr.setZero();
    }
    // a copy takes the fields; it borrows a registrar of its own on first use
    Point_cloud_registration(const Point_cloud_registration &o) : Point_cloud_registration_fields(o) {}
    Point_cloud_registration &operator=(const Point_cloud_registration &o)
    {
        Point_cloud_registration_fields::operator=(o);
        return *this;
    }

    // float refine_blur(in_blur, min_blur, max_blur), PCR:128-141
    float refine_blur(float in_blur, const float &min_blur, const float &max_blur) const
    {
        float res = 1.0f;
        if (m_if_motion_deblur) {
            res = (in_blur - min_blur) / (max_blur - min_blur);
            if (!std::isfinite(res) || res > 1.0f) return 1.0f;
        }
        return res;
    }

    // int find_out_incremental_transfrom(map_corner, map_surf, kd_corner, kd_surf, scan_corner, scan_surf), PCR:163.
    // The KdTreeFLANN arguments are accepted and ignored: the device grid replaces them.  The map is re-uploaded only
    // when a cloud changes (address, size or a sample of its contents), mirroring the match-buffer refresh of
    // laser_mapping.hpp:460-566; a solve that is already running keeps the snapshot it started with.
    template <class CloudPtr, class KdTree>
    int find_out_incremental_transfrom(CloudPtr map_corner, CloudPtr map_surf, KdTree &, KdTree &, CloudPtr scan_corner, CloudPtr scan_surf)
    {
        return find_out_incremental_transfrom(map_corner, map_surf, scan_corner, scan_surf);
    }

    // 4-argument overload, PCR:585-605 (returns 1 without registering when a map cloud is empty, :592-601)
    template <class CloudPtr>
    int find_out_incremental_transfrom(CloudPtr map_corner, CloudPtr map_surf, CloudPtr scan_corner, CloudPtr scan_surf)
    {
        // the solve pins the snapshots it is enqueued against: with upload and enqueue under one lock, a thread registers against
        // the clouds it was given even when another thread (laser_mapping.hpp:1737-1742) uploads other ones meanwhile
        Handle_pool::Shared_map &sm = Handle_pool::instance().shared(device);
        std::unique_lock<std::mutex> lk(sm.upload_mu);
        upload_if_changed(sm, LL_MAP_CORNER, *map_corner);
        upload_if_changed(sm, LL_MAP_SURF, *map_surf);
        return register_scan(scan_corner, scan_surf, &lk);
    }

    // The search structure the registrar matches against.  History_buffer::refresh( pc_reg.map() ) /
    // refresh_cells( pc_reg.map(), ... ) rebuild it on the device (update_buff_for_matching, laser_mapping.hpp:460-566);
    // the 2-argument form below then registers against it without a map cloud ever crossing the bus.
    ll_map *map() { return Handle_pool::instance().shared_map(device); }

    template <class CloudPtr>
    int find_out_incremental_transfrom(CloudPtr scan_corner, CloudPtr scan_surf)
    {
        return register_scan(scan_corner, scan_surf, nullptr);
    }

    // The scan a Spinning_laser holds (Spinning_laser::extract_device), registered against map() where the extractor left it:
    // corner stack = its less-sharp cloud, surface stack = its less-flat cloud (ll_reg_enqueue_spin).  The same bits as the
    // 2-argument form on the downloaded clouds.  m_if_motion_deblur must be 0 (the call throws otherwise: the spinning
    // extractor's intensity is not a time stamp).
    int find_out_incremental_transfrom(Spinning_laser &spin)
    {
        if (!spin.handle()) throw std::runtime_error("find_out_incremental_transfrom: the Spinning_laser has not extracted a scan");
        const int need = spin.capacity() > max_features ? spin.capacity() : max_features;
        if (reg_ && reg_cap_ < need) reg_.reset();  // too small: back to the pool
        ll_reg *reg = registrar(need);
        ll_reg_params p;
        fill_params(p);
        pose_from_members();
        {
            Information_switch sw(reg, m_if_compute_information);
            check(ll_reg_enqueue_spin(reg, map(), spin.handle(), 1, &p, m_para_buffer_RT_last, m_para_buffer_RT, m_para_buffer_incremental),
                  "ll_reg_enqueue_spin");
        }
        return collect();
    }

    // A map per slot (ll_reg_enqueue_fe_maps / ll_reg_enqueue_fe_downsampled_maps): scan b of a batched extractor registered against
    // maps[b] (nullptr = idle slot) with frame_index[b] (nullptr = m_current_frame_index for every slot), the start-up gate decided
    // per slot.  The batch handles are the caller's C handles (a registrar created with max_scans >= n_scans; voxel filters with
    // max_clouds >= n_scans); this object contributes its configuration fields.  Collect with ll_reg_collect( reg, n_scans, ... ).
    // m_if_motion_deblur = 1 needs set_time_ranges( reg, ... ) in front of the call (which throws otherwise).
    // set_time_ranges: a time range per scan for the NEXT enqueue_fe_maps on `reg` only (ll_reg_set_time_ranges) -- slot b runs from
    // minimum_pt_time_stamp[b] to maximum_pt_time_stamp[b] where a registration reads m_minimum_pt_time_stamp / m_maximum_pt_time_stamp.
    static void set_time_ranges(ll_reg *reg, const float *minimum_pt_time_stamp, const float *maximum_pt_time_stamp, int n_scans)
    {
        if (!&ll_reg_set_time_ranges) throw std::runtime_error("set_time_ranges: this program is linked against a library without ll_reg_set_time_ranges");
        check(ll_reg_set_time_ranges(reg, minimum_pt_time_stamp, maximum_pt_time_stamp, n_scans), "ll_reg_set_time_ranges");
    }
    void enqueue_fe_maps(ll_reg *reg, const ll_map *const *maps, ll_fe *fe, int n_scans, const int32_t *frame_index, const double *poses_last,
                         const double *poses_curr) const
    {
        ll_reg_params p;
        fill_params(p);
        check(ll_reg_enqueue_fe_maps(reg, maps, fe, n_scans, &p, frame_index, poses_last, poses_curr, nullptr), "ll_reg_enqueue_fe_maps");
    }
    // ... with the corner / surface clouds voxel-filtered on the device first (m_if_input_downsample_mode, laser_mapping.hpp:1367-1373)
    void enqueue_fe_maps(ll_reg *reg, const ll_map *const *maps, ll_fe *fe, ll_voxel *vox_corner, ll_voxel *vox_surf, float line_res,
                         float plane_res, int n_scans, const int32_t *frame_index, const double *poses_last, const double *poses_curr) const
    {
        ll_reg_params p;
        fill_params(p);
        check(ll_reg_enqueue_fe_downsampled_maps(reg, maps, fe, vox_corner, vox_surf, line_res, plane_res, n_scans, &p, frame_index, poses_last,
                                                 poses_curr, nullptr),
              "ll_reg_enqueue_fe_downsampled_maps");
    }

    // The information of the last registration made with m_if_compute_information = 1: the Gauss-Newton matrix of its last
    // linearisation (ll_reg_information), its eigen decomposition and the same matrix in the pose's own frame.  This object registers
    // one scan per call, so scan must be 0.
    Registration_information information(int scan = 0) const
    {
        if (scan != 0) throw std::runtime_error("information: this object registers one scan per call (scan must be 0)");
        if (!m_information_valid) throw std::runtime_error("information: no registration was made with m_if_compute_information = 1");
        Registration_information out;
        const ll_reg_information_record &r = m_information_record;
        std::memcpy(out.H, r.H, sizeof(out.H));
        std::memcpy(out.g, r.g, sizeof(out.g));
        out.cost = r.cost;
        out.n_line = r.n_line, out.n_plane = r.n_plane, out.status = r.status;
        symmetric_eigen6(out.H, out.eigenvalues, out.eigenvectors);
        information_in_pose_frame(out.H, m_para_buffer_RT_last, out.H_pose);
        return out;
    }

    // void pointAssociateToMap ... see below
   private:
    // ll_reg_set_information around ONE enqueue: the switch is read by the enqueue, and the registrar goes back to a pool whose other
    // borrowers did not ask.  Nothing is called when the member is 0.
    struct Information_switch {
        ll_reg *r;
        Information_switch(ll_reg *reg, int on) : r(on ? reg : nullptr)
        {
            if (!r) return;
            if (!&ll_reg_set_information || !&ll_reg_information)
                throw std::runtime_error("m_if_compute_information: this program is linked against a library without ll_reg_set_information");
            check(ll_reg_set_information(r, 1), "ll_reg_set_information");
        }
        ~Information_switch()
        {
            if (r) (void)ll_reg_set_information(r, 0);
        }
        Information_switch(const Information_switch &) = delete;
        Information_switch &operator=(const Information_switch &) = delete;
    };
    template <class CloudPtr>
    int register_scan(CloudPtr scan_corner, CloudPtr scan_surf, std::unique_lock<std::mutex> *held_until_enqueued)
    {
        ll_reg *reg = registrar(max_features);
        ll_map *m = map();
        const std::vector<float> c = cloud_to_xyzi(*scan_corner), s = cloud_to_xyzi(*scan_surf);
        ll_reg_params p;
        fill_params(p);
        pose_from_members();
        // ll_reg_solve in its three steps (upload the scan's features, enqueue = pin the map snapshots + launch, collect)
        const int32_t nc = (int32_t)(c.size() / 4), ns = (int32_t)(s.size() / 4);
        check(ll_reg_upload_features(reg, 1, xyzi_or_dummy(c), &nc, nc > 0 ? nc : 1, xyzi_or_dummy(s), &ns, ns > 0 ? ns : 1), "ll_reg_upload_features");
        {
            Information_switch sw(reg, m_if_compute_information);
            check(ll_reg_enqueue_uploaded(reg, m, 1, &p, m_para_buffer_RT_last, m_para_buffer_RT, m_para_buffer_incremental), "ll_reg_enqueue_uploaded");
        }
        if (held_until_enqueued) held_until_enqueued->unlock();
        return collect();
    }
    void fill_params(ll_reg_params &p) const
    {
        ll_reg_default_params(&p);
        p.if_motion_deblur = m_if_motion_deblur;
        p.icp_max_iterations = m_para_icp_max_iterations;
        p.ceres_max_iterations = m_para_cere_max_iterations;
        p.ceres_prerun_times = m_para_cere_prerun_times;
        p.icp_line = ICP_LINE;
        p.icp_plane = ICP_PLANE;
        p.if_line_feature_check = IF_LINE_FEATURE_CHECK;
        p.if_plane_feature_check = IF_PLANE_FEATURE_CHECK;
        p.current_frame_index = m_current_frame_index;
        p.mapping_init_accumulate_frames = m_mapping_init_accumulate_frames;
        p.maximum_allow_residual_block = m_maximum_allow_residual_block;
        p.subsample_seed = m_subsample_seed;
        p.maximum_dis_line_for_match = m_maximum_dis_line_for_match;
        p.maximum_dis_plane_for_match = m_maximum_dis_plane_for_match;
        p.inliner_dis = m_inliner_dis;
        p.inlier_ratio = m_inlier_ratio;
        p.minimum_icp_R_diff = m_minimum_icp_R_diff;
        p.minimum_icp_T_diff = m_minimum_icp_T_diff;
        p.para_max_angular_rate = m_para_max_angular_rate;
        p.para_max_speed = m_para_max_speed;
        p.max_final_cost = m_max_final_cost;
        p.minimum_pt_time_stamp = m_minimum_pt_time_stamp;
        p.maximum_pt_time_stamp = m_maximum_pt_time_stamp;
    }
    int collect()
    {
        ll_reg_report rep;
        int32_t ret = 0;
        check(ll_reg_collect(reg_.get(), 1, m_para_buffer_RT, m_para_buffer_incremental, &rep, &ret), "ll_reg_collect");
        m_information_valid = 0;
        m_interp_valid = 0;
        if (m_if_compute_information) {  // (no device work: the records came back with the collect)
            check(ll_reg_information(reg_.get(), 1, &m_information_record), "ll_reg_information");
            m_information_valid = 1;
        }
        members_from_pose();
        m_inlier_threshold = rep.inlier_threshold;
        m_angular_diff = rep.angular_diff_deg;
        m_t_diff = rep.t_diff;
        summary = Opt_summary::from(rep);
        if (ret == 1 && !rep.gated) m_final_opt_summary = summary;  // PCR:574
        if (ret == 0) m_last_time_stamp = m_minimum_pt_time_stamp;   // PCR:569
        return ret;
    }

   public:

    // void pointAssociateToMap(pi, po, interpolate_s = 1.0, if_undistore = 0), PCR:622-661.  The node calls it per point
    // with g_if_undistore == 0 (laser_mapping.hpp:80, 1424, 1430): p_w = q_w_curr * p + t_w_curr in double, stored to
    // float, with Eigen's rotation formula  v + w (2 q x v) + q x (2 q x v).  The Rodrigues-interpolated form (PCR:633-654,
    // if_undistore != 0 with m_if_motion_deblur and interpolate_s != 1) runs on the host with the state of the last registration,
    // fetched once per registration (ll_reg_interpolation): the arithmetic of ll_reg_core.h point_to_map_undistort.
    template <class P>
    void pointAssociateToMap(P const *const pi, P *const po, double interpolate_s = 1.0, int if_undistore = 0)
    {
        if (!(m_if_motion_deblur == 0 || if_undistore == 0 || interpolate_s == 1.0)) {
            fetch_interpolation();
            const double s = interpolate_s;
            const double T[3] = {m_interp_incre[4] * (s * 1.0), m_interp_incre[5] * (s * 1.0), m_interp_incre[6] * (s * 1.0)};  // PCR:641
            const double th = m_interp_theta * s;
            const double sn = std::sin(th), cs1 = 1.0 - std::cos(th);
            const double pc[3] = {(double)pi->x, (double)pi->y, (double)pi->z};
            double inner[3];
            for (int i = 0; i < 3; i++) {  // PCR:642-645
                double acc = 0.0;
                for (int j = 0; j < 3; j++) {
                    const double rij = ((i == j) ? 1.0 : 0.0) + sn * m_interp_hat[i * 3 + j] + cs1 * m_interp_hat_sq[i * 3 + j];
                    acc += rij * pc[j];
                }
                inner[i] = acc + T[i];
            }
            const double *q = m_interp_last;  // PCR:646
            double uv[3] = {q[1] * inner[2] - q[2] * inner[1], q[2] * inner[0] - q[0] * inner[2], q[0] * inner[1] - q[1] * inner[0]};
            uv[0] += uv[0];
            uv[1] += uv[1];
            uv[2] += uv[2];
            const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
            po->x = (float)((inner[0] + q[3] * uv[0] + c[0]) + q[4]);
            po->y = (float)((inner[1] + q[3] * uv[1] + c[1]) + q[5]);
            po->z = (float)((inner[2] + q[3] * uv[2] + c[2]) + q[6]);
            po->intensity = pi->intensity;
            return;
        }
        const double qx = m_q_w_curr.x(), qy = m_q_w_curr.y(), qz = m_q_w_curr.z(), qw = m_q_w_curr.w();
        const double v[3] = {(double)pi->x, (double)pi->y, (double)pi->z};
        double uv[3] = {qy * v[2] - qz * v[1], qz * v[0] - qx * v[2], qx * v[1] - qy * v[0]};
        uv[0] += uv[0];
        uv[1] += uv[1];
        uv[2] += uv[2];
        const double c[3] = {qy * uv[2] - qz * uv[1], qz * uv[0] - qx * uv[2], qx * uv[1] - qy * uv[0]};
        po->x = (float)((v[0] + qw * uv[0] + c[0]) + m_t_w_curr(0));
        po->y = (float)((v[1] + qw * uv[1] + c[1]) + m_t_w_curr(1));
        po->z = (float)((v[2] + qw * uv[2] + c[2]) + m_t_w_curr(2));
        po->intensity = pi->intensity;
    }

    // unsigned int pointcloudAssociateToMap(pc_in, pt_out, if_undistore = 0), PCR:673-685
    template <class Cloud>
    unsigned int pointcloudAssociateToMap(const Cloud &pc_in, Cloud &pt_out, int if_undistore = 0)
    {
        ll_reg *reg = registrar(max_features);
        pose_from_members();
        const std::vector<float> in = cloud_to_xyzi(pc_in);
        std::vector<float> out(in.size());
        if (if_undistore != 0 && m_if_motion_deblur != 0) {  // PCR:627: every point with the pose interpolated at its time stamp
            if (!&ll_cloud_undistort) throw std::runtime_error("pointcloudAssociateToMap: this program is linked against a library without ll_cloud_undistort");
            check(ll_cloud_undistort(reg, 0, in.data(), out.data(), (int)(in.size() / 4)), "ll_cloud_undistort");
            xyzi_to_cloud(out.data(), (int)(in.size() / 4), pt_out);
            return (unsigned int)(in.size() / 4);
        }
        check(ll_cloud_transform(reg, in.data(), out.data(), (int)(in.size() / 4), m_para_buffer_RT), "ll_cloud_transform");
        xyzi_to_cloud(out.data(), (int)(in.size() / 4), pt_out);
        return (unsigned int)(in.size() / 4);
    }

    // the registrar this object registers with (History_buffer::set_undistort); null before the first call that needs one
    ll_reg *handle() { return reg_.get(); }

   private:
    // m_interpolatation_theta / _omega_hat / _omega_hat_sq_2 (PCR:58,66-68), m_q_w_last / m_t_w_last and the increment of the last
    // collected registration, fetched by the first per-point call after it
    double m_interp_theta = 0.0, m_interp_hat[9] = {}, m_interp_hat_sq[9] = {}, m_interp_last[7] = {0, 0, 0, 1, 0, 0, 0}, m_interp_incre[7] = {0, 0, 0, 1, 0, 0, 0};
    int m_interp_valid = 0;
    void fetch_interpolation()
    {
        if (m_interp_valid) return;
        if (!&ll_reg_interpolation) throw std::runtime_error("pointAssociateToMap: this program is linked against a library without ll_reg_interpolation");
        if (!reg_) throw std::runtime_error("pointAssociateToMap: if_undistore needs a registration (find_out_incremental_transfrom) first");
        check(ll_reg_interpolation(reg_.get(), 1, &m_interp_theta, m_interp_hat, m_interp_last, m_interp_incre), "ll_reg_interpolation");
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double a = 0;
                for (int k = 0; k < 3; k++) a += m_interp_hat[i * 3 + k] * m_interp_hat[k * 3 + j];
                m_interp_hat_sq[i * 3 + j] = a;
            }
        m_interp_valid = 1;
    }
    void pose_from_members()
    {
        to_pose7(m_q_w_curr, m_t_w_curr, m_para_buffer_RT);
        to_pose7(m_q_w_last, m_t_w_last, m_para_buffer_RT_last);
    }
    void members_from_pose() { from_pose7(m_para_buffer_RT, m_q_w_curr, m_t_w_curr); }
    // the registrar borrowed from the pool, of `capacity` features when this call is the one that borrows it
    ll_reg *registrar(int capacity)
    {
        if (!reg_) reg_.reset(Handle_pool::instance().acquire(device, reg_cap_ = capacity));
        return reg_.get();
    }
    template <class Cloud>
    void upload_if_changed(Handle_pool::Shared_map &sm, int kind, const Cloud &c)
    {
        Handle_pool::Key now;
        now.n = c.points.size();
        uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)now.n;
        for (size_t i = 0; i < now.n; i++) {  // every point: ~1 ns each, against a grid build of milliseconds
            uint32_t b[3];
            const float v[3] = {c.points[i].x, c.points[i].y, c.points[i].z};
            std::memcpy(b, v, 12);
            h = (h ^ (((uint64_t)b[1] << 32) | b[0])) * 0xD6E8FEB86659FD93ull;
            h = (h ^ (h >> 32) ^ b[2]) * 0xFF51AFD7ED558CCDull;
        }
        now.hash = h;
        Handle_pool::Key &k = sm.key[kind];
        if (k.n == now.n && k.hash == now.hash && k.generation == ll_map_generation(sm.map, kind)) return;  // same contents, still the published structure
        int64_t gen = -1;  // the generation of OUR publication, reported from inside the map's lock
        if (now.n == 0) {
            check(ll_map_upload_gen(sm.map, kind, xyzi_or_dummy(std::vector<float>()), 4, 0, 0.0f, &gen), "ll_map_upload");
        } else {
            // ll_map_upload takes x, y, z at any float stride: a point type whose coordinates are three consecutive floats
            // (pcl::PointXYZI: 8 floats per point) goes as it lies, without a staging copy
            const auto &p0 = c.points[0];
            const bool strided = sizeof(p0) % sizeof(float) == 0 && (const void *)(&p0.x + 1) == (const void *)&p0.y &&
                                 (const void *)(&p0.x + 2) == (const void *)&p0.z;
            if (strided) {
                check(ll_map_upload_gen(sm.map, kind, &p0.x, (int32_t)(sizeof(p0) / sizeof(float)), (int64_t)now.n, 0.0f, &gen), "ll_map_upload");
            } else {
                const std::vector<float> v = cloud_to_xyzi(c);
                check(ll_map_upload_gen(sm.map, kind, v.data(), 4, (int64_t)now.n, 0.0f, &gen), "ll_map_upload");
            }
        }
        now.generation = gen;  // (not ll_map_generation() now: a refresh may have published in between, and the key would then vouch for it)
        k = now;
    }
    struct Give_back {
        void operator()(ll_reg *r) const { Handle_pool::instance().release(r); }
    };
    std::unique_ptr<ll_reg, Give_back> reg_;  // borrowed from Handle_pool, given back with this object
    int reg_cap_ = 0;                         // the feature capacity reg_ was acquired with
};

// ------------------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------------------
// Ceres_pose_graph_3d (ceres_pose_graph_3d.hpp:30-352): the types the loop detector fills and pose_graph_optimization, which runs on
// the device (ll_pose_graph_solve: the same problem, the same trust-region sequence, pose poses.begin() held constant).  Pose ids are
// the map's keys; the constraints name them.  Nothing is printed or written; the solver's summary is returned instead.
namespace Ceres_pose_graph_3d {

// the information matrix of a constraint, read and written as information( i, j ) like the reference's Eigen matrix
struct Matrix6d {
    double c[36];
    double &operator()(int i, int j) { return c[i * 6 + j]; }
    double operator()(int i, int j) const { return c[i * 6 + j]; }
    void setIdentity()
    {
        for (int i = 0; i < 36; i++) c[i] = i % 7 == 0 ? 1.0 : 0.0;
    }
};

struct Pose3d {
    Vector3d p;
    Quaterniond q;
    Pose3d()
    {
        q.setIdentity();
        p.setZero();
    }
    Pose3d(const Quaterniond &in_q, const Vector3d &in_t) : p(in_t), q(in_q) {}
#if defined(LOAM_LIVOX_ADAPTER_EIGEN)
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
#endif
};

struct Constraint3d {
    int id_begin = 0, id_end = 0;
    Pose3d t_be;            // the measurement: the pose of id_end in the frame of id_begin
    Matrix6d information;   // identity unless set
    Constraint3d() { information.setIdentity(); }
    Constraint3d(int id_a, int id_b, const Quaterniond &q_a2b, const Vector3d &t_a2b) : id_begin(id_a), id_end(id_b), t_be(q_a2b, t_a2b)
    {
        information.setIdentity();
    }
#if defined(LOAM_LIVOX_ADAPTER_EIGEN)
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
#endif
};

#if defined(LOAM_LIVOX_ADAPTER_EIGEN) && defined(EIGEN_WORLD_VERSION)
typedef std::map<int, Pose3d, std::less<int>, Eigen::aligned_allocator<std::pair<const int, Pose3d>>> MapOfPoses;
typedef std::vector<Constraint3d, Eigen::aligned_allocator<Constraint3d>> VectorOfConstraints;
typedef std::vector<Pose3d, Eigen::aligned_allocator<Pose3d>> VectorOfPose;
#else
typedef std::map<int, Pose3d> MapOfPoses;
typedef std::vector<Constraint3d> VectorOfConstraints;
typedef std::vector<Pose3d> VectorOfPose;
#endif

// :336-352.  The poses are optimised in place.
inline ll_pose_graph_summary pose_graph_optimization(MapOfPoses &poses, VectorOfConstraints &constraints, int device = 0)
{
    ll_pose_graph_summary summary = ll_pose_graph_summary();
    summary.termination = LL_POSE_GRAPH_NOTHING_TO_OPTIMISE;
    if (poses.empty()) return summary;
    std::map<int, int> index;
    std::vector<double> x;
    for (MapOfPoses::const_iterator it = poses.begin(); it != poses.end(); ++it) {
        index[it->first] = (int)index.size();
        double row[7];
        to_pose7(it->second.q, it->second.p, row);
        x.insert(x.end(), row, row + 7);
    }
    const int64_t n = (int64_t)poses.size(), e = (int64_t)constraints.size();
    std::vector<int32_t> ab, first((size_t)n, 0);
    std::vector<double> meas, info;
    for (int64_t k = 1; k < n; k++) first[(size_t)k] = (int32_t)(k - 1);
    for (size_t k = 0; k < constraints.size(); k++) {
        const Constraint3d &c = constraints[k];
        if (!index.count(c.id_begin) || !index.count(c.id_end)) check(-1, "pose_graph_optimization: a constraint names a pose that is not in the map");
        const int a = index[c.id_begin], b = index[c.id_end];
        ab.push_back(a), ab.push_back(b);
        double row[7];
        to_pose7(c.t_be.q, c.t_be.p, row);
        meas.insert(meas.end(), row, row + 7);
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) info.push_back(c.information(i, j));
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        if (lo >= 1 && first[(size_t)hi] > lo - 1) first[(size_t)hi] = lo - 1;
    }
    int64_t blocks = 1;
    for (int64_t k = 1; k < n; k++) blocks += (k - 1) - first[(size_t)k] + 1;
    Handle<ll_pose_graph, ll_pose_graph_destroy> h;
    make_handle(h, "ll_pose_graph_create", [&](ll_pose_graph **out) { return ll_pose_graph_create(device, 1, n, e > 0 ? e : 1, blocks, out); });
    const int64_t pose_offsets[2] = {0, n}, edge_offsets[2] = {0, e};
    check(ll_pose_graph_solve(h.get(), nullptr, 1, pose_offsets, x.data(), edge_offsets, ab.data(), meas.data(), info.data(), &summary),
          "ll_pose_graph_solve");  // (h goes on both ways out, after the error's text is taken)
    size_t k = 0;
    for (MapOfPoses::iterator it = poses.begin(); it != poses.end(); ++it, k++) from_pose7(&x[7 * k], it->second.q, it->second.p);
    return summary;
}

// Eigen's quaternion arithmetic on {x, y, z, w}, for builds with and without Eigen
namespace detail {
inline void q_mul(const double a[4], const double b[4], double o[4])
{
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
inline void q_inverse(const double q[4], double o[4])
{
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    o[0] = -q[0] / n2, o[1] = -q[1] / n2, o[2] = -q[2] / n2, o[3] = q[3] / n2;
}
inline void q_rotate(const double q[4], const double v[3], double o[3])
{
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int i = 0; i < 3; i++) uv[i] = uv[i] + uv[i];
    const double uuv[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int i = 0; i < 3; i++) o[i] = v[i] + q[3] * uv[i] + uuv[i];
}
}  // namespace detail

}  // namespace Ceres_pose_graph_3d

// Scene_alignment (scene_alignment.hpp:19-391): two key frames, each held as a Points_cloud_map, registered against each other coarse
// to fine, on the device from the cell maps to the pose (ll_scene_align_run: no point of either key frame crosses to the host).
// Member names and defaults are the reference's.  What differs, by design:
//   - the key frames' cells come in ascending cell order, not in the order of their heap addresses;
//   - every call starts from the identity and the centre offset: the previous pair's m_q_w_incre is not kept;
//   - nothing is written to disk: if_save and mapping_save_path are accepted and ignored, init() takes no directory to create;
//   - m_pc_reg is where the RESULT is read (m_q_w_curr, m_t_w_curr, m_inlier_threshold, summary); the registrar's settings are the
//     class defaults, or those of init() once it has been called, and the fields of find_tranfrom_of_two_mappings (:296-303) on top.
class Scene_alignment {
   public:
    float m_line_res = 0.4f;                                    // :27
    float m_plane_res = 0.4f;                                   // :28
    int pair_idx = 0;                                           // :31
    Point_cloud_registration m_pc_reg;                          // :32
    int m_para_scene_alignments_maximum_residual_block = 5000;  // :34
    int m_maximum_icp_iteration = 10;                           // :35
    float m_accepted_threshold = 0.2f;                          // :36
    int m_if_verbose_screen_printf = 1;
    int m_subsample_seed = 1;   // ll_reg_params.subsample_seed of the registrations
    int device = 0;
    int64_t initial_points = 1 << 16;  // what the handle starts with; it grows
    std::vector<Point_cloud_registration::Opt_summary> reports;  // one per registration the last call ran (<= 3)

    Scene_alignment() {}
    explicit Scene_alignment(std::string path) { init(path); }

    void set_downsample_resolution(const float &line_res, const float &plane_res)  // :55-62
    {
        m_line_res = line_res;
        m_plane_res = plane_res;
    }
    // :222-245 without the log directory: the registrar settings the loop detector aligns with (laser_mapping.hpp:896)
    void init(std::string path = std::string())
    {
        (void)path;
        registrar_init_ = 1;
        m_pc_reg.ICP_LINE = 0;
        m_pc_reg.m_max_final_cost = 20000;
        m_pc_reg.m_para_max_speed = 1000.0;
        m_pc_reg.m_para_max_angular_rate = 360 * 57.3;
        m_pc_reg.m_inliner_dis = 0.2;
    }
    // Registers key frame b (the scan) against key frame a (the map); returns m_pc_reg.m_inlier_threshold (:389)
    double find_tranfrom_of_two_mappings(Points_cloud_map *keyframe_a, Points_cloud_map *keyframe_b, int if_save = 0,
                                         std::string mapping_save_path = std::string(" "))
    {
        (void)if_save;
        (void)mapping_save_path;
        if (!keyframe_a || !keyframe_b) check(-1, "Scene_alignment::find_tranfrom_of_two_mappings: null key frame");
        if (!h_) make_handle(h_, "ll_scene_align_create", [&](ll_scene_align **out) { return ll_scene_align_create(device, initial_points, out); });
        ll_scene_align_params p;
        ll_scene_align_default_params(&p);
        p.line_res = m_line_res;
        p.plane_res = m_plane_res;
        p.maximum_icp_iteration = m_maximum_icp_iteration;
        p.accepted_threshold = m_accepted_threshold;
        p.maximum_residual_block = m_para_scene_alignments_maximum_residual_block;
        p.registrar_init = registrar_init_;
        p.subsample_seed = m_subsample_seed;
        double pose[7], thr = 0.0;
        ll_reg_report rep[3];
        int32_t n_rep = 0;
        check(ll_scene_align_run(h_.get(), keyframe_a->handle(), keyframe_b->handle(), &p, pose, &thr, rep, &n_rep), "ll_scene_align_run");
        from_pose7(pose, m_pc_reg.m_q_w_curr, m_pc_reg.m_t_w_curr);
        m_pc_reg.m_inlier_threshold = thr;
        reports.clear();
        for (int i = 0; i < n_rep; i++) reports.push_back(Point_cloud_registration::Opt_summary::from(rep[i]));
        if (n_rep > 0) m_pc_reg.summary = m_pc_reg.m_final_opt_summary = reports.back();
        pair_idx++;
        return thr;
    }
    // test tap (ll_scene_align_work) on the last call
    void work(int64_t out[4]) { check(ll_scene_align_work(h_.get(), out), "ll_scene_align_work"); }

    // :97-129: the loop constraint s_idx -> t_idx from the poses of the two key frames and the alignment's inverted transform:
    // q_res = q_b^-1 icp_q^-1 q_a, t_res = q_b^-1 ( icp_q^-1 ( t_a - icp_t ) - t_b ).  fp64 on the host, Eigen's operation order.
    static Ceres_pose_graph_3d::Constraint3d add_constrain_of_loop(int s_idx, int t_idx, Quaterniond q_a, Vector3d t_a, Quaterniond q_b, Vector3d t_b,
                                                                   Quaterniond icp_q, Vector3d icp_t, int if_verbose = 1)
    {
        (void)if_verbose;
        namespace d = Ceres_pose_graph_3d::detail;
        const double qa[4] = {q_a.x(), q_a.y(), q_a.z(), q_a.w()}, qb[4] = {q_b.x(), q_b.y(), q_b.z(), q_b.w()};
        const double qi[4] = {icp_q.x(), icp_q.y(), icp_q.z(), icp_q.w()};
        double qbi[4], qii[4], m[4], q_res[4], v[3], w[3], t_res[3];
        d::q_inverse(qb, qbi);
        d::q_inverse(qi, qii);
        d::q_mul(qbi, qii, m);
        d::q_mul(m, qa, q_res);
        for (int i = 0; i < 3; i++) v[i] = t_a(i) - icp_t(i);
        d::q_rotate(qii, v, w);
        for (int i = 0; i < 3; i++) w[i] = w[i] - t_b(i);
        d::q_rotate(qbi, w, t_res);
        Ceres_pose_graph_3d::Constraint3d c;
        c.id_begin = s_idx, c.id_end = t_idx;
        c.t_be.q.x() = q_res[0], c.t_be.q.y() = q_res[1], c.t_be.q.z() = q_res[2], c.t_be.q.w() = q_res[3];
        for (int i = 0; i < 3; i++) c.t_be.p(i) = t_res[i];
        return c;
    }

   private:
    Handle<ll_scene_align, ll_scene_align_destroy> h_;
    int registrar_init_ = 0;
};

// ------------------------------------------------------------------------------------------------------------
// Keyframe_bank: the line and plane image of every processed key frame kept on the device (ll_keyframe_bank_*), for the walk of
// service_loop_detection over the earlier key frames (laser_mapping.hpp:988-1057): add a key frame when it is analysed, then ask for
// max_similiarity_of_two_image of the new one against any number of earlier ones in ONE call.  The floats are those of
// Points_cloud_map::max_similiarity_of_two_image, bit for bit.  Ids count from 0 in the order of the adds.
class Keyframe_bank {
   public:
    explicit Keyframe_bank(int64_t initial_entries = 256, int device = 0)
    {
        make_handle(h_, "ll_keyframe_bank_create", [&](ll_keyframe_bank **out) { return ll_keyframe_bank_create(device, initial_entries, out); });
    }

    // Points_cloud_map::analyze with the same outputs; the key frame's line and plane image also become a new entry, whose id is returned
    int64_t add(Points_cloud_map &keyframe, std::vector<float> &images, float ratio_nonzero[4], float roi_ratio = 0.9f)
    {
        images.assign((size_t)4 * 60 * 60, 0.f);
        int64_t id = -1;
        check(ll_keyframe_bank_add_cellmap(h_.get(), keyframe.handle(), roi_ratio, images.data(), ratio_nonzero, nullptr, nullptr, nullptr, &id),
              "ll_keyframe_bank_add_cellmap");
        return id;
    }
    // an entry from two 60 x 60 host images
    int64_t add(const float *img_line, const float *img_plane)
    {
        int64_t id = -1;
        check(ll_keyframe_bank_add_images(h_.get(), img_line, img_plane, &id), "ll_keyframe_bank_add_images");
        return id;
    }
    int64_t size() const { return ll_keyframe_bank_size(h_.get()); }
    // sim_line[p], sim_plane[p] of ( ids_a[p] = the new key frame, ids_b[p] = the old one )
    void match(const std::vector<int64_t> &ids_a, const std::vector<int64_t> &ids_b, std::vector<float> &sim_line, std::vector<float> &sim_plane)
    {
        if (ids_a.size() != ids_b.size()) check(-1, "Keyframe_bank::match: ids_a and ids_b differ in length");
        sim_line.assign(ids_a.size(), 0.f);
        sim_plane.assign(ids_a.size(), 0.f);
        check(ll_keyframe_bank_match(h_.get(), (int64_t)ids_a.size(), ids_a.data(), ids_b.data(), sim_line.data(), sim_plane.data()), "ll_keyframe_bank_match");
    }
    // test tap (ll_keyframe_bank_work) on the last match
    void work(int64_t out[4]) { check(ll_keyframe_bank_work(h_.get(), out), "ll_keyframe_bank_work"); }
    ll_keyframe_bank *handle() { return h_.get(); }

   private:
    Handle<ll_keyframe_bank, ll_keyframe_bank_destroy> h_;
};

// ------------------------------------------------------------------------------------------------------------
// Mapping_refine (ceres_pose_graph_3d.hpp:368-538): the corrected key-frame clouds behind a closed loop, on the device
// (ll_map_refine_*).  Templated on the cloud type like VoxelGrid above (the reference's is on the point type:
// Mapping_refine< pcl::PointCloud< PointType > > here).  The clouds of map_idx_pc are uploaded as they are the first time a call meets
// them (ll_map_refine_add_stored; a key whose cloud has changed in size is uploaded again) and stay on the device for the later
// calls of the node's loop at laser_mapping.hpp:1091-1100.  if_save must be 0: the JSON dumps are out of scope.
//   refine_pointcloud   VoxelGrid at m_down_sample_res, then the centroids moved with R_opm R_ori^T (:476-485): ll_map_refine_run, mode 0
//   refine_mapping      every cloud moved, then VoxelGrid (:511-533), ONE run for all clouds (mode 1); fills m_pts_aft_refind
//   refine_pts          the affine and the move of :437-452 on the host; it takes the two poses, not their rotation matrices --
//                       toRotationMatrix is part of the arithmetic (ll_map_refine_affine)
// Output intensity is 0, as eigen_to_pcl_pt leaves it.
template <class Cloud>
class Mapping_refine {
   public:
    Ceres_pose_graph_3d::MapOfPoses pose3d_map_oir, pose3d_map_opm;
    Cloud m_pts_aft_refind;
    float m_down_sample_res = 0.2f;
    int m_step_skip = 2;

    explicit Mapping_refine(int64_t initial_points = 1 << 20, int device = 0) : initial_points_(initial_points), device_(device) {}

    void set_down_sample_resolution(float res) { m_down_sample_res = res; }
    // ( laser_mapping.hpp:902 ) kept, not used: nothing is written
    void set_save_dir(const std::string &path_name) { m_save_path = path_name; }
    std::string m_save_path;

#if defined(__clang__)
#define LOAM_LIVOX_NO_CONTRACT
#elif defined(__GNUC__)
#define LOAM_LIVOX_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define LOAM_LIVOX_NO_CONTRACT
#endif
    // V: a 3-vector of float read and written as v( i ) (Eigen::Matrix< float, 3, 1 >)
    template <class V>
    LOAM_LIVOX_NO_CONTRACT static std::vector<V> refine_pts(const std::vector<V> &raw_pt_vec, const Quaterniond &q_ori, const Vector3d &t_ori,
                                                             const Quaterniond &q_opm, const Vector3d &t_opm)
    {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        float R[9], T[3];
        double ori[7], opm[7];
        to_pose7(q_ori, t_ori, ori);
        to_pose7(q_opm, t_opm, opm);
        check(ll_map_refine_affine(ori, opm, R, T), "ll_map_refine_affine");
        std::vector<V> out(raw_pt_vec.size());
        for (size_t k = 0; k < raw_pt_vec.size(); k++) {
            const float x = raw_pt_vec[k](0), y = raw_pt_vec[k](1), z = raw_pt_vec[k](2);
            for (int i = 0; i < 3; i++) {
                const float e0 = R[3 * i] * x, e1 = R[3 * i + 1] * y, e2 = R[3 * i + 2] * z;
                out[k](i) = (e0 + (e1 + e2)) + T[i];
            }
        }
        return out;
    }

    Cloud refine_pointcloud(const std::map<int, Cloud> &map_idx_pc, const Ceres_pose_graph_3d::MapOfPoses &poses_ori,
                            const Ceres_pose_graph_3d::MapOfPoses &poses_opm, int idx = 0, int if_save = 0)
    {
        if (if_save != 0) check_arg("Mapping_refine::refine_pointcloud: if_save must be 0 (the JSON dumps are out of scope)");
        Cloud out;
        if (idx < 0 || (size_t)idx >= map_idx_pc.size()) return out;  // ( it == map_idx_pc.end(), :465-468 )
        typename std::map<int, Cloud>::const_iterator it = map_idx_pc.begin();
        std::advance(it, idx);
        std::vector<int> keys(1, it->first);
        std::vector<Cloud> got = run(0, map_idx_pc, poses_ori, poses_opm, keys);
        return got[0];
    }

    void refine_mapping(const std::map<int, Cloud> &map_idx_pc, const Ceres_pose_graph_3d::MapOfPoses &poses_ori,
                        const Ceres_pose_graph_3d::MapOfPoses &poses_opm, int if_save = 0)
    {
        if (if_save != 0) check_arg("Mapping_refine::refine_mapping: if_save must be 0 (the JSON dumps are out of scope)");
        std::vector<int> keys;
        for (Ceres_pose_graph_3d::MapOfPoses::const_iterator it = poses_ori.begin(); it != poses_ori.end(); ++it) keys.push_back(it->first);  // :512
        std::vector<Cloud> got = run(1, map_idx_pc, poses_ori, poses_opm, keys);
        for (size_t k = 0; k < got.size(); k++) m_pts_aft_refind.points.insert(m_pts_aft_refind.points.end(), got[k].points.begin(), got[k].points.end());  // :533
    }

    // :577-578 over the last refine_mapping / refine_pointcloud outputs still on the device: VoxelGrid of them as one cloud
    Cloud merge_last()
    {
        Cloud out;
        if (!h_) return out;
        int64_t n = 0;
        check(ll_map_refine_merge(h_.get(), m_down_sample_res, &n, nullptr), "ll_map_refine_merge");
        read_cloud("ll_map_refine_fetch_merged", out,
                   [&](float *xyzi, int64_t capacity) { return xyzi ? (int64_t)ll_map_refine_fetch_merged(h_.get(), xyzi, capacity) : n; });
        return out;
    }
    // ll_map_refine_add_logged: request r is the concatenation of the logged scans of groups_per_request[r] (ids of
    // History_batch::hand_over), filtered at `leaf` into the store, device to device; the groups are consumed.  Returns the store's ids
    // (for ll_map_refine_run on handle()); n_kept and status when given.
    std::vector<int64_t> add_logged(History_batch &batch, const std::vector<std::vector<int64_t> > &groups_per_request, float leaf,
                                    std::vector<int64_t> *n_kept = nullptr, std::vector<int32_t> *status = nullptr)
    {
        ensure();
        const size_t R = groups_per_request.size();
        const std::vector<int64_t> off = csr_offsets(groups_per_request);
        std::vector<int64_t> gids, ids(R > 0 ? R : 1, -1), kept(R > 0 ? R : 1, 0);
        std::vector<int32_t> st(R > 0 ? R : 1, 0);
        for (size_t r = 0; r < R; r++) gids.insert(gids.end(), groups_per_request[r].begin(), groups_per_request[r].end());
        check(ll_map_refine_add_logged(h_.get(), batch.handle(), (int64_t)R, off.data(), gids.empty() ? nullptr : gids.data(), leaf, ids.data(), kept.data(),
                                       st.data()),
              "ll_map_refine_add_logged");
        ids.resize(R), kept.resize(R), st.resize(R);
        if (n_kept) *n_kept = kept;
        if (status) *status = st;
        return ids;
    }
    // test tap (ll_map_refine_work) on the last run and its fetch
    void work(int64_t out[4]) { check(ll_map_refine_work(h_.get(), out), "ll_map_refine_work"); }
    ll_map_refine *handle() { return h_.get(); }

   private:
    static void check_arg(const char *what) { throw std::runtime_error(what); }
    void ensure()  // the handle is made by the first call that needs it
    {
        if (!h_) make_handle(h_, "ll_map_refine_create", [&](ll_map_refine **out) { return ll_map_refine_create(device_, initial_points_, out); });
    }

    int64_t stored_id(int key, const Cloud &c)
    {
        std::map<int, std::pair<int64_t, size_t> >::const_iterator it = ids_.find(key);
        if (it != ids_.end() && it->second.second == c.points.size()) return it->second.first;
        const std::vector<float> v = cloud_to_xyzi(c);
        int64_t id = -1;
        check(ll_map_refine_add_stored(h_.get(), v.empty() ? nullptr : v.data(), (int64_t)c.points.size(), &id), "ll_map_refine_add_stored");
        ids_[key] = std::make_pair(id, c.points.size());
        return id;
    }

    std::vector<Cloud> run(int mode, const std::map<int, Cloud> &map_idx_pc, const Ceres_pose_graph_3d::MapOfPoses &poses_ori,
                           const Ceres_pose_graph_3d::MapOfPoses &poses_opm, const std::vector<int> &keys)
    {
        if (map_idx_pc.size() != poses_ori.size() || map_idx_pc.size() != poses_opm.size())   // ( the asserts of :461-462, :508-509 )
            check_arg("Mapping_refine: map_idx_pc, poses_ori and poses_opm differ in size");
        ensure();
        std::vector<int64_t> ids;
        std::vector<double> ori, opm;
        for (size_t k = 0; k < keys.size(); k++) {
            typename std::map<int, Cloud>::const_iterator pc = map_idx_pc.find(keys[k]);
            Ceres_pose_graph_3d::MapOfPoses::const_iterator a = poses_ori.find(keys[k]), b = poses_opm.find(keys[k]);
            if (pc == map_idx_pc.end() || a == poses_ori.end() || b == poses_opm.end()) check_arg("Mapping_refine: an id is missing from a map");
            ids.push_back(stored_id(keys[k], pc->second));
            double ra[7], rb[7];
            to_pose7(a->second.q, a->second.p, ra);
            to_pose7(b->second.q, b->second.p, rb);
            ori.insert(ori.end(), ra, ra + 7);
            opm.insert(opm.end(), rb, rb + 7);
        }
        std::vector<int64_t> offsets(keys.size() + 1, 0);
        std::vector<int32_t> status(keys.size() + 1, 0);
        check(ll_map_refine_run(h_.get(), mode, (int64_t)keys.size(), ids.data(), ori.data(), opm.data(), m_down_sample_res, offsets.data(), status.data()),
              "ll_map_refine_run");
        const std::vector<float> v = read_xyzi("ll_map_refine_fetch", [&](float *xyzi, int64_t capacity) {
            return xyzi ? (int64_t)ll_map_refine_fetch(h_.get(), xyzi, capacity) : offsets.back();
        });
        std::vector<Cloud> out(keys.size());
        for (size_t k = 0; k < keys.size(); k++) xyzi_to_cloud(v.data() + 4 * offsets[k], (int)(offsets[k + 1] - offsets[k]), out[k]);
        return out;
    }

    int64_t initial_points_;
    int device_;
    Handle<ll_map_refine, ll_map_refine_destroy> h_;
    std::map<int, std::pair<int64_t, size_t> > ids_;  // key of map_idx_pc -> (id in the store, points it had when uploaded)
};

}  // namespace loam_livox_hip
