// CPU tier of include/loam_livox_adapter.hpp, calls: every method that goes through one of the header's shared helpers, run against the
// recording stand-in on clouds of 0, 1 and 5 points.  The stand-in's log and what the methods return go to stdout, one line each, and
// tests/test_adapter_calls_host.py compares them with tests/adapter_calls.txt, recorded with the header of the commit before the
// helpers existed.  Built with -DLOAM_LIVOX_ADAPTER_NO_EIGEN: the header's own pose types.
#include "adapter_standin.cpp"

#include "loam_livox_adapter.hpp"

namespace ll = loam_livox_hip;
namespace pg = loam_livox_hip::Ceres_pose_graph_3d;

struct Pt {
    float x, y, z, intensity;
};
struct Cloud {
    std::vector<Pt> points;
};
struct Pt8 {  // pcl::PointXYZI's layout: x, y, z consecutive, 8 floats per point
    float x, y, z, pad, intensity, a, b, c;
};
struct Cloud8 {
    std::vector<Pt8> points;
};
struct Pt_apart {  // coordinates that do not lie side by side: the staging copy of upload_if_changed
    float x, intensity, y, z;
};
struct Cloud_apart {
    std::vector<Pt_apart> points;
};
struct Kd {};

static const int SIZES[3] = {0, 1, 5};

template <class C>
static C cloud(int n, float base = 0.0f)
{
    C c;
    c.points.resize((size_t)n);
    for (int i = 0; i < n; i++) c.points[i].x = base + i, c.points[i].y = base + i + 0.5f, c.points[i].z = base - i, c.points[i].intensity = 0.125f * i;
    return c;
}
static void note(const std::string &s) { standin::log().push_back(s); }
static void title(const std::string &s) { note("== " + s); }
template <class C>
static std::string show(const C &c)
{
    const std::vector<float> v = ll::cloud_to_xyzi(c);
    return v.empty() ? "cloud f32[0]" : "cloud " + standin::arr("f32", v.data(), (int64_t)v.size());
}
template <class T>
static std::string show(const std::vector<T> &v)
{
    return v.empty() ? "v[0]" : standin::arr("v", v.data(), (int64_t)v.size());
}
static std::string pose(const ll::Quaterniond &q, const ll::Vector3d &t)
{
    const double p[7] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2)};
    return standin::arr("pose", p, 7);
}
static std::string state(ll::Point_cloud_registration &r)
{
    return "-> curr " + pose(r.m_q_w_curr, r.m_t_w_curr) + " incre " + standin::arr("f64", r.m_para_buffer_incremental, 7) + " threshold " +
           standin::num(r.m_inlier_threshold) + " diffs " + standin::num(r.m_angular_diff) + " " + standin::num(r.m_t_diff) + " blocks " +
           std::to_string(r.summary.num_residual_blocks) + " " + std::to_string(r.m_final_opt_summary.num_residual_blocks) + " cost " +
           standin::num(r.summary.final_cost);
}

static void readers()
{
    ll::History_buffer hist(4, 100, 0.4f, 0.8f);
    ll::History_batch batch(2, 4, 100, 0.4f, 0.8f);
    ll::Points_cloud_map map(1000);
    for (int n : SIZES) {
        title("History_buffer::map_cloud, " + std::to_string(n) + " points");
        standin::size()["ll_history_map_cloud"] = n;
        Cloud c = cloud<Cloud>(3);
        hist.map_cloud(1, c);
        note("-> " + show(c));
        title("History_batch::map_cloud, " + std::to_string(n) + " points");
        standin::size()["ll_history_batch_map_cloud"] = n;
        batch.map_cloud(1, 0, c);
        note("-> " + show(c));
        title("History_batch::read_group, " + std::to_string(n) + " points");
        standin::size()["ll_history_batch_scan_log_read"] = n;
        note("-> " + show(batch.read_group(42)));
        title("Points_cloud_map::find_cells_in_radius_filtered, " + std::to_string(n) + " points");
        standin::size()["ll_cellmap_result"] = n;
        const double at[7] = {0, 0, 0, 1, 1, 2, 3};
        map.find_cells_in_radius_filtered(at, 10.0f, 0.4f, c);
        note("-> " + show(c));
    }
    const int lines_planes[3][2] = {{0, 0}, {1, 5}, {5, 0}};
    for (const int *lp : lines_planes) {
        title("Points_cloud_map::extract_specify_points, " + std::to_string(lp[0]) + " line and " + std::to_string(lp[1]) + " plane points");
        standin::size()["n_line"] = lp[0], standin::size()["n_plane"] = lp[1];
        note("-> line " + show(map.extract_specify_points<Cloud>(ll::Points_cloud_map::e_feature_line)));
        note("-> plane " + show(map.extract_specify_points<Cloud>(ll::Points_cloud_map::e_feature_plane)));
    }
}

static std::vector<std::array<int, 3>> cells(int n, int base)
{
    std::vector<std::array<int, 3>> c;
    for (int i = 0; i < n; i++) c.push_back(std::array<int, 3>{{base + i, -i, 2 * i}});
    return c;
}

static void cell_lists()
{
    ll::Points_cloud_map src(1000), a(10), b(10), c(10);
    ll::History_batch batch(3, 4, 100, 0.4f, 0.8f);
    for (int n : SIZES) {
        title("Points_cloud_map::extract_cells, " + std::to_string(n) + " cells");
        int64_t n_points = -1;
        const int64_t found = src.extract_cells(cells(n, 7), a, &n_points);
        note("-> found " + std::to_string(found) + " points " + std::to_string(n_points));
    }
    title("History_batch::extract_cells, no request");
    std::vector<int64_t> n_points(1, -1);
    std::vector<int64_t> found = batch.extract_cells<ll::Points_cloud_map>(2, {}, {}, {}, &n_points);
    note("-> found " + show(found) + " points " + show(n_points));
    title("History_batch::extract_cells, lists of 5, 0 and 1 cells");
    found = batch.extract_cells<ll::Points_cloud_map>(2, {2, 0, 1}, {cells(5, 1), cells(0, 0), cells(1, -9)}, {&a, &b, &c}, &n_points);
    note("-> found " + show(found) + " points " + show(n_points));
}

static void map_refine()
{
    ll::History_batch batch(3, 4, 100, 0.4f, 0.8f);
    {
        ll::Mapping_refine<Cloud> first_is_add_logged(1 << 10);
        title("Mapping_refine::merge_last before any call");
        note("-> " + show(first_is_add_logged.merge_last()));
        title("Mapping_refine::add_logged, no request");
        std::vector<int64_t> kept;
        std::vector<int32_t> status;
        std::vector<int64_t> ids = first_is_add_logged.add_logged(batch, {}, 0.2f, &kept, &status);
        note("-> ids " + show(ids) + " kept " + show(kept) + " status " + show(status));
        title("Mapping_refine::add_logged, requests of 0, 1 and 5 groups");
        ids = first_is_add_logged.add_logged(batch, {{}, {7}, {1, 2, 3, 4, 5}}, 0.2f, &kept, &status);
        note("-> ids " + show(ids) + " kept " + show(kept) + " status " + show(status));
    }
    std::map<int, Cloud> clouds;
    pg::MapOfPoses ori, opm;
    for (int k = 0; k < 3; k++) {
        clouds[10 + k] = cloud<Cloud>(SIZES[k], 100.0f * k);
        ori[10 + k].p(0) = k, ori[10 + k].q.x() = 0.5 * k;
        opm[10 + k].p(1) = -k, opm[10 + k].q.w() = 1.0 - 0.25 * k;
    }
    ll::Mapping_refine<Cloud> mr(1 << 10);
    mr.set_down_sample_resolution(0.3f);
    for (int n : SIZES) {
        standin::size()["ll_map_refine_run"] = n;
        title("Mapping_refine::refine_pointcloud, an output of " + std::to_string(n) + " points");
        note("-> " + show(mr.refine_pointcloud(clouds, ori, opm, 2)));
        title("Mapping_refine::refine_mapping, outputs of " + std::to_string(n) + " points");
        mr.m_pts_aft_refind.points.clear();
        mr.refine_mapping(clouds, ori, opm);
        note("-> " + show(mr.m_pts_aft_refind));
        title("Mapping_refine::merge_last, " + std::to_string(n) + " points");
        standin::size()["ll_map_refine_merge"] = n;
        note("-> " + show(mr.merge_last()));
    }
    title("Mapping_refine::refine_pointcloud past the end");
    note("-> " + show(mr.refine_pointcloud(clouds, ori, opm, 3)));
}

static void spinning()
{
    standin::size()["ll_spin_default_params"] = 4;  // the library's default capacity: the scan of 5 points does not fit
    ll::Spinning_laser spin, spin_device;
    for (int n : SIZES) {
        title("Spinning_laser::extract, " + std::to_string(n) + " points");
        standin::size()["ll_spin_cloud"] = n > 4 ? 4 : n;
        Cloud out[5];
        spin.extract(cloud<Cloud>(n), out[0], out[1], out[2], out[3], out[4]);
        for (const Cloud &c : out) note("-> " + show(c));
        note("-> capacity " + std::to_string(spin.capacity()));
        title("Spinning_laser::extract_device, " + std::to_string(n) + " points");
        const int status = spin_device.extract_device(cloud<Cloud>(n));
        note("-> status " + std::to_string(status) + " capacity " + std::to_string(spin_device.capacity()));
    }
    title("Spinning_laser::extract_device, a line overflows");
    standin::size()["ll_spin_extract"] = LL_SPIN_STATUS_LINE_OVERFLOW;
    note("-> status " + std::to_string(spin_device.extract_device(cloud<Cloud>(1))));
    title("Spinning_laser::extract, a line overflows");
    try {
        Cloud out[5];
        spin.extract(cloud<Cloud>(1), out[0], out[1], out[2], out[3], out[4]);
        note("-> no exception");
    } catch (const std::runtime_error &e) {
        note(std::string("-> throws: ") + e.what());
    }
    standin::size()["ll_spin_extract"] = 0;
}

static void loop_closure()
{
    ll::Points_cloud_map a(100), b(100);
    ll::Scene_alignment sa;
    title("Scene_alignment::find_tranfrom_of_two_mappings");
    const double thr = sa.find_tranfrom_of_two_mappings(&a, &b);
    note("-> threshold " + standin::num(thr) + " pose " + pose(sa.m_pc_reg.m_q_w_curr, sa.m_pc_reg.m_t_w_curr) + " reports " + std::to_string(sa.reports.size()) +
         " blocks " + std::to_string(sa.reports[0].num_residual_blocks) + " " + std::to_string(sa.reports[1].num_residual_blocks) + " summary " +
         std::to_string(sa.m_pc_reg.summary.num_residual_blocks) + " " + std::to_string(sa.m_pc_reg.m_final_opt_summary.num_residual_blocks) + " pair_idx " +
         std::to_string(sa.pair_idx));
    title("Scene_alignment::find_tranfrom_of_two_mappings after init()");
    sa.init();
    sa.find_tranfrom_of_two_mappings(&a, &b);

    for (int n : SIZES) {
        title("pose_graph_optimization, " + std::to_string(n) + " poses");
        pg::MapOfPoses poses;
        pg::VectorOfConstraints constraints;
        for (int k = 0; k < n; k++) {
            pg::Pose3d &p = poses[3 * k + 1];
            p.q.x() = 0.1 * k, p.q.y() = -0.2 * k, p.q.z() = 0.3, p.q.w() = 0.9, p.p(0) = k, p.p(1) = 2 * k, p.p(2) = -k;
        }
        for (int k = 0; k + 1 < n; k++) constraints.push_back(pg::Constraint3d(3 * k + 1, 3 * k + 4, poses[1].q, poses[3 * k + 4].p));
        if (n > 2) {
            constraints.push_back(pg::Constraint3d(3 * (n - 1) + 1, 1, poses[4].q, poses[4].p));  // the loop
            constraints.back().information(2, 3) = 0.5;
        }
        const ll_pose_graph_summary s = pg::pose_graph_optimization(poses, constraints);
        std::string got = "-> termination " + std::to_string(s.termination) + " iterations " + std::to_string(s.iterations);
        for (const auto &kv : poses) got += " " + std::to_string(kv.first) + ":" + pose(kv.second.q, kv.second.p);
        note(got);
    }
}

static void registration()
{
    const std::shared_ptr<Cloud> map_corner(new Cloud(cloud<Cloud>(5, 10.0f))), map_surf(new Cloud(cloud<Cloud>(5, 20.0f)));
    Kd kd;
    ll::Point_cloud_registration reg;
    reg.m_t_w_curr(0) = 1.0, reg.m_q_w_last.x() = 0.5, reg.m_para_icp_max_iterations = 7, reg.m_current_frame_index = 3;
    for (int n : SIZES) {
        title("find_out_incremental_transfrom with map clouds, scans of " + std::to_string(n) + " and " + std::to_string(5 - n) +
              " points" + (n ? ", the map unchanged" : ""));
        const std::shared_ptr<Cloud> corner(new Cloud(cloud<Cloud>(n))), surf(new Cloud(cloud<Cloud>(5 - n, 3.0f)));
        const int ret = n == 1 ? reg.find_out_incremental_transfrom(map_corner, map_surf, kd, kd, corner, surf)
                               : reg.find_out_incremental_transfrom(map_corner, map_surf, corner, surf);
        note("-> " + std::to_string(ret) + " " + state(reg));
    }
    const std::shared_ptr<Cloud> scan(new Cloud(cloud<Cloud>(5)));
    title("find_out_incremental_transfrom with map clouds, an empty corner map and a changed surface map");
    const std::shared_ptr<Cloud> none(new Cloud), changed(new Cloud(cloud<Cloud>(5, 20.5f)));
    reg.find_out_incremental_transfrom(none, changed, scan, scan);
    title("find_out_incremental_transfrom with map clouds of 8 floats per point");
    {
        const std::shared_ptr<Cloud8> m8(new Cloud8(cloud<Cloud8>(5, 30.0f))), s8(new Cloud8(cloud<Cloud8>(1)));
        reg.find_out_incremental_transfrom(m8, m8, s8, s8);
    }
    title("find_out_incremental_transfrom with map clouds whose coordinates lie apart");
    {
        const std::shared_ptr<Cloud_apart> ma(new Cloud_apart(cloud<Cloud_apart>(5, 40.0f))), sa(new Cloud_apart(cloud<Cloud_apart>(1)));
        reg.find_out_incremental_transfrom(ma, ma, sa, sa);
    }
    for (int n : SIZES) {
        title("find_out_incremental_transfrom against map(), scans of " + std::to_string(n) + " points");
        const std::shared_ptr<Cloud> s(new Cloud(cloud<Cloud>(n)));
        ll::Point_cloud_registration fresh;  // a registrar per scan, as the node makes them: borrowed from the pool
        const int ret = fresh.find_out_incremental_transfrom(s, s);
        note("-> " + std::to_string(ret) + " " + state(fresh));
    }
    ll::Spinning_laser spin;
    spin.max_points = 8;
    spin.extract_device(cloud<Cloud>(5));
    title("find_out_incremental_transfrom( spin )");
    reg.max_features = 4;
    int ret = reg.find_out_incremental_transfrom(spin);
    note("-> " + std::to_string(ret) + " " + state(reg));
    title("find_out_incremental_transfrom( spin ), a registrar that is too small goes back to the pool");
    ll::Point_cloud_registration small;
    small.max_features = 2;
    small.find_out_incremental_transfrom(scan, scan);
    ret = small.find_out_incremental_transfrom(spin);
    note("-> " + std::to_string(ret) + " " + state(small));
    for (int n : SIZES) {
        title("pointcloudAssociateToMap, " + std::to_string(n) + " points");
        Cloud out = cloud<Cloud>(2);
        const unsigned int m = reg.pointcloudAssociateToMap(cloud<Cloud>(n), out);
        note("-> " + std::to_string(m) + " " + show(out));
    }
}

int main()
{
    readers();
    cell_lists();
    map_refine();
    spinning();
    loop_closure();
    registration();
    for (const std::string &l : standin::log()) std::printf("%s\n", l.c_str());
    std::string which;
    if (standin::leaked(&which)) {
        std::fprintf(stderr, "handles not destroyed exactly once: %s\n", which.c_str());
        return 1;
    }
    return 0;
}
