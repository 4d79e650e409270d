// CPU tier of include/loam_livox_adapter.hpp, ownership: every class that owns an ll_* handle is constructed, used, move-constructed,
// move-assigned over a live object and destroyed against the recording stand-in, which counts every handle's create and destroy.
// Exits 0, or prints what failed.  Also built with -fsanitize=address,undefined.  -DLOAM_LIVOX_ADAPTER_NO_EIGEN: the header's own pose types.
#include "adapter_standin.cpp"

#include <type_traits>

#include "loam_livox_adapter.hpp"

namespace ll = loam_livox_hip;
namespace pg = loam_livox_hip::Ceres_pose_graph_3d;

struct Pt {
    float x, y, z, intensity;
};
struct Cloud {
    std::vector<Pt> points;
};
static Cloud cloud(int n)
{
    Cloud c;
    for (int i = 0; i < n; i++) c.points.push_back(Pt{(float)i, i + 0.5f, (float)-i, 0.125f * i});
    return c;
}

static int failures = 0;
#define CHECK(cond) \
    if (!(cond)) failures++, std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond)

// owners move and do not copy (Livox_laser included: the reference's call sites keep one as a member and never copy it)
template <class T>
constexpr bool moves_only()
{
    return !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value && std::is_move_constructible<T>::value &&
           std::is_move_assignable<T>::value;
}
static_assert(moves_only<ll::Livox_laser>(), "Livox_laser");
static_assert(moves_only<ll::Spinning_laser>(), "Spinning_laser");
static_assert(moves_only<ll::History_buffer>(), "History_buffer");
static_assert(moves_only<ll::History_batch>(), "History_batch");
static_assert(moves_only<ll::Points_cloud_map>(), "Points_cloud_map");
static_assert(moves_only<ll::Scene_alignment>(), "Scene_alignment");
static_assert(moves_only<ll::Keyframe_bank>(), "Keyframe_bank");
static_assert(moves_only<ll::Mapping_refine<Cloud>>(), "Mapping_refine");
static_assert(moves_only<ll::Handle<ll_fe, ll_fe_destroy>>(), "Handle");
static_assert(std::is_copy_constructible<ll::VoxelGrid<Cloud>>::value && std::is_copy_constructible<ll::Point_cloud_registration>::value,
              "the two classes the node copies");

template <class F>
static std::string thrown_by(F f)
{
    try {
        f();
    } catch (const std::runtime_error &e) {
        return e.what();
    }
    return "";
}
static bool refused(const std::string &what) { return what.find("null handle") != std::string::npos; }
static int alive()  // handles created and not yet destroyed, the pool's aside
{
    int n = 0;
    for (const auto &kv : standin::handles())
        if (kv.second.created > kv.second.destroyed && kv.second.name.compare(0, 4, "reg#") && kv.second.name.compare(0, 4, "map#")) n++;
    return n;
}

// construct (make), use once, move-construct, move-assign over a live object, a call on the moved-from object, destroy
template <class T, class Make, class Use>
static void owner(const char *name, Make make, Use use, bool lazy)
{
    const int before = alive();
    {
        T a = make();
        use(a);
        CHECK(alive() == before + 1);
        T b(std::move(a));
        CHECK(alive() == before + 1);
        const std::string why = thrown_by([&] { use(a); });
        if (lazy) {  // a moved-from object whose handle is made on first use makes a new one
            CHECK(why.empty() && alive() == before + 2);
        } else {
            CHECK(refused(why));
        }
        use(b);
        T c = make();
        use(c);
        const int with_c = alive();
        c = std::move(b);  // what c held is destroyed
        CHECK(alive() == with_c - 1);
        use(c);
        if (!lazy) CHECK(refused(thrown_by([&] { use(b); })));
    }
    CHECK(alive() == before);
    if (alive() != before) std::fprintf(stderr, "  (%s)\n", name);
}

int main()
{
    Cloud out, five = cloud(5);
    owner<ll::Livox_laser>("Livox_laser", [] { return ll::Livox_laser(); }, [&](ll::Livox_laser &x) { Cloud in; x.extract_laser_features(in); }, true);
    owner<ll::Spinning_laser>("Spinning_laser", [] { return ll::Spinning_laser(); }, [&](ll::Spinning_laser &x) { x.extract_device(five); }, true);
    owner<ll::History_buffer>("History_buffer", [] { return ll::History_buffer(4, 100, 0.4f, 0.8f); }, [&](ll::History_buffer &x) { x.map_cloud(0, out); }, false);
    owner<ll::History_batch>("History_batch", [] { return ll::History_batch(2, 4, 100, 0.4f, 0.8f); }, [&](ll::History_batch &x) { x.map_cloud(1, 0, out); },
                             false);
    owner<ll::Points_cloud_map>("Points_cloud_map", [] { return ll::Points_cloud_map(100); }, [&](ll::Points_cloud_map &x) { x.get_cells_size(); }, false);
    owner<ll::Keyframe_bank>("Keyframe_bank", [] { return ll::Keyframe_bank(8); }, [&](ll::Keyframe_bank &x) { int64_t w[4]; x.work(w); }, false);
    {
        ll::Points_cloud_map ka(100), kb(100);
        owner<ll::Scene_alignment>("Scene_alignment", [] { return ll::Scene_alignment(); }, [&](ll::Scene_alignment &x) { x.find_tranfrom_of_two_mappings(&ka, &kb); },
                                   true);
        ll::History_batch batch(2, 4, 100, 0.4f, 0.8f);
        owner<ll::Mapping_refine<Cloud>>("Mapping_refine", [] { return ll::Mapping_refine<Cloud>(1 << 10); },
                                         [&](ll::Mapping_refine<Cloud> &x) { x.add_logged(batch, {{1}}, 0.2f); }, true);
        // moved-from objects that make no handle of their own in the call: refused
        ll::Scene_alignment sa, sb(std::move(sa));
        int64_t w[4];
        CHECK(refused(thrown_by([&] { sa.work(w); })));
        ll::Mapping_refine<Cloud> ma(1 << 10), mb(std::move(ma));
        CHECK(refused(thrown_by([&] { ma.work(w); })));
        ll::Livox_laser la;
        la.extract_laser_features(out);
        ll::Livox_laser lb(std::move(la));
        CHECK(refused(thrown_by([&] { la.get_features(out, out, out); })));
    }
    CHECK(alive() == 0);

    // VoxelGrid: a copy takes the configuration and makes its own handle on first use
    {
        ll::VoxelGrid<Cloud> a;
        a.setLeafSize(0.5f, 0.5f, 0.5f);
        a.setInputCloud(&five);
        a.filter(out);
        CHECK(alive() == 1 && out.points.size() == 5);
        ll::VoxelGrid<Cloud> b(a);
        CHECK(alive() == 1);  // nothing yet
        b.setInputCloud(&five);
        b.filter(out);
        CHECK(alive() == 2 && standin::made()["voxel"] == 2);
        CHECK(standin::log().back().find("f32[3]{0.5 0.5 0.5}") != std::string::npos);  // ... with the leaf of the source
        a = b;
        a.setInputCloud(&five);
        a.filter(out);
        CHECK(alive() == 2 && standin::made()["voxel"] == 2);  // an assignment leaves both handles where they are
    }
    CHECK(alive() == 0);

    // pose_graph_optimization: the handle goes on both ways out
    {
        pg::MapOfPoses poses;
        pg::VectorOfConstraints constraints;
        poses[0] = pg::Pose3d(), poses[1] = pg::Pose3d();
        constraints.push_back(pg::Constraint3d(0, 1, poses[0].q, poses[1].p));
        pg::pose_graph_optimization(poses, constraints);
        CHECK(alive() == 0 && standin::made()["pose_graph"] == 1 && poses[1].p(0) == 1.0);
        standin::size()["ll_pose_graph_solve"] = -1;
        const std::string why = thrown_by([&] { pg::pose_graph_optimization(poses, constraints); });
        CHECK(why == "ll_pose_graph_solve: ll_pose_graph_solve: the stand-in was told to fail");
        CHECK(alive() == 0 && standin::made()["pose_graph"] == 2);
    }

    // History_buffer::map_cloud and the batched one on a negative count: both throw
    {
        ll::History_buffer h(4, 100, 0.4f, 0.8f);
        ll::History_batch hb(2, 4, 100, 0.4f, 0.8f);
        standin::size()["ll_history_map_cloud"] = standin::size()["ll_history_batch_map_cloud"] = -1;
        Cloud kept = cloud(2);
        CHECK(thrown_by([&] { h.map_cloud(0, kept); }) == "ll_history_map_cloud: ll_history_map_cloud: the stand-in was told to fail");
        CHECK(thrown_by([&] { hb.map_cloud(0, 0, kept); }) == "ll_history_batch_map_cloud: ll_history_batch_map_cloud: the stand-in was told to fail");
        CHECK(kept.points.size() == 2);
    }

    // Point_cloud_registration: a copy has every public field, views of its own buffer, and a registrar of its own
    {
        const std::shared_ptr<Cloud> scan(new Cloud(five));
        int logger = 0;
        ll::Point_cloud_registration a;
        a.ICP_PLANE = 0, a.ICP_LINE = 0, a.IF_LINE_FEATURE_CHECK = 1, a.IF_PLANE_FEATURE_CHECK = 1, a.line_search_num = 4, a.plane_search_num = 3;
        a.m_if_motion_deblur = 0, a.m_current_frame_index = 9, a.m_mapping_init_accumulate_frames = 8, a.m_last_time_stamp = 7, a.m_para_max_angular_rate = 6;
        a.m_para_max_speed = 5, a.m_max_final_cost = 4, a.m_para_icp_max_iterations = 3, a.m_para_cere_max_iterations = 2, a.m_para_cere_prerun_times = 1;
        a.m_minimum_pt_time_stamp = 0.5f, a.m_maximum_pt_time_stamp = 0.75f, a.m_minimum_icp_R_diff = 0.1, a.m_minimum_icp_T_diff = 0.2, a.m_inliner_dis = 0.3;
        a.m_inlier_ratio = 0.4, a.m_maximum_dis_plane_for_match = 0.6, a.m_maximum_dis_line_for_match = 0.7, a.m_maximum_allow_residual_block = 11;
        a.m_subsample_seed = 12, a.m_if_verbose_screen_printf = 0, a.device = 0, a.max_features = 13;
        a.m_logger_common = &logger, a.m_logger_pcd = &logger, a.m_logger_timer = &logger, a.m_timer = &logger;
        a.m_q_w_last.x() = 0.5, a.m_t_w_last(1) = 2.5;
        a.find_out_incremental_transfrom(scan, scan);  // fills the buffers, the poses, the summaries; borrows a registrar
        const int lent = standin::made()["reg"];
        ll::Point_cloud_registration b(a), c;
        c = a;
        for (ll::Point_cloud_registration *x : {&b, &c}) {
            CHECK(x->ICP_PLANE == 0 && x->ICP_LINE == 0 && x->IF_LINE_FEATURE_CHECK == 1 && x->IF_PLANE_FEATURE_CHECK == 1 && x->line_search_num == 4 &&
                  x->plane_search_num == 3);
            CHECK(x->m_if_motion_deblur == 0 && x->m_current_frame_index == 9 && x->m_mapping_init_accumulate_frames == 8 && x->m_last_time_stamp == a.m_last_time_stamp &&
                  x->m_para_max_angular_rate == 6 && x->m_para_max_speed == 5 && x->m_max_final_cost == 4);
            CHECK(x->m_para_icp_max_iterations == 3 && x->m_para_cere_max_iterations == 2 && x->m_para_cere_prerun_times == 1 && x->m_minimum_pt_time_stamp == 0.5f &&
                  x->m_maximum_pt_time_stamp == 0.75f);
            CHECK(x->m_minimum_icp_R_diff == 0.1 && x->m_minimum_icp_T_diff == 0.2 && x->m_inliner_dis == 0.3 && x->m_inlier_ratio == 0.4 &&
                  x->m_maximum_dis_plane_for_match == 0.6 && x->m_maximum_dis_line_for_match == 0.7);
            CHECK(x->m_maximum_allow_residual_block == 11 && x->m_subsample_seed == 12 && x->m_if_verbose_screen_printf == 0 && x->device == 0 && x->max_features == 13);
            CHECK(x->m_logger_common.p == &logger && x->m_logger_pcd.p == &logger && x->m_logger_timer.p == &logger && x->m_timer.p == &logger);
            CHECK(!std::memcmp(x->m_para_buffer_RT, a.m_para_buffer_RT, 56) && !std::memcmp(x->m_para_buffer_RT_last, a.m_para_buffer_RT_last, 56) &&
                  !std::memcmp(x->m_para_buffer_incremental, a.m_para_buffer_incremental, 56));
            CHECK(a.m_para_buffer_RT[4] == 1.0 && a.m_para_buffer_RT_last[0] == 0.5 && a.m_para_buffer_incremental[5] == 1.0);  // (they were filled)
            double pa[7], px[7];
            ll::to_pose7(a.m_q_w_curr, a.m_t_w_curr, pa), ll::to_pose7(x->m_q_w_curr, x->m_t_w_curr, px);
            CHECK(!std::memcmp(pa, px, 56) && pa[5] == 2.0);
            ll::to_pose7(a.m_q_w_last, a.m_t_w_last, pa), ll::to_pose7(x->m_q_w_last, x->m_t_w_last, px);
            CHECK(!std::memcmp(pa, px, 56) && pa[0] == 0.5 && pa[5] == 2.5);
            CHECK(x->m_inlier_threshold == 0.125 && x->m_angular_diff == 0.5 && x->m_t_diff == 0.75);
            CHECK(x->summary.num_residual_blocks == 11 && x->summary.final_cost == 0.25 && x->m_final_opt_summary.num_residual_blocks == 11 &&
                  x->m_final_opt_summary.lm_iterations_total == 17);
            // the views read and write this object's own increment
            ll::to_pose7(x->m_q_w_incre, x->m_t_w_incre, px);
            CHECK(!std::memcmp(px, x->m_para_buffer_incremental, 56));
            x->m_t_w_incre(0) = 40.0 + (x == &c);
            CHECK(x->m_para_buffer_incremental[4] == 40.0 + (x == &c) && a.m_para_buffer_incremental[4] == 0.5);
        }
        CHECK(standin::made()["reg"] == lent);  // copying borrows nothing ...
        b.find_out_incremental_transfrom(scan, scan);
        CHECK(standin::made()["reg"] == lent + 1);  // ... the copy's first use does, while the source keeps its own
        CHECK(standin::log()[standin::log().size() - 1].find("ll_reg_collect(reg#" + std::to_string(lent)) == 0);
        a.find_out_incremental_transfrom(scan, scan);
        CHECK(standin::log().back().find("ll_reg_collect(reg#" + std::to_string(lent - 1)) == 0);
    }
    // the pool got back every registrar it lent: as many objects as it ever made registrars are served without a new one
    {
        const std::shared_ptr<Cloud> scan(new Cloud(five));
        const int lent = standin::made()["reg"];
        CHECK(lent == 2);
        std::vector<ll::Point_cloud_registration> regs((size_t)lent);
        for (ll::Point_cloud_registration &r : regs) r.max_features = 13, r.find_out_incremental_transfrom(scan, scan);
        CHECK(standin::made()["reg"] == lent);
        ll::Point_cloud_registration one_more;
        one_more.max_features = 13;
        one_more.find_out_incremental_transfrom(scan, scan);
        CHECK(standin::made()["reg"] == lent + 1);  // (and the count does tell: one more object at the same time needs one more)
    }

    std::string which;
    CHECK(standin::leaked(&which) == 0);
    if (!which.empty()) std::fprintf(stderr, "handles not destroyed exactly once: %s\n", which.c_str());
    if (failures) return 1;
    std::printf("ok: %d handles created, each destroyed once\n", (int)standin::handles().size());
    return 0;
}
