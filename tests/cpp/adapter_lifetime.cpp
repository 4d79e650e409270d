// GPU tier of the ownership rule of include/loam_livox_adapter.hpp (tests/cpp/adapter_lifetime_host.cpp is the CPU tier): the owners
// whose handle changes hands or is made again, on the device, on inputs of 64 points.  One process; exits 0 or prints what differed.
#include <cstdio>
#include <cstring>

#include "loam_livox_adapter.hpp"

namespace ll = loam_livox_hip;
namespace pg = loam_livox_hip::Ceres_pose_graph_3d;

struct Pt {
    float x, y, z, intensity;
};
struct Cloud {
    std::vector<Pt> points;
};

static int failures = 0;
#define CHECK(cond) \
    if (!(cond)) failures++, std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond)

static bool same(const Cloud &a, const Cloud &b)
{
    return a.points.size() == b.points.size() && (a.points.empty() || !std::memcmp(a.points.data(), b.points.data(), a.points.size() * sizeof(Pt)));
}
// n points of a 16-line spinning lidar: line k at elevation -15 + 2 k degrees, the azimuth going round once, walls at 5 to 9 m
static Cloud sweep(int n)
{
    Cloud c;
    const int per_line = n / 16 > 0 ? n / 16 : 1;
    for (int i = 0; i < n; i++) {
        const int line = (i / per_line) % 16, k = i % per_line;
        const double az = 6.283185307179586 * k / per_line, el = (-15.0 + 2.0 * line) * 0.017453292519943295;
        const double r = 5.0 + 4.0 * (0.5 + 0.5 * std::cos(3.0 * az)) + (k % 7 == 0 ? 0.8 : 0.0);
        c.points.push_back(Pt{(float)(r * std::cos(el) * std::cos(az)), (float)(r * std::cos(el) * std::sin(az)), (float)(r * std::sin(el)), 0.0f});
    }
    return c;
}
// 64 points in the cells around the origin, a few to a cell
static Cloud block()
{
    Cloud c;
    for (int i = 0; i < 64; i++) c.points.push_back(Pt{0.3f * (float)(i % 8) + 0.01f * (float)i, 0.3f * (float)(i / 8), 0.05f * (float)(i % 5), (float)i});
    return c;
}
template <class F>
static bool throws(F f)
{
    try {
        f();
    } catch (const std::runtime_error &) {
        return true;
    }
    return false;
}

int main()
{
    const double origin[7] = {0, 0, 0, 1, 0, 0, 0};
    const Cloud pts = block();
    {  // a cell map appended to, moved, and read through the new owner
        ll::Points_cloud_map a(256);
        a.append_cloud(pts);
        Cloud before, after, again;
        a.find_cells_in_radius_filtered(origin, 10.0f, 0.05f, before);
        const int64_t cells = a.get_cells_size();
        CHECK(cells > 0 && !before.points.empty());
        ll::Points_cloud_map b(std::move(a));
        b.find_cells_in_radius_filtered(origin, 10.0f, 0.05f, after);
        CHECK(same(before, after) && b.get_cells_size() == cells);
        CHECK(throws([&] { a.get_cells_size(); }));
        ll::Points_cloud_map c(64);  // ... and move-assigned over a live map, whose handle goes
        c = std::move(b);
        c.find_cells_in_radius_filtered(origin, 10.0f, 0.05f, again);
        CHECK(same(before, again) && c.get_cells_size() == cells);
        c.reserve_for(1000);  // (the capacity came along: it doubles from 256)
        c.append_cloud(pts);
        CHECK(c.get_cells_size() == cells);
    }
    {  // a filter used, copied, both used again
        ll::VoxelGrid<Cloud> f;
        f.setLeafSize(0.7f, 0.7f, 0.7f);
        Cloud first, of_source, of_copy;
        f.setInputCloud(&pts);
        f.filter(first);
        ll::VoxelGrid<Cloud> g(f);
        f.setInputCloud(&pts);
        f.filter(of_source);
        g.setInputCloud(&pts);
        g.filter(of_copy);
        CHECK(!first.points.empty() && first.points.size() < pts.points.size() && same(first, of_source) && same(first, of_copy));
        CHECK(f.status == 0 && g.status == 0);
    }
    {  // an extractor that outgrows its first capacity between two extractions
        const Cloud small = sweep(64), large = sweep(33024);  // the library's default capacity is 32768 points
        ll::Spinning_laser spin, reference;
        Cloud s0[5], l0[5], s1[5], want[5];
        spin.extract(small, s0[0], s0[1], s0[2], s0[3], s0[4]);
        const int first_capacity = spin.capacity();
        CHECK(first_capacity >= 64 && first_capacity < 33024);
        spin.extract(large, l0[0], l0[1], l0[2], l0[3], l0[4]);
        CHECK(spin.capacity() == 33024 && l0[0].points.size() > s0[0].points.size());
        reference.max_points = 33024;  // an extractor that was large enough from the start
        reference.extract(large, want[0], want[1], want[2], want[3], want[4]);
        spin.extract(small, s1[0], s1[1], s1[2], s1[3], s1[4]);
        for (int k = 0; k < 5; k++) CHECK(same(l0[k], want[k]) && same(s0[k], s1[k]));
        CHECK(!s0[0].points.empty());
    }
    {  // the two entrances of Mapping_refine's ensure(): add_logged first, refine_pointcloud first
        ll::History_batch batch(1, 2, 64, 0.4f, 0.8f);
        ll::check(ll_history_batch_enable_full_maps(batch.handle(), 64, 1.0f, 3), "ll_history_batch_enable_full_maps");
        batch.enable_scan_log(2, 4);
        std::map<int, Cloud> clouds;
        clouds[7] = pts;
        pg::MapOfPoses ori, opm;
        ori[7] = pg::Pose3d();
        opm[7] = pg::Pose3d();
        opm[7].p(0) = 1.0;
        ll::Mapping_refine<Cloud> logged_first(64), refine_first(64);
        CHECK(logged_first.handle() == nullptr);
        std::vector<int64_t> kept;
        const std::vector<int64_t> ids = logged_first.add_logged(batch, {{batch.hand_over(0)}}, 0.5f, &kept);  // a group of no scans
        CHECK(logged_first.handle() != nullptr && ids.size() == 1 && ids[0] == 0 && kept.size() == 1 && kept[0] == 0);
        const Cloud a = logged_first.refine_pointcloud(clouds, ori, opm, 0), b = refine_first.refine_pointcloud(clouds, ori, opm, 0);
        CHECK(!a.points.empty() && a.points.size() <= 64 && same(a, b));
        ll::Mapping_refine<Cloud> moved(std::move(logged_first));
        CHECK(same(moved.refine_pointcloud(clouds, ori, opm, 0), a) && same(moved.merge_last(), refine_first.merge_last()));
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
