// Mapping_refine of include/loam_livox_adapter.hpp, called the way laser_mapping.hpp:1091-1100 calls the reference's class
// (tests/test_adapter_map_refine.py).
//   adapter_map_refine <in.bin> <out.bin>
//   in : int32 K, float leaf, per key frame int32 n and float xyzi[n][4], then double ori[K][7], double opm[K][7]
//   out: records of int32 n and float xyzi[n][4]: refine_pointcloud for pc_idx = K - 1, K - 3, ... >= 0; refine_pointcloud with idx = K
//        (empty); m_pts_aft_refind after refine_mapping; merge_last; refine_pts of key frame 0's points (intensity 0); then int32 flags:
//        if_save = 1 refused by refine_pointcloud, by refine_mapping; int64 work[4] of the last refine_pointcloud
#include <cstdio>
#include <cstdlib>

#include "../../include/loam_livox_adapter.hpp"

using namespace loam_livox_hip;

struct PointXYZI {
    float x, y, z, intensity;
};
struct Cloud {
    std::vector<PointXYZI> points;
};
struct Vec3f {
    float c[3];
    float &operator()(int i) { return c[i]; }
    float operator()(int i) const { return c[i]; }
};

static void put(FILE *f, const Cloud &c)
{
    const int32_t n = (int32_t)c.points.size();
    fwrite(&n, sizeof n, 1, f);
    if (n) fwrite(c.points.data(), sizeof(PointXYZI), (size_t)n, f);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t K = 0;
    float leaf = 0.f;
    if (!f || fread(&K, 4, 1, f) != 1 || fread(&leaf, 4, 1, f) != 1) return 2;
    std::map<int, Cloud> map_id_pc;
    for (int k = 0; k < K; k++) {
        int32_t n = 0;
        if (fread(&n, 4, 1, f) != 1) return 2;
        Cloud c;
        c.points.resize((size_t)n);
        if (n && fread(c.points.data(), sizeof(PointXYZI), (size_t)n, f) != (size_t)n) return 2;
        map_id_pc.insert(std::make_pair((int)map_id_pc.size(), c));   // :946
    }
    Ceres_pose_graph_3d::MapOfPoses pose3d_map_ori, temp_pose_3d_map;
    for (int which = 0; which < 2; which++)
        for (int k = 0; k < K; k++) {
            double p[7];
            if (fread(p, 8, 7, f) != 7) return 2;
            Ceres_pose_graph_3d::Pose3d pose;
            pose.q.x() = p[0], pose.q.y() = p[1], pose.q.z() = p[2], pose.q.w() = p[3];
            for (int i = 0; i < 3; i++) pose.p(i) = p[4 + i];
            (which ? temp_pose_3d_map : pose3d_map_ori).insert(std::make_pair(k, pose));
        }
    fclose(f);
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 2;
    try {
        Mapping_refine<Cloud> map_rfn;
        map_rfn.set_save_dir(std::string("unused"));   // :902
        map_rfn.set_down_sample_resolution(leaf);
        for (int pc_idx = (int)map_id_pc.size() - 1; pc_idx >= 0; pc_idx -= 2) {   // :1091-1094
            auto refined_pt = map_rfn.refine_pointcloud(map_id_pc, pose3d_map_ori, temp_pose_3d_map, pc_idx, 0);
            put(g, refined_pt);
        }
        int64_t work[4];
        map_rfn.work(work);
        put(g, map_rfn.refine_pointcloud(map_id_pc, pose3d_map_ori, temp_pose_3d_map, K, 0));
        map_rfn.refine_mapping(map_id_pc, pose3d_map_ori, temp_pose_3d_map, 0);
        put(g, map_rfn.m_pts_aft_refind);
        put(g, map_rfn.merge_last());
        std::vector<Vec3f> raw;
        for (const PointXYZI &p : map_id_pc[0].points) raw.push_back(Vec3f{{p.x, p.y, p.z}});
        const std::vector<Vec3f> moved = Mapping_refine<Cloud>::refine_pts(raw, pose3d_map_ori[0].q, pose3d_map_ori[0].p, temp_pose_3d_map[0].q, temp_pose_3d_map[0].p);
        Cloud mc;
        for (const Vec3f &v : moved) mc.points.push_back(PointXYZI{v(0), v(1), v(2), 0.f});
        put(g, mc);
        int32_t refused[2] = {0, 0};
        try {
            map_rfn.refine_pointcloud(map_id_pc, pose3d_map_ori, temp_pose_3d_map, 0, 1);
        } catch (const std::runtime_error &) {
            refused[0] = 1;
        }
        try {
            map_rfn.refine_mapping(map_id_pc, pose3d_map_ori, temp_pose_3d_map, 1);
        } catch (const std::runtime_error &) {
            refused[1] = 1;
        }
        fwrite(refused, 4, 2, g);
        fwrite(work, 8, 4, g);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    fclose(g);
    return 0;
}
