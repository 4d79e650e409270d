// Scene_alignment and Points_cloud_map::extract_specify_points of include/loam_livox_adapter.hpp (tests/test_gpu_scene_align.py).
// argv: <a.bin> <b.bin> <resolution> <maximum_icp_iteration> <accepted_threshold> <out.txt>  (raw float32 xyzi rows)
// out.txt: "line_a plane_a line_b plane_b" (points of extract_specify_points), an FNV-1a checksum of a's two clouds, the inlier
// threshold and the pose {qx qy qz qw tx ty tz} as hexadecimal doubles, the number of registrations and the work tap's four values.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/loam_livox_adapter.hpp"

struct PointXYZI {
    float x, y, z, intensity;
};
struct Cloud {
    std::vector<PointXYZI> points;
};

static Cloud read_cloud(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<float> raw((size_t)bytes / sizeof(float));
    if (!raw.empty() && fread(raw.data(), sizeof(float), raw.size(), f) != raw.size()) exit(3);
    fclose(f);
    Cloud c;
    for (size_t i = 0; i + 3 < raw.size(); i += 4) c.points.push_back(PointXYZI{raw[i], raw[i + 1], raw[i + 2], raw[i + 3]});
    return c;
}

static unsigned long long fnv(unsigned long long h, const Cloud &c)
{
    for (const PointXYZI &p : c.points) {
        const unsigned char *b = (const unsigned char *)&p;
        for (size_t i = 0; i < sizeof(p); i++) h = (h ^ b[i]) * 1099511628211ull;
    }
    return h;
}

int main(int argc, char **argv)
{
    if (argc != 7) return 2;
    const Cloud a = read_cloud(argv[1]), b = read_cloud(argv[2]);
    FILE *out = fopen(argv[6], "w");
    if (!out) return 2;
    using loam_livox_hip::Points_cloud_map;
    Points_cloud_map map_a((int64_t)a.points.size() + 1, 1.0f), map_b((int64_t)b.points.size() + 1, 1.0f);
    map_a.append_cloud(a);
    map_b.append_cloud(b);
    const Cloud line_a = map_a.extract_specify_points<Cloud>(Points_cloud_map::e_feature_line), plane_a = map_a.extract_specify_points<Cloud>(Points_cloud_map::e_feature_plane);
    const Cloud line_b = map_b.extract_specify_points<Cloud>(Points_cloud_map::e_feature_line), plane_b = map_b.extract_specify_points<Cloud>(Points_cloud_map::e_feature_plane);
    fprintf(out, "%zu %zu %zu %zu\n%llu\n", line_a.points.size(), plane_a.points.size(), line_b.points.size(), plane_b.points.size(),
            fnv(fnv(14695981039346656037ull, line_a), plane_a));

    loam_livox_hip::Scene_alignment scene_align;
    scene_align.initial_points = 1024;  // (the handle has to grow)
    scene_align.init();
    const float res = (float)atof(argv[3]);
    scene_align.set_downsample_resolution(res, res);
    scene_align.m_maximum_icp_iteration = atoi(argv[4]);
    scene_align.m_accepted_threshold = (float)atof(argv[5]);
    const double thr = scene_align.find_tranfrom_of_two_mappings(&map_a, &map_b);
    const auto &q = scene_align.m_pc_reg.m_q_w_curr;
    const auto &t = scene_align.m_pc_reg.m_t_w_curr;
    fprintf(out, "%a\n%a %a %a %a %a %a %a\n", thr, q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2));
    int64_t work[4];
    scene_align.work(work);
    fprintf(out, "%zu %lld %lld %lld %lld\n", scene_align.reports.size(), (long long)work[0], (long long)work[1], (long long)work[2], (long long)work[3]);
    fclose(out);
    return thr == scene_align.m_pc_reg.m_inlier_threshold ? 0 : 5;
}
