// Ceres_pose_graph_3d and Scene_alignment::add_constrain_of_loop of include/loam_livox_adapter.hpp (tests/test_gpu_pose_graph.py).
// argv: <in.bin> <out.txt>
// in.bin: int64 {N, E, s_idx, t_idx}; double poses[7 N] {qx, qy, qz, qw, tx, ty, tz}; int32 ab[2 E]; double meas[7 E];
//         double {q_a[4], t_a[3], q_b[4], t_b[3], icp_q[4], icp_t[3]} of the loop.
// Pose k gets the map key 10 k + 3 (the keys are names, not positions); the E constraints are followed by the loop constraint of
// add_constrain_of_loop.  out.txt: the loop constraint's seven values, then the N optimised poses, seven hexadecimal floats a line;
// last "iterations successful unsuccessful termination".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/loam_livox_adapter.hpp"

using namespace loam_livox_hip;

static Quaterniond quat(const double *v)
{
    Quaterniond q;
    q.x() = v[0], q.y() = v[1], q.z() = v[2], q.w() = v[3];
    return q;
}
static Vector3d vec(const double *v)
{
    Vector3d t;
    t(0) = v[0], t(1) = v[1], t(2) = v[2];
    return t;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t head[4];
    if (fread(head, sizeof(int64_t), 4, f) != 4 || head[0] < 1 || head[0] > 4096 || head[1] < 0 || head[1] > 8192) return 3;
    const size_t n = (size_t)head[0], e = (size_t)head[1];
    std::vector<double> poses(7 * n), meas(7 * e), loop(21);
    std::vector<int32_t> ab(2 * e);
    if (fread(poses.data(), sizeof(double), poses.size(), f) != poses.size() || fread(ab.data(), sizeof(int32_t), ab.size(), f) != ab.size() ||
        fread(meas.data(), sizeof(double), meas.size(), f) != meas.size() || fread(loop.data(), sizeof(double), 21, f) != 21)
        return 3;
    fclose(f);

    Ceres_pose_graph_3d::MapOfPoses map;
    for (size_t k = 0; k < n; k++) map.insert(std::make_pair((int)(10 * k + 3), Ceres_pose_graph_3d::Pose3d(quat(&poses[7 * k]), vec(&poses[7 * k + 4]))));
    Ceres_pose_graph_3d::VectorOfConstraints constraints;
    for (size_t k = 0; k < e; k++)
        constraints.push_back(Ceres_pose_graph_3d::Constraint3d(10 * ab[2 * k] + 3, 10 * ab[2 * k + 1] + 3, quat(&meas[7 * k]), vec(&meas[7 * k + 4])));
    Ceres_pose_graph_3d::Constraint3d lc = Scene_alignment::add_constrain_of_loop((int)head[2], (int)head[3], quat(&loop[0]), vec(&loop[4]), quat(&loop[7]),
                                                                                   vec(&loop[11]), quat(&loop[14]), vec(&loop[18]));
    FILE *out = fopen(argv[2], "w");
    if (!out) return 2;
    fprintf(out, "%a %a %a %a %a %a %a\n", lc.t_be.q.x(), lc.t_be.q.y(), lc.t_be.q.z(), lc.t_be.q.w(), lc.t_be.p(0), lc.t_be.p(1), lc.t_be.p(2));
    lc.id_begin = 10 * lc.id_begin + 3, lc.id_end = 10 * lc.id_end + 3;
    constraints.push_back(lc);
    const ll_pose_graph_summary s = Ceres_pose_graph_3d::pose_graph_optimization(map, constraints);
    for (Ceres_pose_graph_3d::MapOfPoses::const_iterator it = map.begin(); it != map.end(); ++it)
        fprintf(out, "%a %a %a %a %a %a %a\n", it->second.q.x(), it->second.q.y(), it->second.q.z(), it->second.q.w(), it->second.p(0), it->second.p(1),
                it->second.p(2));
    fprintf(out, "%d %d %d %d\n", s.iterations, s.successful_steps, s.unsuccessful_steps, s.termination);
    fclose(out);
    return 0;
}
