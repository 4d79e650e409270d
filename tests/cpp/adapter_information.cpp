// GPU tier of the adapter's registration information (tests/test_gpu_adapter_information.py): one scan registered through
// loam_livox_hip::Point_cloud_registration with m_if_compute_information = 1, then once more with the member at 0.
//   adapter_information <map_corner.f32> <map_surf.f32> <scan_corner.f32> <scan_surf.f32> <pose7.f64> <out.bin>
// out: int32 {ret, n_line, n_plane, status, threw_when_off}, double {H[36], g[6], cost, eigenvalues[6], eigenvectors[36], H_pose[36]}
#include <cstdio>
#include <vector>

#define LOAM_LIVOX_ADAPTER_NO_EIGEN
#include "loam_livox_adapter.hpp"

struct PointXYZI {
    float x = 0, y = 0, z = 0, intensity = 0;
};
struct Cloud {
    std::vector<PointXYZI> points;
};
namespace ll = loam_livox_hip;

static std::shared_ptr<Cloud> read_cloud(const char *path)
{
    std::shared_ptr<Cloud> c(new Cloud());
    FILE *f = fopen(path, "rb");
    PointXYZI p;
    while (f && fread(&p, 4, 4, f) == 4) c->points.push_back(p);
    if (f) fclose(f);
    return c;
}

static void configure(ll::Point_cloud_registration &r, const double pose[7])
{
    r.m_para_icp_max_iterations = 4;
    r.m_para_cere_max_iterations = 20;
    r.m_para_max_angular_rate = 20.0f;
    r.m_para_max_speed = 0.3f;
    r.m_current_frame_index = 100;
    r.m_mapping_init_accumulate_frames = 50;
    r.m_subsample_seed = 0;
    r.m_q_w_curr.x() = pose[0], r.m_q_w_curr.y() = pose[1], r.m_q_w_curr.z() = pose[2], r.m_q_w_curr.w() = pose[3];
    r.m_q_w_last = r.m_q_w_curr;
    for (int i = 0; i < 3; i++) r.m_t_w_curr(i) = r.m_t_w_last(i) = pose[4 + i];
}

int main(int argc, char **argv)
{
    if (argc != 7) return 2;
    std::shared_ptr<Cloud> mc = read_cloud(argv[1]), ms = read_cloud(argv[2]), sc = read_cloud(argv[3]), ss = read_cloud(argv[4]);
    double pose[7];
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(pose, 8, 7, f) != 7) return 2;
    fclose(f);
    int ret = 0;
    ll::Registration_information info;
    double pose_on[7];
    {
        ll::Point_cloud_registration on;
        configure(on, pose);
        on.m_if_compute_information = 1;
        ret = on.find_out_incremental_transfrom(mc, ms, sc, ss);
        info = on.information();
        for (int i = 0; i < 7; i++) pose_on[i] = on.m_para_buffer_RT[i];
    }  // (its registrar is back in the pool)
    // the same registrar comes back from the pool for an object that does not ask: it must not compute, and information() must say so
    ll::Point_cloud_registration off;
    configure(off, pose);
    off.find_out_incremental_transfrom(mc, ms, sc, ss);
    int threw = 0;
    try {
        (void)off.information();
    } catch (const std::runtime_error &) {
        threw = 1;
    }
    for (int i = 0; i < 7; i++)
        if (off.m_para_buffer_RT[i] != pose_on[i]) threw = -1;  // (the switch changes no pose)
    FILE *o = fopen(argv[6], "wb");
    if (!o) return 2;
    const int32_t head[5] = {ret, info.n_line, info.n_plane, info.status, threw};
    fwrite(head, 4, 5, o);
    fwrite(info.H, 8, 36, o);
    fwrite(info.g, 8, 6, o);
    fwrite(&info.cost, 8, 1, o);
    fwrite(info.eigenvalues, 8, 6, o);
    fwrite(info.eigenvectors, 8, 36, o);
    fwrite(info.H_pose, 8, 36, o);
    fclose(o);
    return 0;
}
