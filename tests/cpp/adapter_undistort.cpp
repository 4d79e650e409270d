// GPU tier of the adapter's deskewed clouds (tests/test_gpu_undistort.py): one scan registered with m_if_motion_deblur = 1 through
// loam_livox_hip::Point_cloud_registration, then its surface cloud moved three ways with if_undistore = 1.
//   adapter_undistort <map_corner.f32> <map_surf.f32> <scan_corner.f32> <scan_surf.f32> <pose7.f64> <min_ts> <max_ts> <out.bin>
// out: int32 {ret, n, threw_plain_differs, history_frames}, then float [n][4] three times: pointcloudAssociateToMap( in, out, 1 ), the C call
// ll_cloud_undistort on the object's registrar, and pointAssociateToMap( &p, &q, refine_blur( intensity ), 1 ) point by point
#include <cstdio>
#include <cstdlib>
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

int main(int argc, char **argv)
{
    if (argc != 9) return 2;
    std::shared_ptr<Cloud> mc = read_cloud(argv[1]), ms = read_cloud(argv[2]), sc = read_cloud(argv[3]), ss = read_cloud(argv[4]);
    double pose[7];
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(pose, 8, 7, f) != 7) return 2;
    fclose(f);
    ll::Point_cloud_registration r;
    r.m_para_icp_max_iterations = 4;
    r.m_para_cere_max_iterations = 20;
    r.m_para_max_angular_rate = 20.0f;
    r.m_para_max_speed = 0.3f;
    r.m_current_frame_index = 100;
    r.m_mapping_init_accumulate_frames = 50;
    r.m_subsample_seed = 0;
    r.m_if_motion_deblur = 1;
    r.m_minimum_pt_time_stamp = (float)atof(argv[6]);
    r.m_maximum_pt_time_stamp = (float)atof(argv[7]);
    r.m_q_w_curr.x() = pose[0], r.m_q_w_curr.y() = pose[1], r.m_q_w_curr.z() = pose[2], r.m_q_w_curr.w() = pose[3];
    r.m_q_w_last = r.m_q_w_curr;
    for (int i = 0; i < 3; i++) r.m_t_w_curr(i) = r.m_t_w_last(i) = pose[4 + i];
    const int ret = r.find_out_incremental_transfrom(mc, ms, sc, ss);
    const int n = (int)ss->points.size();
    Cloud assoc, plain;
    r.pointcloudAssociateToMap(*ss, assoc, 1);
    r.pointcloudAssociateToMap(*ss, plain, 0);
    int differs = 0;
    for (int i = 0; i < n; i++) differs |= (assoc.points[i].x != plain.points[i].x);
    std::vector<float> in((size_t)n * 4), c_call((size_t)n * 4), per_point((size_t)n * 4), a((size_t)n * 4);
    for (int i = 0; i < n; i++) {
        const PointXYZI &p = ss->points[i];
        in[4 * i] = p.x, in[4 * i + 1] = p.y, in[4 * i + 2] = p.z, in[4 * i + 3] = p.intensity;
        const PointXYZI &q = assoc.points[i];
        a[4 * i] = q.x, a[4 * i + 1] = q.y, a[4 * i + 2] = q.z, a[4 * i + 3] = q.intensity;
    }
    if (ll_cloud_undistort(r.handle(), 0, in.data(), c_call.data(), n) != 0) {
        fprintf(stderr, "%s\n", ll_last_error());
        return 3;
    }
    for (int i = 0; i < n; i++) {
        PointXYZI q;
        r.pointAssociateToMap(&ss->points[i], &q, r.refine_blur(ss->points[i].intensity, r.m_minimum_pt_time_stamp, r.m_maximum_pt_time_stamp), 1);
        per_point[4 * i] = q.x, per_point[4 * i + 1] = q.y, per_point[4 * i + 2] = q.z, per_point[4 * i + 3] = q.intensity;
    }
    // the history's undistort form: the frame is taken, with the registered pose gating
    ll::History_buffer hist(10, 24000, 0.1f, 0.4f);
    hist.set_undistort(r.handle(), 0);
    const int frames = hist.add(*sc, *ss, r.m_para_buffer_RT) ? 1 : 0;
    FILE *o = fopen(argv[8], "wb");
    if (!o) return 2;
    const int32_t head[4] = {ret, n, differs, frames};
    fwrite(head, 4, 4, o);
    fwrite(a.data(), 4, a.size(), o);
    fwrite(c_call.data(), 4, c_call.size(), o);
    fwrite(per_point.data(), 4, per_point.size(), o);
    fclose(o);
    return 0;
}
