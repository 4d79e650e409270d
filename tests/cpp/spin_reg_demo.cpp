// The Spinning_laser overloads of include/loam_livox_adapter.hpp: one spinning-lidar scan is
// registered against a map and pushed into a history twice -- device to device (extract_device, find_out_incremental_transfrom( spin ),
// History_buffer::add( spin, pose )) and through the host clouds (extract, the 2-argument find_out_incremental_transfrom, add( corner,
// surface, pose )).  argv: corner_map.bin surf_map.bin (n x xyz float32) scan.bin (n x xyzi float32) scan_line pose.bin (7 doubles)
// out.bin.  out.bin: per route int32 ret, 7 doubles pose, then the two match-buffer clouds (int32 n + n x xyzi).
#include <cstdio>
#include <cstdlib>
#include <memory>
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

static std::vector<float> read_floats(const char *path)
{
    std::vector<float> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    float x;
    while (fread(&x, 4, 1, f) == 1) v.push_back(x);
    fclose(f);
    return v;
}

static void configure(ll::Point_cloud_registration &r, const double pose[7])
{
    r.m_para_icp_max_iterations = 10;
    r.m_para_cere_max_iterations = 20;
    r.m_para_max_angular_rate = 20.0f;
    r.m_para_max_speed = 0.3f;
    r.m_current_frame_index = 100;
    r.m_mapping_init_accumulate_frames = 50;
    r.m_q_w_curr.x() = pose[0], r.m_q_w_curr.y() = pose[1], r.m_q_w_curr.z() = pose[2], r.m_q_w_curr.w() = pose[3];
    r.m_q_w_last = r.m_q_w_curr;
    for (int i = 0; i < 3; i++) r.m_t_w_curr(i) = r.m_t_w_last(i) = pose[4 + i];
}

static void write_route(FILE *o, int ret, ll::Point_cloud_registration &r, ll::History_buffer &h)
{
    fwrite(&ret, 4, 1, o);
    fwrite(r.m_para_buffer_RT, 8, 7, o);
    for (int kind = 0; kind < 2; kind++) {
        Cloud c;
        h.map_cloud(kind, c);
        const int n = (int)c.points.size();
        fwrite(&n, 4, 1, o);
        for (const PointXYZI &p : c.points) fwrite(&p, 4, 4, o);
    }
}

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const std::vector<float> mc = read_floats(argv[1]), ms = read_floats(argv[2]), sc = read_floats(argv[3]);
    double pose[7];
    FILE *pf = fopen(argv[5], "rb");
    if (!pf || fread(pose, 8, 7, pf) != 7) return 3;
    fclose(pf);
    Cloud in;
    for (size_t i = 0; i + 3 < sc.size(); i += 4) in.points.push_back({sc[i], sc[i + 1], sc[i + 2], sc[i + 3]});
    FILE *o = fopen(argv[6], "wb");
    if (!o) return 3;
    try {
        ll::Spinning_laser spin;
        spin.scan_line = atoi(argv[4]);
        // device to device
        ll::Point_cloud_registration dev;
        configure(dev, pose);
        if (ll_map_upload(dev.map(), LL_MAP_CORNER, mc.data(), 3, (int64_t)(mc.size() / 3), 0.0f) ||
            ll_map_upload(dev.map(), LL_MAP_SURF, ms.data(), 3, (int64_t)(ms.size() / 3), 0.0f))
            throw std::runtime_error(ll_last_error());
        if (spin.extract_device(in) != LL_SPIN_STATUS_OK) return 5;
        const int ret_dev = dev.find_out_incremental_transfrom(spin);
        ll_map *scratch_a = nullptr, *scratch_b = nullptr;  // the histories refresh maps of their own: the registrar's map stays as uploaded
        if (ll_map_create(0, &scratch_a) || ll_map_create(0, &scratch_b)) throw std::runtime_error(ll_last_error());
        ll::History_buffer hist_dev(3, spin.capacity(), 0.2f, 0.4f);
        hist_dev.add(spin, dev.m_para_buffer_RT);
        hist_dev.refresh(scratch_a);
        write_route(o, ret_dev, dev, hist_dev);
        // through the host clouds
        auto full = std::make_shared<Cloud>(), sharp = std::make_shared<Cloud>(), less_sharp = std::make_shared<Cloud>(),
             flat = std::make_shared<Cloud>(), less_flat = std::make_shared<Cloud>();
        spin.extract(in, *full, *sharp, *less_sharp, *flat, *less_flat);
        ll::Point_cloud_registration host;
        configure(host, pose);
        const int ret_host = host.find_out_incremental_transfrom(less_sharp, less_flat);
        ll::History_buffer hist_host(3, spin.capacity(), 0.2f, 0.4f);
        hist_host.add(*less_sharp, *less_flat, host.m_para_buffer_RT);
        hist_host.refresh(scratch_b);
        write_route(o, ret_host, host, hist_host);
        // the deblur flag is refused, not ignored
        dev.m_if_motion_deblur = 1;
        int refused = 0;
        try {
            dev.find_out_incremental_transfrom(spin);
        } catch (const std::exception &e) {
            refused = 1;
        }
        fwrite(&refused, 4, 1, o);
        ll_map_destroy(scratch_a);
        ll_map_destroy(scratch_b);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        fclose(o);
        return 4;
    }
    fclose(o);
    return 0;
}
