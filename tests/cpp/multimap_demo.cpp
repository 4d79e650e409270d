// The map-per-slot overloads of include/loam_livox_adapter.hpp (Point_cloud_registration::enqueue_fe_maps): two scans of a batched
// extractor are registered in one call, each against a map of its own, un-filtered and voxel-filtered, and each once more alone
// through the single-map C calls.  argv: corner_a.bin surf_a.bin corner_b.bin surf_b.bin (n x xyz float32) scan_a.bin scan_b.bin
// (n x xyzi float32, equally many points) poses.bin (2 x 7 doubles) out.bin.  out.bin: per route (maps, maps down-sampled, alone,
// alone down-sampled) and scan: int32 result, 7 doubles pose; then int32 refused (1: m_if_motion_deblur was refused).
#include <cstdio>
#include <cstdlib>
#include <vector>

#define LOAM_LIVOX_ADAPTER_NO_EIGEN
#include "loam_livox_adapter.hpp"

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

static void need(int rc, const char *what)
{
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + ll_last_error());
}

static void write_results(FILE *o, ll_reg *reg, int n)
{
    std::vector<double> pc(7 * n), pi(7 * n);
    std::vector<int32_t> res(n);
    std::vector<ll_reg_report> rep(n);
    need(ll_reg_collect(reg, n, pc.data(), pi.data(), rep.data(), res.data()), "ll_reg_collect");
    for (int b = 0; b < n; b++) {
        fwrite(&res[b], 4, 1, o);
        fwrite(&pc[7 * b], 8, 7, o);
    }
}

int main(int argc, char **argv)
{
    if (argc < 9) return 2;
    std::vector<float> cloud[4], scan[2];
    for (int i = 0; i < 4; i++) cloud[i] = read_floats(argv[1 + i]);
    for (int i = 0; i < 2; i++) scan[i] = read_floats(argv[5 + i]);
    if (scan[0].empty() || scan[0].size() != scan[1].size()) return 3;
    double poses[14];
    FILE *pf = fopen(argv[7], "rb");
    if (!pf || fread(poses, 8, 14, pf) != 14) return 3;
    fclose(pf);
    FILE *o = fopen(argv[8], "wb");
    if (!o) return 3;
    const int n_pts = (int)(scan[0].size() / 4);
    const float line_res = 0.1f, plane_res = 0.4f;
    try {
        ll_map *maps[2] = {nullptr, nullptr};
        for (int m = 0; m < 2; m++) {
            need(ll_map_create(0, &maps[m]), "ll_map_create");
            need(ll_map_upload(maps[m], LL_MAP_CORNER, cloud[2 * m].data(), 3, (int64_t)(cloud[2 * m].size() / 3), 0.0f), "ll_map_upload");
            need(ll_map_upload(maps[m], LL_MAP_SURF, cloud[2 * m + 1].data(), 3, (int64_t)(cloud[2 * m + 1].size() / 3), 0.0f), "ll_map_upload");
        }
        ll_fe_params fp;
        ll_fe_default_params(&fp);
        fp.max_points = n_pts, fp.max_scans = 2, fp.piecewise_number = 1;
        ll_fe *fe = nullptr, *fe1 = nullptr;
        need(ll_fe_create(&fp, &fe), "ll_fe_create");
        fp.max_scans = 1;
        need(ll_fe_create(&fp, &fe1), "ll_fe_create");
        ll_reg *reg = nullptr, *reg1 = nullptr;
        need(ll_reg_create(0, 2, n_pts, &reg), "ll_reg_create");
        need(ll_reg_create(0, 1, n_pts, &reg1), "ll_reg_create");
        ll_voxel *vox[4];
        for (int i = 0; i < 4; i++) need(ll_voxel_create(0, i < 2 ? 2 : 1, n_pts, &vox[i]), "ll_voxel_create");
        std::vector<float> both(scan[0]);
        both.insert(both.end(), scan[1].begin(), scan[1].end());
        const double stamps[2] = {1.0, 1.0};
        need(ll_fe_upload(fe, 0, 2, both.data(), n_pts, stamps), "ll_fe_upload");
        need(ll_fe_extract_batch(fe, 2), "ll_fe_extract_batch");
        need(ll_fe_resolve(fe), "ll_fe_resolve");
        need(ll_fe_select_batch(fe, 2, -1, 0.0f, 1.0f), "ll_fe_select_batch");

        ll::Point_cloud_registration pcr;
        pcr.m_para_icp_max_iterations = 6;
        pcr.m_para_cere_max_iterations = 20;
        pcr.m_para_max_angular_rate = 20.0f;
        pcr.m_para_max_speed = 0.3f;
        pcr.m_current_frame_index = 100;
        pcr.m_mapping_init_accumulate_frames = 50;
        pcr.m_maximum_allow_residual_block = n_pts;
        pcr.m_subsample_seed = 0;
        // the two overloads
        pcr.enqueue_fe_maps(reg, maps, fe, 2, nullptr, poses, poses);
        write_results(o, reg, 2);
        pcr.enqueue_fe_maps(reg, maps, fe, vox[0], vox[1], line_res, plane_res, 2, nullptr, poses, poses);
        write_results(o, reg, 2);
        // every scan alone through the single-map calls
        ll_reg_params p;
        ll_reg_default_params(&p);
        p.icp_max_iterations = 6, p.ceres_max_iterations = 20, p.para_max_angular_rate = 20.0f, p.para_max_speed = 0.3f;
        p.current_frame_index = 100, p.mapping_init_accumulate_frames = 50, p.maximum_allow_residual_block = n_pts, p.subsample_seed = 0;
        for (int down = 0; down < 2; down++)
            for (int b = 0; b < 2; b++) {
                need(ll_fe_upload(fe1, 0, 1, scan[b].data(), n_pts, stamps), "ll_fe_upload");
                need(ll_fe_extract_batch(fe1, 1), "ll_fe_extract_batch");
                need(ll_fe_resolve(fe1), "ll_fe_resolve");
                need(ll_fe_select_batch(fe1, 1, -1, 0.0f, 1.0f), "ll_fe_select_batch");
                if (down)
                    need(ll_reg_enqueue_fe_downsampled(reg1, maps[b], fe1, vox[2], vox[3], line_res, plane_res, 1, &p, poses + 7 * b, poses + 7 * b, nullptr),
                         "ll_reg_enqueue_fe_downsampled");
                else
                    need(ll_reg_enqueue_fe(reg1, maps[b], fe1, 1, &p, poses + 7 * b, poses + 7 * b, nullptr), "ll_reg_enqueue_fe");
                write_results(o, reg1, 1);
            }
        // the deblur flag is refused, not ignored
        pcr.m_if_motion_deblur = 1;
        int refused = 0;
        try {
            pcr.enqueue_fe_maps(reg, maps, fe, 2, nullptr, poses, poses);
        } catch (const std::exception &e) {
            refused = 1;
        }
        fwrite(&refused, 4, 1, o);
        for (int i = 0; i < 4; i++) ll_voxel_destroy(vox[i]);
        ll_reg_destroy(reg);
        ll_reg_destroy(reg1);
        ll_fe_destroy(fe);
        ll_fe_destroy(fe1);
        ll_map_destroy(maps[0]);
        ll_map_destroy(maps[1]);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        fclose(o);
        return 4;
    }
    fclose(o);
    return 0;
}
