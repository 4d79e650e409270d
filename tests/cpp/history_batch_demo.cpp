// History_batch of include/loam_livox_adapter.hpp: the match buffers of two sequences in one handle.  Two scans of a batched extractor
// are added (un-filtered features, then once more the voxel-filtered stacks of an enqueue with filters, slot 1 inactive in the second
// step) and refreshed into a map per slot.  argv: scan_a.bin scan_b.bin (n x xyzi float32, equally many points) poses.bin (4 x 7
// doubles: the poses of step 1, then of step 2) out.bin.  out.bin, per step and slot: int32 added, int32 history size, int64 map
// generation (corner), int64 ll_map_size and ll_map_cells per kind, then per kind int64 n and n x xyzi float32 of the match buffer.
#include <cstdio>
#include <cstdlib>
#include <vector>

#define LOAM_LIVOX_ADAPTER_NO_EIGEN
#include "loam_livox_adapter.hpp"

namespace ll = loam_livox_hip;

struct Pt {
    float x, y, z, intensity;
};
struct Cloud {
    std::vector<Pt> points;
};

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

static void write_state(FILE *o, ll::History_batch &hb, ll_map *const *maps, const int32_t *added)
{
    for (int s = 0; s < hb.n_sequences(); s++) {
        const int32_t sz = hb.size(s);
        const int64_t gen = ll_map_generation(maps[s], LL_MAP_CORNER);
        fwrite(&added[s], 4, 1, o);
        fwrite(&sz, 4, 1, o);
        fwrite(&gen, 8, 1, o);
        for (int k = 0; k < 2; k++) {
            const int64_t n = ll_map_size(maps[s], k), c = ll_map_cells(maps[s], k);
            fwrite(&n, 8, 1, o);
            fwrite(&c, 8, 1, o);
        }
        for (int k = 0; k < 2; k++) {
            Cloud cl;
            hb.map_cloud(s, k, cl);
            const int64_t n = (int64_t)cl.points.size();
            fwrite(&n, 8, 1, o);
            if (n > 0) fwrite(cl.points.data(), sizeof(Pt), (size_t)n, o);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    std::vector<float> scan[2] = {read_floats(argv[1]), read_floats(argv[2])};
    if (scan[0].empty() || scan[0].size() != scan[1].size()) return 3;
    double poses[28];
    FILE *pf = fopen(argv[3], "rb");
    if (!pf || fread(poses, 8, 28, pf) != 28) return 3;
    fclose(pf);
    FILE *o = fopen(argv[4], "wb");
    if (!o) return 3;
    const int n_pts = (int)(scan[0].size() / 4);
    const float line_res = 0.1f, plane_res = 0.4f;
    try {
        ll::History_batch hb(2, 3, n_pts, line_res, plane_res);
        ll_map *maps[2] = {nullptr, nullptr};
        for (int m = 0; m < 2; m++) need(ll_map_create(0, &maps[m]), "ll_map_create");
        ll_fe_params fp;
        ll_fe_default_params(&fp);
        fp.max_points = n_pts, fp.max_scans = 2, fp.piecewise_number = 1;
        ll_fe *fe = nullptr;
        need(ll_fe_create(&fp, &fe), "ll_fe_create");
        ll_reg *reg = nullptr;
        need(ll_reg_create(0, 2, n_pts, &reg), "ll_reg_create");
        ll_voxel *vox[2];
        for (int i = 0; i < 2; i++) need(ll_voxel_create(0, 2, n_pts, &vox[i]), "ll_voxel_create");
        std::vector<float> both(scan[0]);
        both.insert(both.end(), scan[1].begin(), scan[1].end());
        const double stamps[2] = {1.0, 1.0};
        need(ll_fe_upload(fe, 0, 2, both.data(), n_pts, stamps), "ll_fe_upload");
        need(ll_fe_extract_batch(fe, 2), "ll_fe_extract_batch");
        need(ll_fe_resolve(fe), "ll_fe_resolve");
        need(ll_fe_select_batch(fe, 2, -1, 0.0f, 1.0f), "ll_fe_select_batch");

        // step 1: the extractor's features of both slots
        int32_t added[2] = {0, 0};
        hb.add(fe, poses, nullptr, nullptr, 0.0, 0.0, added);
        hb.refresh(maps);
        write_state(o, hb, maps, added);

        // step 2: the voxel-filtered stacks an enqueue with filters leaves behind, slot 0 only, gated on the poses of step 1
        ll::Point_cloud_registration pcr;
        pcr.m_para_icp_max_iterations = 2;
        pcr.m_para_cere_max_iterations = 5;
        pcr.m_current_frame_index = 100;
        pcr.m_mapping_init_accumulate_frames = 50;
        pcr.m_maximum_allow_residual_block = n_pts;
        pcr.m_subsample_seed = 0;
        pcr.enqueue_fe_maps(reg, maps, fe, vox[0], vox[1], line_res, plane_res, 2, nullptr, poses, poses);
        std::vector<double> pc(14), pi(14);
        std::vector<int32_t> res(2);
        std::vector<ll_reg_report> rep(2);
        need(ll_reg_collect(reg, 2, pc.data(), pi.data(), rep.data(), res.data()), "ll_reg_collect");
        const int32_t active[2] = {1, 0};
        hb.add(vox[0], vox[1], poses + 14, poses, active, 0.0, 0.0, added);
        hb.refresh(maps, active);
        write_state(o, hb, maps, added);

        for (int i = 0; i < 2; i++) ll_voxel_destroy(vox[i]);
        ll_reg_destroy(reg);
        ll_fe_destroy(fe);
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
