// History_batch::extract_cells of include/loam_livox_adapter.hpp (tests/test_gpu_cellmap_batch_extract.py): two sequences in one
// handle with cell maps, one add of a batched extractor's features, then the surface cells named in two lists copied into two
// Points_cloud_map in ONE call, the requests in the order {slot 1, slot 0}; the destinations start at 16 points.
// argv: scan_a.bin scan_b.bin (n x xyzi float32, equally many points) poses.bin (2 x 7 doubles) cells_a.bin cells_b.bin (int32 ijk
// rows) out.txt.  out.txt, per slot 0 and 1: "cells points frame counts_ok" and an FNV-1a checksum of the destination's dump
// (points, cell indices, cell_start, stamps).
#include <cstdio>
#include <cstdlib>
#include <vector>

#define LOAM_LIVOX_ADAPTER_NO_EIGEN
#include "loam_livox_adapter.hpp"

namespace ll = loam_livox_hip;

template <typename T>
static std::vector<T> read_all(const char *path)
{
    std::vector<T> v;
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(3);
    fclose(f);
    return v;
}

static unsigned long long fnv(unsigned long long h, const void *p, size_t bytes)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < bytes; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

static void need(int rc, const char *what)
{
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + ll_last_error());
}

static void report(FILE *out, ll::Points_cloud_map &m, int64_t n_found, int64_t n_points)
{
    int64_t nc = 0, np = 0;
    int32_t frame = 0;
    need(ll_cellmap_stats(m.handle(), &nc, &np, &frame), "ll_cellmap_stats");
    std::vector<float> xyzi((size_t)(np > 0 ? np : 1) * 4);
    std::vector<int32_t> ijk((size_t)(nc > 0 ? nc : 1) * 3), start((size_t)nc + 1), last((size_t)(nc > 0 ? nc : 1));
    need(ll_cellmap_dump(m.handle(), xyzi.data(), np > 0 ? np : 1, ijk.data(), start.data(), last.data(), nc > 0 ? nc : 1), "ll_cellmap_dump");
    unsigned long long h = 14695981039346656037ull;
    h = fnv(h, xyzi.data(), (size_t)np * 16);
    h = fnv(h, ijk.data(), (size_t)nc * 12);
    h = fnv(h, start.data(), (size_t)(nc + 1) * 4);
    h = fnv(h, last.data(), (size_t)nc * 4);
    fprintf(out, "%lld %lld %d %d\n%llu\n", (long long)nc, (long long)np, (int)frame, (int)(nc == n_found && np == n_points), h);
}

static std::vector<std::array<int, 3>> triples(const std::vector<int32_t> &v)
{
    std::vector<std::array<int, 3>> list;
    for (size_t i = 0; i + 2 < v.size(); i += 3) list.push_back(std::array<int, 3>{v[i], v[i + 1], v[i + 2]});
    return list;
}

int main(int argc, char **argv)
{
    if (argc != 7) return 2;
    std::vector<float> scan[2] = {read_all<float>(argv[1]), read_all<float>(argv[2])};
    if (scan[0].empty() || scan[0].size() != scan[1].size()) return 3;
    const std::vector<double> poses = read_all<double>(argv[3]);
    if (poses.size() != 14) return 3;
    const std::vector<std::array<int, 3>> cells[2] = {triples(read_all<int32_t>(argv[4])), triples(read_all<int32_t>(argv[5]))};
    FILE *out = fopen(argv[6], "w");
    if (!out) return 3;
    const int n_pts = (int)(scan[0].size() / 4);
    try {
        ll::History_batch hb(2, 3, n_pts, 0.1f, 0.4f);
        hb.enable_cell_maps(n_pts, 1.0f, 5000);
        ll_fe_params fp;
        ll_fe_default_params(&fp);
        fp.max_points = n_pts, fp.max_scans = 2, fp.piecewise_number = 1;
        ll_fe *fe = nullptr;
        need(ll_fe_create(&fp, &fe), "ll_fe_create");
        std::vector<float> both(scan[0]);
        both.insert(both.end(), scan[1].begin(), scan[1].end());
        const double stamps[2] = {1.0, 1.0};
        need(ll_fe_upload(fe, 0, 2, both.data(), n_pts, stamps), "ll_fe_upload");
        need(ll_fe_extract_batch(fe, 2), "ll_fe_extract_batch");
        need(ll_fe_resolve(fe), "ll_fe_resolve");
        need(ll_fe_select_batch(fe, 2, -1, 0.0f, 1.0f), "ll_fe_select_batch");
        int32_t added[2] = {0, 0};
        hb.add(fe, poses.data(), nullptr, nullptr, 0.0, 0.0, added);
        {
            ll::Points_cloud_map key_a(16, 1.0f), key_b(16, 1.0f);  // the destinations have to grow
            std::vector<int64_t> n_points;
            const std::vector<ll::Points_cloud_map *> dst = {&key_b, &key_a};
            const std::vector<int64_t> n_found = hb.extract_cells(1, {1, 0}, {cells[1], cells[0]}, dst, &n_points);
            report(out, key_a, n_found[1], n_points[1]);
            report(out, key_b, n_found[0], n_points[0]);
        }
        ll_fe_destroy(fe);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        fclose(out);
        return 4;
    }
    fclose(out);
    return 0;
}
