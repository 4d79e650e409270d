// Points_cloud_map::extract_cells of include/loam_livox_adapter.hpp (tests/test_gpu_cellmap_extract.py).
// argv: <cloud.bin> <cells.bin> <out.txt>  (raw float32 xyzi rows; raw int32 ijk rows)
// out.txt: "cells points frame capacity_ok" of the extracted map, then an FNV-1a checksum of its dump (points, cell indices,
// cell_start, stamps), then the same two lines after a second, smaller extraction into the same destination.
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

static void report(FILE *out, loam_livox_hip::Points_cloud_map &m, int64_t n_found, int64_t n_points)
{
    int64_t nc = 0, np = 0;
    int32_t frame = 0;
    if (ll_cellmap_stats(m.handle(), &nc, &np, &frame) != 0) exit(4);
    std::vector<float> xyzi((size_t)(np > 0 ? np : 1) * 4);
    std::vector<int32_t> ijk((size_t)(nc > 0 ? nc : 1) * 3), start((size_t)nc + 1), last((size_t)(nc > 0 ? nc : 1));
    if (ll_cellmap_dump(m.handle(), xyzi.data(), np > 0 ? np : 1, ijk.data(), start.data(), last.data(), nc > 0 ? nc : 1) != 0) exit(4);
    unsigned long long h = 14695981039346656037ull;
    h = fnv(h, xyzi.data(), (size_t)np * 16);
    h = fnv(h, ijk.data(), (size_t)nc * 12);
    h = fnv(h, start.data(), (size_t)(nc + 1) * 4);
    h = fnv(h, last.data(), (size_t)nc * 4);
    fprintf(out, "%lld %lld %d %d\n%llu\n", (long long)nc, (long long)np, (int)frame, (int)(nc == n_found && np == n_points), h);
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const std::vector<float> raw = read_all<float>(argv[1]);
    const std::vector<int32_t> cells = read_all<int32_t>(argv[2]);
    Cloud cloud;
    for (size_t i = 0; i + 3 < raw.size(); i += 4) cloud.points.push_back(PointXYZI{raw[i], raw[i + 1], raw[i + 2], raw[i + 3]});
    std::vector<std::array<int, 3>> list;
    for (size_t i = 0; i + 2 < cells.size(); i += 3) list.push_back(std::array<int, 3>{cells[i], cells[i + 1], cells[i + 2]});
    FILE *out = fopen(argv[3], "w");
    if (!out) return 2;
    loam_livox_hip::Points_cloud_map full((int64_t)cloud.points.size() + 1, 1.0f), key_frame(1024, 1.0f);  // the destination has to grow
    full.append_cloud(cloud);
    int64_t n_points = 0;
    int64_t n_found = full.extract_cells(list, key_frame, &n_points);
    report(out, key_frame, n_found, n_points);
    list.resize(list.size() / 4);
    n_found = full.extract_cells(list, key_frame, &n_points);
    report(out, key_frame, n_found, n_points);
    fclose(out);
    return 0;
}
