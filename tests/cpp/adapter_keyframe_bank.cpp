// Keyframe_bank of include/loam_livox_adapter.hpp (tests/test_gpu_keyframe_bank.py).
// argv: <images.bin> <n_entries> <out.txt>  (per entry the line image, then the plane image, 60 x 60 float32 each)
// out.txt: the entries held; then, for every ordered pair (a, b) with a and b in 0 .. n_entries - 1, a-major, one line "sim_line
// sim_plane" as hexadecimal floats -- all from ONE match; last the work tap's four values.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/loam_livox_adapter.hpp"

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const int n = atoi(argv[2]);
    if (n < 1 || n > 64) return 2;
    std::vector<float> img((size_t)n * 2 * 3600);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(img.data(), sizeof(float), img.size(), f) != img.size()) return 3;
    fclose(f);
    loam_livox_hip::Keyframe_bank bank(2);  // (the bank has to grow)
    for (int e = 0; e < n; e++)
        if (bank.add(&img[(size_t)e * 7200], &img[(size_t)e * 7200 + 3600]) != e) return 4;
    std::vector<int64_t> ids_a, ids_b;
    for (int a = 0; a < n; a++)
        for (int b = 0; b < n; b++) ids_a.push_back(a), ids_b.push_back(b);
    std::vector<float> sim_line, sim_plane;
    bank.match(ids_a, ids_b, sim_line, sim_plane);
    FILE *out = fopen(argv[3], "w");
    if (!out) return 2;
    fprintf(out, "%lld\n", (long long)bank.size());
    for (size_t p = 0; p < ids_a.size(); p++) fprintf(out, "%a %a\n", (double)sim_line[p], (double)sim_plane[p]);
    int64_t work[4];
    bank.work(work);
    fprintf(out, "%lld %lld %lld %lld\n", (long long)work[0], (long long)work[1], (long long)work[2], (long long)work[3]);
    fclose(out);
    return 0;
}
