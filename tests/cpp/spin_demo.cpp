// Spinning_laser of include/loam_livox_adapter.hpp called the way INTEGRATION.md section 6 places it in the feature node:
// one message in, the five published clouds out.  argv: scan.bin (n x xyzi float32) scan_line out.bin (five clouds, int32 n + n x xyzi).
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

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    Cloud in;
    float v[4];
    while (fread(v, 4, 4, f) == 4) in.points.push_back({v[0], v[1], v[2], v[3]});
    fclose(f);
    loam_livox_hip::Spinning_laser spin;
    spin.scan_line = atoi(argv[2]);
    Cloud full, sharp, less_sharp, flat, less_flat;
    try {
        spin.extract(in, full, sharp, less_sharp, flat, less_flat);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 4;
    }
    FILE *o = fopen(argv[3], "wb");
    if (!o) return 3;
    for (const Cloud *c : {&full, &sharp, &less_sharp, &flat, &less_flat}) {
        const int n = (int)c->points.size();
        fwrite(&n, 4, 1, o);
        for (const PointXYZI &p : c->points) fwrite(&p, 4, 4, o);
    }
    fclose(o);
    return 0;
}
