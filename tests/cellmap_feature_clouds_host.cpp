// Test-only: the launch chain behind ll_cellmap_feature_clouds / ll_scene_align_run's selection step on the CPU
// (tests/test_scene_align_host.py).  The kernels of ll_cellmap_select_kernels.hip themselves, compiled against tests/cellmap_batch_shim
// and driven the way ll_api_scene_align.hip drives them: the cell labels (cm_stats_kernel's body, cell_stats of ll_cellmap_core.h, one
// cell after the other), then cellmap_select_features.  The map comes in dump form.
//
//   cellmap_feature_clouds_host IN OUT
// IN : int32 n_points, n_cells; float32 resolution; n_points x {x, y, z, w} float; n_cells uint64 cell keys; n_cells + 1 int32 cell_start.
// OUT: int32 n_line, n_plane; n_cells int32 labels; n_line x 4 float; n_plane x 4 float.
// Both clouds are allocated for exactly the points they get, with a guard band behind and a pattern in front: exit code 7 when a band
// was written, the pattern in the output where an entry that should have been written was not.  (The library gives each cloud room
// for all the map's points; the exact size here is the stricter check.)
#include <hip/hip_runtime.h>
#include "../loam_livox_amd/csrc/ll_cellmap_select_kernels.hip"
#include <stdio.h>
#include <stdlib.h>
using namespace ll;
static const size_t GUARD = 64;
template <typename T> static void al(T *&p, size_t n)
{
    p = (T *)malloc((n + GUARD) * sizeof(T));
    memset(p, 0xAB, (n + GUARD) * sizeof(T));
}
template <typename T> static bool guard_ok(const T *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)(p + n);
    for (size_t i = 0; i < GUARD * sizeof(T); i++)
        if (b[i] != 0xAB) return false;
    return true;
}
static void rd(void *p, size_t size, size_t n, FILE *f)
{
    if (n && fread(p, size, n, f) != n) exit(3);
}
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int np, nc;
    float resolution;
    rd(&np, 4, 1, in); rd(&nc, 4, 1, in); rd(&resolution, 4, 1, in);
    if (np < 0 || nc < 0 || nc > np) return 2;
    CellMapDev m; memset(&m, 0, sizeof(m));
    m.cap = np > 0 ? np : 1; m.n_pts = np; m.n_cells = nc; m.resolution = resolution; m.geom = cell_geom(resolution);
    al(m.pts, np); al(m.ckey, nc); al(m.cstart, nc + 1);
    al(m.skey, nc + 1); al(m.skey2, nc + 1);  // the scratch the chain names
    m.tmp = malloc(64); m.tmp_bytes = 64;
    rd(m.pts, sizeof(float4), np, in); rd(m.ckey, 8, nc, in); rd(m.cstart, 4, nc + 1, in);
    CellStats *stats; al(stats, nc);
    int n_line = 0, n_plane = 0;
    for (int c = 0; c < nc; c++) {  // cm_stats_kernel, one cell per thread
        int k[3];
        cell_unpack(m.ckey[c], k);
        float ctr[3];
        cell_centre(k, m.geom, ctr);
        const int first = m.cstart[c], n = m.cstart[c + 1] - first;
        cell_stats((const float *)(m.pts + first), 4, n, ctr, m.geom.box, stats[c]);
        if (stats[c].type == LL_FEATURE_LINE) n_line += n;
        if (stats[c].type == LL_FEATURE_PLANE) n_plane += n;
    }
    float4 *line, *plane;
    al(line, n_line); al(plane, n_plane);
    int *counts; al(counts, 2);
    const char *err = nullptr;
    if (cellmap_select_features(m, stats, line, plane, counts, counts + 1, nullptr, &err)) { printf("select: %s\n", err); return 1; }
    if (!guard_ok(line, n_line) || !guard_ok(plane, n_plane) || !guard_ok(counts, 2) || !guard_ok(m.skey, nc + 1) || !guard_ok(m.skey2, nc + 1)) return 7;
    fwrite(counts, 4, 2, out);
    for (int c = 0; c < nc; c++) fwrite(&stats[c].type, 4, 1, out);
    fwrite(line, sizeof(float4), counts[0] == n_line ? n_line : 0, out);
    fwrite(plane, sizeof(float4), counts[1] == n_plane ? n_plane : 0, out);
    fclose(out);
    return 0;
}
