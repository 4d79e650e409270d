// Test-only: ll_cellmap_extract_cells' launch chain on the CPU (tests/test_cellmap_extract_host.py).  The kernels of
// ll_cellmap_extract_kernels.hip themselves, compiled against tests/cellmap_batch_shim and driven the way ll_api_cellmap.hip drives
// them: cellmap_extract_mark on the source, the two totals read, a destination with room for exactly that many points, then
// cellmap_extract_cells.  The source map comes in dump form.
//
//   cellmap_extract_host IN OUT
// IN : int32 n_points, n_cells, n_list; n_points x {x, y, z, w} float; n_points uint64 point keys; n_cells uint64 cell keys;
//      n_cells + 1 int32 cell_start; n_list x 3 int32.
// OUT: int32 n_found, n_points, frame, host mirrors n_cells, n_pts; n_found uint64 cell keys; n_found + 1 int32 cell_start (one 0
//      when n_found == 0); n_found int32 stamps; n_points x 4 float; n_points uint64 point keys.
// Every destination array is allocated with a guard band behind the part the call may write and filled with a pattern first: exit
// code 7 when the band was written, the pattern in the output where an entry that should have been written was not.
#include <hip/hip_runtime.h>
#include "../loam_livox_amd/csrc/ll_cellmap_extract_kernels.hip"
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
    int np, nc, nl;
    rd(&np, 4, 1, in); rd(&nc, 4, 1, in); rd(&nl, 4, 1, in);
    if (np < 0 || nc < 0 || nl < 0 || nc > np) return 2;
    CellMapDev s; memset(&s, 0, sizeof(s));
    s.cap = np > 0 ? np : 1; s.n_pts = np; s.n_cells = nc; s.frame = 9;
    al(s.pts, np); al(s.pkey, np); al(s.ckey, nc); al(s.cstart, nc + 1);
    al(s.skey, nc + 1); al(s.skey2, nc + 1); al(s.flag, nc + 1);  // the scratch the chain names
    s.tmp = malloc(64); s.tmp_bytes = 64;
    int *ijk; al(ijk, 3 * (size_t)nl);
    rd(s.pts, sizeof(float4), np, in); rd(s.pkey, 8, np, in); rd(s.ckey, 8, nc, in); rd(s.cstart, 4, nc + 1, in); rd(ijk, 4, 3 * (size_t)nl, in);
    if (nc == 0) s.cstart[0] = 0;
    const char *err = nullptr;
    if (cellmap_extract_mark(s, nl ? ijk : nullptr, nl, nullptr, &err)) { printf("mark: %s\n", err); return 1; }
    const unsigned long long totals = s.skey2[nc];
    const int found = (int)(totals >> 32), points = (int)(totals & 0xffffffffu);
    CellMapDev d; memset(&d, 0, sizeof(d));
    d.cap = points > 0 ? points : 1; d.frame = 5; d.n_pts = 3; d.n_cells = 2; d.n_filt = 1; d.n_sel = 1;  // (a used map: all of it must go)
    al(d.pts, points); al(d.pkey, points); al(d.ckey, found); al(d.cstart, found + 1); al(d.clast, found);
    if (cellmap_extract_cells(s, d, found, points, nullptr, &err)) { printf("extract: %s\n", err); return 1; }
    if (!guard_ok(d.pts, points) || !guard_ok(d.pkey, points) || !guard_ok(d.ckey, found) || !guard_ok(d.cstart, found + 1) || !guard_ok(d.clast, found) ||
        !guard_ok(s.skey, nc + 1) || !guard_ok(s.skey2, nc + 1) || !guard_ok(s.flag, nc + 1))
        return 7;
    if (d.n_filt != 0 || d.n_sel != 0) return 8;
    const int head[5] = {found, points, d.frame, d.n_cells, d.n_pts};
    fwrite(head, 4, 5, out);
    fwrite(d.ckey, 8, found, out);
    if (found > 0) fwrite(d.cstart, 4, found + 1, out);
    else { const int z = 0; fwrite(&z, 4, 1, out); }
    fwrite(d.clast, 4, found, out);
    fwrite(d.pts, sizeof(float4), points, out);
    fwrite(d.pkey, 8, points, out);
    fclose(out);
    return 0;
}
