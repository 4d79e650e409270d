// Test-only: ll_history_batch_extract_cells' launch chain on the CPU (tests/test_cellmap_batch_extract_host.py).  The kernels of
// ll_cellmap_batch_extract_kernels.hip and of ll_cellmap_batch_kernels.hip themselves, compiled against tests/cellmap_batch_shim and
// driven the way ll_api_history_batch_extract.hip drives them: appends and materialisations build the store of S slots
// (tests/cellmap_batch_rig.h); an extraction stages the requests with cxb_stage, runs cxb_mark, reads the totals, gives every request a destination with room for exactly
// its points, and runs cxb_extract.  Also built as it stands with -fsanitize=address,undefined: every buffer is freed at the end.
//
//   cellmap_batch_extract_host IN OUT
// IN : int32 S, float resolution, then operations until the end of the file, each led by an int32:
//      1 append       per slot int32 n (-1: the slot sits out) and n x {x, y, z} float
//      2 materialise
//      3 extract      int32 R, R int32 slots, R + 1 int32 list offsets, offsets[R] x 3 int32 cell indices
//      4 dump         the store, per slot
// OUT: per dump and slot  int32 n_cells, n_points; n_cells uint64 keys; n_cells + 1 int32 cell_start; n_points x 4 float; n_points
//      uint64 point keys.  Per extraction and request (in the caller's order)  int32 found, points, frame, host mirrors n_cells, n_pts;
//      found uint64 keys; found + 1 int32 cell_start (one 0 when found == 0); found int32 stamps; points x 4 float; points uint64.
// Every destination array has a guard band behind the part the call may write and is filled with a pattern first: exit code 7 when
// a band was written, the pattern in the output where an entry that should have been written was not.
#include <hip/hip_runtime.h>
#include "../loam_livox_amd/csrc/ll_cellmap_batch_kernels.hip"
#include "../loam_livox_amd/csrc/ll_cellmap_batch_extract_kernels.hip"
#include "cellmap_batch_rig.h"
using namespace rig;
static const size_t GUARD = 64;
// what the call changes of a destination cell map: its live arrays and host mirrors
struct Dst {
    int cap, frame, n_pts, n_cells, n_filt, n_sel;
    float4 *pts;
    unsigned long long *pkey, *ckey;
    int *cstart, *clast;
};
template <typename T> static void alg(T *&p, size_t n)
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
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int S; float res;
    rd(&S, 4, 1, in); rd(&res, 4, 1, in);
    if (S < 1 || S > 64) return 2;
    Store st(S, res, 1 << 30, 20000, 1200);
    CbDev &m = st.m;
    int &launches = st.launches;
    int rc = 0, op; const char *err = nullptr;
    bool ordered = true;
    while (rc == 0 && fread(&op, 4, 1, in) == 1) {
        if (op == 1) {
            st.read_clouds(in);
            const long long n_new = st.append();
            if (n_new < 0) { rc = 1; break; }
            if (n_new > 0) ordered = false;
        } else if (op == 2) {
            if (st.materialise()) { rc = 1; break; }
            ordered = true;
        } else if (op == 4) {
            if (!ordered) { rc = 6; break; }
            for (int s = 0; s < S; s++) {
                const int c0 = m.coff[s], nc = m.coff[s + 1] - c0, p0 = m.poff[s], np = m.poff[s + 1] - p0;
                put_i(out, nc); put_i(out, np);
                fwrite(m.ckey + c0, 8, nc, out);
                for (int c = 0; c <= nc; c++) put_i(out, nc > 0 ? m.cstart[c0 + s + c] : 0);
                fwrite(m.pts + p0, sizeof(float4), np, out);
                fwrite(m.pkey + p0, 8, np, out);
            }
        } else if (op == 3) {
            if (!ordered) { rc = 6; break; }
            int R; rd(&R, 4, 1, in);
            if (R < 1 || R > S) return 2;
            std::vector<int> seq(R), off(R + 1);
            rd(seq.data(), 4, R, in); rd(off.data(), 4, R + 1, in);
            if (off[0] != 0) return 2;  // (the lists start at the first triple of the operation)
            const int n_list = off[R];
            std::vector<int> order(R), ijk((size_t)3 * n_list + 1), d_in(cxb_in_ints(R, n_list)), d_out(cxb_out_ints(R));
            rd(ijk.data(), 4, (size_t)3 * n_list, in);
            cxb_stage(d_in.data(), order.data(), R, seq.data(), off.data(), ijk.data());
            std::vector<Dst> dst(R);
            std::vector<CxbDst> tab(R);
            bool made = false;
            if (cxb_mark(m, d_in.data(), R, n_list, d_out.data(), nullptr, &launches, &err)) { printf("mark: %s\n", err); rc = 1; }
            if (rc == 0) {
                const CxbOut o = cxb_out(d_out.data(), R);
                const int *found = o.found, *points = o.points;
                for (int q = 0; q < R; q++) {
                    Dst &d = dst[order[q]]; memset(&d, 0, sizeof(d));
                    d.cap = points[q] > 0 ? points[q] : 1; d.frame = 5; d.n_pts = 3; d.n_cells = 2; d.n_filt = 1; d.n_sel = 1;  // (a used map)
                    alg(d.pts, points[q]); alg(d.pkey, points[q]); alg(d.ckey, found[q]); alg(d.cstart, found[q] + 1); alg(d.clast, found[q]);
                    tab[q] = CxbDst{d.ckey, d.cstart, d.clast, d.pts, d.pkey};
                }
                made = true;
                if (cxb_extract(m, d_in.data(), R, d_out.data(), tab.data(), o.qrank[R], o.qpos[R], nullptr, &launches, &err)) { printf("extract: %s\n", err); rc = 1; }
                for (int q = 0; q < R && rc == 0; q++) {
                    Dst &d = dst[order[q]];
                    if (!guard_ok(d.pts, points[q]) || !guard_ok(d.pkey, points[q]) || !guard_ok(d.ckey, found[q]) || !guard_ok(d.cstart, found[q] + 1) ||
                        !guard_ok(d.clast, found[q]))
                        rc = 7;
                    d.n_pts = points[q]; d.n_cells = points[q] > 0 ? found[q] : 0; d.frame = points[q] > 0 ? 2 : 0; d.n_filt = d.n_sel = 0;
                }
                for (int r = 0; r < R && rc == 0; r++) {
                    int q = 0;
                    while (order[q] != r) q++;
                    const Dst &d = dst[r];
                    const int head[5] = {found[q], points[q], d.frame, d.n_cells, d.n_pts};
                    fwrite(head, 4, 5, out);
                    fwrite(d.ckey, 8, found[q], out);
                    if (found[q] > 0) fwrite(d.cstart, 4, found[q] + 1, out);
                    else put_i(out, 0);
                    fwrite(d.clast, 4, found[q], out);
                    fwrite(d.pts, sizeof(float4), points[q], out);
                    fwrite(d.pkey, 8, points[q], out);
                }
            }
            if (made)
                for (int r = 0; r < R; r++) { free(dst[r].pts); free(dst[r].pkey); free(dst[r].ckey); free(dst[r].cstart); free(dst[r].clast); }
        } else {
            rc = 2;
        }
    }
    fclose(in);
    fclose(out);
    return rc ? rc : (launches > 0 ? 0 : 5);
}
