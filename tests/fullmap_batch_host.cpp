// Test-only: the full-cloud maps of the batched match buffer on the CPU (tests/test_fullmap_batch_host.py).  The launch chains of an
// ll_history_batch_append_full_fe -- fb_gather, cb_append on a third store, fb_touched_chain -- and cb_materialise, the kernels of
// ll_fullmap_batch_kernels.hip and ll_cellmap_batch_kernels.hip themselves, compiled against tests/cellmap_batch_shim and driven the
// way ll_api_history_batch.hip drives them: slot tables, thresholds (fb_need), frame counters and cell counts on the host.  The clouds
// are gathered through a reversed index table with the identity pose, which leaves every finite coordinate as it is.
//
//   fullmap_batch_host IN OUT
// IN : int32 n_maps, n_steps, threshold, min_points; float resolution; per step: int32 read; per map: int32 n (-1: the map sits the
//      step out), n x 3 float.
// OUT: after every step, per map: int32 n_touched of the list the map holds, n_touched x 3 int32; after a step with read != 0
//      additionally per map the dump of tests/cellmap_batch_kernels_host.cpp (frame, n_cells, n_points, cell indices, cell_start,
//      stamps, points).  Last: int32 materialisations.
#include <hip/hip_runtime.h>
static inline int atomicAdd(int *p, int v) { int o = *p; *p += v; return o; }
#include "../loam_livox_amd/csrc/ll_cellmap_batch_kernels.hip"
#include "../loam_livox_amd/csrc/ll_fullmap_batch_kernels.hip"
#include <stdio.h>
#include <stdlib.h>
using namespace ll;
template <typename T> static void al(T *&p, size_t n) { p = (T *)calloc(n + 8, sizeof(T)); }
static void put_i(FILE *f, int v) { fwrite(&v, 4, 1, f); }
static void rd(void *p, size_t size, size_t n, FILE *f)
{
    if (fread(p, size, n, f) != n) exit(3);
}
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int S, T, thr, min_points; float res;
    rd(&S, 4, 1, in); rd(&T, 4, 1, in); rd(&thr, 4, 1, in); rd(&min_points, 4, 1, in); rd(&res, 4, 1, in);
    const size_t CAP = 20000, MAXP = 400;
    CbDev m; memset(&m, 0, sizeof(m));
    m.S = S; m.geom = cell_geom(res); m.threshold = thr;
    al(m.pts, CAP); al(m.pts2, CAP); al(m.pkey, CAP); al(m.pkey2, CAP); al(m.pslot, CAP); al(m.pslot2, CAP); al(m.pep, CAP); al(m.pep2, CAP); m.cap = CAP;
    al(m.ckey, CAP); al(m.ckey2, CAP); al(m.cslot, CAP); al(m.cslot2, CAP); al(m.clast, CAP); al(m.clast2, CAP); al(m.cep, CAP); al(m.cep2, CAP); m.ccap = CAP;
    al(m.coff, S + 1); al(m.coff2, S + 1); al(m.poff, S + 1); al(m.cstart, CAP + S + 1);
    al(m.akey, CAP); al(m.akey2, CAP); al(m.aslot, CAP); al(m.aslot2, CAP); al(m.aflag, CAP); al(m.arank, CAP); m.acap = CAP;
    al(m.mkey, CAP); al(m.mkey2, CAP); al(m.mval, CAP); al(m.mval2, CAP); al(m.mslot, CAP); al(m.mslot2, CAP); m.mcap = CAP;
    m.tmp = malloc(64); m.tmp_bytes = 64; al(m.counts, 4); al(m.tab, S);
    FbDev t; memset(&t, 0, sizeof(t));
    al(t.xf, S * MAXP); al(t.tab, S); al(t.cnt, CAP); al(t.flag, CAP); al(t.rank, CAP); al(t.cells, 3 * CAP); t.tcap = CAP; al(t.toff, S + 1);
    t.tmp = malloc(64); t.tmp_bytes = 64;
    std::vector<int> frame(S, 0);
    std::vector<std::vector<int>> lists(S);
    float4 *xyzi; al(xyzi, S * MAXP);
    int *full_idx; al(full_idx, S * MAXP);
    int mats = 0, launches = 0; const char *err = nullptr;
    for (int step = 0; step < T; step++) {
        int read; rd(&read, 4, 1, in);
        long long n_new = 0; int max_n = 0;
        std::vector<int> act(S, 0), ncb(S);
        for (int s = 0; s < S; s++) {
            ncb[s] = m.coff[s + 1] - m.coff[s];
            int n; rd(&n, 4, 1, in);
            memset(&m.tab[s], 0, sizeof(CbSlot));
            memset(&t.tab[s], 0, sizeof(FbSlot));
            if (n < 0) continue;
            if ((size_t)n > MAXP) return 6;
            for (int i = 0; i < n; i++) {  // point i of the cloud lies at n - 1 - i of the scan
                float p[3]; rd(p, 4, 3, in);
                xyzi[s * MAXP + (n - 1 - i)] = make_float4(p[0], p[1], p[2], 7.f);
                full_idx[s * MAXP + i] = n - 1 - i;
            }
            m.tab[s].off = m.n_log + n_new; m.tab[s].n = n; m.tab[s].frame = frame[s]; m.tab[s].active = 1; act[s] = 1;
            t.tab[s].n = n; t.tab[s].active = 1; t.tab[s].need = fb_need(ncb[s] == 0, min_points); t.tab[s].pose[3] = 1.0;
            n_new += n; max_n = n > max_n ? n : max_n;
        }
        if (n_new > 0) {
            const int n_upper = m.n_cells + (int)n_new;
            if (fb_gather(t, xyzi, full_idx, (int)MAXP, S, (int)MAXP, max_n, nullptr, &launches, &err)) { printf("gather: %s\n", err); return 1; }
            if (cb_append(m, t.xf, MAXP, max_n, n_new, nullptr, &launches, &err)) { printf("append: %s\n", err); return 1; }
            if (fb_touched_chain(m, t, max_n, n_upper, nullptr, &launches, &err)) { printf("touched: %s\n", err); return 1; }
            m.n_cells = m.counts[1];
        }
        for (int s = 0; s < S; s++) {
            if (!act[s]) continue;
            frame[s] += cb_frame_step(ncb[s] == 0);
            lists[s].clear();
            if (n_new > 0) lists[s].assign(t.cells + 3 * t.toff[s], t.cells + 3 * t.toff[s + 1]);
        }
        for (int s = 0; s < S; s++) {
            put_i(out, (int)lists[s].size() / 3);
            if (!lists[s].empty()) fwrite(lists[s].data(), 4, lists[s].size(), out);
        }
        if (!read) continue;
        if (cb_materialise(m, nullptr, &launches, &err)) { printf("mat: %s\n", err); return 1; }
        m.n_log = m.poff[S]; mats++;
        for (int s = 0; s < S; s++) {
            const int c0 = m.coff[s], nc = m.coff[s + 1] - c0, p0 = m.poff[s], np = m.poff[s + 1] - p0;
            put_i(out, frame[s]); put_i(out, nc); put_i(out, np);
            for (int c = 0; c < nc; c++) { int k[3]; cell_unpack(m.ckey[c0 + c], k); fwrite(k, 4, 3, out); }
            for (int c = 0; c <= nc; c++) put_i(out, nc > 0 ? m.cstart[c0 + s + c] : 0);
            for (int c = 0; c < nc; c++) put_i(out, m.clast[c0 + c]);
            for (int i = 0; i < np; i++) fwrite(&m.pts[p0 + i].x, 4, 3, out);
        }
    }
    put_i(out, mats);
    fclose(out);
    return launches > 0 ? 0 : 5;
}
