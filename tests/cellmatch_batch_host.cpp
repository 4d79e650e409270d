// Test-only: the cell-mode refresh of the batched match buffer on the CPU.  The launch chains of ll_cellmap_batch_kernels.hip (append,
// materialise) and of ll_cellmatch_batch_kernels.hip (cmb_query, cmb_scatter, cmb_replace) -- the kernels themselves, whose per-cell and
// per-point decisions are the LL_HD functions of ll_cellmatch_batch_core.h -- compiled against tests/cellmap_batch_shim and driven the
// way ll_api_history_batch.hip drives them: slot tables, frame counters, leaf counts, the capacity check and the compaction rule
// (cmb_compact_now) on the host.  Two kinds (corner, surface) with their own leaf and range, S maps each.
//
// IN : int S, T, thr, replace; float cell_res, leaf[2], radius[2], fov;
//      per step: int read; per kind, per map: int n (-1: the map sits the step out) + n * 3 floats; per map: 7 doubles (the view pose)
// OUT: per step, per kind: int n_log, n_live (after the replace), compacted (0 / 1); per map: int n_leaves + n_leaves * 3 floats (the
//      concatenation of the per-cell VoxelGrids); on a read step additionally per kind, per map the dump of
//      tests/cellmap_batch_kernels_host.cpp (frame, cells, points, ijk, cell_start, stamps, points)
#include "../loam_livox_amd/csrc/ll_cellmap_batch_kernels.hip"
#include "../loam_livox_amd/csrc/ll_cellmatch_batch_kernels.hip"
#include <stdio.h>
#include <stdlib.h>
using namespace ll;
template <typename T> static void al(T *&p, size_t n) { p = (T *)calloc(n + 8, sizeof(T)); }
static void put_i(FILE *f, int v) { fwrite(&v, 4, 1, f); }
static void rd(void *p, size_t size, size_t n, FILE *f)
{
    if (fread(p, size, n, f) != n) exit(3);
}
static const size_t CAP = 40000, MAXP = 400;
static void alloc_store(CbDev &m, int S, float res, int thr)
{
    memset(&m, 0, sizeof(m));
    m.S = S; m.geom = cell_geom(res); m.threshold = thr;
    al(m.pts, CAP); al(m.pts2, CAP); al(m.pkey, CAP); al(m.pkey2, CAP); al(m.pslot, CAP); al(m.pslot2, CAP); al(m.pep, CAP); al(m.pep2, CAP); m.cap = CAP;
    al(m.ckey, CAP); al(m.ckey2, CAP); al(m.cslot, CAP); al(m.cslot2, CAP); al(m.clast, CAP); al(m.clast2, CAP); al(m.cep, CAP); al(m.cep2, CAP); m.ccap = CAP;
    al(m.coff, S + 1); al(m.coff2, S + 1); al(m.poff, S + 1); al(m.cstart, CAP + S + 1);
    al(m.akey, CAP); al(m.akey2, CAP); al(m.aslot, CAP); al(m.aslot2, CAP); al(m.aflag, CAP); al(m.arank, CAP); m.acap = CAP;
    al(m.mkey, CAP); al(m.mkey2, CAP); al(m.mval, CAP); al(m.mval2, CAP); al(m.mslot, CAP); al(m.mslot2, CAP); m.mcap = CAP;
    m.tmp = malloc(64); m.tmp_bytes = 64; al(m.counts, 4); al(m.tab, S);
}
static void alloc_query(CmbDev &q, int S)
{
    memset(&q, 0, sizeof(q));
    al(q.csel, CAP); al(q.cflag, CAP); al(q.crank, CAP); al(q.ccell, CAP); al(q.key, CAP); al(q.key2, CAP); al(q.val, CAP); al(q.val2, CAP);
    al(q.hflag, CAP); al(q.hrank, CAP); al(q.head, CAP); al(q.leaf, CAP); al(q.leaf_cell, CAP); al(q.out, S + 4);
    q.ncap = q.ccap = CAP; q.tmp = malloc(64); q.tmp_bytes = 64;
}
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int S, T, thr, replace; float res, leaf[2], radius[2], fov;
    rd(&S, 4, 1, in); rd(&T, 4, 1, in); rd(&thr, 4, 1, in); rd(&replace, 4, 1, in); rd(&res, 4, 1, in); rd(leaf, 4, 2, in); rd(radius, 4, 2, in); rd(&fov, 4, 1, in);
    CbDev m[2]; CmbDev q[2];
    std::vector<int> frame[2];
    for (int k = 0; k < 2; k++) { alloc_store(m[k], S, res, thr); alloc_query(q[k], S); frame[k].assign(S, 0); }
    float4 *src, *concat; al(src, S * MAXP); al(concat, S * CAP);
    CmbSlot *tab; al(tab, S);
    int launches = 0, compactions = 0; const char *err = nullptr;
    for (int t = 0; t < T; t++) {
        int read; rd(&read, 4, 1, in);
        std::vector<int> act(S, 0);
        for (int k = 0; k < 2; k++) {
            long long n_new = 0; int max_n = 0;
            std::vector<int> ncb(S);
            for (int s = 0; s < S; s++) {
                ncb[s] = m[k].coff[s + 1] - m[k].coff[s];
                int n; rd(&n, 4, 1, in);
                memset(&m[k].tab[s], 0, sizeof(CbSlot));
                act[s] = n >= 0;
                if (n < 0) continue;
                for (int i = 0; i < n; i++) { float p[3]; rd(p, 4, 3, in); src[s * MAXP + i] = make_float4(p[0], p[1], p[2], 7.f); }
                m[k].tab[s].off = m[k].n_log + n_new; m[k].tab[s].n = n; m[k].tab[s].frame = frame[k][s]; m[k].tab[s].active = 1;
                n_new += n; max_n = n > max_n ? n : max_n;
            }
            if (n_new > 0) {
                if (cb_append(m[k], src, MAXP, max_n, n_new, nullptr, &launches, &err)) { printf("append: %s\n", err); return 1; }
                m[k].n_cells = m[k].counts[1];
            }
            for (int s = 0; s < S; s++) if (act[s]) frame[k][s] += cb_frame_step(ncb[s] == 0);
        }
        for (int s = 0; s < S; s++) { memset(&tab[s], 0, sizeof(CmbSlot)); rd(tab[s].pose, 8, 7, in); tab[s].active = act[s]; }
        // ---- the refresh: query both kinds, check, scatter, replace, compaction rule
        bool dirty = false;
        long long live[2] = {0, 0};
        for (int k = 0; k < 2; k++) {
            const bool run = m[k].n_log > 0 && m[k].n_cells > 0;
            for (int s = 0; s < S + 4; s++) q[k].out[s] = 0;
            if (run && cmb_query(m[k], q[k], tab, radius[k], fov, leaf[k], nullptr, &launches, &err)) { printf("query: %s\n", err); return 1; }
            const int *loff = q[k].out, n_leaves = loff[S];
            int stride = 1;
            for (int s = 0; s < S; s++) {
                const int n = loff[s + 1] - loff[s];
                if (n < 0 || (!act[s] && n)) { printf("leaf counts\n"); return 1; }
                stride = n > stride ? n : stride;
            }
            if ((size_t)stride > CAP) return 4;
            if (run && cmb_scatter(m[k], q[k], n_leaves, concat, stride, nullptr, &launches, &err)) return 1;
            live[k] = loff[S + 2];
            if (run && replace && n_leaves > 0) {
                if (cmb_replace(m[k], q[k], n_leaves, nullptr, &launches, &err)) { printf("replace: %s\n", err); return 1; }
                live[k] += n_leaves - loff[S + 1];
                dirty = true;
            }
            put_i(out, (int)m[k].n_log); put_i(out, (int)live[k]);
            for (int s = 0; s < S; s++) {
                const int n = loff[s + 1] - loff[s];
                put_i(out, n);
                for (int i = 0; i < n; i++) fwrite(&concat[(size_t)s * stride + i].x, 4, 3, out);
            }
        }
        const bool compact = dirty && (cmb_compact_now(m[0].n_log, live[0]) || cmb_compact_now(m[1].n_log, live[1]));
        put_i(out, compact ? 1 : 0);
        compactions += compact;
        if (!compact && !read) continue;
        for (int k = 0; k < 2; k++) {
            if (cb_materialise(m[k], nullptr, &launches, &err)) { printf("mat: %s\n", err); return 1; }
            m[k].n_log = m[k].poff[S];
        }
        if (!read) continue;
        for (int k = 0; k < 2; k++)
            for (int s = 0; s < S; s++) {
                const int c0 = m[k].coff[s], nc = m[k].coff[s + 1] - c0, p0 = m[k].poff[s], np = m[k].poff[s + 1] - p0;
                put_i(out, frame[k][s]); put_i(out, nc); put_i(out, np);
                for (int c = 0; c < nc; c++) { int ijk[3]; cell_unpack(m[k].ckey[c0 + c], ijk); fwrite(ijk, 4, 3, out); }
                for (int c = 0; c <= nc; c++) put_i(out, nc > 0 ? m[k].cstart[c0 + s + c] : 0);
                for (int c = 0; c < nc; c++) put_i(out, m[k].clast[c0 + c]);
                for (int i = 0; i < np; i++) fwrite(&m[k].pts[p0 + i].x, 4, 3, out);
            }
    }
    put_i(out, compactions);
    fclose(out);
    return launches > 0 ? 0 : 5;
}
