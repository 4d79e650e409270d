// Test-only: the cell-mode refresh of the batched match buffer on the CPU.  The launch chains of ll_cellmap_batch_kernels.hip (append,
// materialise) and of ll_cellmatch_batch_kernels.hip (cmb_query, cmb_scatter, cmb_replace) -- the kernels themselves, whose per-cell and
// per-point decisions are the LL_HD functions of ll_cellmatch_batch_core.h -- compiled against tests/cellmap_batch_shim and driven the
// way ll_api_history_batch_cells.hip drives them: the stores through tests/cellmap_batch_rig.h; leaf counts, the capacity check and the
// compaction rule (cmb_compact_now) on the host.  Two kinds (corner, surface) with their own leaf and range, S maps each.
//
// IN : int S, T, thr, replace; float cell_res, leaf[2], radius[2], fov;
//      per step: int read; per kind, per map: int n (-1: the map sits the step out) + n * 3 floats; per map: 7 doubles (the view pose)
// OUT: per step, per kind: int n_log, n_live (after the replace), compacted (0 / 1); per map: int n_leaves + n_leaves * 3 floats (the
//      concatenation of the per-cell VoxelGrids); on a read step additionally per kind, per map the dump of
//      tests/cellmap_batch_kernels_host.cpp (frame, cells, points, ijk, cell_start, stamps, points)
#include "../loam_livox_amd/csrc/ll_cellmap_batch_kernels.hip"
#include "../loam_livox_amd/csrc/ll_cellmatch_batch_kernels.hip"
#include "cellmap_batch_rig.h"
#include <memory>
using namespace rig;
static const size_t CAP = 40000, MAXP = 400;
static void alloc_query(Owned &own, CmbDev &q, int S)
{
    memset(&q, 0, sizeof(q));
    own.al(q.csel, CAP); own.al(q.cflag, CAP); own.al(q.crank, CAP); own.al(q.ccell, CAP); own.al(q.key, CAP); own.al(q.key2, CAP); own.al(q.val, CAP);
    own.al(q.val2, CAP); own.al(q.hflag, CAP); own.al(q.hrank, CAP); own.al(q.head, CAP); own.al(q.leaf, CAP); own.al(q.leaf_cell, CAP); own.al(q.out, S + 4);
    char *tmp; own.al(tmp, 64);
    q.ncap = q.ccap = CAP; q.tmp = tmp; q.tmp_bytes = 64;
}
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int S, T, thr, replace; float res, leaf[2], radius[2], fov;
    rd(&S, 4, 1, in); rd(&T, 4, 1, in); rd(&thr, 4, 1, in); rd(&replace, 4, 1, in); rd(&res, 4, 1, in); rd(leaf, 4, 2, in); rd(radius, 4, 2, in); rd(&fov, 4, 1, in);
    std::unique_ptr<Store> st[2];
    Owned own;
    CmbDev q[2];
    for (int k = 0; k < 2; k++) { st[k].reset(new Store(S, res, thr, CAP, MAXP)); alloc_query(own, q[k], S); }
    float4 *concat; own.al(concat, S * CAP);
    CmbSlot *tab; own.al(tab, S);
    int launches = 0, compactions = 0; const char *err = nullptr;
    for (int t = 0; t < T; t++) {
        int read; rd(&read, 4, 1, in);
        for (int k = 0; k < 2; k++) {
            st[k]->read_clouds(in);
            if (st[k]->append() < 0) return 1;
        }
        const Store &last = *st[1];  // (both kinds name the same slots)
        for (int s = 0; s < S; s++) { memset(&tab[s], 0, sizeof(CmbSlot)); rd(tab[s].pose, 8, 7, in); tab[s].active = last.active(s); }
        // ---- the refresh: query both kinds, check, scatter, replace, compaction rule
        bool dirty = false;
        long long live[2] = {0, 0};
        for (int k = 0; k < 2; k++) {
            CbDev &m = st[k]->m;
            const bool run = m.n_log > 0 && m.n_cells > 0;
            for (int s = 0; s < S + 4; s++) q[k].out[s] = 0;
            if (run && cmb_query(m, q[k], tab, radius[k], fov, leaf[k], nullptr, &launches, &err)) { printf("query: %s\n", err); return 1; }
            const int *loff = q[k].out, n_leaves = loff[S];
            int stride = 1;
            for (int s = 0; s < S; s++) {
                const int n = loff[s + 1] - loff[s];
                if (n < 0 || (!last.active(s) && n)) { printf("leaf counts\n"); return 1; }
                stride = n > stride ? n : stride;
            }
            if ((size_t)stride > CAP) return 4;
            if (run && cmb_scatter(m, q[k], n_leaves, concat, stride, nullptr, &launches, &err)) return 1;
            live[k] = loff[S + 2];
            if (run && replace && n_leaves > 0) {
                if (cmb_replace(m, q[k], n_leaves, nullptr, &launches, &err)) { printf("replace: %s\n", err); return 1; }
                live[k] += n_leaves - loff[S + 1];
                dirty = true;
            }
            put_i(out, (int)m.n_log); put_i(out, (int)live[k]);
            for (int s = 0; s < S; s++) {
                const int n = loff[s + 1] - loff[s];
                put_i(out, n);
                for (int i = 0; i < n; i++) fwrite(&concat[(size_t)s * stride + i].x, 4, 3, out);
            }
        }
        const bool compact = dirty && (cmb_compact_now(st[0]->m.n_log, live[0]) || cmb_compact_now(st[1]->m.n_log, live[1]));
        put_i(out, compact ? 1 : 0);
        compactions += compact;
        if (!compact && !read) continue;
        for (int k = 0; k < 2; k++)
            if (st[k]->materialise()) return 1;
        if (!read) continue;
        for (int k = 0; k < 2; k++) st[k]->dump(out);
    }
    put_i(out, compactions);
    fclose(in);
    fclose(out);
    return launches + st[0]->launches + st[1]->launches > 0 ? 0 : 5;
}
