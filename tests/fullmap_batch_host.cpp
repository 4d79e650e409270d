// Test-only: the full-cloud maps of the batched match buffer on the CPU (tests/test_fullmap_batch_host.py).  The launch chains of an
// ll_history_batch_append_full_fe -- fb_gather, cb_append on a third store, fb_touched_chain -- and cb_materialise, the kernels of
// ll_fullmap_batch_kernels.hip and ll_cellmap_batch_kernels.hip themselves, compiled against tests/cellmap_batch_shim and driven
// through tests/cellmap_batch_rig.h and fb_fill_slots, the host functions ll_api_history_batch_stores.hip drives them with.  The clouds
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
#include "cellmap_batch_rig.h"
using namespace rig;
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int S, T, thr, min_points; float res;
    rd(&S, 4, 1, in); rd(&T, 4, 1, in); rd(&thr, 4, 1, in); rd(&min_points, 4, 1, in); rd(&res, 4, 1, in);
    const size_t CAP = 20000, MAXP = 400;
    Store st(S, res, thr, CAP, MAXP);
    CbDev &m = st.m;
    Owned own;
    FbDev t; memset(&t, 0, sizeof(t));
    own.al(t.xf, S * MAXP); own.al(t.tab, S); own.al(t.cnt, CAP); own.al(t.flag, CAP); own.al(t.rank, CAP); own.al(t.cells, 3 * CAP); t.tcap = CAP; own.al(t.toff, S + 1);
    char *tmp; own.al(tmp, 64); t.tmp = tmp; t.tmp_bytes = 64;
    std::vector<std::vector<int>> lists(S);
    std::vector<double> poses(7 * (size_t)S, 0.0);
    for (int s = 0; s < S; s++) poses[7 * s + 3] = 1.0;
    float4 *xyzi; own.al(xyzi, S * MAXP);
    int *full_idx; own.al(full_idx, S * MAXP);
    int mats = 0; const char *err = nullptr;
    for (int step = 0; step < T; step++) {
        int read; rd(&read, 4, 1, in);
        st.read_clouds(in);
        for (int s = 0; s < S; s++)
            for (int i = 0; i < st.n[s]; i++) {  // point i of the cloud lies at n - 1 - i of the scan
                xyzi[s * MAXP + (st.n[s] - 1 - i)] = st.src[s * MAXP + i];
                full_idx[s * MAXP + i] = st.n[s] - 1 - i;
            }
        int max_n = 0;
        const long long n_new = fb_fill_slots(m.tab, t.tab, S, [&](int s) { return st.n[s]; }, st.frame.data(), st.coff.data(), min_points, poses.data(),
                                              m.n_log, &max_n);
        if (n_new > 0) {
            const int n_upper = m.n_cells + (int)n_new;
            if (fb_gather(t, xyzi, full_idx, (int)MAXP, S, (int)MAXP, max_n, nullptr, &st.launches, &err)) { printf("gather: %s\n", err); return 1; }
            if (cb_append(m, t.xf, MAXP, max_n, n_new, nullptr, &st.launches, &err)) { printf("append: %s\n", err); return 1; }
            if (fb_touched_chain(m, t, max_n, n_upper, nullptr, &st.launches, &err)) { printf("touched: %s\n", err); return 1; }
        }
        st.end_append(n_new > 0);
        for (int s = 0; s < S; s++) {
            if (st.active(s)) lists[s].clear();
            if (st.active(s) && n_new > 0) lists[s].assign(t.cells + 3 * t.toff[s], t.cells + 3 * t.toff[s + 1]);
            put_i(out, (int)lists[s].size() / 3);
            if (!lists[s].empty()) fwrite(lists[s].data(), 4, lists[s].size(), out);
        }
        if (!read) continue;
        if (st.materialise()) return 1;
        mats++;
        st.dump(out);
    }
    put_i(out, mats);
    fclose(in);
    fclose(out);
    return st.launches > 0 ? 0 : 5;
}
