// Test-only: the launch chains of the batched cell maps -- cb_append and cb_materialise of ll_cellmap_batch_kernels.hip, the kernels
// themselves, not a restatement -- compiled for the CPU against tests/cellmap_batch_shim and driven through tests/cellmap_batch_rig.h:
// the host functions ll_api_history_batch_stores.hip drives them with.  Same IN / OUT files as tests/cellmap_batch_host.cpp.
#include "../loam_livox_amd/csrc/ll_cellmap_batch_kernels.hip"
#include "cellmap_batch_rig.h"
using namespace rig;
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int S, T, thr; float res;
    rd(&S, 4, 1, in); rd(&T, 4, 1, in); rd(&thr, 4, 1, in); rd(&res, 4, 1, in);
    Store st(S, res, thr, 20000, 400);
    int mats = 0;
    for (int t = 0; t < T; t++) {
        int read; rd(&read, 4, 1, in);
        st.read_clouds(in);
        if (st.append() < 0) return 1;
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
