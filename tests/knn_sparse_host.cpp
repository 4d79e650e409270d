// Test-only host build of the reuse-record arithmetic of ll_knn_core.h (tests/test_knn_sparse_host.py compiles it into a temporary
// directory): the order budget a search result leaves, as the tile kernel stores it, and the displacement the classification
// pass compares with it.
#include <cmath>
#include <cstdint>

#include "../loam_livox_amd/csrc/ll_knn_core.h"

using namespace ll;

extern "C" {

// m_strong of n results given as the tile search returns them: five squared distances (ascending, +inf beyond count), lb2, out2
void ks_m_strong(int n, const float *d2, const int32_t *count, const float *lb2, const float *out2, float max_d2, float *m_strong)
{
    for (int i = 0; i < n; i++) {
        Knn5 r;
        knn5_init(r);
        for (int k = 0; k < 5; k++) {
            r.d2[k] = d2[5 * i + k];
            r.pos[k] = k < count[i] ? k : -1;
        }
        r.count = count[i];
        r.lb2 = lb2[i];
        r.out2 = out2[i];
        KnnRef ref;
        knn5_make_ref(r, 0.0f, 0.0f, 0.0f, max_d2, ref);
        m_strong[i] = ref.m_strong;
    }
}

// knn5_ref_delta of n (record position, new position) pairs
void ks_delta(int n, const float *ref_xyz, const float *q_xyz, float *delta)
{
    for (int i = 0; i < n; i++) {
        KnnRef ref;
        ref.qx = ref_xyz[3 * i];
        ref.qy = ref_xyz[3 * i + 1];
        ref.qz = ref_xyz[3 * i + 2];
        delta[i] = knn5_ref_delta(ref, q_xyz[3 * i], q_xyz[3 * i + 1], q_xyz[3 * i + 2]);
    }
}
}
