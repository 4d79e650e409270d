// The map refinement's arithmetic and plan on the CPU (tests/test_map_refine_host.py): the chain of ll_map_refine_kernels.hip run from
// the text the kernels run -- mr_filter_input, mr_key, mr_centroid, mr_output of loam_livox_amd/csrc/ll_map_refine_core.h, voxel_params
// and voxel_index of ll_voxel_core.h -- over the plan the C ABI makes (mr_plan of ll_map_refine.h), with a stable sort between them.
//   map_refine_host chain <in.bin> <out.bin>
//       in : int32 mode, float leaf, int32 n_clouds, int64 off[n_clouds + 1], float store[off[n_clouds]][4], int32 n_sel, int64 ids[n_sel],
//            double ori[n_sel][7], double opm[n_sel][7]
//       out: int64 offsets[n_sel + 1], int32 status[n_sel], float points[offsets[n_sel]][4]
//   map_refine_host affine <in.bin> <out.bin>
//       in : int32 n_pairs, int32 n_pts, then per pair double ori[7], opm[7], float pts[n_pts][3]
//       out: per pair float R[9], T[3], moved[n_pts][3]
//   map_refine_host refusals        prints "<case>: <text>" for every argument check of a run
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>

#include "ll_map_refine.h"

using namespace ll;

struct P4 {
    float x, y, z, w;
};

template <typename T>
static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return v;
}

static int chain(const char *pin, const char *pout)
{
    FILE *f = fopen(pin, "rb");
    if (!f) return 2;
    const int mode = take<int32_t>(f, 1)[0];
    const float leaf = take<float>(f, 1)[0];
    const int n_clouds = take<int32_t>(f, 1)[0];
    const std::vector<int64_t> off = take<int64_t>(f, (size_t)n_clouds + 1);
    const std::vector<P4> store = take<P4>(f, (size_t)off.back());
    const int n_sel = take<int32_t>(f, 1)[0];
    const std::vector<int64_t> ids = take<int64_t>(f, (size_t)n_sel);
    const std::vector<double> ori = take<double>(f, (size_t)n_sel * 7), opm = take<double>(f, (size_t)n_sel * 7);
    fclose(f);
    MrPlan plan;
    const std::string why = mr_plan(mode, n_sel, ids.data(), ori.data(), opm.data(), leaf, off, &plan);
    if (!why.empty()) {
        fprintf(stderr, "refused: %s\n", why.c_str());
        return 3;
    }
    const size_t total = (size_t)plan.total;
    const float inv1 = 1.0f / leaf;
    const float inv[3] = {inv1, inv1, inv1};
    const P4 *src = store.data();
    // bounds and parameters per selection, over the work list as the device walks it
    std::vector<VoxelParams> prm((size_t)n_sel);
    {
        const float big = std::numeric_limits<float>::infinity();
        std::vector<float> lo((size_t)n_sel * 3, big), hi((size_t)n_sel * 3, -big);
        std::vector<int> cnt((size_t)n_sel, 0);
        for (const MrWork &w : plan.work) {
            const MrSel &e = plan.sel[(size_t)w.sel];
            for (int i = w.first; i < std::min(e.n, w.first + MR_CHUNK); i++) {
                const P4 p = mr_filter_input(mode, e.aff, src[e.src_off + i]);
                if (!mr_finite(p.x, p.y, p.z)) continue;
                const float c[3] = {p.x, p.y, p.z};
                for (int d = 0; d < 3; d++) lo[3 * w.sel + d] = fminf(lo[3 * w.sel + d], c[d]), hi[3 * w.sel + d] = fmaxf(hi[3 * w.sel + d], c[d]);
                cnt[(size_t)w.sel]++;
            }
        }
        for (int s = 0; s < n_sel; s++) voxel_params(&lo[3 * s], &hi[3 * s], cnt[(size_t)s], inv, prm[(size_t)s]);
    }
    std::vector<unsigned long long> keys(total), keys2(total);
    std::vector<unsigned int> vals(total), vals2(total);
    for (const MrWork &w : plan.work) {
        const MrSel &e = plan.sel[(size_t)w.sel];
        for (int i = w.first; i < std::min(e.n, w.first + MR_CHUNK); i++) {
            const size_t g = (size_t)e.in_off + i;
            keys[g] = mr_key(w.sel, mr_filter_input(mode, e.aff, src[e.src_off + i]), inv, prm[(size_t)w.sel]);
            vals[g] = (unsigned int)g;
        }
    }
    std::vector<size_t> order(total);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
    for (size_t i = 0; i < total; i++) keys2[i] = keys[order[i]], vals2[i] = vals[order[i]];
    std::vector<std::vector<P4>> outs((size_t)n_sel);
    for (size_t i = 0; i < total; i++) {
        if (keys2[i] == MR_SENTINEL || (i > 0 && keys2[i - 1] == keys2[i])) continue;
        const int s = (int)(keys2[i] >> 32);
        const MrSel &e = plan.sel[(size_t)s];
        outs[(size_t)s].push_back(mr_output(mode, e.aff, mr_centroid(mode, src, e, keys2.data(), vals2.data(), i, total)));
    }
    for (int s = 0; s < n_sel; s++) {
        const MrSel &e = plan.sel[(size_t)s];
        if (prm[(size_t)s].status != VOX_PASSTHROUGH) continue;
        for (int i = 0; i < e.n; i++) outs[(size_t)s].push_back(mr_output(mode, e.aff, mr_filter_input(mode, e.aff, src[e.src_off + i])));
    }
    f = fopen(pout, "wb");
    if (!f) return 2;
    int64_t at = 0;
    for (int s = 0; s <= n_sel; s++) {
        fwrite(&at, sizeof at, 1, f);
        if (s < n_sel) at += (int64_t)outs[(size_t)s].size();
    }
    for (int s = 0; s < n_sel; s++) {
        const int32_t st = prm[(size_t)s].status;
        fwrite(&st, sizeof st, 1, f);
    }
    for (int s = 0; s < n_sel; s++)
        if (!outs[(size_t)s].empty()) fwrite(outs[(size_t)s].data(), sizeof(P4), outs[(size_t)s].size(), f);
    fclose(f);
    return 0;
}

static int affine(const char *pin, const char *pout)
{
    FILE *f = fopen(pin, "rb"), *g = fopen(pout, "wb");
    if (!f || !g) return 2;
    const int n_pairs = take<int32_t>(f, 1)[0], n_pts = take<int32_t>(f, 1)[0];
    for (int p = 0; p < n_pairs; p++) {
        const std::vector<double> ori = take<double>(f, 7), opm = take<double>(f, 7);
        const std::vector<float> pts = take<float>(f, (size_t)n_pts * 3);
        MrAffine a;
        mr_affine(ori.data(), opm.data(), a.R, a.T);
        fwrite(a.R, sizeof(float), 9, g);
        fwrite(a.T, sizeof(float), 3, g);
        for (int i = 0; i < n_pts; i++) {
            float m[3];
            mr_move(a, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], m);
            fwrite(m, sizeof(float), 3, g);
        }
    }
    fclose(f);
    fclose(g);
    return 0;
}

static int refusals()
{
    const std::vector<int64_t> off{0, 5, 5, 12};  // three clouds: 5, 0 and 7 points
    const int64_t ids[3] = {2, 0, 1}, low[1] = {-1}, high[1] = {3};
    double pose[21];
    for (int s = 0; s < 3; s++)
        for (int i = 0; i < 7; i++) pose[7 * s + i] = i == 3 ? 1.0 : 0.0;
    double nan_pose[21], inf_pose[21];
    memcpy(nan_pose, pose, sizeof pose);
    memcpy(inf_pose, pose, sizeof pose);
    nan_pose[9] = std::nan("");
    inf_pose[20] = std::numeric_limits<double>::infinity();
    const float inf = std::numeric_limits<float>::infinity();
    MrPlan plan;
    plan.total = -7;
    auto show = [&](const char *name, const std::string &why) { printf("%s: %s\n", name, why.c_str()); };
    show("accepted", mr_plan(0, 3, ids, pose, pose, 0.2f, off, &plan));
    printf("plan: %lld points, %zu selections, %zu work items\n", (long long)plan.total, plan.sel.size(), plan.work.size());
    plan.total = -7;
    show("mode", mr_plan(3, 3, ids, pose, pose, 0.2f, off, &plan));
    show("mode_negative", mr_plan(-1, 3, ids, pose, pose, 0.2f, off, &plan));
    show("negative_count", mr_plan(0, -1, ids, pose, pose, 0.2f, off, &plan));
    show("too_many", mr_plan(0, (1 << 20) + 1, ids, pose, pose, 0.2f, off, &plan));
    show("null_ids", mr_plan(0, 3, nullptr, pose, pose, 0.2f, off, &plan));
    show("null_ori", mr_plan(0, 3, ids, nullptr, pose, 0.2f, off, &plan));
    show("null_opm", mr_plan(1, 3, ids, pose, nullptr, 0.2f, off, &plan));
    show("id_low", mr_plan(0, 1, low, pose, pose, 0.2f, off, &plan));
    show("id_high", mr_plan(0, 1, high, pose, pose, 0.2f, off, &plan));
    show("leaf_zero", mr_plan(0, 3, ids, pose, pose, 0.f, off, &plan));
    show("leaf_negative", mr_plan(0, 3, ids, pose, pose, -0.2f, off, &plan));
    show("leaf_inf", mr_plan(0, 3, ids, pose, pose, inf, off, &plan));
    show("leaf_nan", mr_plan(0, 3, ids, pose, pose, std::nanf(""), off, &plan));
    show("pose_nan", mr_plan(0, 3, ids, pose, nan_pose, 0.2f, off, &plan));
    show("pose_inf", mr_plan(1, 3, ids, inf_pose, pose, 0.2f, off, &plan));
    {  // 2^31 points: two clouds of 2^30 each, selected once each (nothing of that size is allocated: the plan is refused first)
        const std::vector<int64_t> big{0, 1LL << 30, 1LL << 31};
        const int64_t both[2] = {0, 1};
        show("capacity", mr_plan(0, 2, both, pose, pose, 0.2f, big, &plan));
    }
    printf("untouched: %d\n", plan.total == -7 ? 1 : 0);  // no refusal wrote the plan
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "chain")) return chain(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "affine")) return affine(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "refusals")) return refusals();
    fprintf(stderr, "usage: map_refine_host chain|affine <in> <out> | refusals\n");
    return 2;
}
