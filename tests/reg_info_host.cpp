// CPU tier of the registration information (tests/test_reg_information_host.py): loam_livox_amd/csrc/ll_reg_info_core.h -- the text
// reg_information_kernel runs -- under g++, its 256 thread loops and its reduction walked serially; and the two host helpers of
// include/loam_livox_adapter.hpp, symmetric_eigen6 and information_in_pose_frame.  Also built with -fsanitize=address,undefined.
//
//   reg_info_host <in> <out>
// in: int64 header {mode, deblur, n_corner, n_surf, cap_c, cap_s, n_map_c, n_map_s, n_mats, gated, aborted, icp_iters}, then
//   mode 0: double {pose_last[7], x[7], huber_a, min_ts, max_ts}, uint8 flag0[cap_c + cap_s] (padded to 8 bytes), int32 nn[cap][4],
//           float corner[n_corner][4], surf[n_surf][4], map_c[n_map_c][4], map_s[n_map_s][4]
//           -> double {H[36], g[6], cost, n_line, n_plane, status}
//   mode 1: double H[n_mats][36] -> per matrix double {w[6], V[36], sweeps}
//   mode 2: double {H[36], pose_last[7]}[n_mats] -> per matrix double H_pose[36]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ll_reg_info_core.h"
#define LOAM_LIVOX_ADAPTER_NO_EIGEN 1
#include "loam_livox_adapter.hpp"

template <class T>
static bool take(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <int DEBLUR>
static void run_scan(const ll::InfoScan &s, const double x[7], double sum[LL_NACC], int &n_line, int &n_plane)
{
    ll::InfoCtx c;
    ll::info_context<DEBLUR>(x, c);
    std::vector<double> acc((size_t)LL_INFO_THREADS * LL_NACC);
    n_line = n_plane = 0;
    for (int tid = 0; tid < LL_INFO_THREADS; tid++) {  // the kernel's threads, one after the other
        int nl = 0, np = 0;
        ll::info_thread<DEBLUR>(s, c, tid, LL_INFO_THREADS, &acc[(size_t)tid * LL_NACC], nl, np);
        n_line += nl;
        n_plane += np;
    }
    ll::info_reduce_serial(reinterpret_cast<const double(*)[LL_NACC]>(acc.data()), LL_INFO_THREADS, sum);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[12];
    if (fread(h, sizeof(int64_t), 12, f) != 12) return 2;
    const int mode = (int)h[0];
    std::vector<double> out;
    if (mode == 0) {
        const int deblur = (int)h[1], nC = (int)h[2], nS = (int)h[3], cap_c = (int)h[4], cap_s = (int)h[5], nmc = (int)h[6], nms = (int)h[7];
        const size_t cap = (size_t)cap_c + cap_s;
        if (nC < 0 || nS < 0 || nC > cap_c || nS > cap_s || nmc < 0 || nms < 0) return 2;
        std::vector<double> d;
        std::vector<unsigned char> flag0;
        std::vector<int32_t> nn;
        std::vector<float> corner, surf, map_c, map_s;
        if (!take(f, d, 17) || !take(f, flag0, (cap + 7) / 8 * 8) || !take(f, nn, cap * 4) || !take(f, corner, (size_t)nC * 4) ||
            !take(f, surf, (size_t)nS * 4) || !take(f, map_c, (size_t)nmc * 4) || !take(f, map_s, (size_t)nms * 4))
            return 2;
        static_assert(sizeof(ll::f4) == 16, "a map point is four floats");
        std::vector<ll::f4> pc((size_t)nmc), ps((size_t)nms);
        if (nmc) memcpy(pc.data(), map_c.data(), (size_t)nmc * 16);
        if (nms) memcpy(ps.data(), map_s.data(), (size_t)nms * 16);
        ll::InfoScan s;
        s.flag0 = flag0.data();
        s.nn = nn.data();
        s.corner = corner.data();
        s.surf = surf.data();
        s.map_c = pc.data();
        s.map_s = ps.data();
        s.n_map_c = nmc;
        s.n_map_s = nms;
        s.n_corner = nC;
        s.n_surf = nS;
        s.cap_c = cap_c;
        s.huber_a = d[14];
        s.min_ts = (float)d[15];
        s.max_ts = (float)d[16];
        for (int i = 0; i < 7; i++) s.pose_last[i] = d[i];
        const int status = ll::info_status((int)h[9], (int)h[10], (int)h[11], nC + nS);
        double sum[LL_NACC] = {0};
        int n_line = 0, n_plane = 0;
        if (!status) {
            if (deblur)
                run_scan<1>(s, &d[7], sum, n_line, n_plane);
            else
                run_scan<0>(s, &d[7], sum, n_line, n_plane);
        }
        for (int e = 0; e < LL_INFO_RECORD_DOUBLES; e++) out.push_back(status ? 0.0 : ll::info_record_entry(sum, e));
        out.push_back(n_line);
        out.push_back(n_plane);
        out.push_back(status);
    } else if (mode == 1 || mode == 2) {
        const size_t n = (size_t)h[8], per = mode == 1 ? 36 : 43;
        std::vector<double> in;
        if (!take(f, in, n * per)) return 2;
        for (size_t m = 0; m < n; m++) {
            if (mode == 1) {
                double w[6], V[36];
                const int sweeps = loam_livox_hip::symmetric_eigen6(&in[m * 36], w, V);
                out.insert(out.end(), w, w + 6);
                out.insert(out.end(), V, V + 36);
                out.push_back(sweeps);
            } else {
                double Hp[36];
                loam_livox_hip::information_in_pose_frame(&in[m * 43], &in[m * 43 + 36], Hp);
                out.insert(out.end(), Hp, Hp + 36);
            }
        }
    } else {
        return 2;
    }
    fclose(f);
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 2;
    if (!out.empty() && fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 2;
    fclose(g);
    return 0;
}
