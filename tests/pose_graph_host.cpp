// pose_graph_host.cpp -- runs the text of loam_livox_amd/csrc/ll_pose_graph_core.h (what pg_solve_kernel runs) and the call plan of
// ll_pose_graph.h with a host compiler, one work item per graph (tests/test_pose_graph_host.py).
//
//   pose_graph_host <in> <out>
// in:  int64 {mode, G, P, E, has_information, has_params}; when has_params int64 {max_num_iterations,
//      max_num_consecutive_invalid_steps} and double {initial, max, min trust-region radius, min_relative_decrease, min, max
//      lm_diagonal, function, gradient, parameter tolerance} -- ll_pose_graph_params in its order, the defaults otherwise;
//      int64 pose_offsets[G + 1], int64 edge_offsets[G + 1], double poses[7 P], int32 edge_ab[2 E], double meas[7 E],
//      double information[36 E] when has_information.
// out, mode 0 (solve): double poses[7 P], then per graph double {iterations, successful, unsuccessful, termination, initial cost, final cost}.
// out, mode 1 (one graph, the first linearisation): double J[72 E] unscaled, double n, A[n n] damped normal matrix expanded from its
//      envelope, rhs[n], y[n] of the envelope solve, double ok.
// out, mode 2 (the plan alone): per graph double envelope blocks, then double envelope blocks of the call.
// A call the plan refuses: its text on stdout, exit status 3.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "ll_pose_graph.h"

using namespace ll;

template <typename T>
static bool read_n(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> head, pose_off, edge_off;
    std::vector<double> poses, meas, info;
    std::vector<int32_t> ab;
    if (!read_n(f, head, 6)) return 2;
    const int64_t mode = head[0], G = head[1], P = head[2], E = head[3];
    std::vector<int64_t> prm_i;
    std::vector<double> prm_d;
    if (head[5] && (!read_n(f, prm_i, 2) || !read_n(f, prm_d, 9))) return 2;
    if (!read_n(f, pose_off, G + 1) || !read_n(f, edge_off, G + 1) || !read_n(f, poses, 7 * P) || !read_n(f, ab, 2 * E) || !read_n(f, meas, 7 * E)) return 2;
    if (head[4] && !read_n(f, info, 36 * E)) return 2;
    fclose(f);

    PgPlan plan;
    const std::string why = pg_plan(G, pose_off.data(), poses.data(), edge_off.data(), ab.data(), meas.data(), head[4] ? info.data() : nullptr, &plan);
    if (!why.empty()) {
        printf("%s\n", why.c_str());
        return 3;
    }
    std::vector<double> cand(7 * P), r(6 * E), J(72 * E), ecost(E), H(36 * plan.envelope_blocks + 1), scale(6 * P), diag(6 * P), g(6 * P), rhs(6 * P),
        y(6 * P), ps0(P), ps1(P);
    std::vector<ll_pose_graph_summary> summary(G);
    if (plan.info_l.empty()) plan.info_l.assign(1, 0.0);
    PgView v{};
    v.graphs = plan.graphs.data(), v.x = poses.data(), v.cand = cand.data(), v.edge_ab = ab.data(), v.meas = meas.data();
    v.info_l = plan.info_l.data(), v.edge_has_l = plan.edge_has_l.data(), v.r = r.data(), v.J = J.data(), v.ecost = ecost.data();
    v.inc_start = plan.inc_start.data(), v.inc = plan.inc.data(), v.first = plan.first.data(), v.strip = plan.strip.data(), v.H = H.data();
    v.scale = scale.data(), v.diag = diag.data(), v.g = g.data(), v.rhs = rhs.data(), v.y = y.data(), v.ps0 = ps0.data(), v.ps1 = ps1.data();
    v.summary = summary.data();
    v.prm.max_num_iterations = 200, v.prm.max_num_consecutive_invalid_steps = 5;
    v.prm.initial_trust_region_radius = 1e4, v.prm.max_trust_region_radius = 1e16, v.prm.min_trust_region_radius = 1e-32;
    v.prm.min_relative_decrease = 1e-3, v.prm.min_lm_diagonal = 1e-6, v.prm.max_lm_diagonal = 1e32;
    v.prm.function_tolerance = 1e-6, v.prm.gradient_tolerance = 1e-10, v.prm.parameter_tolerance = 1e-8;
    if (head[5]) {
        v.prm.max_num_iterations = (int32_t)prm_i[0], v.prm.max_num_consecutive_invalid_steps = (int32_t)prm_i[1];
        v.prm.initial_trust_region_radius = prm_d[0], v.prm.max_trust_region_radius = prm_d[1], v.prm.min_trust_region_radius = prm_d[2];
        v.prm.min_relative_decrease = prm_d[3], v.prm.min_lm_diagonal = prm_d[4], v.prm.max_lm_diagonal = prm_d[5];
        v.prm.function_tolerance = prm_d[6], v.prm.gradient_tolerance = prm_d[7], v.prm.parameter_tolerance = prm_d[8];
    }
    std::unique_ptr<PgShared> sh(new PgShared());

    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (mode == 0) {
        for (int64_t gi = 0; gi < G; gi++) pg_solve_graph(v, (int)gi, sh.get(), 0, 1);
        fwrite(poses.data(), sizeof(double), poses.size(), o);
        for (const ll_pose_graph_summary &s : summary) {
            const double rec[6] = {(double)s.iterations, (double)s.successful_steps, (double)s.unsuccessful_steps, (double)s.termination, s.initial_cost, s.final_cost};
            fwrite(rec, sizeof(double), 6, o);
        }
    } else if (mode == 2) {
        for (int64_t gi = 0; gi < G; gi++) {
            double blocks = 0.0;
            for (int64_t k = 1; k < plan.graphs[gi].n_poses; k++) blocks += (double)(k - plan.first[pose_off[gi] + k]);
            fwrite(&blocks, sizeof(double), 1, o);
        }
        const double all = (double)plan.envelope_blocks;
        fwrite(&all, sizeof(double), 1, o);
    } else {
        if (G != 1 || P < 2 || E < 1) return 2;
        const PgGraph gr = plan.graphs[0];
        pg_phase_eval(v, gr, v.x, true, 0, 1);
        fwrite(J.data(), sizeof(double), J.size(), o);
        sh->radius = v.prm.initial_trust_region_radius, sh->reuse_diag = 0, sh->chol_ok = 1;
        pg_linearise(v, gr, sh.get(), true, 0, 1);
        pg_phase_assemble(v, gr, 0, 1);
        pg_phase_damp(v, gr, sh.get(), 0, 1);
        const int n = 6 * (gr.n_poses - 1);
        std::vector<double> A((size_t)n * n, 0.0);
        for (int fr = 0; fr < gr.n_poses - 1; fr++)
            for (int row = 0; row < 6; row++)
                for (int col = 6 * plan.first[1 + fr]; col <= 6 * fr + row; col++)
                    A[(size_t)(6 * fr + row) * n + col] = A[(size_t)col * n + 6 * fr + row] = *pg_h(v, 1 + fr, fr, row, col);
        pg_factor(v, gr, sh.get(), 0, 1);
        std::vector<double> sol(n);
        pg_solve_triangular(v, gr, sh.get(), sol.data(), 0, 1);
        const bool ok = sh->chol_ok != 0;
        const double nd = n, okd = ok ? 1.0 : 0.0;
        fwrite(&nd, sizeof(double), 1, o);
        fwrite(A.data(), sizeof(double), A.size(), o);
        fwrite(rhs.data() + 6, sizeof(double), n, o);
        fwrite(sol.data(), sizeof(double), n, o);
        fwrite(&okd, sizeof(double), 1, o);
    }
    fclose(o);
    return 0;
}
