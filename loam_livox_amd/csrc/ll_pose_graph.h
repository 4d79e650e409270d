// ll_pose_graph.h -- the host side of the pose-graph optimiser: the check and the plan of a call (plain C++, shared by
// ll_api_pose_graph.hip and tests/pose_graph_host.cpp) and the entry point of ll_pose_graph_kernels.hip.
//
// The structure of a call is host knowledge: from the edge lists alone pg_plan derives, per graph, where its poses and edges lie in
// the concatenated arrays; per pose its incidence list (2 * edge + side, ascending: the order every sum over a pose's edges runs
// in), the first block column of its row of the normal matrix and where that row's strip starts; per edge the lower Cholesky factor
// of its information matrix, or the mark that it is the identity.  Nothing of this is computed on the device.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "ll_pose_graph_core.h"

namespace ll {

struct PgPlan {
    int64_t n_poses = 0, n_edges = 0, envelope_blocks = 0;
    bool any_information = false;
    std::vector<PgGraph> graphs;
    std::vector<int32_t> inc_start, inc, first, edge_has_l;
    std::vector<int64_t> strip;
    std::vector<double> info_l;  // [E][36], zeros where the information is the identity
};

static const int64_t kPgMaxCount = 1 << 24;  // poses, edges: 72 doubles per edge are indexed with 32 bits

// The lower Cholesky factor of a 6 x 6 matrix given row-major; its lower triangle is read (as Eigen's llt does).  False when it is
// not positive definite.  *identity: the lower triangle is exactly the identity's.
inline bool pg_information_factor(const double *m, double *l, bool *identity)
{
    *identity = true;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++)
            if (m[i * 6 + j] != (i == j ? 1.0 : 0.0)) *identity = false;
    for (int i = 0; i < 36; i++) l[i] = 0.0;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++) {
            double s = m[i * 6 + j];
            for (int k = 0; k < j; k++) s -= l[i * 6 + k] * l[j * 6 + k];
            if (i == j) {
                if (!(s > 0.0) || !std::isfinite(s)) return false;
                l[i * 6 + i] = sqrt(s);
            } else {
                l[i * 6 + j] = s / l[j * 6 + j];
            }
        }
    return true;
}

// Checks a call and plans it.  Returns the empty string, or why the call is refused.
inline std::string pg_plan(int64_t n_graphs, const int64_t *pose_offsets, const double *poses7, const int64_t *edge_offsets, const int32_t *edge_ab,
                           const double *edge_meas7, const double *edge_information, PgPlan *plan)
{
    if (n_graphs < 0) return "n_graphs out of range";
    if (!plan) return "null argument";
    *plan = PgPlan();
    if (n_graphs == 0) return "";
    if (!pose_offsets || !edge_offsets) return "null argument";
    if (pose_offsets[0] != 0 || edge_offsets[0] != 0) return "offsets must start at 0";
    for (int64_t g = 0; g < n_graphs; g++)
        if (pose_offsets[g + 1] < pose_offsets[g] || edge_offsets[g + 1] < edge_offsets[g]) return "offsets must not descend";
    const int64_t P = pose_offsets[n_graphs], E = edge_offsets[n_graphs];
    char text[160];
    if (P > kPgMaxCount || E > kPgMaxCount) {
        snprintf(text, sizeof text, "%lld poses and %lld edges: a call holds at most %lld of either", (long long)P, (long long)E, (long long)kPgMaxCount);
        return text;
    }
    if ((P > 0 && !poses7) || (E > 0 && (!edge_ab || !edge_meas7))) return "null argument";
    for (int64_t i = 0; i < 7 * P; i++)
        if (!std::isfinite(poses7[i])) return "a pose is not finite";
    for (int64_t i = 0; i < 7 * E; i++)
        if (!std::isfinite(edge_meas7[i])) return "a measurement is not finite";
    if (edge_information)
        for (int64_t i = 0; i < 36 * E; i++)
            if (!std::isfinite(edge_information[i])) return "an information matrix is not finite";
    plan->n_poses = P, plan->n_edges = E;
    plan->graphs.resize(n_graphs);
    plan->first.assign(P, 0);
    plan->strip.assign(P, 0);
    plan->edge_has_l.assign(E, 0);
    std::vector<int32_t> degree(P + 1, 0);
    for (int64_t g = 0; g < n_graphs; g++) {
        const int64_t p0 = pose_offsets[g], n = pose_offsets[g + 1] - p0;
        plan->graphs[g] = {(int32_t)p0, (int32_t)n, (int32_t)edge_offsets[g], (int32_t)(edge_offsets[g + 1] - edge_offsets[g])};
        for (int64_t k = 1; k < n; k++) plan->first[p0 + k] = (int32_t)(k - 1);
        for (int64_t e = edge_offsets[g]; e < edge_offsets[g + 1]; e++) {
            const int64_t a = edge_ab[2 * e], b = edge_ab[2 * e + 1];
            if (a < 0 || a >= n || b < 0 || b >= n) {
                snprintf(text, sizeof text, "edge %lld of graph %lld names a pose out of range", (long long)(e - edge_offsets[g]), (long long)g);
                return text;
            }
            if (a == b) {
                snprintf(text, sizeof text, "edge %lld of graph %lld joins a pose to itself", (long long)(e - edge_offsets[g]), (long long)g);
                return text;
            }
            degree[p0 + a]++, degree[p0 + b]++;
            const int64_t hi = a > b ? a : b, lo = a > b ? b : a;
            if (lo >= 1 && plan->first[p0 + hi] > lo - 1) plan->first[p0 + hi] = (int32_t)(lo - 1);
        }
    }
    if (edge_information) {
        plan->info_l.assign(36 * (size_t)E, 0.0);
        for (int64_t e = 0; e < E; e++) {
            bool identity = false;
            if (!pg_information_factor(edge_information + 36 * e, plan->info_l.data() + 36 * e, &identity)) {
                snprintf(text, sizeof text, "the information matrix of edge %lld of the call is not positive definite", (long long)e);
                return text;
            }
            plan->edge_has_l[e] = identity ? 0 : 1;
            if (!identity) plan->any_information = true;
        }
    }
    // a pose's incidence list, ascending in the edge index
    plan->inc_start.assign(P + 1, 0);
    for (int64_t p = 0; p < P; p++) plan->inc_start[p + 1] = plan->inc_start[p] + degree[p];
    plan->inc.assign(2 * (size_t)E, 0);
    std::vector<int32_t> fill(plan->inc_start.begin(), plan->inc_start.end() - 1);
    for (int64_t g = 0; g < n_graphs; g++)
        for (int64_t e = edge_offsets[g]; e < edge_offsets[g + 1]; e++)
            for (int side = 0; side < 2; side++) plan->inc[fill[pose_offsets[g] + edge_ab[2 * e + side]]++] = (int32_t)(2 * e + side);
    // the strips of the block envelope, one after the other
    int64_t blocks = 0;
    for (int64_t g = 0; g < n_graphs; g++)
        for (int64_t k = 1; k < plan->graphs[g].n_poses; k++) {
            const int64_t p = pose_offsets[g] + k;
            plan->strip[p] = 36 * blocks;
            blocks += (k - 1) - plan->first[p] + 1;
        }
    plan->envelope_blocks = blocks;
    return "";
}

// the views of a plan's arrays (host vectors, or their device copies) are filled in by the caller

#if defined(__HIPCC__)
// one workgroup per graph, the whole minimisation in the launch.  Only enqueues on s.
int pose_graph_launch(const PgView &view, int n_graphs, hipStream_t s, const char **err);
#endif

}  // namespace ll
