// ll_pose_graph_core.h -- the pose-graph optimiser (ll_pose_graph_kernels.hip), written once for the device and for a host compiler:
// tests/pose_graph_host.cpp runs the text below with g++.
//
// The problem is ceres_pose_graph_3d.hpp's (:198-352): poses {p, q}, pose 0 constant, an edge (a, b, p_m, q_m, information) with
//     q_ab = conj(q_a) (x) q_b      p_ab = conj(q_a) . (p_b - p_a)      dq = q_m (x) conj(q_ab)      e = [ p_ab - p_m ; 2 vec(dq) ]
// and the residual L e, L the lower Cholesky factor of the information matrix (factored on the host).  conj, not inverse, and the
// vector rotation v + w uv + u x uv with uv = 2 (u x v): both are what the reference's functor evaluates, for quaternions of any norm.
// Translation moves additively; a quaternion moves by Plus(q, d) = dq(d) (x) q, dq = ( sin|d| / |d| d, cos|d| ), no renormalisation.
// A free pose has the six local coordinates { dp, d }, in that order; the system has 6 (N - 1).
//
// The Jacobian is analytic.  Plus is linear in d to first order, q(d) = ( d, 1 ) (x) q, and e is a polynomial in the eight quaternion
// components, so a column is the directional derivative of that polynomial along ( e_k, 0 ) (x) q, written out term by term below
// (pg_edge_eval).  This is what automatic differentiation through the functor times the parameterisation's Jacobian gives.
//
// The minimiser is Ceres' trust-region Levenberg-Marquardt without loss, bounds or line search:
//     Jacobi column scales 1 / (1 + ||col||) from the first Jacobian, kept; diag = clamp( diag(J'J), min, max ), reused after a
//     rejected step; ( J'J + diag / radius ) y = J'r solved exactly, step = -y; model cost change -sum m (r + m / 2), m = J step; a step
//     that cannot be solved or does not lower the model halves the radius, and a run of them ends the solve; parameter tolerance on
//     |x - Plus(x, delta)| against |x| of the free poses; function tolerance on the cost change; accepted when the ratio passes
//     min_relative_decrease: radius /= max( 1/3, 1 - (2 rho - 1)^3 ), capped; rejected: radius /= f, f *= 2; gradient tolerance on
//     max |x - Plus(x, -g)|; radius floor; iteration cap.
//
// One workgroup owns a graph for the whole loop.  The text is a sequence of PHASES: in a phase every work item runs a loop strided by
// the item count over independent pieces (edges, poses, rows), and LL_PG_SYNC() stands between phases.  On the device LL_PG_SYNC is
// the workgroup barrier; a host compiler runs one item (tid 0 of 1) with an empty LL_PG_SYNC, which executes the same pieces in
// sequence.  No piece reads what another piece of its phase writes, so both give the same bits.
//
// Every sum has one order, fixed by the data: an edge's rows in sequence; over edges in ascending edge index through the host-built
// incidence list of a pose; over poses in ascending index by item 0.  There is no atomic.  Nothing depends on where a graph lies in
// the batch except the offsets its arrays are found at.
//
// The normal matrix is kept as a block envelope (skyline): block row f (free pose f + 1) holds the 6 x 6 blocks first[f] .. f as one
// 6 x w strip, w = 6 (f - first[f] + 1), row-major.  first[f] is the lowest free pose an edge joins to f from below, so a chain is
// block-tridiagonal and a loop edge lengthens one row.  Cholesky fills a row only between its first entry and the diagonal, so the
// factor overwrites the strips and is exact.  Element (row, k) is computed as in the dense row-oriented algorithm, the sum over
// earlier columns ascending, with the columns outside either row's envelope -- exact zeros -- left out.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/loam_livox_hip.h"

#ifndef LL_HD
#if defined(__HIPCC__)
#define LL_HD __host__ __device__ __forceinline__
#else
#define LL_HD inline
#endif
#endif
#if defined(__HIPCC__)
#define LL_PG_FN __host__ __device__ inline
#else
#define LL_PG_FN inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define LL_PG_SYNC() __syncthreads()
#else
#define LL_PG_SYNC() ((void)0)   // one work item: the phases run in sequence
#endif

namespace ll {

#define LL_PG_THREADS 256
#define LL_PG_LDS_VEC 2048   // doubles: a graph of up to 342 poses keeps the vector of the triangular solves in LDS
#define LL_PG_DBL_MAX 1.7976931348623157e308

// One graph of a call.  Poses and edges of all graphs are concatenated; every index below is into the concatenated arrays.
struct PgGraph {
    int32_t pose0, n_poses, edge0, n_edges;
};

// The arrays of a call.  P poses, E edges in total.
struct PgView {
    const PgGraph *graphs;
    double *x;                // [P][7] {qx, qy, qz, qw, tx, ty, tz}, in and out
    double *cand;             // [P][7]
    const int32_t *edge_ab;   // [E][2] pose ids within the graph
    const double *meas;       // [E][7]
    const double *info_l;     // [E][36] lower factors, row-major; read where edge_has_l is set
    const int32_t *edge_has_l;  // [E]
    double *r;                // [E][6]
    double *J;                // [E][2][36]: d residual / d local coordinates of a, of b; [row][column]
    double *ecost;            // [E]
    const int32_t *inc_start; // [P + 1] a pose's incidence list: inc[inc_start[p] .. inc_start[p + 1])
    const int32_t *inc;       // 2 * edge + side, ascending
    const int32_t *first;     // [P] first block column (free index) of the pose's strip; unused for a graph's pose 0
    const int64_t *strip;     // [P] where the pose's strip starts in H, in doubles
    double *H;
    double *scale, *diag, *g, *rhs, *y;  // [6 P], entry 6 p + c of pose p; the six of a graph's pose 0 are not used
    double *ps0, *ps1;        // [P] per-pose partial results
    ll_pose_graph_summary *summary;  // [G]
    ll_pose_graph_params prm;
};

// the loop's scalars, shared by the work items of a graph
struct PgShared {
    double cost, x_norm, gmax, radius, decrease_factor, model_cost_change, initial_cost;
    int32_t reuse_diag, invalid, iteration, n_succ, n_unsucc, term, go, chol_ok, action;  // action: 0 next iteration, 1 try the step, 2 accept
    double vec[LL_PG_LDS_VEC];
};

// ---------------------------------------------------------------------------------------------------------- quaternions {x, y, z, w}
LL_HD void pg_qmul(const double a[4], const double b[4], double o[4])
{
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
LL_HD void pg_qconj(const double a[4], double o[4])
{
    o[0] = -a[0], o[1] = -a[1], o[2] = -a[2], o[3] = a[3];
}
LL_HD void pg_cross(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
// v + w uv + u x uv, uv = 2 (u x v)
LL_HD void pg_qrot(const double q[4], const double v[3], double o[3])
{
    double uv[3], uuv[3];
    pg_cross(q, v, uv);
    for (int i = 0; i < 3; i++) uv[i] = 2.0 * uv[i];
    pg_cross(q, uv, uuv);
    for (int i = 0; i < 3; i++) o[i] = v[i] + q[3] * uv[i] + uuv[i];
}
// the derivative of pg_qrot(q, v) along dq (v constant)
LL_HD void pg_qrot_d(const double q[4], const double dq[4], const double v[3], double o[3])
{
    double uv[3], duv[3], a[3], b[3];
    pg_cross(q, v, uv);
    pg_cross(dq, v, duv);
    for (int i = 0; i < 3; i++) uv[i] = 2.0 * uv[i], duv[i] = 2.0 * duv[i];
    pg_cross(dq, uv, a);
    pg_cross(q, duv, b);
    for (int i = 0; i < 3; i++) o[i] = dq[3] * uv[i] + q[3] * duv[i] + a[i] + b[i];
}
// Plus of one pose: x, out {q, p}; d {dp, d}
LL_HD void pg_plus(const double x[7], const double d[6], double out[7])
{
    const double n = sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
    if (n > 0.0) {
        const double s = sin(n) / n;
        const double dq[4] = {s * d[3], s * d[4], s * d[5], cos(n)};
        pg_qmul(dq, x, out);
    } else {
        for (int i = 0; i < 4; i++) out[i] = x[i];
    }
    for (int i = 0; i < 3; i++) out[4 + i] = x[4 + i] + d[i];
}

// One edge at the poses xa, xb: e (or L e) into r; with Ja / Jb the 6 x 6 derivatives by the local coordinates of a and of b.
LL_HD void pg_edge_eval(const double xa[7], const double xb[7], const double m[7], const double *L, double r[6], double *Ja, double *Jb)
{
    double ca[4], qab[4], cqab[4], dq[4], d[3], pab[3], e[6];
    pg_qconj(xa, ca);
    pg_qmul(ca, xb, qab);
    for (int i = 0; i < 3; i++) d[i] = xb[4 + i] - xa[4 + i];
    pg_qrot(ca, d, pab);
    pg_qconj(qab, cqab);
    pg_qmul(m, cqab, dq);
    for (int i = 0; i < 3; i++) e[i] = pab[i] - m[4 + i], e[3 + i] = 2.0 * dq[i];
    if (Ja) {
        double A[36], B[36];
        for (int k = 0; k < 3; k++) {
            double ek[3] = {0.0, 0.0, 0.0}, col[3];
            ek[k] = 1.0;
            pg_qrot(ca, ek, col);
            for (int i = 0; i < 3; i++) {
                A[i * 6 + k] = -col[i], B[i * 6 + k] = col[i];
                A[(3 + i) * 6 + k] = 0.0, B[(3 + i) * 6 + k] = 0.0;
            }
            double unit[4] = {0.0, 0.0, 0.0, 0.0}, dqa[4], dca[4], dqab[4], cd[4], ddq[4], dp[3];
            unit[k] = 1.0;
            // along a's rotation
            pg_qmul(unit, xa, dqa);
            pg_qconj(dqa, dca);
            pg_qrot_d(ca, dca, d, dp);
            pg_qmul(dca, xb, dqab);
            pg_qconj(dqab, cd);
            pg_qmul(m, cd, ddq);
            for (int i = 0; i < 3; i++) A[i * 6 + 3 + k] = dp[i], A[(3 + i) * 6 + 3 + k] = 2.0 * ddq[i];
            // along b's rotation
            double dqb[4];
            pg_qmul(unit, xb, dqb);
            pg_qmul(ca, dqb, dqab);
            pg_qconj(dqab, cd);
            pg_qmul(m, cd, ddq);
            for (int i = 0; i < 3; i++) B[i * 6 + 3 + k] = 0.0, B[(3 + i) * 6 + 3 + k] = 2.0 * ddq[i];
        }
        for (int i = 0; i < 6; i++)
            for (int c = 0; c < 6; c++) {
                if (L) {
                    double sa = 0.0, sb = 0.0;
                    for (int k = 0; k <= i; k++) sa += L[i * 6 + k] * A[k * 6 + c], sb += L[i * 6 + k] * B[k * 6 + c];
                    Ja[i * 6 + c] = sa, Jb[i * 6 + c] = sb;
                } else {
                    Ja[i * 6 + c] = A[i * 6 + c], Jb[i * 6 + c] = B[i * 6 + c];
                }
            }
    }
    for (int i = 0; i < 6; i++) {
        if (L) {
            double s = 0.0;
            for (int k = 0; k <= i; k++) s += L[i * 6 + k] * e[k];
            r[i] = s;
        } else {
            r[i] = e[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- phases
#define LL_PG_FOR(i, n) for (int i = tid; i < (n); i += nt)

// residuals (and Jacobians) of every edge at the poses `at`; ecost[e] = sum of squares
LL_PG_FN void pg_phase_eval(const PgView &v, const PgGraph &gr, const double *at, bool with_j, int tid, int nt)
{
    LL_PG_FOR(k, gr.n_edges)
    {
        const int e = gr.edge0 + k;
        const double *xa = at + 7 * (size_t)(gr.pose0 + v.edge_ab[2 * e]), *xb = at + 7 * (size_t)(gr.pose0 + v.edge_ab[2 * e + 1]);
        const double *L = v.edge_has_l[e] ? v.info_l + 36 * (size_t)e : nullptr;
        double r[6];
        if (with_j) {
            double Ja[36], Jb[36];
            pg_edge_eval(xa, xb, v.meas + 7 * (size_t)e, L, r, Ja, Jb);
            double *J = v.J + 72 * (size_t)e;
            for (int i = 0; i < 36; i++) J[i] = Ja[i], J[36 + i] = Jb[i];
            for (int i = 0; i < 6; i++) v.r[6 * (size_t)e + i] = r[i];
        } else {
            pg_edge_eval(xa, xb, v.meas + 7 * (size_t)e, L, r, nullptr, nullptr);
        }
        double s = 0.0;
        for (int i = 0; i < 6; i++) s += r[i] * r[i];
        v.ecost[e] = s;
    }
}

// gradient J'r of the unscaled Jacobian per local coordinate; with `init` also the column scales
LL_PG_FN void pg_phase_gradient(const PgView &v, const PgGraph &gr, bool init, int tid, int nt)
{
    LL_PG_FOR(k, 6 * (gr.n_poses - 1))
    {
        const int p = gr.pose0 + 1 + k / 6, c = k % 6;
        double g = 0.0, s = 0.0;
        for (int t = v.inc_start[p]; t < v.inc_start[p + 1]; t++) {
            const int e = v.inc[t] >> 1, side = v.inc[t] & 1;
            const double *J = v.J + 72 * (size_t)e + 36 * side, *r = v.r + 6 * (size_t)e;
            for (int i = 0; i < 6; i++) {
                g += J[i * 6 + c] * r[i];
                s += J[i * 6 + c] * J[i * 6 + c];
            }
        }
        v.g[6 * (size_t)p + c] = g;
        if (init) v.scale[6 * (size_t)p + c] = 1.0 / (1.0 + sqrt(s));
    }
}

// J <- J scaled by columns; per pose max |x - Plus(x, -g)| into ps0 and |x|^2 into ps1 (a pose without edges is not in the program)
LL_PG_FN void pg_phase_scale_and_norms(const PgView &v, const PgGraph &gr, int tid, int nt)
{
    LL_PG_FOR(k, 2 * gr.n_edges)
    {
        const int e = gr.edge0 + (k >> 1), side = k & 1, a = v.edge_ab[2 * e + side];
        if (a == 0) continue;
        double *J = v.J + 72 * (size_t)e + 36 * side;
        const double *sc = v.scale + 6 * (size_t)(gr.pose0 + a);
        for (int i = 0; i < 6; i++)
            for (int c = 0; c < 6; c++) J[i * 6 + c] *= sc[c];
    }
    LL_PG_FOR(k, gr.n_poses - 1)
    {
        const int p = gr.pose0 + 1 + k;
        const double *x = v.x + 7 * (size_t)p;
        double m = 0.0, s = 0.0;
        if (v.inc_start[p + 1] > v.inc_start[p]) {
            double ng[6], xp[7];
            for (int c = 0; c < 6; c++) ng[c] = -v.g[6 * (size_t)p + c];
            pg_plus(x, ng, xp);
            for (int i = 0; i < 7; i++) {
                m = fmax(m, fabs(x[i] - xp[i]));
                s += x[i] * x[i];
            }
        }
        v.ps0[p] = m, v.ps1[p] = s;
    }
}

// the strips of J'J and the right-hand side J'r of the scaled Jacobian: one piece per (free pose, row)
LL_PG_FN void pg_phase_assemble(const PgView &v, const PgGraph &gr, int tid, int nt)
{
    LL_PG_FOR(k, 6 * (gr.n_poses - 1))
    {
        const int f = k / 6, row = k % 6, p = gr.pose0 + 1 + f;
        const int first = v.first[p], w = 6 * (f - first + 1);
        double *h = v.H + v.strip[p] + (size_t)row * w;
        for (int c = 0; c < w; c++) h[c] = 0.0;
        double rhs = 0.0;
        for (int t = v.inc_start[p]; t < v.inc_start[p + 1]; t++) {
            const int e = v.inc[t] >> 1, side = v.inc[t] & 1;
            const double *Jf = v.J + 72 * (size_t)e + 36 * side, *Jo = v.J + 72 * (size_t)e + 36 * (1 - side), *r = v.r + 6 * (size_t)e;
            const int o = v.edge_ab[2 * e + 1 - side] - 1;     // the other end's free index (-1: the constant pose)
            double *hd = h + 6 * (f - first);
            for (int i = 0; i < 6; i++) {
                const double jf = Jf[i * 6 + row];
                rhs += jf * r[i];
                for (int c = 0; c < 6; c++) hd[c] += jf * Jf[i * 6 + c];
            }
            if (o >= 0 && o < f) {
                double *ho = h + 6 * (o - first);
                for (int i = 0; i < 6; i++) {
                    const double jf = Jf[i * 6 + row];
                    for (int c = 0; c < 6; c++) ho[c] += jf * Jo[i * 6 + c];
                }
            }
        }
        v.rhs[6 * (size_t)p + row] = rhs;
    }
}

// diag = clamp( diag(J'J) ) unless kept from the rejected step before; J'J += diag / radius on the diagonal
LL_PG_FN void pg_phase_damp(const PgView &v, const PgGraph &gr, const PgShared *sh, int tid, int nt)
{
    LL_PG_FOR(k, 6 * (gr.n_poses - 1))
    {
        const int f = k / 6, row = k % 6, p = gr.pose0 + 1 + f;
        const int w = 6 * (f - v.first[p] + 1);
        double *hd = v.H + v.strip[p] + (size_t)row * w + (w - 6 + row);
        if (!sh->reuse_diag) v.diag[6 * (size_t)p + row] = fmin(fmax(*hd, v.prm.min_lm_diagonal), v.prm.max_lm_diagonal);
        *hd += v.diag[6 * (size_t)p + row] / sh->radius;
    }
}

// element (row of strip p, scalar column col) of the envelope; col must lie inside the strip
LL_HD double *pg_h(const PgView &v, int p, int f, int row, int col)
{
    const int first = v.first[p], w = 6 * (f - first + 1);
    return v.H + v.strip[p] + (size_t)row * w + (col - 6 * first);
}

// Cholesky of the envelope in place, block row after block row.  Per block row f, for every block column jb left of the diagonal:
//   (1a) the 36 entries of block (f, jb), one piece each: A[r][j] less sum_k L[r][k] L[j][k] over the columns k left of block jb that
//        both envelopes hold;
//   (1b) the six rows of the block, one piece each, column after column: the rest of the sum (k inside block jb), then / L[j][j];
// then (2) the lower triangle of the diagonal block less the products of the strip's rows left of it, one piece per entry, and
// (3) the 6 x 6 factor of that block, one piece.  Every entry is ( A[r][j] - sum_k L[r][k] L[j][k] ) / L[j][j] with k ascending, as in
// the dense row-oriented algorithm.  A pivot that is not positive clears sh->chol_ok; the arithmetic goes on (on NaNs) and the
// caller discards the result.
LL_PG_FN void pg_factor(const PgView &v, const PgGraph &gr, PgShared *sh, int tid, int nt)
{
    const int n = gr.n_poses - 1;
    for (int f = 0; f < n; f++) {
        const int p = gr.pose0 + 1 + f, c0 = 6 * v.first[p], w = 6 * f + 6 - c0;
        double *strip = v.H + v.strip[p];
        for (int jb = v.first[p]; jb < f; jb++) {
            const int pj = gr.pose0 + 1 + jb, c0j = 6 * v.first[pj], wj = 6 * jb + 6 - c0j;
            const double *stripj = v.H + v.strip[pj];
            const int k0 = c0 > c0j ? c0 : c0j;
            LL_PG_FOR(t, 36)
            {
                const int row = t / 6, c = t % 6, j = 6 * jb + c;
                double *h = strip + (size_t)row * w - c0;      // h[col]
                const double *hj = stripj + (size_t)c * wj - c0j;
                double s = h[j];
                for (int k = k0; k < 6 * jb; k++) s -= h[k] * hj[k];
                h[j] = s;
            }
            LL_PG_SYNC();
            LL_PG_FOR(row, 6)
            {
                double *h = strip + (size_t)row * w - c0 + 6 * jb;     // the row's six entries of the block, worked on in registers
                double hv[6];
                for (int c = 0; c < 6; c++) hv[c] = h[c];
                for (int c = 0; c < 6; c++) {
                    const double *hj = stripj + (size_t)c * wj - c0j + 6 * jb;
                    double s = hv[c];
                    for (int k = 0; k < c; k++) s -= hv[k] * hj[k];
                    hv[c] = s / hj[c];
                }
                for (int c = 0; c < 6; c++) h[c] = hv[c];
            }
            LL_PG_SYNC();
        }
        LL_PG_FOR(t, 36)
        {
            const int row = t / 6, jj = t % 6;
            if (jj > row) continue;
            double *h = strip + (size_t)row * w - c0;
            const double *hj = strip + (size_t)jj * w - c0;
            double s = h[6 * f + jj];
            for (int k = c0; k < 6 * f; k++) s -= h[k] * hj[k];
            h[6 * f + jj] = s;
        }
        LL_PG_SYNC();
        if (tid == 0) {
            double d[6][6];                                            // the block's lower triangle, factored in registers
            for (int i = 0; i < 6; i++)
                for (int j = 0; j <= i; j++) d[i][j] = strip[(size_t)i * w - c0 + 6 * f + j];
            for (int i = 0; i < 6; i++)
                for (int j = 0; j <= i; j++) {
                    double s = d[i][j];
                    for (int k = 0; k < j; k++) s -= d[i][k] * d[j][k];
                    if (i == j) {
                        if (!(s > 0.0)) sh->chol_ok = 0;
                        d[i][i] = sqrt(s);
                    } else {
                        d[i][j] = s / d[j][j];
                    }
                }
            for (int i = 0; i < 6; i++)
                for (int j = 0; j <= i; j++) strip[(size_t)i * w - c0 + 6 * f + j] = d[i][j];
        }
        LL_PG_SYNC();
    }
}

// L z = rhs, then L' y = z, in `y` (entry 6 f + c of free pose f), block row after block row.  Forward: the six rows of a strip less
// their products with the solved entries left of the diagonal block, one piece per row; then item 0 finishes the six inside the
// block.  Backward: item 0 solves the six of the block (rows 5 .. 0); then every earlier entry k of the strip's span, one piece each,
// takes y[k] -= L[row][k] y[row] for rows 5 .. 0.  Per entry the operations and their order are those of the plain row-by-row
// solves.  A value that is not finite clears sh->chol_ok.
LL_PG_FN void pg_solve_triangular(const PgView &v, const PgGraph &gr, PgShared *sh, double *y, int tid, int nt)
{
    const int n = gr.n_poses - 1;
    for (int f = 0; f < n; f++) {
        const int p = gr.pose0 + 1 + f, c0 = 6 * v.first[p], w = 6 * f + 6 - c0;
        const double *strip = v.H + v.strip[p];
        LL_PG_FOR(row, 6)
        {
            const double *h = strip + (size_t)row * w - c0;
            double s = v.rhs[6 * (size_t)p + row];
            for (int k = c0; k < 6 * f; k++) s -= h[k] * y[k];
            y[6 * f + row] = s;
        }
        LL_PG_SYNC();
        if (tid == 0) {
            double yv[6];
            for (int row = 0; row < 6; row++) yv[row] = y[6 * f + row];
            for (int row = 0; row < 6; row++) {
                const double *h = strip + (size_t)row * w - c0 + 6 * f;
                double s = yv[row];
                for (int k = 0; k < row; k++) s -= h[k] * yv[k];
                yv[row] = s / h[row];
            }
            for (int row = 0; row < 6; row++) y[6 * f + row] = yv[row];
        }
        LL_PG_SYNC();
    }
    for (int f = n - 1; f >= 0; f--) {
        const int p = gr.pose0 + 1 + f, c0 = 6 * v.first[p], w = 6 * f + 6 - c0;
        const double *strip = v.H + v.strip[p];
        if (tid == 0) {
            double yv[6];
            for (int row = 0; row < 6; row++) yv[row] = y[6 * f + row];
            for (int row = 5; row >= 0; row--) {
                const double *h = strip + (size_t)row * w - c0 + 6 * f;
                const double xr = yv[row] / h[row];
                yv[row] = xr;
                for (int k = 0; k < row; k++) yv[k] -= h[k] * xr;
                if (!(fabs(xr) <= LL_PG_DBL_MAX)) sh->chol_ok = 0;
            }
            for (int row = 0; row < 6; row++) y[6 * f + row] = yv[row];
        }
        LL_PG_SYNC();
        LL_PG_FOR(t, 6 * f - c0)
        {
            const int k = c0 + t;
            double yk = y[k];
            for (int row = 5; row >= 0; row--) yk -= strip[(size_t)row * w - c0 + k] * y[6 * f + row];
            y[k] = yk;
        }
        LL_PG_SYNC();
    }
}

// per edge sum over its rows of m (r + m / 2), m = (scaled J) step, step = -y, the columns in ascending order
LL_PG_FN void pg_phase_model(const PgView &v, const PgGraph &gr, const double *y, int tid, int nt)
{
    LL_PG_FOR(k, gr.n_edges)
    {
        const int e = gr.edge0 + k, a = v.edge_ab[2 * e], b = v.edge_ab[2 * e + 1];
        const int lo = a < b ? 0 : 1;
        double acc = 0.0;
        for (int i = 0; i < 6; i++) {
            double m = 0.0;
            for (int s2 = 0; s2 < 2; s2++) {
                const int side = s2 == 0 ? lo : 1 - lo, q = v.edge_ab[2 * e + side];
                if (q == 0) continue;
                const double *J = v.J + 72 * (size_t)e + 36 * side + 6 * i, *ys = y + 6 * (q - 1);
                for (int c = 0; c < 6; c++) m += J[c] * -ys[c];
            }
            acc += m * (v.r[6 * (size_t)e + i] + m / 2.0);
        }
        v.ecost[e] = acc;
    }
}

// cand = Plus(x, step scaled back); per pose |x - cand|^2 into ps0
LL_PG_FN void pg_phase_candidate(const PgView &v, const PgGraph &gr, const double *y, int tid, int nt)
{
    LL_PG_FOR(k, gr.n_poses)
    {
        const int p = gr.pose0 + k;
        const double *x = v.x + 7 * (size_t)p;
        double *c = v.cand + 7 * (size_t)p;
        double s = 0.0;
        if (k == 0) {
            for (int i = 0; i < 7; i++) c[i] = x[i];
        } else {
            double d[6];
            for (int i = 0; i < 6; i++) d[i] = -y[6 * (k - 1) + i] * v.scale[6 * (size_t)p + i];
            pg_plus(x, d, c);
            for (int i = 0; i < 7; i++) s += (x[i] - c[i]) * (x[i] - c[i]);
        }
        v.ps0[p] = s;
    }
}

LL_PG_FN void pg_phase_take_candidate(const PgView &v, const PgGraph &gr, int tid, int nt)
{
    LL_PG_FOR(k, 7 * gr.n_poses) v.x[7 * (size_t)gr.pose0 + k] = v.cand[7 * (size_t)gr.pose0 + k];
}

// item 0, after pg_phase_eval: the cost, each block's half sum of squares added in edge order
LL_HD double pg_cost(const PgView &v, const PgGraph &gr)
{
    double c = 0.0;
    for (int k = 0; k < gr.n_edges; k++) c += 0.5 * v.ecost[gr.edge0 + k];
    return c;
}
// item 0, after pg_phase_scale_and_norms
LL_HD void pg_norms(const PgView &v, const PgGraph &gr, PgShared *sh)
{
    double m = 0.0, s = 0.0;
    for (int k = 1; k < gr.n_poses; k++) m = fmax(m, v.ps0[gr.pose0 + k]), s += v.ps1[gr.pose0 + k];
    sh->gmax = m, sh->x_norm = sqrt(s);
}

// residuals, Jacobian, gradient, (scales,) scaled Jacobian, cost, |x|, gradient maximum at v.x
LL_PG_FN void pg_linearise(const PgView &v, const PgGraph &gr, PgShared *sh, bool init, int tid, int nt)
{
    pg_phase_eval(v, gr, v.x, true, tid, nt);
    LL_PG_SYNC();
    pg_phase_gradient(v, gr, init, tid, nt);
    LL_PG_SYNC();
    pg_phase_scale_and_norms(v, gr, tid, nt);
    LL_PG_SYNC();
    if (tid == 0) {
        sh->cost = pg_cost(v, gr);
        pg_norms(v, gr, sh);
    }
    LL_PG_SYNC();
}

// The whole solve of graph `gi` by the nt work items of one workgroup (tid 0 .. nt - 1; every item makes the same calls).
LL_PG_FN void pg_solve_graph(const PgView &v, int gi, PgShared *sh, int tid, int nt)
{
    const PgGraph gr = v.graphs[gi];
    const ll_pose_graph_params &o = v.prm;
    ll_pose_graph_summary *out = v.summary + gi;
    if (gr.n_poses < 2 || gr.n_edges == 0) {
        if (tid == 0) {
            out->iterations = out->successful_steps = out->unsuccessful_steps = 0;
            out->termination = LL_POSE_GRAPH_NOTHING_TO_OPTIMISE;
            out->initial_cost = out->final_cost = 0.0;
        }
        return;
    }
    const int n6 = 6 * (gr.n_poses - 1);
    double *y = n6 <= LL_PG_LDS_VEC ? sh->vec : v.y + 6 * (size_t)(gr.pose0 + 1);
    if (tid == 0) {
        sh->radius = o.initial_trust_region_radius, sh->decrease_factor = 2.0;
        sh->reuse_diag = 0, sh->invalid = 0, sh->iteration = 0, sh->n_succ = 0, sh->n_unsucc = 0, sh->term = LL_POSE_GRAPH_MAX_ITERATIONS;
    }
    pg_linearise(v, gr, sh, true, tid, nt);
    if (tid == 0) sh->initial_cost = sh->cost;
    // (every pass makes a bounded number of barrier-separated phases, and there are at most max_num_iterations passes)
    for (int pass = 0; pass <= o.max_num_iterations; pass++) {
        if (tid == 0) {
            sh->go = 0;
            if (sh->iteration >= o.max_num_iterations) sh->term = LL_POSE_GRAPH_MAX_ITERATIONS;
            else if (sh->gmax <= o.gradient_tolerance) sh->term = LL_POSE_GRAPH_GRADIENT;
            else if (sh->radius <= o.min_trust_region_radius) sh->term = LL_POSE_GRAPH_RADIUS;
            else sh->go = 1, sh->iteration++, sh->chol_ok = 1;
        }
        LL_PG_SYNC();
        if (!sh->go) break;
        pg_phase_assemble(v, gr, tid, nt);
        LL_PG_SYNC();
        pg_phase_damp(v, gr, sh, tid, nt);
        LL_PG_SYNC();
        pg_factor(v, gr, sh, tid, nt);
        pg_solve_triangular(v, gr, sh, y, tid, nt);
        if (tid == 0) sh->reuse_diag = 1;
        LL_PG_SYNC();
        if (sh->chol_ok) pg_phase_model(v, gr, y, tid, nt);
        LL_PG_SYNC();
        if (tid == 0) {
            double change = 0.0;
            if (sh->chol_ok)
                for (int k = 0; k < gr.n_edges; k++) change -= v.ecost[gr.edge0 + k];
            sh->model_cost_change = change;
            sh->action = 1;
            if (!sh->chol_ok || !(change > 0.0)) {
                if (++sh->invalid >= o.max_num_consecutive_invalid_steps) {
                    sh->term = LL_POSE_GRAPH_INVALID_STEPS, sh->action = 3;
                } else {
                    sh->radius *= 0.5, sh->reuse_diag = 1, sh->n_unsucc++, sh->action = 0;
                }
            } else {
                sh->invalid = 0;
            }
        }
        LL_PG_SYNC();
        if (sh->action == 3) break;
        if (sh->action == 0) continue;
        pg_phase_candidate(v, gr, y, tid, nt);
        LL_PG_SYNC();
        pg_phase_eval(v, gr, v.cand, false, tid, nt);
        LL_PG_SYNC();
        if (tid == 0) {
            double cand_cost = pg_cost(v, gr), step2 = 0.0;
            if (!(fabs(cand_cost) <= LL_PG_DBL_MAX)) cand_cost = LL_PG_DBL_MAX;
            for (int k = 1; k < gr.n_poses; k++) step2 += v.ps0[gr.pose0 + k];
            const double cost_change = sh->cost - cand_cost;
            sh->action = 0;
            if (sqrt(step2) <= o.parameter_tolerance * (sh->x_norm + o.parameter_tolerance)) {
                sh->term = LL_POSE_GRAPH_PARAMETER, sh->action = 3;
            } else if (fabs(cost_change) <= o.function_tolerance * sh->cost) {
                sh->term = LL_POSE_GRAPH_FUNCTION, sh->action = 3;
            } else {
                const double rho = cost_change / sh->model_cost_change;
                if (rho > o.min_relative_decrease) {
                    const double t = 2.0 * rho - 1.0;
                    sh->radius = fmin(o.max_trust_region_radius, sh->radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
                    sh->decrease_factor = 2.0, sh->reuse_diag = 0, sh->n_succ++, sh->action = 2;
                } else {
                    sh->radius = sh->radius / sh->decrease_factor;
                    sh->decrease_factor *= 2.0, sh->reuse_diag = 1, sh->n_unsucc++;
                }
            }
        }
        LL_PG_SYNC();
        if (sh->action == 3) break;
        if (sh->action == 2) {
            pg_phase_take_candidate(v, gr, tid, nt);
            LL_PG_SYNC();
            pg_linearise(v, gr, sh, false, tid, nt);
        }
    }
    if (tid == 0) {
        out->iterations = sh->iteration, out->successful_steps = sh->n_succ, out->unsuccessful_steps = sh->n_unsucc;
        out->termination = sh->term, out->initial_cost = sh->initial_cost, out->final_cost = sh->cost;
    }
}

}  // namespace ll
