// lm_wave_host.cpp -- CPU tier of the wavefront form of the LM controller (tests/test_lm_wave_host.py builds and runs it).
//
// loam_livox_amd/csrc/ll_lm_wave.h (lmw_init / lmw_update, a loop over 64 lanes standing in for the wavefront) against the scalar
// controller of ll_reg_core.h (lm_init / lm_update, taken in lm_update's own pieces so that the answer of every piece is known), both
// compiled with -ffp-contract=off.  Every sequence drives the two forms with the same evaluations -- the scalar form's candidates are
// evaluated, the wave form's must be the same bytes -- and after every call the whole LmCtl and the return codes are compared.
//
//   lm_wave_host N [DUMP N_DUMP]
// runs sequences 0 .. N-1 (kind = index % 16, parameters drawn from the index: fixed seeds) and prints one line per sequence:
//   index kind calls mask mismatches
// mask: which branches of the controller the sequence reached (bits below).  DUMP: the first N_DUMP sequences' inputs for the device tap
// (ll_debug_lm_sequence): per sequence 12 doubles {x0[7], bound, max_iter, n_active, calls, 0} and LMW_MAX_CALLS * 28 evaluations.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../loam_livox_amd/csrc/ll_lm_wave.h"

using namespace ll;

enum {
    B_ACCEPT = 0, B_REJECT, B_REUSE0, B_REUSE1, B_INVALID, B_INVALID5, B_PARAM_TOL, B_FUNC_TOL, B_GMAX, B_NACTIVE0, B_RADIUS, B_UNBOUNDED, B_CUBIC, B_FIT,
    B_FIRST_FALLBACK, B_CLAMPED, B_ND0, B_ND_BIG, B_NONFINITE_COST, B_MAXITER, B_FIRST_AT_ONCE, B_SEARCH_OK
};
#define LMW_MAX_CALLS 32
#define LMW_SEQ_LIMIT 400

struct Rng {
    uint64_t s;
    double u()  // [0, 1)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)((s >> 11) & ((1ull << 53) - 1)) / 9007199254740992.0;
    }
    double n() { return sqrt(-2.0 * log(1.0 - u())) * cos(6.283185307179586 * u()); }
};

// a random 6-parameter Huber problem: features f_i, true increment (q*, t*), a plane or a line through R* f + t* + noise
struct Problem {
    int n;
    std::vector<int> kind;
    std::vector<double> f, a, v;
    double huber_a;
    void eval(const double x[7], double e[LL_NACC]) const
    {
        double R[9];
        quat_to_mat(x, R);
        for (int i = 0; i < LL_NACC; i++) e[i] = 0.0;
        for (int i = 0; i < n; i++) block_accumulate(kind[i], R, x + 4, &f[3 * i], &a[3 * i], &v[3 * i], huber_a, e);
    }
};

static void make_problem(Rng &r, Problem &p, double rot, double trans, double noise, double outliers)
{
    p.n = 24 + (int)(r.u() * 40);
    p.huber_a = 0.1;
    p.kind.resize(p.n);
    p.f.resize(3 * p.n), p.a.resize(3 * p.n), p.v.resize(3 * p.n);
    double ax[3] = {r.n(), r.n(), r.n()};
    const double an = sqrt(dot3(ax, ax));
    const double q[4] = {sin(0.5 * rot) * ax[0] / an, sin(0.5 * rot) * ax[1] / an, sin(0.5 * rot) * ax[2] / an, cos(0.5 * rot)};
    const double t[3] = {trans * r.n(), trans * r.n(), trans * r.n()};
    for (int i = 0; i < p.n; i++) {
        double *f = &p.f[3 * i], *a = &p.a[3 * i], *v = &p.v[3 * i], w[3];
        for (int k = 0; k < 3; k++) f[k] = 20.0 * (r.u() - 0.5);
        quat_rot(q, f, w);
        const double s = r.u() < outliers ? 3.0 : noise;
        for (int k = 0; k < 3; k++) w[k] += t[k] + s * r.n();
        for (int k = 0; k < 3; k++) v[k] = r.n();
        const double vn = sqrt(dot3(v, v));
        for (int k = 0; k < 3; k++) v[k] /= vn;
        p.kind[i] = (i % 4 == 0) ? BLK_LINE : BLK_PLANE;
        if (p.kind[i] == BLK_LINE) {
            a[0] = w[0], a[1] = w[1], a[2] = w[2];
        } else {
            a[0] = dot3(v, w), a[1] = 0.0, a[2] = 0.0;
        }
    }
}

// hand-made sums: H = h on the diagonal and off in H(0,1), the gradient g, the cost
static void hand_made(double e[LL_NACC], double h, double off01, const double g[6], double cost)
{
    for (int i = 0; i < LL_NACC; i++) e[i] = 0.0;
    for (int j = 0; j < 6; j++) e[hidx(j, j)] = h, e[21 + j] = g[j];
    e[hidx(0, 1)] = off01;
    e[27] = cost;
}

struct Seq {
    int kind, max_iter, n_active;
    double x0[7], bound;
    Problem p;
    // evaluation number k (0: at the start) at the point x
    void eval(int k, const double x[7], double e[LL_NACC]) const
    {
        const double g1[6] = {1, 1, 1, 1, 1, 1};
        double g[6];
        switch (kind) {
        default: p.eval(x, e); break;
        case 8: p.eval(x, e); break;                     // (n_active = 0)
        case 9: hand_made(e, 1.0, 5.0, g1, 1.0); break;  // indefinite: the second pivot is negative
        case 10:                                         // pivots positive, the solution overflows
            for (int j = 0; j < 6; j++) g[j] = 1e308;
            hand_made(e, 1e-300, 0.0, g, 1.0);
            break;
        case 11:  // the model cost change underflows to zero
            for (int j = 0; j < 6; j++) g[j] = 2e-10;
            hand_made(e, 1e308, 0.0, g, 1.0);
            break;
        case 12:  // every candidate is worse: the radius shrinks until it ends the solve
            for (int j = 0; j < 6; j++) g[j] = 1e45;
            hand_made(e, 1.0, 0.0, g, k == 0 ? 1.0 : 2.0);
            break;
        case 13:  // no rotation in the step (nd == 0), then a gradient of zero (gmax ends the solve)
            for (int j = 0; j < 6; j++) g[j] = (j < 3 || k >= 3) ? 0.0 : 0.1 / (1 + k);
            hand_made(e, 1.0, 0.0, g, 1.0 / (1 + k));
            break;
        case 14: {  // a line search on scripted costs: not finite, then too high (cubic, then the fit), then low enough
            static const double cost[8] = {1.0, NAN, 1.5, 1.4, 1.3, 0.5, 0.49, 0.489};
            for (int j = 0; j < 6; j++) g[j] = (k & 1) ? -0.3 : 0.2;
            hand_made(e, 1.0, 0.1, g, k < 8 ? cost[k] : 0.489 - 1e-3 * k);
            break;
        }
        case 15:  // a line search that never finds its step: twenty contractions, then the full step's evaluation comes back
            for (int j = 0; j < 6; j++) g[j] = 0.2;
            hand_made(e, 1.0, 0.1, g, k == 0 ? 1.0 : 1.0 + 1.0 / (1 + k));
            break;
        }
    }
};

static void make_seq(int index, Seq &s)
{
    Rng r{0x9E3779B97F4A7C15ull * (uint64_t)(index + 1)};
    s.kind = index % 16;
    s.max_iter = 100;
    s.n_active = 1;
    s.bound = -1.0;
    const double id[7] = {0, 0, 0, 1, 0, 0, 0};
    for (int i = 0; i < 7; i++) s.x0[i] = id[i];
    double rot = 0.02 * r.u(), trans = 0.1, noise = 0.01, outliers = 0.1;
    switch (s.kind) {
    case 0: break;                                             // small motion, no bound
    case 1: s.bound = 10.0; break;                             // bound far away
    case 2: s.bound = 0.05 + 0.1 * r.u(), trans = 0.3; break;  // the translation runs into the bound
    case 3: s.bound = 0.002 + 0.02 * r.u(), trans = 0.5; break;
    case 4: rot = 0.8 + 1.2 * r.u(), trans = 1.0; break;       // a large rotation: steps with nd >= 0.25
    case 5: rot = 0.5 + r.u(), trans = 1.0, s.bound = 0.2 + r.u(); break;
    case 6: s.max_iter = 1 + (int)(3 * r.u()), s.bound = (index & 16) ? 0.1 : -1.0, trans = 0.3; break;
    case 7: noise = 0.0, outliers = 0.0, s.bound = (index & 16) ? 1.0 : -1.0; break;  // exact data
    case 8: s.n_active = 0; break;
    case 13: s.bound = (index & 16) ? 0.04 : -1.0; break;
    case 14: s.bound = 0.5 + r.u(); break;
    case 15: s.bound = 0.5 + r.u(); break;
    default: break;
    }
    if (s.kind <= 8) {
        make_problem(r, s.p, rot, trans, noise, outliers);
        if (s.kind == 3 && (index & 32)) s.x0[4] = 5.0 * s.bound;  // a start outside the bounds (lm_begin projects it)
    }
}

static int g_mismatch_reports = 0;
static int compare(const LmCtl &a, const LmCtl &b, int ra, int rb, int index, int call)
{
    if (memcmp(&a, &b, sizeof(LmCtl)) == 0 && ra == rb) return 0;
    if (g_mismatch_reports++ < 8) {
        fprintf(stderr, "sequence %d call %d: return %d / %d\n", index, call, ra, rb);
        const unsigned char *pa = (const unsigned char *)&a, *pb = (const unsigned char *)&b;
        for (size_t o = 0; o < sizeof(LmCtl); o += 8)
            if (memcmp(pa + o, pb + o, 8)) {
                double da, db;
                memcpy(&da, pa + o, 8), memcpy(&db, pb + o, 8);
                fprintf(stderr, "  offset %zu: %.17g / %.17g\n", o, da, db);
            }
    }
    return 1;
}

static inline void flag(unsigned &m, int b) { m |= 1u << b; }

// what a proposal (c.cand just made from c.x, c.delta * ls) says about state_plus
static void note_proposal(const LmCtl &c, double ls, unsigned &mask)
{
    const double nd = ls * sqrt(c.delta[0] * c.delta[0] + c.delta[1] * c.delta[1] + c.delta[2] * c.delta[2]);
    if (nd == 0.0) flag(mask, B_ND0);
    if (nd >= 0.25) flag(mask, B_ND_BIG);
    if (c.bound >= 0)
        for (int i = 0; i < 3; i++)
            if (c.cand[4 + i] == c.bound || c.cand[4 + i] == -c.bound) flag(mask, B_CLAMPED);
}

static void note_propose_end(const LmCtl &before, const LmCtl &c, int ret, unsigned &mask)
{
    if (ret) {
        note_proposal(c, 1.0, mask);
    } else {
        if (c.invalid_steps >= 5) flag(mask, B_INVALID5);
        if (c.radius < 1e-32) flag(mask, B_RADIUS);
        if (c.gmax <= 1e-10) flag(mask, B_GMAX);
        if (c.iteration >= c.max_iter && !(c.gmax <= 1e-10) && !(c.radius < 1e-32) && c.invalid_steps < 5) flag(mask, B_MAXITER);
    }
    if (c.iteration > before.iteration) flag(mask, before.reuse_diagonal ? B_REUSE1 : B_REUSE0);
    if (c.invalid_steps > 0) flag(mask, B_INVALID);
}

int main(int argc, char **argv)
{
    const int N = argc > 1 ? atoi(argv[1]) : 2048;
    FILE *dump = argc > 3 ? fopen(argv[2], "wb") : nullptr;
    const int n_dump = argc > 3 ? atoi(argv[3]) : 0;
    int total_mismatch = 0;
    std::vector<double> rec(12 + LMW_MAX_CALLS * LL_NACC);
    for (int index = 0; index < N; index++) {
        Seq s;
        make_seq(index, s);
        LmCtl cs, cw;  // scalar, wave
        memset(&cs, 0, sizeof cs), memset(&cw, 0, sizeof cw);
        double fit[10], e[LL_NACC];
        unsigned mask = 0;
        int mism = 0, calls = 0;
        std::fill(rec.begin(), rec.end(), 0.0);
        if (s.bound < 0) flag(mask, B_UNBOUNDED);
        lm_begin(cs, s.x0, s.max_iter, s.bound);
        lm_begin(cw, s.x0, s.max_iter, s.bound);
        s.eval(0, cs.x, e);
        if (calls < LMW_MAX_CALLS) memcpy(&rec[12 + calls * LL_NACC], e, sizeof e);
        calls++;
        LmCtl before = cs;
        int rs = lm_init(cs, e, s.n_active), rw = lmw_init(cw, e, s.n_active, 0);
        mism += compare(cs, cw, rs, rw, index, 0);
        if (s.n_active == 0) flag(mask, B_NACTIVE0);
        else note_propose_end(before, cs, rs, mask);
        while (rs && rw && calls < LMW_SEQ_LIMIT) {
            s.eval(calls, cs.cand, e);
            if (calls < LMW_MAX_CALLS) memcpy(&rec[12 + calls * LL_NACC], e, sizeof e);
            before = cs;
            // the scalar form, in the pieces of lm_update
            double e_in[LL_NACC], cur_cost = 0.0, cg = 0.0;
            for (int i = 0; i < LL_NACC; i++) e_in[i] = e[i];
            int code = lm_update_pre(cs, e_in, &cur_cost, &cg);
            if (!((e[27] - e[27]) == 0.0)) flag(mask, B_NONFINITE_COST);
            if (code == LM_FIT) {
                flag(mask, B_FIT);
                code = lm_update_post(cs, cur_cost, cg,
                                      lm_quintic_min_step(cs.cost, cs.gd, cs.ls_step, cur_cost, cg, cs.ls_prev_x, cs.ls_prev_f, cs.ls_prev_g, 1e-3 * cs.ls_step,
                                                          0.6 * cs.ls_step));
            } else if (code == LM_EVAL && before.bound >= 0 && !before.ls_prev_valid && (e[27] - e[27]) == 0.0) {
                flag(mask, B_CUBIC);
            }
            if (code == LM_EVAL) note_proposal(cs, cs.ls_step, mask);
            if (code == LM_FINISH_FIRST) flag(mask, cs.ls_iter > 1 ? B_FIRST_FALLBACK : B_FIRST_AT_ONCE);
            if (code == LM_FINISH_E && before.ls_iter > 0) flag(mask, B_SEARCH_OK);
            int proposes = -1;  // lm_update_finish goes on to lm_propose: with reuse_diagonal 0 (accepted) or 1 (rejected)
            if (code != LM_EVAL) {  // which of lm_update_finish's ends this call takes
                const double *ee = code == LM_FINISH_FIRST ? cs.first_eval : e_in;
                double cc = ee[27], sn = 0.0;
                if (!((cc - cc) == 0.0)) cc = DBL_MAX;
                for (int i = 0; i < 7; i++) sn += (cs.x[i] - cs.cand[i]) * (cs.x[i] - cs.cand[i]);
                if (sqrt(sn) <= 1e-8 * (cs.x_norm + 1e-8)) flag(mask, B_PARAM_TOL);
                else if (fabs(cs.cost - cc) <= 1e-6 * cs.cost) flag(mask, B_FUNC_TOL);
                else proposes = (cs.cost - cc) / cs.model_cost_change > 1e-3 ? 0 : 1;
                if (proposes >= 0) flag(mask, proposes ? B_REJECT : B_ACCEPT);
            }
            LmCtl at = cs;  // (of the iterate lm_propose starts from, its iteration count and reuse flag are looked at)
            rs = lm_update_close(cs, e_in, code);
            if (proposes >= 0) {
                at.reuse_diagonal = proposes;
                note_propose_end(at, cs, rs, mask);
            }
            rw = lmw_update(cw, e, fit, 0);
            mism += compare(cs, cw, rs, rw, index, calls);
            calls++;
        }
        total_mismatch += mism;
        printf("%d %d %d %u %d\n", index, s.kind, calls, mask, mism);
        if (dump && index < n_dump) {
            for (int i = 0; i < 7; i++) rec[i] = s.x0[i];
            rec[7] = s.bound, rec[8] = s.max_iter, rec[9] = s.n_active, rec[10] = calls < LMW_MAX_CALLS ? calls : LMW_MAX_CALLS;
            fwrite(rec.data(), sizeof(double), rec.size(), dump);
        }
    }
    if (dump) fclose(dump);
    return total_mismatch ? 1 : 0;
}
