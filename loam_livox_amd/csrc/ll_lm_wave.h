// ll_lm_wave.h -- the Levenberg-Marquardt controller step (ll_reg_core.h lm_init / lm_update / lm_propose) on the controller's whole
// wavefront.  The scalar form in ll_reg_core.h is the specification; this text computes the same LmCtl, byte for byte, after every call:
// every sum takes its terms in the scalar form's index order, nothing is reassociated, every division stays a division.  What changes is
// who does the work while the workgroup waits at its barrier:
//   * lane i copies value i of the evaluation (first_eval, H, g) instead of lane 0 copying 28;
//   * lanes 0 .. 5 own row a of the scaled system: Hs, A, the Cholesky factor L, gs[a], diag[a] and row a of Hs * step, six registers
//     per array instead of three 6 x 6 arrays on one lane.  A column of L is one multiply-subtract sweep on all rows at once; the pivot
//     (square root and reciprocal), the back substitution and the two dot products are made once from values every lane reads;
//   * the two state_plus of an accepted step -- the projected gradient at the new x and the candidate -- are the same code on two lanes.
//     The gmax <= 1e-10 test of lm_propose is applied afterwards and nothing of the proposal is stored when it ends the solve;
//   * the norm of the step and the norm of the candidate (the new x_norm) are the same seven-term sum on two lanes.
// The text is written against a small lane-exchange vocabulary (below) so that a host compiler builds it too, a loop over 64 lanes standing
// in for the wavefront (tests/lm_wave_host.cpp):
//   LMW_VAR / LMW_ARR   a value (an array) every lane has its own copy of;   LMW_V / LMW_A   this lane's copy, inside LMW_FOR( l )
//   LMW_FOR( l )        the lanes' work between two exchanges;               LMW_BC / LMW_BCA  lane src's copy, outside the block that wrote it
//   LMW_ONE             once (lane 0), for stores of values all lanes hold;  LMW_FENCE()       LDS stores of one lane before loads of the others
// Everything outside LMW_FOR is computed by all lanes from the same operands (uniform).  All 64 lanes must call these functions.
#pragma once
#include "ll_reg_core.h"

#if defined(__HIP_DEVICE_COMPILE__)
namespace ll {
__device__ __forceinline__ double lmw_readlane(double v, int src)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
__device__ __forceinline__ void lmw_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // same wavefront: its LDS operations execute in order
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
}  // namespace ll
#define LMW_FOR(l) for (int l = lane_, lmw_once_ = 1; lmw_once_; lmw_once_ = 0)
#define LMW_VAR(T, name) T name
#define LMW_ARR(T, name, n) T name[n]
#define LMW_V(name) name
#define LMW_A(name, k) name[k]
#define LMW_BC(name, src) lmw_readlane(name, src)
#define LMW_BCA(name, k, src) lmw_readlane(name[k], src)
#define LMW_BCI(name, src) __builtin_amdgcn_readlane(name, src)
#define LMW_ONE if (lane_ == 0)
#define LMW_FENCE() lmw_fence()
#define LMW_QUINTIC(a) lm_quintic_min_step_wave_call(a, lane_)
#else
#define LMW_FOR(l) for (int l = 0; l < 64; l++)
#define LMW_VAR(T, name) T name[64]
#define LMW_ARR(T, name, n) T name[64][n]
#define LMW_V(name) name[l]
#define LMW_A(name, k) name[l][k]
#define LMW_BC(name, src) name[src]
#define LMW_BCA(name, k, src) name[src][k]
#define LMW_BCI(name, src) name
#define LMW_ONE
#define LMW_FENCE() ((void)0)
#define LMW_QUINTIC(a) lm_quintic_min_step(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9])
#endif

namespace ll {

// lm_propose.  defer_gmax: the caller has accepted a step (or starts the solve) and c.gmax at the new c.x is still to be made: it is made
// beside the candidate and tested before anything of the proposal is stored.  stop: the solve ends whatever the iterate (lm_init without
// an active block).  Returns 1 if c.cand must be evaluated, 0 if finished (the same on every lane).
LL_HD int lmw_propose(LmCtl &c, bool defer_gmax, bool stop, int lane_)
{
    (void)lane_;
    LMW_FENCE();  // the caller's stores to c, lane by lane, before everybody's loads
    int iteration = c.iteration, invalid_steps = c.invalid_steps, reuse = c.reuse_diagonal;
    const int max_iter = c.max_iter;
    double radius = c.radius;
    const double bound = c.bound;
    bool need_gmax = defer_gmax;
    if (!defer_gmax && c.gmax <= 1e-10) stop = true;
    double xv[7], gv[6], scv[6];
    LL_UNROLL
    for (int i = 0; i < 7; i++) xv[i] = c.x[i];
    LL_UNROLL
    for (int i = 0; i < 6; i++) gv[i] = c.g[i], scv[i] = c.scale[i];
    // row a of the scaled system on lane a (the lanes beyond 5 repeat row 5)
    LMW_ARR(double, Hs, 6);
    LMW_VAR(double, gs);
    LMW_VAR(double, Hd);
    LMW_VAR(double, dg);
    LMW_FOR(l)
    {
        const int a = l < 6 ? l : 5;
        const double sa = c.scale[a];
        LMW_V(gs) = c.g[a] * sa;
        LL_UNROLL
        for (int b = 0; b < 6; b++) {
            const double h = (a <= b) ? c.H[hidx(a, b)] : c.H[hidx(b, a)];
            LMW_A(Hs, b) = h * sa * scv[b];
        }
        LMW_V(Hd) = c.H[hidx(a, a)] * sa * sa;  // Hs[a][a]
        LMW_V(dg) = c.diag[a];
    }
    int ret;
    double step[6], delta[6] = {0, 0, 0, 0, 0, 0}, mcc = 0.0, gd = 0.0, dmax = 0.0;
    LMW_ARR(double, po, 7);  // state_plus on lane 0 (the candidate) and lane 1 (the projected gradient step)
    LMW_VAR(double, pm);
    for (;;) {
        int mode;  // 0: a valid step, 1: an invalid one, 2: the solve ends here
        if (stop || iteration >= max_iter || radius < 1e-32) {
            if (!need_gmax) {
                ret = 0;
                break;
            }
            mode = 2;
        } else {
            iteration++;
            if (!reuse) {
                LMW_FOR(l) LMW_V(dg) = fmin(fmax(LMW_V(Hd), 1e-6), 1e32);
            }
            reuse = 1;
            LMW_ARR(double, Ar, 6);
            LMW_ARR(double, Lr, 6);
            LMW_VAR(double, s);
            LMW_FOR(l)
            {
                const double dr = LMW_V(dg) / radius;
                LL_UNROLL
                for (int b = 0; b < 6; b++) {
                    LMW_A(Ar, b) = (b == l) ? LMW_A(Hs, b) + dr : LMW_A(Hs, b);
                    LMW_A(Lr, b) = 0.0;
                }
            }
            // chol_solve6: column j of L on all rows at once, the pivot once
            int ok = 1;
            double inv[6];
            LL_UNROLL
            for (int j = 0; j < 6; j++) {
                LMW_FOR(l)
                {
                    double t = LMW_A(Ar, j);
                    LL_UNROLL
                    for (int k = 0; k < 6; k++)
                        if (k < j) t -= LMW_A(Lr, k) * LMW_BCA(Lr, k, j);
                    LMW_V(s) = t;
                }
                const double sp = LMW_BC(s, j);
                if (!(sp > 0.0)) ok = 0;
                const double d = sqrt(sp);
                inv[j] = 1.0 / d;
                LMW_FOR(l) LMW_A(Lr, j) = (l == j) ? d : LMW_V(s) * inv[j];
            }
            // L y = gs: row i is complete once y[0 .. i) have been taken from it, in that order
            double y[6], x[6];
            LMW_VAR(double, fs);
            LMW_FOR(l) LMW_V(fs) = LMW_V(gs);
            LL_UNROLL
            for (int i = 0; i < 6; i++) {
                y[i] = LMW_BC(fs, i) * inv[i];
                LMW_FOR(l) LMW_V(fs) -= LMW_A(Lr, i) * y[i];
            }
            // L^T x = y: the terms of x[i] in the order k = i + 1 .. 5, as in the scalar form
            LL_UNROLL
            for (int i = 5; i >= 0; i--) {
                double t = y[i];
                LL_UNROLL
                for (int k = 0; k < 6; k++)
                    if (k > i) t -= LMW_BCA(Lr, i, k) * x[k];
                x[i] = t * inv[i];
            }
            LL_UNROLL
            for (int i = 0; i < 6; i++)
                if (!((x[i] - x[i]) == 0.0)) ok = 0;
            mcc = 0.0;
            if (ok) {
                double sg = 0.0, sHs = 0.0;
                LL_UNROLL
                for (int a = 0; a < 6; a++) step[a] = -x[a];
                LMW_VAR(double, tr);
                LMW_FOR(l)
                {
                    double t = 0.0;
                    LL_UNROLL
                    for (int b = 0; b < 6; b++) t += LMW_A(Hs, b) * step[b];
                    LMW_V(tr) = t;
                }
                LL_UNROLL
                for (int a = 0; a < 6; a++) {
                    sg += step[a] * LMW_BC(gs, a);
                    sHs += step[a] * LMW_BC(tr, a);
                }
                mcc = -sg - 0.5 * sHs;
            }
            mode = (ok && mcc > 0.0) ? 0 : 1;
        }
        if (mode == 0) {
            gd = 0.0;
            dmax = 0.0;
            LL_UNROLL
            for (int j = 0; j < 6; j++) {
                delta[j] = step[j] * scv[j];
                gd += gv[j] * delta[j];
                dmax = fmax(dmax, fabs(delta[j]));
            }
        }
        if (mode == 0 || need_gmax) {
            LMW_FOR(l)
            {
                const bool grad = need_gmax && (l == 1 || mode != 0);
                double d[6], out[7], m = 0.0;
                LL_UNROLL
                for (int j = 0; j < 6; j++) d[j] = grad ? -gv[j] : delta[j];
                state_plus(xv, d, bound, out);
                LL_UNROLL
                for (int i = 0; i < 7; i++) {
                    m = fmax(m, fabs(xv[i] - out[i]));  // lm_gradient_max_norm
                    LMW_A(po, i) = out[i];
                }
                LMW_V(pm) = m;
            }
        }
        if (need_gmax) {
            const double gm = LMW_BC(pm, 1);
            need_gmax = false;
            LMW_ONE c.gmax = gm;
            if (gm <= 1e-10 || mode == 2) {  // lm_propose ends the solve before it touches anything else
                LMW_ONE c.done = 1;
                return 0;
            }
        }
        if (mode == 1) {
            if (++invalid_steps >= 5) {
                ret = 0;
                break;
            }
            radius *= 0.5;
            continue;
        }
        invalid_steps = 0;
        ret = 1;
        break;
    }
    LMW_FOR(l)
    {
        if (l < 6) c.diag[l] = LMW_V(dg);
        if (l == 0 && ret)
            for (int i = 0; i < 7; i++) c.cand[i] = LMW_A(po, i);
    }
    LMW_ONE
    {
        c.iteration = iteration;
        c.reuse_diagonal = reuse;
        c.invalid_steps = invalid_steps;
        c.radius = radius;
        if (ret) {
            c.model_cost_change = mcc;
            c.gd = gd;
            c.dmax = dmax;
            for (int j = 0; j < 6; j++) c.delta[j] = delta[j];
            c.ls_step = 1.0;
            c.ls_iter = 0;
            c.ls_active = 0;
            c.ls_prev_valid = 0;
        } else {
            c.done = 1;
        }
    }
    return ret;
}

// lm_init: e = the 28 sums of the first evaluation (at c.x after lm_begin)
LL_HD int lmw_init(LmCtl &c, const double *e, int n_active, int lane_)
{
    (void)lane_;
    LMW_FOR(l)
    {
        const double ev = e[l < LL_NACC ? l : LL_NACC - 1];
        if (l < 21)
            c.H[l] = ev;
        else if (l < 27)
            c.g[l - 21] = ev;
        if (l < 6) c.scale[l] = 1.0 / (1.0 + sqrt(e[hidx(l, l)]));
    }
    LMW_ONE
    {
        c.cost = e[27];
        c.initial_cost = e[27];
        c.final_cost = e[27];
        c.iteration = 0;
        c.radius = 1e4;
        c.decrease_factor = 2.0;
        c.reuse_diagonal = 0;
        c.invalid_steps = 0;
    }
    return lmw_propose(c, true, n_active == 0, lane_);
}

// the line search's decision of lm_update_pre, on the lane that holds the controller: cur_cost and eg are the cost and the gradient of the
// evaluation at c.cand (the copy to c.first_eval is the wavefront's)
LL_HD int lmw_line_search(LmCtl &c, double cur_cost, const double eg[6], double *cg_out)
{
    const bool finite_cost = (cur_cost - cur_cost) == 0.0;
    if (!finite_cost || cur_cost > c.cost + 1e-4 * c.gd * c.ls_step) {
        int failed = 0;
        double new_step = 0.0, cg = 0.0;
        if (++c.ls_iter >= 20) {
            failed = 1;
        } else {
            if (!finite_cost) {
                new_step = fmin(fmax(c.ls_step * 0.5, 1e-3 * c.ls_step), 0.6 * c.ls_step);
            } else {
                for (int j = 0; j < 6; j++) cg += eg[j] * c.delta[j];
                if (c.ls_prev_valid) {  // three samples: the quintic (second and later contractions)
                    *cg_out = cg;
                    return LM_FIT;
                }
                new_step = lm_cubic_min_step(c.cost, c.gd, c.ls_step, cur_cost, cg, 1e-3 * c.ls_step, 0.6 * c.ls_step);
            }
            if (new_step * c.dmax < 1e-9) failed = 1;
        }
        return lm_update_contract(c, failed, new_step, finite_cost ? 1 : 0, cur_cost, cg);
    } else if (c.ls_step != 1.0) {
        for (int j = 0; j < 6; j++) c.delta[j] *= c.ls_step;
    }
    return LM_FINISH_E;
}

// lm_update: sum = the 28 sums of the evaluation at c.cand, fit = ten doubles the wavefront shares (the arguments of a three-sample fit).
// Returns 1 if another evaluation (at the new c.cand) is needed (the same on every lane).
LL_HD int lmw_update(LmCtl &c, const double *sum, double *fit, int lane_)
{
    (void)lane_;
    LMW_VAR(double, ev);  // lane i < 28: value i of the evaluation that stands
    LMW_FOR(l) LMW_V(ev) = sum[l < LL_NACC ? l : LL_NACC - 1];
    const bool bounded = c.bound >= 0;
    const int ls_active = c.ls_active;
    int code = LM_FINISH_E;
    if (bounded && !ls_active) {
        LMW_FOR(l)
        {
            if (l < LL_NACC) c.first_eval[l] = LMW_V(ev);
            if (l < 7) c.first_cand[l] = c.cand[l];
        }
        LMW_FENCE();  // (a search that fails at once takes c.first_cand back on lane 0)
    }
    {
        const double cur_cost = LMW_BC(ev, 27);
        double eg[6];
        LL_UNROLL
        for (int j = 0; j < 6; j++) eg[j] = LMW_BC(ev, 21 + j);
        LMW_ONE
        {
            c.last_accept = 0;
            if (bounded) {
                c.ls_active = 1;
                double cg = 0.0;
                code = lmw_line_search(c, cur_cost, eg, &cg);
                if (code == LM_FIT) {
                    fit[0] = c.cost, fit[1] = c.gd, fit[2] = c.ls_step, fit[3] = cur_cost, fit[4] = cg, fit[5] = c.ls_prev_x, fit[6] = c.ls_prev_f, fit[7] = c.ls_prev_g;
                    fit[8] = 1e-3 * c.ls_step, fit[9] = 0.6 * c.ls_step;
                }
            }
        }
        code = LMW_BCI(code, 0);
    }
    if (code == LM_FIT) {
        LMW_FENCE();
        const double step = LMW_QUINTIC(fit);
        LMW_ONE code = lm_update_post(c, fit[3], fit[4], step);
        code = LMW_BCI(code, 0);
    }
    if (code == LM_EVAL) return 1;
    // ---- lm_update_finish
    LMW_FENCE();  // lane 0's c.cand, c.delta and c.ls_iter
    const int from_first = (code == LM_FINISH_FIRST && c.ls_iter > 1) ? 1 : 0;
    if (code == LM_FINISH_FIRST) {
        LMW_FOR(l) LMW_V(ev) = c.first_eval[l < LL_NACC ? l : LL_NACC - 1];  // (what this lane stored)
    }
    double cand_cost = LMW_BC(ev, 27);
    if (!((cand_cost - cand_cost) == 0.0)) cand_cost = DBL_MAX;
    // the norm of the step on lane 0, of the candidate (x_norm if it is accepted) on lane 1
    LMW_VAR(double, nrm);
    LMW_FOR(l)
    {
        double n = 0.0;
        LL_UNROLL
        for (int i = 0; i < 7; i++) {
            const double xi = c.x[i], ci = c.cand[i];
            const double v = (l == 1) ? ci : xi - ci;
            n += v * v;
        }
        LMW_V(nrm) = sqrt(n);
    }
    const double step_norm = LMW_BC(nrm, 0), cand_norm = LMW_BC(nrm, 1);
    if (step_norm <= 1e-8 * (c.x_norm + 1e-8)) {  // ParameterToleranceReached
        LMW_ONE c.done = 1;
        return 0;
    }
    const double cost = c.cost;
    const double cost_change = cost - cand_cost;
    if (fabs(cost_change) <= 1e-6 * cost) {  // FunctionToleranceReached
        LMW_ONE c.done = 1;
        return 0;
    }
    const double relative_decrease = cost_change / c.model_cost_change;
    const bool accepted = relative_decrease > 1e-3;
    if (accepted) {
        LMW_FOR(l)
        {
            if (l < 7) c.x[l] = c.cand[l];
            if (l < 21)
                c.H[l] = LMW_V(ev);
            else if (l < 27)
                c.g[l - 21] = LMW_V(ev);
        }
        LMW_ONE
        {
            c.last_accept = from_first ? 2 : 1;
            c.x_norm = cand_norm;
            c.cost = cand_cost;
            if (cand_cost < c.final_cost) c.final_cost = cand_cost;
            const double t = 2.0 * relative_decrease - 1.0;
            c.radius = c.radius / fmax(1.0 / 3.0, 1.0 - t * t * t);
            c.radius = fmin(1e16, c.radius);
            c.decrease_factor = 2.0;
            c.reuse_diagonal = 0;
        }
    } else {
        LMW_ONE
        {
            c.radius = c.radius / c.decrease_factor;
            c.decrease_factor *= 2.0;
            c.reuse_diagonal = 1;
        }
    }
    return lmw_propose(c, accepted, false, lane_);
}

}  // namespace ll
