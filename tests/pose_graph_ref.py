"""The yardstick of the pose-graph tests: a float64 numpy restatement of the problem ceres_pose_graph_3d.hpp poses and of the
trust-region Levenberg-Marquardt sequence Ceres runs on it with the reference's options -- written from those definitions, not from
the device code.  Dense normal equations, numpy.linalg.cholesky, the Jacobian by complex step through the linearised Plus
( q(d) = (d, 1) (x) q ), vectorised over the edges.

Poses and measurements are rows {qx, qy, qz, qw, tx, ty, tz}; pose 0 is constant.

solve() also records how far every decision of its run was from flipping (`margins`: relative distance of the two sides of every
comparison it made), so a test can require that a case is not decided by rounding, and sensitivity() measures how far the solution
moves when the inputs move by one unit in the last place."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

try:
    from scipy.linalg import solve_triangular
except ImportError:                                            # (the general solver on the triangular factor: slower, as exact)
    def solve_triangular(a, b, lower=False, trans=0):
        return np.linalg.solve(a.T if trans else a, b)

TERMINATION = ("max_iterations", "gradient", "parameter", "function", "radius", "invalid_steps", "nothing")
OPTIONS = dict(max_num_iterations=200, max_num_consecutive_invalid_steps=5, initial_trust_region_radius=1e4, max_trust_region_radius=1e16,
               min_trust_region_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32,
               function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8)


# ---------------------------------------------------------------------------------------------------- quaternions {x, y, z, w}, any dtype
def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def qconj(a):
    return a * np.array([-1.0, -1.0, -1.0, 1.0])


def qrot(q, v):
    """Eigen's quaternion * vector: v + w uv + u x uv, uv = 2 (u x v) -- no normalisation"""
    u, w = q[..., :3], q[..., 3:]
    uv = 2.0 * np.cross(u, v)
    return v + w * uv + np.cross(u, uv)


def qinv(q):
    """Eigen's inverse(): conjugate / squared norm"""
    return qconj(q) / np.sum(q * q, axis=-1, keepdims=True)


def plus(x, d):
    """x [n, 7], d [n, 6] {dp, dtheta}: translation additive, q <- ( sin|d| / |d| d, cos|d| ) (x) q, unchanged where |d| == 0"""
    out = x.copy()
    out[:, 4:7] = x[:, 4:7] + d[:, 0:3]
    n = np.sqrt(np.sum(d[:, 3:6] ** 2, axis=1))
    nz = n > 0.0
    if nz.any():
        dq = np.concatenate([(np.sin(n[nz]) / n[nz])[:, None] * d[nz, 3:6], np.cos(n[nz])[:, None]], axis=1)
        out[nz, 0:4] = qmul(dq, x[nz, 0:4])
    return out


def errors(xa, xb, meas):
    """e = [ conj(q_a) . (p_b - p_a) - p_m ; 2 vec( q_m (x) conj( conj(q_a) (x) q_b ) ) ] per edge, [E, 6]"""
    ca = qconj(xa[:, 0:4])
    q_ab = qmul(ca, xb[:, 0:4])
    p_ab = qrot(ca, xb[:, 4:7] - xa[:, 4:7])
    dq = qmul(meas[:, 0:4], qconj(q_ab))
    return np.concatenate([p_ab - meas[:, 4:7], 2.0 * dq[:, 0:3]], axis=1)


def information_factors(information, n_edges):
    if information is None:
        return None
    info = np.asarray(information, np.float64).reshape(n_edges, 6, 6)
    return np.stack([np.linalg.cholesky(np.tril(m) + np.tril(m, -1).T) for m in info])     # (llt reads the lower triangle)


def residuals(x, ab, meas, L):
    e = errors(x[ab[:, 0]], x[ab[:, 1]], meas)
    return e if L is None else np.einsum("eij,ej->ei", L, e)


def jacobians(x, ab, meas, L, h=1e-30):
    """d residual / d local coordinates of a and of b, [E, 6, 6] each, by complex step along the linearised Plus"""
    xa, xb = x[ab[:, 0]].astype(np.complex128), x[ab[:, 1]].astype(np.complex128)
    Ja, Jb = np.zeros((len(ab), 6, 6)), np.zeros((len(ab), 6, 6))
    for k in range(6):
        for side, J in ((0, Ja), (1, Jb)):
            pa, pb = xa.copy(), xb.copy()
            tgt = pa if side == 0 else pb
            if k < 3:
                tgt[:, 4 + k] += 1j * h
            else:
                unit = np.zeros(4)
                unit[k - 3] = 1.0
                tgt[:, 0:4] += 1j * h * qmul(np.broadcast_to(unit, (len(ab), 4)), tgt[:, 0:4].real)
            J[:, :, k] = errors(pa, pb, meas).imag / h
    if L is not None:
        Ja, Jb = np.einsum("eij,ejk->eik", L, Ja), np.einsum("eij,ejk->eik", L, Jb)
    return Ja, Jb


class _Margins(list):
    def test(self, name, a, b):
        """records the relative distance of a and b; the caller makes the comparison"""
        den = max(abs(a), abs(b))
        self.append((name, abs(a - b) / den if den > 0 and np.isfinite(den) else np.inf))


def solve(poses7, edge_ab, edge_meas7, information=None, options=None):
    """-> (poses [N, 7], summary dict).  summary: iterations, successful_steps, unsuccessful_steps, initial_cost, final_cost,
    termination (a name of TERMINATION), margins [(test, relative distance)], rho [accept ratios]"""
    o = dict(OPTIONS, **(options or {}))
    x = np.array(poses7, np.float64).reshape(-1, 7)
    ab = np.asarray(edge_ab, np.int64).reshape(-1, 2)
    meas = np.asarray(edge_meas7, np.float64).reshape(-1, 7)
    N, E = len(x), len(ab)
    summary = dict(iterations=0, successful_steps=0, unsuccessful_steps=0, initial_cost=0.0, final_cost=0.0, termination="nothing",
                   margins=_Margins(), rho=[])
    if N < 2 or E == 0:
        return x, summary
    L = information_factors(information, E)
    n = 6 * (N - 1)
    in_program = np.zeros(N, bool)
    in_program[ab.ravel()] = True
    in_program[0] = False                                   # the constant pose is not in the reduced program
    cols = lambda pose: 6 * (pose - 1)[:, None] + np.arange(6)[None, :]      # noqa: E731
    free = [ab[:, s] > 0 for s in (0, 1)]

    def linearise(x):
        r = residuals(x, ab, meas, L)
        Ja, Jb = jacobians(x, ab, meas, L)
        g = np.zeros(n)
        for s, J in ((0, Ja), (1, Jb)):
            np.add.at(g, cols(ab[free[s], s]), np.einsum("eij,ei->ej", J[free[s]], r[free[s]]))
        return r, [Ja, Jb], g, 0.5 * float(np.sum(r * r))

    def gradient_max(x, g):
        xp = x.copy()
        xp[1:] = plus(x[1:], -g.reshape(N - 1, 6))
        return float(np.max(np.abs(x[in_program] - xp[in_program]))) if in_program.any() else 0.0

    def x_norm_of(x):
        return float(np.sqrt(np.sum(x[in_program] ** 2)))

    r, J, g, cost = linearise(x)
    col2 = np.zeros(n)
    for s in (0, 1):
        np.add.at(col2, cols(ab[free[s], s]), np.sum(J[s][free[s]] ** 2, axis=1))
    scale = 1.0 / (1.0 + np.sqrt(col2))

    def scaled(J):
        out = []
        for s in (0, 1):
            sc = np.ones((E, 6))
            sc[free[s]] = scale[cols(ab[free[s], s])]
            out.append(J[s] * sc[:, None, :])
        return out

    Js = scaled(J)
    gmax, x_norm = gradient_max(x, g), x_norm_of(x)
    summary.update(initial_cost=cost, final_cost=cost)
    radius, decrease_factor, reuse_diagonal, invalid, iteration = o["initial_trust_region_radius"], 2.0, False, 0, 0
    diag = np.zeros(n)
    m = summary["margins"]
    term = None
    while term is None:
        if iteration >= o["max_num_iterations"]:
            term = "max_iterations"
            break
        m.test("gradient", gmax, o["gradient_tolerance"])
        if gmax <= o["gradient_tolerance"]:
            term = "gradient"
            break
        if radius <= o["min_trust_region_radius"]:
            term = "radius"
            break
        iteration += 1
        A, rhs = np.zeros((n, n)), np.zeros(n)
        for s in (0, 1):
            f = free[s]
            np.add.at(rhs, cols(ab[f, s]), np.einsum("eij,ei->ej", Js[s][f], r[f]))
            c = cols(ab[f, s])
            np.add.at(A, (c[:, :, None], c[:, None, :]), np.einsum("eij,eik->ejk", Js[s][f], Js[s][f]))
        both = free[0] & free[1]
        ca, cb = cols(ab[both, 0]), cols(ab[both, 1])
        cross = np.einsum("eij,eik->ejk", Js[0][both], Js[1][both])
        np.add.at(A, (ca[:, :, None], cb[:, None, :]), cross)
        np.add.at(A, (cb[:, :, None], ca[:, None, :]), np.transpose(cross, (0, 2, 1)))
        if not reuse_diagonal:
            diag = np.clip(np.diag(A).copy(), o["min_lm_diagonal"], o["max_lm_diagonal"])
        reuse_diagonal = True
        ok, model_cost_change = True, 0.0
        try:
            C = np.linalg.cholesky(A + np.diag(diag / radius))
            y = solve_triangular(C, solve_triangular(C, rhs, lower=True), lower=True, trans=1)
            ok = bool(np.all(np.isfinite(y)))
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            step = -y
            padded = np.concatenate([np.zeros(6), step])                    # (the constant pose's coordinates: zeros, its Jacobian is unused)
            mr = sum(np.einsum("eij,ej->ei", Js[s], padded[6 * ab[:, s][:, None] + np.arange(6)[None, :]] * free[s][:, None]) for s in (0, 1))
            model_cost_change = -float(np.sum(mr * (r + mr / 2.0)))
            m.test("model", model_cost_change, 0.0)
        if not ok or not model_cost_change > 0.0:
            invalid += 1
            if invalid >= o["max_num_consecutive_invalid_steps"]:
                term = "invalid_steps"
                break
            radius *= 0.5
            summary["unsuccessful_steps"] += 1
            continue
        invalid = 0
        cand = x.copy()
        cand[1:] = plus(x[1:], (step * scale).reshape(N - 1, 6))
        cand_cost = 0.5 * float(np.sum(residuals(cand, ab, meas, L) ** 2))
        if not np.isfinite(cand_cost):
            cand_cost = np.finfo(np.float64).max
        step_norm = float(np.sqrt(np.sum((x[in_program] - cand[in_program]) ** 2)))
        bound = o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"])
        m.test("parameter", step_norm, bound)
        if step_norm <= bound:
            term = "parameter"
            break
        cost_change = cost - cand_cost
        m.test("function", abs(cost_change), o["function_tolerance"] * cost)
        if abs(cost_change) <= o["function_tolerance"] * cost:
            term = "function"
            break
        rho = cost_change / model_cost_change
        summary["rho"].append(rho)
        m.test("accept", rho, o["min_relative_decrease"])
        if rho > o["min_relative_decrease"]:
            x = cand
            r, J, g, cost = linearise(x)
            Js = scaled(J)
            gmax, x_norm = gradient_max(x, g), x_norm_of(x)
            summary["final_cost"] = min(summary["final_cost"], cost)
            t = 2.0 * rho - 1.0
            radius = min(o["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - t * t * t))
            decrease_factor, reuse_diagonal = 2.0, False
            summary["successful_steps"] += 1
        else:
            radius /= decrease_factor
            decrease_factor *= 2.0
            summary["unsuccessful_steps"] += 1
    summary.update(iterations=iteration, termination=term)
    return x, summary


def pose_distance(a, b):
    """(largest translation difference [m], largest rotation difference [rad]) of two pose arrays"""
    a, b = np.asarray(a).reshape(-1, 7), np.asarray(b).reshape(-1, 7)
    dt = float(np.max(np.linalg.norm(a[:, 4:7] - b[:, 4:7], axis=1))) if len(a) else 0.0
    rel = qmul(qconj(a[:, 0:4]), b[:, 0:4]) / (np.linalg.norm(a[:, 0:4], axis=1) * np.linalg.norm(b[:, 0:4], axis=1))[:, None]
    dr = float(np.max(2.0 * np.arctan2(np.linalg.norm(rel[:, 0:3], axis=1), np.abs(rel[:, 3])))) if len(a) else 0.0
    return dt, dr


def sensitivity(poses7, edge_ab, edge_meas7, information=None, trials=8, seed=0, base=None, options=None, rows=None):
    """the largest pose change (m, rad) of solve()'s result when every input moves by one unit in the last place, up or down at
    random, over `trials` draws; rows: the poses the change is measured on (all of them when None)"""
    rng = np.random.default_rng(seed)
    base = solve(poses7, edge_ab, edge_meas7, information, options)[0] if base is None else base
    worst = (0.0, 0.0)

    def nudge(a):
        a = np.asarray(a, np.float64)
        return np.nextafter(a, np.where(rng.integers(0, 2, a.shape) == 1, np.inf, -np.inf))

    draws = [(nudge(poses7), nudge(edge_meas7), None if information is None else nudge(information)) for _ in range(trials)]
    with ThreadPoolExecutor(max_workers=trials) as pool:       # (the draws are made above, in sequence: the result does not depend on the threads)
        results = list(pool.map(lambda d: solve(d[0], edge_ab, d[1], d[2], options)[0], draws))
    for got in results:
        d = pose_distance(base, got) if rows is None else pose_distance(base[rows], got[rows])
        worst = (max(worst[0], d[0]), max(worst[1], d[1]))
    return worst
