"""Seeded pose graphs for the pose-graph tests, shaped like what the loop detector hands over: a closed loop of 20 m across with gentle
roll and pitch; the estimates drift; chain edges are built from the DRIFTED estimates (as the detector builds them from its key-frame
poses), so they are satisfied exactly at the start; loop edges come from the true relative pose plus a little noise.

consistent=True builds every edge from the truth without noise (the drifted estimates are only the start): the optimum is the truth,
which is what ground-truth recovery is asserted on.  hard=True perturbs the start by up to 3 m / 1.5 rad."""
import functools

import numpy as np

from tests import pose_graph_ref as ref


def quat_from_euler(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=-1)


def small_rotation(v):
    """unit quaternions of the rotation vectors v [n, 3]"""
    a = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.concatenate([np.sin(a / 2) * v / np.where(a > 0, a, 1.0), np.cos(a / 2)], axis=-1)


def relative(xa, xb):
    """the measurement an edge a -> b carries when the poses are xa, xb: { inv(q_a) q_b, inv(q_a) (p_b - p_a) }"""
    qi = ref.qinv(xa[..., 0:4])
    return np.concatenate([ref.qmul(qi, xb[..., 0:4]), ref.qrot(qi, xb[..., 4:7] - xa[..., 4:7])], axis=-1)


def compose(x, rel):
    """x (+) rel: the pose whose measurement from x is rel"""
    return np.concatenate([ref.qmul(x[..., 0:4], rel[..., 0:4]), x[..., 4:7] + ref.qrot(x[..., 0:4], rel[..., 4:7])], axis=-1)


def truth_trajectory(n):
    th = 2.0 * np.pi * np.arange(n) / n
    p = np.stack([10.0 * np.cos(th) - 10.0, 10.0 * np.sin(th), 0.3 * np.sin(2 * th)], axis=1)
    q = quat_from_euler(0.05 * np.sin(3 * th), 0.04 * np.cos(2 * th), th + np.pi / 2)
    return np.concatenate([q, p], axis=1)


def make_graph(n, loops, seed, consistent=False, hard=False, information=False, offset=None, reverse_chain_every=0):
    """-> dict(poses [n, 7] start, ab [E, 2] int32, meas [E, 7], information [E, 36] or None, truth [n, 7])
    loops: [(a, b)] edges a -> b besides the chain k -> k + 1; reverse_chain_every: every such chain edge runs k + 1 -> k."""
    rng = np.random.default_rng(seed)
    truth = truth_trajectory(n)
    if offset is not None:
        truth[:, 4:7] += np.asarray(offset, np.float64)
    est = truth.copy()
    for k in range(1, n):
        rel = relative(truth[k - 1], truth[k])
        rel[0:4] = ref.qmul(rel[0:4], small_rotation(rng.normal(0, 0.004, 3)[None])[0])
        rel[4:7] += rng.normal(0, 0.02, 3)
        est[k] = compose(est[k - 1], rel)
    src = truth if consistent else est
    ab, meas = [], []
    for k in range(n - 1):
        a, b = (k + 1, k) if reverse_chain_every and k % reverse_chain_every == reverse_chain_every - 1 else (k, k + 1)
        ab.append((a, b))
        meas.append(relative(src[a], src[b]))
    for a, b in loops:
        m = relative(truth[a], truth[b])
        if not consistent:
            m[0:4] = ref.qmul(m[0:4], small_rotation(rng.normal(0, 1e-3, 3)[None])[0])
            m[4:7] += rng.normal(0, 2e-3, 3)
        ab.append((a, b))
        meas.append(m)
    start = est.copy()
    if hard:
        start[1:, 4:7] += rng.uniform(-1.0, 1.0, (n - 1, 3)) * (3.0 / np.sqrt(3.0))
        start[1:, 0:4] = ref.qmul(start[1:, 0:4], small_rotation(rng.uniform(-1.0, 1.0, (n - 1, 3)) * (1.5 / np.sqrt(3.0))))
    info = None
    if information:
        info = np.tile(np.eye(6).ravel(), (len(ab), 1))
        for e in range(0, len(ab), 3):
            m = rng.normal(0, 1, (6, 6))
            info[e] = (m @ m.T + 6.0 * np.eye(6)).ravel() * rng.uniform(0.5, 4.0)
    return dict(poses=start, ab=np.array(ab, np.int32).reshape(-1, 2), meas=np.array(meas, np.float64).reshape(-1, 7), information=info, truth=truth)


# name -> make_graph arguments.  The seeds were chosen on the CPU with pose_graph_ref.solve (tests/test_pose_graph_host.py checks the
# conditions again): every accept ratio and tolerance test of the reference's run stays at least 1e-6 (relative) from its threshold.
CASES = {
    "n2": dict(n=2, loops=[], seed=1, hard=True),
    "n3_loop_to_fixed": dict(n=3, loops=[(2, 0)], seed=2),
    "n17_three_loops": dict(n=17, loops=[(16, 3), (12, 8), (14, 0)], seed=3),
    "n17_far": dict(n=17, loops=[(16, 3), (12, 8), (14, 0)], seed=3, offset=(50e3, -50e3, 50e3)),
    "n33_detector": dict(n=33, loops=[(32, 1)], seed=4),
    "n66": dict(n=66, loops=[(65, 2), (40, 5)], seed=5),
    "n300_six_loops": dict(n=300, loops=[(299, 0), (298, 3), (250, 20), (200, 100), (150, 49), (290, 10)], seed=6),
    "n40_hard": dict(n=40, loops=[(39, 0), (30, 5)], seed=7, hard=True),
    "n66_hard_rejected_steps": dict(n=66, loops=[(65, 2), (40, 5)], seed=24, hard=True),     # two rejected steps
    "n24_information": dict(n=24, loops=[(23, 1), (20, 4)], seed=8, information=True),
    "n20_both_directions": dict(n=20, loops=[(19, 0), (2, 15)], seed=9, reverse_chain_every=3),
    "n17_consistent": dict(n=17, loops=[(16, 3), (12, 8), (14, 0)], seed=10, consistent=True),
    "n30_consistent": dict(n=30, loops=[(29, 0), (20, 3)], seed=11, consistent=True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return make_graph(**CASES[name])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(poses, summary) of pose_graph_ref.solve on the case -- computed once per process, shared, never changed"""
    g = case(name)
    return ref.solve(g["poses"], g["ab"], g["meas"], g["information"])


@functools.lru_cache(maxsize=None)
def reference_sensitivity(name):
    g = case(name)
    return ref.sensitivity(g["poses"], g["ab"], g["meas"], g["information"], base=reference(name)[0])


def tolerance(name):
    """device - reference <= max( 1000 s, 1e-11 ), s the reference's own sensitivity on the case: (metres, radians)"""
    s = reference_sensitivity(name)
    return max(1000.0 * s[0], 1e-11), max(1000.0 * s[1], 1e-11)
