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


def inverse_measurement(m):
    """the measurement of the edge b -> a when a -> b carries m"""
    qi = ref.qinv(m[0:4])
    return np.concatenate([qi, -ref.qrot(qi, m[4:7])])


FAR_POSE = np.array([0.0, 0.0, 0.0, 1.0, 1e6, -1e6, 5e5])


def edgeless_pose(g, at):
    """FAR_POSE inserted at index `at` with no edge; the ids from `at` on move up by one"""
    ab = g["ab"].copy()
    ab[ab >= at] += 1
    return dict(g, poses=np.insert(g["poses"], at, FAR_POSE, axis=0), truth=np.insert(g["truth"], at, FAR_POSE, axis=0), ab=ab)


def floating_component(g):
    """without chain edge 11 and without the loop edges: the poses from 12 on are a component that never touches pose 0"""
    keep = np.array([e for e in range(len(g["poses"]) - 1) if e != 11])
    return dict(g, ab=g["ab"][keep], meas=g["meas"][keep])


def floating_component_loops(g):
    """without chain edge 11 alone; the graph's loop edges must each stay on one side of it"""
    assert all((a > 11) == (b > 11) for a, b in g["ab"][len(g["poses"]) - 1:])
    keep = np.array([e for e in range(len(g["ab"])) if e != 11])
    return dict(g, ab=g["ab"][keep], meas=g["meas"][keep])


def repeated_edges(g):
    """edge 5 twice more, the first loop edge once more, chain edge 7 once more reversed with the inverse measurement"""
    loop = len(g["poses"]) - 1
    ab = np.concatenate([g["ab"], g["ab"][[5, 5, loop]], g["ab"][7:8, ::-1]])
    return dict(g, ab=ab, meas=np.concatenate([g["meas"], g["meas"][[5, 5, loop]], inverse_measurement(g["meas"][7])[None]]))


def information_all(g, seed=1):
    """on every edge Q diag(10^u) Q', u uniform in [-3, 3], Q from the QR of a normal draw"""
    rng = np.random.default_rng(seed)
    info = np.zeros((len(g["ab"]), 36))
    for e in range(len(info)):
        q, _ = np.linalg.qr(rng.normal(0, 1, (6, 6)))
        m = (q * 10.0 ** rng.uniform(-3.0, 3.0, 6)) @ q.T
        info[e] = (0.5 * (m + m.T)).ravel()
    return dict(g, information=info)


def non_unit(g, seed=2):
    """every pose quaternion and every measurement quaternion scaled by a factor in [0.5, 2]"""
    rng = np.random.default_rng(seed)
    poses, meas = g["poses"].copy(), g["meas"].copy()
    poses[:, 0:4] *= rng.uniform(0.5, 2.0, (len(poses), 1))
    meas[:, 0:4] *= rng.uniform(0.5, 2.0, (len(meas), 1))
    return dict(g, poses=poses, meas=meas)


def overflow(g):
    """one coordinate at 1e160: every input is finite, its square is not"""
    poses = g["poses"].copy()
    poses[5, 4] = 1e160
    return dict(g, poses=poses)


def cost_overflow(g, seed=3):
    """every measurement some 100 m off and the information 5e303 I on every edge: the cost is past the largest double while the
    Jacobian's column sums are not, so steps are valid and the cost of a candidate is what overflows"""
    rng = np.random.default_rng(seed)
    meas = g["meas"].copy()
    meas[:, 4:7] += rng.normal(0.0, 100.0, (len(meas), 3))
    return dict(g, meas=meas, information=np.tile((5e303 * np.eye(6)).ravel(), (len(meas), 1)))


EDITS = dict(edgeless_last=lambda g: edgeless_pose(g, len(g["poses"])), edgeless_middle=lambda g: edgeless_pose(g, 10),
             floating_component=floating_component, floating_component_loops=floating_component_loops,
             repeated_edges=repeated_edges, information_all=information_all, non_unit=non_unit,
             overflow=overflow, cost_overflow=cost_overflow)
B24 = dict(n=24, loops=[(23, 1), (20, 4)], seed=41)

# name -> make_graph arguments, and under "edit" the name of the change in EDITS made to that graph afterwards.  The seeds were chosen
# on the CPU with pose_graph_ref.solve (tests/test_pose_graph_host.py checks the conditions again): every accept ratio and tolerance
# test of the reference's run stays at least 1e-6 (relative) from its threshold.
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
    # 6 (N - 1) doubles of the triangular solves' vector: 2046 at N = 342, the last graph that keeps it in LDS; 2052 at N = 343
    "n342_lds_top": dict(n=342, loops=[(341, 1), (300, 40)], seed=31),
    "n343_hbm_first": dict(n=343, loops=[(342, 1), (300, 40)], seed=32),
    "n343_hbm_other": dict(n=343, loops=[(342, 0), (170, 60), (320, 200)], seed=33),
    "b24_edgeless_last": dict(B24, edit="edgeless_last"),
    "b24_edgeless_middle": dict(B24, edit="edgeless_middle"),
    # (its chain edges hold exactly at the start, so the run ends on the gradient before a step; the second has a loop inside either part)
    "b24_floating_component": dict(B24, edit="floating_component"),
    "b24_floating_component_loops": dict(n=24, loops=[(23, 13), (10, 1)], seed=41, edit="floating_component_loops"),
    "b24_repeated_edges": dict(B24, edit="repeated_edges"),
    "b24_information_all": dict(B24, edit="information_all"),
    "b24_non_unit": dict(B24, edit="non_unit"),
    "b24_overflow": dict(B24, edit="overflow"),
    "b24_cost_overflow": dict(B24, edit="cost_overflow"),
}
NEW_CASES = [n for n in CASES if n.startswith(("n342", "n343", "b24_"))]
UNCHANGED = ("b24_overflow", "n66_hard_max_iterations_0", "n66_hard_min_radius_1e4")     # no step is taken: the poses come back as they went in

# name -> (case, options of pose_graph_ref.OPTIONS that differ from the defaults)
OPTION_CASES = {
    "n66_hard_max_iterations_0": ("n66_hard_rejected_steps", dict(max_num_iterations=0)),
    "n66_hard_max_iterations_1": ("n66_hard_rejected_steps", dict(max_num_iterations=1)),
    "n66_hard_max_iterations_3": ("n66_hard_rejected_steps", dict(max_num_iterations=3)),
    "n66_hard_min_radius_1e4": ("n66_hard_rejected_steps", dict(min_trust_region_radius=1e4)),
    "n66_hard_min_radius_6e3": ("n66_hard_rejected_steps", dict(min_trust_region_radius=6e3)),
    "n66_hard_min_radius_3e3": ("n66_hard_rejected_steps", dict(min_trust_region_radius=3e3)),
    "n66_hard_max_radius_1e4": ("n66_hard_rejected_steps", dict(max_trust_region_radius=1e4)),
    "n66_hard_first_radius_1e-3": ("n66_hard_rejected_steps", dict(initial_trust_region_radius=1e-3)),
    "n66_hard_min_decrease_0.9": ("n66_hard_rejected_steps", dict(min_relative_decrease=0.9)),
    "b24_overflow_two_invalid": ("b24_overflow", dict(max_num_consecutive_invalid_steps=2)),
}
UNCHANGED += ("b24_overflow_two_invalid", "b24_cost_overflow")


def resolve(name):
    """(case, options) of a name of CASES or of OPTION_CASES"""
    return OPTION_CASES[name] if name in OPTION_CASES else (name, None)


@functools.lru_cache(maxsize=None)
def case(name):
    name = resolve(name)[0]
    spec = dict(CASES[name])
    edit = spec.pop("edit", None)
    g = make_graph(**spec)
    return EDITS[edit](g) if edit else g


@functools.lru_cache(maxsize=None)
def reference(name):
    """(poses, summary) of pose_graph_ref.solve on the case -- computed once per process, shared, never changed"""
    g = case(name)
    # (a graph that overflows does so in every product of the reference: numpy's warnings are silenced for this call alone)
    with np.errstate(**(dict(over="ignore", invalid="ignore") if resolve(name)[0] in ("b24_overflow", "b24_cost_overflow") else {})):
        return ref.solve(g["poses"], g["ab"], g["meas"], g["information"], options=resolve(name)[1])


@functools.lru_cache(maxsize=None)
def reference_sensitivity(name):
    """measured on the poses that have edges: a pose without any comes back as it went in, and is asserted to"""
    g = case(name)
    rows = np.unique(np.concatenate([[0], np.asarray(g["ab"]).ravel()]))
    return ref.sensitivity(g["poses"], g["ab"], g["meas"], g["information"], base=reference(name)[0], options=resolve(name)[1],
                           rows=None if len(rows) == len(g["poses"]) else rows)


def tolerance(name):
    """device - reference <= max( 1000 s, 1e-11 ), s the reference's own sensitivity on the case: (metres, radians)"""
    s = reference_sensitivity(name)
    return max(1000.0 * s[0], 1e-11), max(1000.0 * s[1], 1e-11)
