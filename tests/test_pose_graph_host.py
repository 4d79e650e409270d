"""CPU tier of the pose-graph optimiser (tests/test_gpu_pose_graph.py is the GPU tier).

Arithmetic: loam_livox_amd/csrc/ll_pose_graph_core.h -- the text pg_solve_kernel runs -- and the call plan of ll_pose_graph.h, compiled
with g++ -ffp-contract=off (tests/pose_graph_host.cpp), against tests/pose_graph_ref.py on the cases of tests/pose_graph_inputs.py,
with the tolerance of the GPU tier: device - reference <= max( 1000 s, 1e-11 ), s the reference's own sensitivity on the case, and
< 1e-7 in every case; equal iteration and step counts and termination.  The analytic Jacobian against the complex step; the envelope
factorisation against the dense solution; the driver once more under the address and undefined-behaviour sanitizers.
Cases: every accept ratio and tolerance test of the reference's run stays 1e-6 (relative) from its threshold; the set holds rejected
steps, each of the three tolerance terminations and the exits on the iteration cap, the radius floor and a run of invalid steps; the
consistent graphs recover the truth.  The new cases stand where the kernel's text changes form: 6 (N - 1) on either side of
LL_PG_LDS_VEC (read from the header here), poses without edges, a component that never touches pose 0, repeated and reversed edges,
information of a wide spectrum on every edge, quaternions far from unit norm, a graph whose normal matrix overflows, and parameters
other than the defaults (tests/pose_graph_inputs.OPTION_CASES), which the driver takes in a block of its input.
Symbols: declared, exported, bound; bad arguments are refused without a device.
Bookkeeping: Keyframe_assembly( pose_graph=stub ) on the scripted walks of tests/test_keyframes.py leaves loops, log, if_end and
state() as pose_graph=False has them, and hands the stub the constraints of the numpy formulas bit for bit; Laser_mapping_batch's
round over stub handles makes one solve for all slots that looped."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from loam_livox_amd import capi
from tests import pose_graph_inputs as pgi
from tests import pose_graph_ref as ref
from tests.pose_graph_driver import build_driver, run_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    text = open(os.path.join(ROOT, "loam_livox_amd", "csrc", "ll_pose_graph_core.h")).read()
    found = re.findall(r"^#define\s+" + name + r"\s+(\d+)\b", text, flags=re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


LDS_VEC, THREADS = header_constant("LL_PG_LDS_VEC"), header_constant("LL_PG_THREADS")
# (the N = 300 case is run by the GPU tier; here its plan and one linearisation are checked, not its eight-fold sensitivity)
SOLVED = ["n2", "n3_loop_to_fixed", "n17_three_loops", "n17_far", "n33_detector", "n66", "n40_hard", "n66_hard_rejected_steps", "n24_information",
          "n20_both_directions", "n17_consistent", "n30_consistent"]
NEW_CASES = list(pgi.NEW_CASES)
OPTION_CASES = list(pgi.OPTION_CASES)


def graph_of(name):
    g = pgi.case(name)
    return dict(poses=g["poses"], ab=g["ab"], meas=g["meas"], information=g["information"])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("pose_graph") / "pose_graph_host"))


@pytest.fixture(scope="module")
def solved(driver, tmp_path_factory):
    """the driver's result of every case, all in ONE call (a batch), computed once and shared"""
    tmp = str(tmp_path_factory.mktemp("pose_graph_run"))
    poses, summaries = run_driver(driver, tmp, [graph_of(n) for n in SOLVED + NEW_CASES])
    out = dict(zip(SOLVED + NEW_CASES, zip(poses, summaries)))
    for name, (_, options) in pgi.OPTION_CASES.items():             # one call per row of parameters
        (x,), (s,) = run_driver(driver, tmp, [graph_of(name)], options=options)
        out[name] = (x, s)
    return out


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", SOLVED + ["n300_six_loops"] + NEW_CASES + OPTION_CASES)
def test_no_decision_of_the_reference_run_is_near_its_threshold(name):
    _, s = pgi.reference(name)
    worst = {}
    for test, margin in s["margins"]:
        worst[test] = min(worst.get(test, np.inf), margin)
    print(name, s["iterations"], s["successful_steps"], s["unsuccessful_steps"], s["termination"], {k: f"{v:.2e}" for k, v in worst.items()})
    assert min(worst.values(), default=np.inf) >= 1e-6, (name, worst)      # (no iteration: no decision was made)


def test_the_set_holds_rejected_steps_and_the_three_terminations():
    runs = {n: pgi.reference(n)[1] for n in SOLVED + NEW_CASES + OPTION_CASES}
    assert runs["n66_hard_rejected_steps"]["unsuccessful_steps"] > 0
    assert {"function", "gradient", "parameter"} <= {runs[n]["termination"] for n in SOLVED}
    assert {"max_iterations", "radius", "invalid_steps"} <= {s["termination"] for s in runs.values()}
    over = runs["b24_overflow"]
    assert over["termination"] == "invalid_steps" and over["successful_steps"] == 0
    assert (over["iterations"], over["unsuccessful_steps"]) == (5, 4)       # four halvings, the fifth invalid step ends the solve
    two = runs["b24_overflow_two_invalid"]                           # one halving, then the run of two ends the solve
    assert (two["iterations"], two["successful_steps"], two["unsuccessful_steps"], two["termination"]) == (2, 0, 1, "invalid_steps")
    for name, want in (("n66_hard_max_iterations_0", (0, 0, 0, "max_iterations")), ("n66_hard_max_iterations_1", (1, 0, 1, "max_iterations")),
                       ("n66_hard_max_iterations_3", (3, 1, 2, "max_iterations")), ("n66_hard_min_radius_1e4", (0, 0, 0, "radius")),
                       ("n66_hard_min_radius_6e3", (1, 0, 1, "radius")), ("n66_hard_min_radius_3e3", (2, 0, 2, "radius"))):
        r = runs[name]
        assert (r["iterations"], r["successful_steps"], r["unsuccessful_steps"], r["termination"]) == want, name
    # the cap on the radius, the small first radius and the raised acceptance bar each change the run they are given to
    base = runs["n66_hard_rejected_steps"]
    for name in ("n66_hard_max_radius_1e4", "n66_hard_first_radius_1e-3", "n66_hard_min_decrease_0.9"):
        assert runs[name]["termination"] == "function" and runs[name]["iterations"] != base["iterations"], name
    assert runs["n66_hard_min_decrease_0.9"]["unsuccessful_steps"] > base["unsuccessful_steps"]
    for name in pgi.UNCHANGED:
        assert pgi.reference(name)[0].tobytes() == np.ascontiguousarray(pgi.case(name)["poses"]).tobytes(), name
    # what the new graphs are there for
    assert 6 * (len(pgi.case("n342_lds_top")["poses"]) - 1) <= LDS_VEC < 6 * (len(pgi.case("n343_hbm_first")["poses"]) - 1)
    assert len(pgi.case("n343_hbm_other")["poses"]) == 343 and not np.array_equal(pgi.case("n343_hbm_other")["ab"], pgi.case("n343_hbm_first")["ab"])
    for name, at in (("b24_edgeless_last", 24), ("b24_edgeless_middle", 10)):
        g = pgi.case(name)
        assert len(g["poses"]) == 25 and not (g["ab"] == at).any() and np.array_equal(g["poses"][at], pgi.FAR_POSE)
        assert pgi.reference(name)[0][at].tobytes() == pgi.FAR_POSE.tobytes()
        assert runs[name]["termination"] == "function" and runs[name]["iterations"] == runs["b24_edgeless_last"]["iterations"] > 1
    for name in ("b24_floating_component", "b24_floating_component_loops"):
        ab = pgi.case(name)["ab"]
        assert not ((ab.min(axis=1) <= 11) & (ab.max(axis=1) >= 12)).any() and (ab.min(axis=1) >= 12).any(), name
    assert runs["b24_floating_component_loops"]["successful_steps"] > 1
    g = pgi.case("b24_repeated_edges")
    pairs = [tuple(e) for e in g["ab"]]
    assert pairs.count((5, 6)) == 3 and pairs.count((23, 1)) == 2 and pairs.count((7, 8)) == 1 and pairs.count((8, 7)) == 1
    assert np.abs(ref.residuals(g["poses"], g["ab"].astype(np.int64)[-1:], g["meas"][-1:], None)).max() < 1e-9     # the inverse measurement
    info = pgi.case("b24_information_all")["information"].reshape(-1, 6, 6)
    eig = np.linalg.eigvalsh(info)
    assert (eig > 0).all() and (eig[:, -1] / eig[:, 0]).min() > 10.0 and eig.max() / eig.min() > 1e5
    assert not any(np.array_equal(m, np.eye(6)) for m in info)
    g = pgi.case("b24_non_unit")
    for q in (g["poses"][:, :4], g["meas"][:, :4]):
        n = np.linalg.norm(q, axis=1)
        assert n.min() < 0.7 and n.max() > 1.5 and 0.5 <= n.min() and n.max() <= 2.0
    assert np.isfinite(pgi.case("b24_overflow")["poses"]).all()
    over = runs["b24_cost_overflow"]                                 # a valid step whose candidate's cost is not finite
    assert (over["iterations"], over["successful_steps"], over["unsuccessful_steps"], over["termination"]) == (1, 0, 0, "function")
    assert np.isinf(over["initial_cost"]) and any(t == "model" for t, _ in over["margins"])
    g = pgi.case("b24_cost_overflow")
    assert np.isfinite(g["meas"]).all() and np.isfinite(g["information"]).all()
    assert {runs[n]["termination"] for n in ("n17_consistent", "n30_consistent", "n2")} >= {"gradient", "parameter"}
    assert len(pgi.case("n66")["ab"]) > 64 and len(pgi.case("n300_six_loops")["ab"]) > 256
    ab = pgi.case("n20_both_directions")["ab"]
    assert (ab[:, 0] > ab[:, 1]).any() and (ab[:, 0] < ab[:, 1]).any()
    for name in SOLVED + NEW_CASES[:3]:                              # chain edges from the estimates: satisfied at the start
        g = pgi.case(name)
        if not pgi.CASES[name].get("consistent") and not pgi.CASES[name].get("hard"):
            chain = np.arange(len(g["poses"]) - 1)
            r = ref.residuals(g["poses"], g["ab"].astype(np.int64)[chain], g["meas"][chain], None)
            assert np.abs(r).max() < 1e-9 * max(1.0, np.abs(g["poses"][:, 4:7]).max()), name


# ------------------------------------------------------------------------------------------------ the kernel's text under g++
def test_the_header_puts_the_new_graphs_on_either_side_of_the_lds_vector():
    """6 (N - 1) doubles: N = 342 is the last graph whose vector fits, N = 343 the first that does not"""
    assert 6 * 341 <= LDS_VEC < 6 * 342
    assert THREADS == 256                                            # more than 64 and more than 256 edges are what the old cases were sized for
    assert len(pgi.case("n66")["ab"]) > 64 and len(pgi.case("n300_six_loops")["ab"]) > THREADS


@pytest.mark.parametrize("name", SOLVED + NEW_CASES + OPTION_CASES)
def test_driver_equals_the_reference(solved, name):
    want, ws = pgi.reference(name)
    got, s = solved[name]
    assert (s["iterations"], s["successful_steps"], s["unsuccessful_steps"], ref.TERMINATION[s["termination"]]) == \
        (ws["iterations"], ws["successful_steps"], ws["unsuccessful_steps"], ws["termination"])
    if name in pgi.UNCHANGED:                                        # no step is taken: nothing to be sensitive about, the bytes of the input
        start = np.ascontiguousarray(pgi.case(name)["poses"])
        print(f"{name}: {s}; reference cost {ws['initial_cost']!r} -> {ws['final_cost']!r}")
        assert got.tobytes() == start.tobytes() == want.tobytes()
        for k in ("initial_cost", "final_cost"):
            assert s[k] == ws[k] if np.isinf(ws[k]) else abs(s[k] - ws[k]) <= 1e-12 * ws[k], (name, k, s[k], ws[k])
        assert s["initial_cost"] == s["final_cost"]
        return
    tol_m, tol_rad = pgi.tolerance(name)
    d_m, d_rad = ref.pose_distance(want, got)
    print(f"{name}: driver - reference {d_m:.3e} m {d_rad:.3e} rad (allowed {tol_m:.3e} m {tol_rad:.3e} rad); {s}")
    assert d_m <= tol_m and d_rad <= tol_rad and d_m < 1e-7 and d_rad < 1e-7
    assert np.array_equal(got[0], pgi.case(name)["poses"][0])
    for at in {"b24_edgeless_last": [24], "b24_edgeless_middle": [10]}.get(name, []):
        assert got[at].tobytes() == pgi.FAR_POSE.tobytes()          # a pose without edges comes back as it went in


def test_envelope_blocks_of_the_python_side_are_the_plans(driver, tmp_path):
    """api.Pose_graph sizes its handle by Pose_graph.envelope_blocks; ll_pose_graph_solve refuses by pg_plan's count"""
    from loam_livox_amd.api import Pose_graph
    names = list(pgi.CASES)
    per_graph, total = run_driver(driver, str(tmp_path), [graph_of(n) for n in names], mode=2)
    want = [Pose_graph.envelope_blocks(len(pgi.case(n)["poses"]), pgi.case(n)["ab"]) for n in names]
    print(dict(zip(names, per_graph)))
    assert per_graph == want and total == sum(want)
    assert Pose_graph.envelope_blocks(1, np.zeros((0, 2))) == 0 and Pose_graph.envelope_blocks(5, np.zeros((0, 2))) == 4
    assert run_driver(driver, str(tmp_path), [dict(poses=pgi.case("n2")["poses"][:1], ab=np.zeros((0, 2), np.int32), meas=np.zeros((0, 7)))], mode=2) == ([0], 0)


@pytest.mark.parametrize("name", ["n17_consistent", "n30_consistent"])
def test_consistent_graphs_recover_the_truth(solved, name):
    truth = pgi.case(name)["truth"]
    assert max(ref.pose_distance(pgi.reference(name)[0], truth)) < 1e-4      # the reference itself recovers
    assert max(ref.pose_distance(solved[name][0], truth)) < 1e-4


def test_a_graphs_result_does_not_depend_on_the_batch(driver, solved, tmp_path):
    (alone,), (s,) = run_driver(driver, str(tmp_path), [graph_of("n17_three_loops")])
    assert alone.tobytes() == solved["n17_three_loops"][0].tobytes() and s == solved["n17_three_loops"][1]
    empty = dict(poses=pgi.case("n2")["poses"], ab=np.zeros((0, 2), np.int32), meas=np.zeros((0, 7)))
    one = dict(poses=pgi.case("n2")["poses"][:1], ab=np.zeros((0, 2), np.int32), meas=np.zeros((0, 7)))
    poses, summaries = run_driver(driver, str(tmp_path), [empty, graph_of("n24_information"), one, graph_of("n17_three_loops")])
    assert poses[3].tobytes() == alone.tobytes() and summaries[3] == s
    assert poses[1].tobytes() == solved["n24_information"][0].tobytes()
    for k, g in ((0, empty), (2, one)):
        assert np.array_equal(poses[k], g["poses"]) and ref.TERMINATION[summaries[k]["termination"]] == "nothing" and summaries[k]["iterations"] == 0


@pytest.mark.parametrize("name", ["n17_three_loops", "n24_information", "n20_both_directions", "n66_hard_rejected_steps", "n300_six_loops"])
def test_analytic_jacobian_and_envelope_solve(driver, tmp_path, name):
    g = pgi.case(name)
    lin = run_driver(driver, str(tmp_path), [graph_of(name)], mode=1)
    L = ref.information_factors(g["information"], len(g["ab"]))
    Ja, Jb = ref.jacobians(g["poses"], g["ab"].astype(np.int64), g["meas"], L)
    want = np.stack([Ja, Jb], axis=1)
    err = np.abs(lin["J"] - want).max()
    print(f"{name}: analytic - complex step {err:.3e}, max |J| {np.abs(want).max():.3e}")
    assert err <= 1e-10 * (1.0 + np.abs(want).max())
    # the envelope factor's solution is the dense factor's: A is the damped normal matrix expanded from the strips
    A, rhs, y = lin["A"], lin["rhs"], lin["y"]
    assert lin["ok"] and np.array_equal(A, A.T)
    Cf = np.linalg.cholesky(A)
    dense = ref.solve_triangular(Cf, ref.solve_triangular(Cf, rhs, lower=True), lower=True, trans=1)
    # both solve the same system backward-stably: they agree to cond(A) * eps; measured against that bound
    bound = 100.0 * np.linalg.cond(A) * np.finfo(np.float64).eps * np.abs(dense).max()
    print(f"{name}: envelope - dense {np.abs(y - dense).max():.3e} (bound {bound:.3e}), residual {np.abs(A @ y - rhs).max():.3e}")
    assert np.abs(y - dense).max() <= bound
    # zeros outside the envelope: an entry joins two poses only if the envelope row of the higher reaches the lower
    n = len(g["poses"]) - 1
    first = np.arange(n)
    for a, b in g["ab"]:
        if min(a, b) >= 1:
            first[max(a, b) - 1] = min(first[max(a, b) - 1], min(a, b) - 1)
    for f in range(n):
        assert not A[6 * f:6 * f + 6, :6 * first[f]].any()


def test_driver_runs_clean_under_the_sanitizers(tmp_path, solved):
    exe = build_driver(str(tmp_path / "pose_graph_host_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    names = ["n17_three_loops", "n24_information", "n66_hard_rejected_steps", "n2"] + NEW_CASES      # (the N = 343 graphs after others: pose0 != 0)
    empty = dict(poses=pgi.case("n2")["poses"], ab=np.zeros((0, 2), np.int32), meas=np.zeros((0, 7)))
    poses, summaries = run_driver(exe, str(tmp_path), [graph_of(n) for n in names] + [empty])     # (asserts exit status 0 and an empty stderr)
    for n, x, s in zip(names, poses, summaries):
        assert x.tobytes() == solved[n][0].tobytes() and s == solved[n][1]
    run_driver(exe, str(tmp_path), [graph_of("n20_both_directions")], mode=1)


def test_the_plan_refuses_bad_calls(driver, tmp_path):
    g = graph_of("n17_three_loops")
    bad = dict(g, ab=g["ab"].copy())
    bad["ab"][4] = (3, 3)
    assert "joins a pose to itself" in run_driver(driver, str(tmp_path), [bad], expect_refusal=True)
    bad["ab"][4] = (3, 17)
    assert "out of range" in run_driver(driver, str(tmp_path), [bad], expect_refusal=True)
    bad = dict(g, poses=g["poses"].copy())
    bad["poses"][2, 1] = np.inf
    assert "not finite" in run_driver(driver, str(tmp_path), [bad], expect_refusal=True)
    info = np.tile(np.eye(6).ravel(), (len(g["ab"]), 1))
    info[3, 0] = 0.0
    assert "not positive definite" in run_driver(driver, str(tmp_path), [dict(g, information=info)], expect_refusal=True)


# ------------------------------------------------------------------------------------------------ entry points without a device
NEW = {"ll_pose_graph_default_params": 1, "ll_pose_graph_create": 6, "ll_pose_graph_destroy": 1, "ll_pose_graph_solve": 10, "ll_pose_graph_work": 2}


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "loam_livox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = capi.load()
    for name, n_args in NEW.items():
        decl = re.search(r"\b(int|void|int64_t)\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl and name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert len(decl.group(2).split(",")) == len(fn.argtypes) == n_args, name
        assert fn.restype is {"int": C.c_int32, "void": None, "int64_t": C.c_int64}[decl.group(1)], name
    p = capi.pose_graph_default_params()
    assert {k: getattr(p, k) for k, _ in capi.PoseGraphParams._fields_} == ref.OPTIONS
    import inspect
    from loam_livox_amd import api
    from loam_livox_amd.keyframes import Keyframe_assembly
    assert all(callable(getattr(api.Pose_graph, m)) for m in ("solve", "work", "close"))
    assert callable(api.relative_constraint) and callable(api.loop_constraint) and callable(Keyframe_assembly.close_loop)
    assert inspect.signature(Keyframe_assembly.__init__).parameters["pose_graph"].default is False


def test_null_handles_and_bad_arguments_are_refused_without_a_device():
    L = capi.load()
    h, work = C.c_void_p(), np.zeros(4, np.int64)
    assert L.ll_pose_graph_create(0, 1, 16, 16, 64, None) < 0 and b"ll_pose_graph_create: null" in L.ll_last_error()
    for args, text in (((0, 16, 16, 64), b"max_graphs out of range"), ((1, 0, 16, 64), b"max_poses_total out of range"),
                       ((1, 16, -1, 64), b"max_edges_total out of range"), ((1, 16, 16, 0), b"max_envelope_blocks out of range"),
                       ((1, (1 << 24) + 1, 16, 64), b"max_poses_total out of range")):
        assert L.ll_pose_graph_create(0, *args, C.byref(h)) < 0 and text in L.ll_last_error() and not h.value, text
    x = pgi.case("n2")["poses"].copy()
    before = x.copy()
    off = np.array([0, 2], np.int64)
    summary = (capi.PoseGraphSummary * 1)()
    assert L.ll_pose_graph_solve(None, None, 1, capi.ptr(off), capi.ptr(x), capi.ptr(off), None, None, None, summary) < 0
    assert b"ll_pose_graph_solve: null" in L.ll_last_error() and np.array_equal(x, before)
    assert L.ll_pose_graph_work(None, capi.ptr(work)) < 0 and b"ll_pose_graph_work: null" in L.ll_last_error()
    L.ll_pose_graph_default_params(None)
    L.ll_pose_graph_destroy(None)


# ------------------------------------------------------------------------------------------------ bookkeeping against stubs
def np_qmul(a, b):
    """Eigen's quaternion product, term for term, on {x, y, z, w}"""
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def np_qinv(q):
    return np.array([-q[0], -q[1], -q[2], q[3]]) / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def np_qrot(q, v):
    uv = np.cross(q[:3], v)
    uv = uv + uv
    return v + q[3] * uv + np.cross(q[:3], uv)


def np_constraints(poses, loop):
    """laser_mapping.hpp:954-958 for every two consecutive poses, then scene_alignment.hpp:104-106 for the loop (last -> his)"""
    ab, meas = [], []
    for k in range(len(poses) - 1):
        qi = np_qinv(poses[k][:4])
        ab.append((k, k + 1))
        meas.append(np.concatenate([np_qmul(qi, poses[k + 1][:4]), np_qrot(qi, poses[k + 1][4:7] - poses[k][4:7])]))
    a, b = poses[loop["his"]], poses[loop["last"]]
    qbi, qii = np_qinv(b[:4]), np_qinv(np.asarray(loop["icp_q"], np.float64))
    ab.append((loop["last"], loop["his"]))
    meas.append(np.concatenate([np_qmul(np_qmul(qbi, qii), a[:4]), np_qrot(qbi, np_qrot(qii, a[4:7] - np.asarray(loop["icp_t"], np.float64)) - b[4:7])]))
    return np.array(ab, np.int32), np.array(meas)


class StubPoseGraph:
    """stands in for api.Pose_graph: records the graphs of every solve and answers with the reference's solution"""

    def __init__(self):
        self.calls = []

    def solve(self, graphs):
        self.calls.append([{k: np.array(v) for k, v in g.items()} for g in graphs])
        out = [ref.solve(g["poses"], g["ab"], g["meas"]) for g in graphs]
        return [x for x, _ in out], [{k: s[k] for k in ("iterations", "successful_steps", "unsuccessful_steps", "initial_cost", "final_cost", "termination")}
                                     for _, s in out]

    def close(self):
        self.closed = True


def key_frame_poses(seed, n):
    est = pgi.make_graph(n, [], seed)["poses"]
    return est


@pytest.mark.parametrize("seed,min_diff", [(2, 1), (4, 2), (6, 2)])      # the scripted walks of tests/test_keyframes.py that end in a loop
def test_close_loop_over_a_stub_leaves_the_walk_as_it_was(monkeypatch, seed, min_diff):
    from tests import test_keyframe_bank_host as kb
    sc = kb.script(seed)
    poses = key_frame_poses(seed, kb.K)
    assemblies = []
    stub = StubPoseGraph()
    for kw in ({}, dict(pose_graph=stub)):
        ka = kb.stub_assembly(monkeypatch, sc, min_diff, [], **kw)
        monkeypatch.setattr("loam_livox_amd.keyframes.keyframe_similarity", ka.similarity)
        for k in range(kb.K):
            kf = kb.waiting_keyframe(sc, k)
            kf.m_pose_q, kf.m_pose_t = poses[k][:4].copy(), poses[k][4:7].copy()
            ka.m_keyframe_need_precession_list.append(kf)
            ka.process_waiting()
        assemblies.append(ka)
    off, on = assemblies
    assert kb.outcome(on) == kb.outcome(off) and off.if_end and len(off.loops) == 1
    assert off.poses_opm is None and off.constraints is None and off.pose_graph_summary is None
    loop = on.loops[0]
    n = len(on.pose3d_vec)
    assert len(stub.calls) == 1 and len(stub.calls[0]) == 1
    g = stub.calls[0][0]
    want_ab, want_meas = np_constraints(poses[:n], loop)
    assert np.array_equal(g["ab"], want_ab) and g["meas"].tobytes() == want_meas.tobytes()       # bit for bit
    assert g["poses"].tobytes() == poses[:n].tobytes() and on.poses_ori.tobytes() == poses[:n].tobytes()
    assert np.array_equal(on.constraints["ab"], want_ab) and on.constraints["meas"].tobytes() == want_meas.tobytes()
    want, ws = ref.solve(poses[:n], want_ab, want_meas)
    assert on.poses_opm.tobytes() == want.tobytes() and on.pose_graph_summary["termination"] == ws["termination"]
    # close_loop is public and repeatable, and touches nothing else
    before = kb.outcome(on)
    again = on.close_loop(loop)
    assert again.tobytes() == want.tobytes() and kb.outcome(on) == before and len(stub.calls) == 2
    on.close()
    assert not hasattr(stub, "closed")                                 # a handle handed in is not closed by the assembly


def test_batched_loop_makes_one_solve_per_round_over_all_slots_that_looped(monkeypatch):
    from loam_livox_amd import keyframes as kfm
    from tests import test_keyframe_bank_host as kb
    S, min_diff = 3, 2
    scripts = [kb.script(seed) for seed in (2, 3, 2)]                 # slots 0 and 2 walk the same script: they loop in the same round
    poses = [key_frame_poses(seed, kb.K) for seed in (12, 13, 14)]    # ... with different key-frame poses
    alone = [kb.stub_assembly(monkeypatch, sc, min_diff, []) for sc in scripts]
    bank, stub = kb.StubBank(), StubPoseGraph()
    slots = [kb.stub_assembly(monkeypatch, sc, min_diff, [], device_bank=True, bank=bank, pose_graph=stub) for sc in scripts]

    class Store:
        def extract_cells(self, kind, sequences, cell_lists, dsts):
            pass

    rounds = kfm.Keyframe_rounds(slots, store=Store(), bank=bank, pose_graph=stub)
    solves_per_step = []
    for k in range(kb.K):
        for s in range(S):
            for ka in (alone[s], slots[s]):
                kf = kb.waiting_keyframe(scripts[s], k)
                kf.m_pose_q, kf.m_pose_t = poses[s][k][:4].copy(), poses[s][k][4:7].copy()
                ka.m_keyframe_need_precession_list.append(kf)
        for s in range(S):
            monkeypatch.setattr(kfm, "keyframe_similarity", alone[s].similarity)
            alone[s].process_waiting()
        before = len(stub.calls)
        rounds.run(list(range(S)))
        solves_per_step.append(len(stub.calls) - before)
    for s in range(S):
        assert kb.outcome(slots[s]) == kb.outcome(alone[s]), s
    looped = [s for s in range(S) if alone[s].loops]
    assert looped == [0, 2] and sum(solves_per_step) == 1
    assert len(stub.calls) == 1 and len(stub.calls[0]) == 2           # ONE solve, for both slots that looped in that round
    for g, s in zip(stub.calls[0], looped):
        n = len(slots[s].pose3d_vec)
        want_ab, want_meas = np_constraints(poses[s][:n], slots[s].loops[0])
        assert np.array_equal(g["ab"], want_ab) and g["meas"].tobytes() == want_meas.tobytes()
        assert slots[s].poses_opm.tobytes() == ref.solve(poses[s][:n], want_ab, want_meas)[0].tobytes() and not slots[s].pending_loops
        assert slots[s].poses_ori.tobytes() == poses[s][:n].tobytes()
    assert slots[1].poses_opm is None and not slots[1].pending_loops
