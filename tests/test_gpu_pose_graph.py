"""-m gpu: the pose-graph optimiser on the device (ll_pose_graph_*; api.Pose_graph, Keyframe_assembly.close_loop) against
tests/pose_graph_ref.py, the float64 numpy restatement of ceres_pose_graph_3d.hpp's problem and of Ceres' trust-region sequence.
tests/test_pose_graph_host.py is the CPU tier (the kernel's text under g++, and the conditions on the cases).

Tolerance.  Per case the reference's own sensitivity s is measured (the largest pose change when its inputs move by one unit in the
last place, 8 draws); device - reference <= max( 1000 s, 1e-11 ) in metres and in radians, and < 1e-7 (the registrar tests' bar) in
every case; iteration, successful-step and unsuccessful-step counts and the termination are equal.  Every figure is printed before it
is asserted.

The shapes are the smallest at which the kernel can go wrong: one pose, no edges, two poses, an envelope row reaching the constant
pose, nested and overlapping envelopes, more than 64 and more than 256 edges (the work items of a workgroup), rejected steps,
information matrices on a third of the edges, edges of both directions, a graph 50 km from the origin, 1 / 5 / 70 graphs of mixed sizes in
one call.

And where the kernel's text changes form: N = 342 and N = 343 (the vector of the triangular solves in LDS, and past LL_PG_LDS_VEC in
the workspace, where two graphs of one call must not share it), poses without edges, a component that never touches pose 0, repeated
and reversed edges, information of a wide spectrum on every edge, quaternions far from unit norm, a normal matrix and a cost that
overflow, the exits on the iteration cap, the radius floor and a run of invalid steps, parameters other than the defaults, handles of
exactly the size a call needs and one short of it, and api.Pose_graph growing."""
import ctypes as C

import numpy as np
import pytest

from tests import pose_graph_inputs as pgi
from tests import pose_graph_ref as ref

pytestmark = pytest.mark.gpu

SINGLE = ["n2", "n3_loop_to_fixed", "n17_three_loops", "n17_far", "n33_detector", "n66", "n300_six_loops", "n40_hard", "n66_hard_rejected_steps",
          "n24_information", "n20_both_directions", "n17_consistent", "n30_consistent"] + [n for n in pgi.NEW_CASES if n not in pgi.UNCHANGED]
HBM_BATCH = ["n17_three_loops", "n343_hbm_first", "n343_hbm_other", "n17_three_loops", "n342_lds_top", "n343_hbm_first"]
ABSOLUTE_BAR = 1e-7


@pytest.fixture(scope="module")
def handle(gpu_lib):
    from loam_livox_amd.api import Pose_graph
    h = Pose_graph(max_graphs=80, max_poses=4096, max_edges=4096, max_envelope_blocks=16384)
    yield h
    h.close()


def graph_of(name):
    g = pgi.case(name)
    return dict(poses=g["poses"], ab=g["ab"], meas=g["meas"], information=g["information"])


def check_unchanged(name, poses, summary):
    """a run that takes no step: the poses of the input in their bytes, the reference's counts and exit, its cost to 1e-12"""
    want, ws = pgi.reference(name)
    print(f"{name}: {summary}; reference cost {ws['initial_cost']!r}")
    assert poses.tobytes() == np.ascontiguousarray(pgi.case(name)["poses"]).tobytes() == want.tobytes(), name
    assert (summary["iterations"], summary["successful_steps"], summary["unsuccessful_steps"], summary["termination"]) == \
        (ws["iterations"], ws["successful_steps"], ws["unsuccessful_steps"], ws["termination"]), (name, summary)
    assert summary["initial_cost"] == summary["final_cost"], (name, summary)
    if np.isinf(ws["initial_cost"]):
        assert summary["initial_cost"] == ws["initial_cost"], (name, summary)
    else:
        assert abs(summary["initial_cost"] - ws["initial_cost"]) <= 1e-12 * ws["initial_cost"], (name, summary, ws["initial_cost"])


def check_against_reference(name, poses, summary):
    if name in pgi.UNCHANGED:
        return check_unchanged(name, poses, summary)
    want, ws = pgi.reference(name)
    tol_m, tol_rad = pgi.tolerance(name)
    d_m, d_rad = ref.pose_distance(want, poses)
    print(f"{name}: device - reference {d_m:.3e} m {d_rad:.3e} rad (allowed {tol_m:.3e} m {tol_rad:.3e} rad); iterations {summary['iterations']} "
          f"({summary['successful_steps']} + {summary['unsuccessful_steps']}) {summary['termination']}; cost {summary['initial_cost']:.6e} -> "
          f"{summary['final_cost']:.6e}")
    assert d_m <= tol_m and d_rad <= tol_rad, (name, d_m, d_rad, tol_m, tol_rad)
    assert d_m < ABSOLUTE_BAR and d_rad < ABSOLUTE_BAR, (name, d_m, d_rad)
    assert (summary["iterations"], summary["successful_steps"], summary["unsuccessful_steps"], summary["termination"]) == \
        (ws["iterations"], ws["successful_steps"], ws["unsuccessful_steps"], ws["termination"]), (name, summary, ws["termination"])


@pytest.mark.parametrize("name", SINGLE)
def test_one_graph_equals_the_reference(handle, name):
    poses, summaries = handle.solve([graph_of(name)])
    check_against_reference(name, poses[0], summaries[0])
    assert np.array_equal(poses[0][0], pgi.case(name)["poses"][0])             # the constant pose, to the bit


@pytest.fixture(scope="module")
def alone(handle):
    """name -> (poses, summary) of the graph solved alone on the shared handle, once"""
    class Alone(dict):
        def __missing__(self, name):
            poses, summaries = handle.solve([graph_of(name)])
            self[name] = (poses[0], summaries[0])
            return self[name]
    return Alone()


@pytest.mark.parametrize("name", ["b24_overflow", "b24_cost_overflow"])
def test_an_overflowing_graph_comes_back_as_it_went_in(handle, name):
    """b24_overflow: no step can be solved, the radius is halved four times and the fifth invalid step ends the solve;
    b24_cost_overflow: the step is valid, the cost of the candidate is not finite and is taken as the largest double"""
    poses, summaries = handle.solve([graph_of(name)])
    check_unchanged(name, poses[0], summaries[0])
    assert summaries[0]["termination"] == {"b24_overflow": "invalid_steps", "b24_cost_overflow": "function"}[name]
    poses, summaries = handle.solve([graph_of("n17_three_loops")])                 # and the handle still works
    check_against_reference("n17_three_loops", poses[0], summaries[0])


def test_the_solve_vector_outside_lds_in_a_batch(handle, alone):
    """the N = 343 graphs keep the vector of the triangular solves in the workspace, at their own poses' offset: two of them beside
    each other, a third later in the call, graphs with the vector in LDS between them.  Were two workgroups' vectors to overlap, a
    graph would not come out as it does alone."""
    poses, summaries = handle.solve([graph_of(n) for n in HBM_BATCH])
    work = handle.work()
    assert work[1] == 1 and work[3] == len(HBM_BATCH), work
    for k, n in enumerate(HBM_BATCH):
        assert poses[k].tobytes() == alone[n][0].tobytes() and summaries[k] == alone[n][1], (k, n)
    for n in sorted(set(HBM_BATCH)):
        check_against_reference(n, *alone[n])


def test_the_solve_vector_outside_lds_of_graphs_that_share_an_l2(handle, alone):
    """The batch above alone does not see two workgroups sharing that vector: with `gr.pose0` taken out of its offset the batch
    still passed on an MI355X.  The workgroups of a launch are dealt to the eight XCDs in turn, each XCD has its own L2, and one
    L2's lines are not refreshed by another's stores within a launch, so three graphs in slots 1, 2 and 5 each saw their own copy.
    Here the N = 343 graphs stand eight slots apart -- 0 and 8, 1 and 9, each pair of two different graphs -- so that, dealt in
    turn, a pair shares an L2 and every store of one is what the other loads."""
    names = ["n343_hbm_first", "n343_hbm_other"] + ["n17_three_loops"] * 6 + ["n343_hbm_other", "n343_hbm_first"]
    poses, summaries = handle.solve([graph_of(n) for n in names])
    assert handle.work()[1] == 1
    for k, n in enumerate(names):
        assert poses[k].tobytes() == alone[n][0].tobytes() and summaries[k] == alone[n][1], (k, n)


@pytest.mark.parametrize("name", list(pgi.OPTION_CASES))
def test_parameters_other_than_the_defaults(gpu_lib, name):
    from loam_livox_amd.api import Pose_graph
    from tests.pose_graph_driver import params_struct
    options = pgi.OPTION_CASES[name][1]
    h = Pose_graph(max_graphs=1, max_poses=80, max_edges=80, max_envelope_blocks=512, params=params_struct(options))
    try:
        poses, summaries = h.solve([graph_of(name)])
        assert h.capacity == [1, 80, 80, 512]
    finally:
        h.close()
    check_against_reference(name, poses[0], summaries[0])
    assert summaries[0]["termination"] == pgi.reference(name)[1]["termination"]


def needs(names):
    from loam_livox_amd.api import Pose_graph
    graphs = [pgi.case(n) for n in names]
    return [len(graphs), sum(len(g["poses"]) for g in graphs), sum(len(g["ab"]) for g in graphs),
            sum(Pose_graph.envelope_blocks(len(g["poses"]), g["ab"]) for g in graphs)]


@pytest.mark.parametrize("names", [["n17_three_loops"], HBM_BATCH], ids=["n17", "hbm_batch"])
def test_a_handle_of_exactly_the_size_and_one_short(gpu_lib, handle, names):
    from loam_livox_amd import capi
    from loam_livox_amd.api import Pose_graph
    from tests.pose_graph_driver import pack
    need = needs(names)
    want_poses, want_summaries = handle.solve([graph_of(n) for n in names])
    assert list(handle.work()[2:4]) == [need[3], need[0]]
    exact = Pose_graph(*need)
    try:
        h0 = exact.h.value
        poses, summaries = exact.solve([graph_of(n) for n in names])
        assert exact.capacity == need and exact.h.value == h0                     # (it did not grow)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(poses, want_poses)) and summaries == want_summaries
    finally:
        exact.close()
    po, x, eo, ab, meas, _ = pack([graph_of(n) for n in names])
    text = ("capacity exceeded: the call needs %d graphs, %d poses, %d edges and %d envelope blocks" % tuple(need)).encode()
    L = gpu_lib
    for k in range(4):
        short = list(need)
        short[k] -= 1
        h = C.c_void_p()
        if short[k] < 1:                                                         # (a handle for no graph at all cannot be created)
            assert L.ll_pose_graph_create(0, *short, C.byref(h)) < 0 and b"out of range" in L.ll_last_error() and not h.value
            continue
        assert L.ll_pose_graph_create(0, *short, C.byref(h)) == 0, L.ll_last_error()
        try:
            xs = x.copy()
            summary = (capi.PoseGraphSummary * len(names))()
            rc = L.ll_pose_graph_solve(h, None, len(names), capi.ptr(po), capi.ptr(xs), capi.ptr(eo), capi.ptr(ab), capi.ptr(meas), None, summary)
            assert rc < 0 and text in L.ll_last_error(), (k, L.ll_last_error())
            assert ("(the handle has %d, %d, %d, %d)" % tuple(short)).encode() in L.ll_last_error()
            assert xs.tobytes() == x.tobytes()
        finally:
            L.ll_pose_graph_destroy(h)


def test_the_python_handle_grows(gpu_lib, handle):
    from loam_livox_amd.api import Pose_graph
    small = Pose_graph(max_graphs=1, max_poses=8, max_edges=8, max_envelope_blocks=8)
    try:
        for names in (["n33_detector"], HBM_BATCH):
            before, h_before = list(small.capacity), small.h.value
            want_poses, want_summaries = handle.solve([graph_of(n) for n in names])
            poses, summaries = small.solve([graph_of(n) for n in names])
            assert all(a.tobytes() == b.tobytes() for a, b in zip(poses, want_poses)) and summaries == want_summaries, names
            need = needs(names)
            assert all(c >= n and c >= b for c, n, b in zip(small.capacity, need, before)) and small.capacity != before
            assert small.h.value and small.h is not None and list(small.work()[2:4]) == [need[3], need[0]]
            print(f"{names[0]} ...: capacity {before} -> {small.capacity}, handle {h_before:#x} -> {small.h.value:#x}")
        again = small.solve([graph_of("n33_detector")])                            # large enough now: the handle stays
        h_now = small.h.value
        assert small.solve([graph_of("n33_detector")])[0][0].tobytes() == again[0][0].tobytes() and small.h.value == h_now
    finally:
        small.close()
    assert small.h is None
    small.close()                                                                # closing twice is harmless


def test_poses_without_edges_and_a_component_apart(handle, alone):
    for name, at in (("b24_edgeless_last", 24), ("b24_edgeless_middle", 10)):
        poses, summary = alone[name]
        assert poses[at].tobytes() == pgi.FAR_POSE.tobytes(), name
        check_against_reference(name, poses, summary)
    # the pose in the middle changes no other pose's arithmetic: the two graphs differ by where it stands alone
    assert np.delete(alone["b24_edgeless_middle"][0], 10, axis=0).tobytes() == alone["b24_edgeless_last"][0][:24].tobytes()
    for name in ("b24_floating_component", "b24_floating_component_loops"):
        poses, summary = alone[name]
        check_against_reference(name, poses, summary)
        want = pgi.reference(name)[0]
        tol_m, tol_rad = pgi.tolerance(name)
        for part in (slice(0, 12), slice(12, 24)):
            d_m, d_rad = ref.pose_distance(want[part], poses[part])
            print(f"{name}: poses {part.start} .. {part.stop - 1}: device - reference {d_m:.3e} m {d_rad:.3e} rad")
            assert d_m <= tol_m and d_rad <= tol_rad
    assert alone["b24_floating_component_loops"][1]["successful_steps"] > 1


def test_rejected_steps_and_all_three_terminations_occur(handle):
    poses, summaries = handle.solve([graph_of(n) for n in SINGLE])
    assert summaries[SINGLE.index("n66_hard_rejected_steps")]["unsuccessful_steps"] > 0
    assert {"function", "gradient", "parameter"} <= {s["termination"] for s in summaries}


@pytest.mark.parametrize("name", ["n17_consistent", "n30_consistent"])
def test_consistent_graphs_recover_the_truth(handle, name):
    """edges from the truth without noise, start from the drifted estimates: the project's contract, 1e-4 m / 1e-4 rad"""
    g = pgi.case(name)
    assert max(ref.pose_distance(pgi.reference(name)[0], g["truth"])) < 1e-4           # (the reference itself recovers)
    poses, _ = handle.solve([graph_of(name)])
    d_m, d_rad = ref.pose_distance(poses[0], g["truth"])
    print(f"{name}: device - truth {d_m:.3e} m {d_rad:.3e} rad; start - truth {ref.pose_distance(g['poses'], g['truth'])}")
    assert d_m < 1e-4 and d_rad < 1e-4


def test_nothing_to_optimise(handle):
    one = dict(poses=pgi.case("n17_three_loops")["poses"][:1], ab=np.zeros((0, 2), np.int32), meas=np.zeros((0, 7)))
    no_edges = dict(poses=pgi.case("n17_three_loops")["poses"][:5], ab=np.zeros((0, 2), np.int32), meas=np.zeros((0, 7)))
    poses, summaries = handle.solve([one, no_edges])
    for g, x, s in zip((one, no_edges), poses, summaries):
        assert np.array_equal(x, g["poses"]) and s["termination"] == "nothing" and s["iterations"] == 0
    assert handle.solve([]) == ([], [])


def mixed_batch(n_graphs):
    """graphs of mixed sizes, the empty one among them; the N = 17 graph at slot 0 and, when there is one, at slot 37"""
    names = ["n17_three_loops", "n2", "n33_detector", "n3_loop_to_fixed", "n66", "n24_information", "n20_both_directions", "n40_hard",
             "n17_consistent", "n66_hard_rejected_steps", "n30_consistent", "n17_far"]
    out = []
    for k in range(n_graphs):
        if k == 3:
            out.append(None)
        elif k == 37:
            out.append("n17_three_loops")
        else:
            out.append(names[k % len(names)] if k else names[0])
    return out


@pytest.mark.parametrize("n_graphs", [1, 5, 70])
def test_batches_of_mixed_sizes(handle, n_graphs):
    names = mixed_batch(n_graphs)
    empty = dict(poses=pgi.case("n2")["poses"], ab=np.zeros((0, 2), np.int32), meas=np.zeros((0, 7)))
    poses, summaries = handle.solve([empty if n is None else graph_of(n) for n in names])
    work = handle.work()
    assert work[1] == 1 and work[3] == n_graphs, work                               # one host wait whatever G is
    alone = {}
    for k, n in enumerate(names):
        if n is None:
            assert summaries[k]["termination"] == "nothing" and np.array_equal(poses[k], empty["poses"])
            continue
        if n not in alone:
            alone[n] = handle.solve([graph_of(n)])
            check_against_reference(n, poses[k], summaries[k])
        # a graph's result does not depend on the batch or on its slot: bit for bit
        assert poses[k].tobytes() == alone[n][0][0].tobytes() and summaries[k] == alone[n][1][0], (k, n)


def test_n17_is_bit_equal_alone_in_a_batch_and_across_runs(handle):
    g = graph_of("n17_three_loops")
    first = handle.solve([g])
    again = handle.solve([g])
    names = mixed_batch(40)
    assert names[0] == names[37] == "n17_three_loops"
    empty = dict(poses=pgi.case("n2")["poses"], ab=np.zeros((0, 2), np.int32), meas=np.zeros((0, 7)))
    poses, summaries = handle.solve([empty if n is None else graph_of(n) for n in names])
    for x, s in ((again[0][0], again[1][0]), (poses[0], summaries[0]), (poses[37], summaries[37])):
        assert x.tobytes() == first[0][0].tobytes() and s == first[1][0]


def test_far_from_the_origin_measures_its_own_sensitivity(handle):
    s_near, s_far = pgi.reference_sensitivity("n17_three_loops"), pgi.reference_sensitivity("n17_far")
    print(f"reference sensitivity: at the origin {s_near}, 50 km away {s_far}")
    poses, summaries = handle.solve([graph_of("n17_far")])
    check_against_reference("n17_far", poses[0], summaries[0])


def test_refusals_leave_the_poses_untouched(gpu_lib, handle):
    import ctypes as C
    from loam_livox_amd import capi
    from loam_livox_amd.api import Pose_graph
    g = graph_of("n17_three_loops")
    x = np.ascontiguousarray(g["poses"], np.float64)
    po, eo = np.array([0, len(x)], np.int64), np.array([0, len(g["ab"])], np.int64)
    ab, meas = np.ascontiguousarray(g["ab"], np.int32), np.ascontiguousarray(g["meas"], np.float64)
    summary = (capi.PoseGraphSummary * 1)()
    L, h = gpu_lib, handle.h

    def refused(text, x_=None, po_=po, eo_=eo, ab_=ab, meas_=meas, info_=None, h_=h, summary_=summary):
        xs = x.copy() if x_ is None else x_
        before = xs.copy()
        rc = L.ll_pose_graph_solve(h_, None, 1, capi.ptr(po_), capi.ptr(xs), capi.ptr(eo_), capi.ptr(ab_), capi.ptr(meas_), capi.ptr(info_), summary_)
        assert rc < 0 and text in L.ll_last_error(), (text, L.ll_last_error())
        assert xs.tobytes() == before.tobytes()

    refused(b"null argument", h_=None)
    refused(b"null argument", summary_=None)
    refused(b"null argument", ab_=None)
    bad = ab.copy()
    bad[5, 1] = 17
    refused(b"out of range", ab_=bad)
    bad = ab.copy()
    bad[5] = (4, 4)
    refused(b"joins a pose to itself", ab_=bad)
    bad = x.copy()
    bad[3, 5] = np.nan
    refused(b"not finite", x_=bad)
    bad = meas.copy()
    bad[2, 0] = np.inf
    refused(b"not finite", meas_=bad)
    info = np.tile(np.eye(6).ravel(), (len(ab), 1))
    info[7, 14] = -1.0                                           # (2, 2): a negative pivot
    refused(b"not positive definite", info_=info)
    refused(b"offsets", po_=np.array([1, len(x)], np.int64))
    small = Pose_graph(max_graphs=1, max_poses=16, max_edges=64, max_envelope_blocks=64)
    try:
        refused(b"capacity exceeded: the call needs 1 graphs, 17 poses, 19 edges and ", h_=small.h)
        assert str(Pose_graph.envelope_blocks(17, ab)).encode() + b" envelope blocks" in L.ll_last_error()
    finally:
        small.close()
    # and the handle still works
    poses, summaries = handle.solve([g])
    check_against_reference("n17_three_loops", poses[0], summaries[0])
    assert handle.work()[2] == Pose_graph.envelope_blocks(17, ab)


def test_close_loop_on_the_real_handle(handle):
    """Keyframe_assembly.close_loop: the chain constraints over pose3d_vec and the loop constraint, solved on the device"""
    from loam_livox_amd.keyframes import Keyframe_assembly
    from tests.test_keyframes import ScriptedMap
    g = pgi.case("n33_detector")
    est, truth = g["poses"], g["truth"]
    ka = Keyframe_assembly(full_cell_map=ScriptedMap([]), pose_graph=handle)
    ka.pose3d_vec = [(p[:4].copy(), p[4:7].copy()) for p in est]
    his, last = 1, 32
    # the alignment's transform maps the new key frame's map onto the old one's: identity when the estimates agree with the truth
    rel_true, rel_est = pgi.relative(truth[last], truth[his]), pgi.relative(est[last], est[his])
    # choose icp_q, icp_t so that the loop constraint is the true relative pose: q_res = q_b^-1 icp_q^-1 q_a
    icp_q = ref.qinv(ref.qmul(ref.qmul(est[last][:4], rel_true[:4]), ref.qinv(est[his][:4])))
    icp_t = est[his][4:7] - ref.qrot(icp_q, ref.qrot(est[last][:4], rel_true[4:7]) + est[last][4:7])
    loop = dict(his=his, last=last, inlier_threshold=0.1, icp_q=icp_q, icp_t=icp_t)
    opm = ka.close_loop(loop)
    graph = ka.loop_graph(loop)
    assert np.allclose(graph["meas"][-1], rel_true, atol=1e-12) and not np.allclose(rel_est, rel_true, atol=1e-4)
    want, ws = ref.solve(graph["poses"], graph["ab"], graph["meas"])
    d = ref.pose_distance(want, opm)
    sens = ref.sensitivity(graph["poses"], graph["ab"], graph["meas"], base=want)
    print(f"close_loop: device - reference {d}, the reference's sensitivity {sens}; {ka.pose_graph_summary}")
    assert d[0] <= max(1000 * sens[0], 1e-11) and d[1] <= max(1000 * sens[1], 1e-11)
    assert ka.pose_graph_summary["iterations"] == ws["iterations"] and ka.pose_graph_summary["termination"] == ws["termination"]
    assert np.array_equal(ka.poses_ori, est) and ka.poses_opm is opm and len(ka.constraints["ab"]) == 33
    # the loop is closed: the optimised poses satisfy the loop constraint far better than the estimates
    err = lambda x: np.linalg.norm(pgi.relative(x[last], x[his])[4:7] - rel_true[4:7])      # noqa: E731
    assert err(opm) < 0.2 * err(est)
    ka.close()
    assert handle.h                                                # a handle handed in is not closed by the assembly


def test_adapter_program_on_the_real_handle(handle, tmp_path):
    """Ceres_pose_graph_3d::pose_graph_optimization and Scene_alignment::add_constrain_of_loop of the C++ adapter: the floats of the
    Python route, bit for bit (the same library call on the same values)"""
    import os
    import subprocess
    from loam_livox_amd import build
    from loam_livox_amd.api import loop_constraint
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = build.build()
    exe = str(tmp_path / "adapter_pose_graph")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "adapter_pose_graph.cpp"), lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    g = pgi.case("n17_three_loops")
    est = np.ascontiguousarray(g["poses"])
    chain_ab, chain_meas = np.ascontiguousarray(g["ab"][:16]), np.ascontiguousarray(g["meas"][:16])
    his, last = 2, 16
    rng = np.random.default_rng(5)
    icp_q = pgi.small_rotation(rng.normal(0, 0.02, (1, 3)))[0]
    icp_t = rng.normal(0, 0.3, 3)
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.txt")
    with open(src, "wb") as f:
        f.write(np.array([17, 16, last, his], np.int64).tobytes() + est.tobytes() + chain_ab.tobytes() + chain_meas.tobytes())
        f.write(np.concatenate([est[his], est[last], icp_q, icp_t]).tobytes())
    subprocess.check_call([exe, src, out], timeout=120)
    rows = [l.split() for l in open(out).read().strip().split("\n")]
    got_loop = np.array([float.fromhex(v) for v in rows[0]])
    got = np.array([[float.fromhex(v) for v in r] for r in rows[1:-1]])
    s_idx, t_idx, m = loop_constraint(last, his, est[his], est[last], icp_q, icp_t)
    assert (s_idx, t_idx) == (16, 2) and got_loop.tobytes() == m.tobytes()
    poses, summaries = handle.solve([dict(poses=est, ab=np.concatenate([chain_ab, [[last, his]]]), meas=np.concatenate([chain_meas, m[None]]))])
    s = summaries[0]
    assert got.tobytes() == poses[0].tobytes()
    assert [int(v) for v in rows[-1]] == [s["iterations"], s["successful_steps"], s["unsuccessful_steps"], ref.TERMINATION.index(s["termination"])]
    assert s["iterations"] > 1
