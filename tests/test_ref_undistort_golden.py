"""Committed outputs of the REFERENCE'S OWN CLASS for the undistort branch (tests/golden/ref_undistort.npz, written by
tests/golden/gen_ref_undistort.py from oracle/_ref/libll_ref.so): the state four registrations of the scene of ref_scene2.npz leave in
Point_cloud_registration -- from the identity increment, from (0,0,0,-1, 0,0,0), rejected by the cost limit, returned by the gate --
and the clouds pointcloudAssociateToMap( ., ., 1 ) makes of it.  They travel where the reference does not:

  CPU tier : the oracle's registration reproduces the state to test_ref_golden.py's 1e-9; given the state, the oracle's cloud form and
             the host build of csrc/ll_reg_core.h reproduce the clouds IN BITS (builds of the same operations with -ffp-contract=off
             against the same libm), the numpy restatement tests/undistort_ref.py under its rule;
  GPU tier : Point_cloud_registration with if_motion_deblur = 1 registers the scene once per case; its state (ll_reg_interpolation) and
             poses lie within 1e-12 of the fixture's, and ll_cloud_undistort of the fixture's inputs within the rule of
             tests/undistort_ref.py: every coordinate within one fp32 ulp, at most 1 in 10 000 unequal.  The rule follows from the
             state bound: a state gap g moves a coordinate's double by about g, so the share of coordinates that round to the other
             float is g / ulp -- below 2e-5 for 1e-12 m and coordinates from 0.5 m up (ulp 6e-8).
"""
import numpy as np
import pytest

from loam_livox_amd import synth
from oracle import orc
from tests import undistort_pin as up
from tests import undistort_ref as ur

STATE_TOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    g = np.load(up.FIXTURE)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return up.build_host_lib(tmp_path_factory.mktemp("ref_undistort_golden"))


@pytest.fixture(scope="module")
def trees():
    s = up.scene()
    return orc.KdTree(s["corner_map"]), orc.KdTree(s["surf_map"])


def state_of(fx, case):
    """(pose_last, pose_curr, pose_incre, theta, hat, hat_sq) of the reference object after the case's registration"""
    return (up.scene()["pose_init"], fx[f"{case}_pose_out"], fx[f"{case}_pose_incre"], float(fx[f"{case}_theta"]), fx[f"{case}_omega_hat"],
            fx[f"{case}_omega_hat_sq2"])


def end_of_scan(cloud):
    """points the reference moves with pose_curr: s == 1, s > 1 and non-finite stamps (PCR:134, 627)"""
    s = up.scene()
    return ur.blur_ratio(cloud[:, 3], 1, s["t_min"], s["t_max"]) == 1


def test_what_the_reference_recorded(fx):
    s = up.scene()
    assert sorted(fx) == sorted(f"{c}_{f}" for c in up.CASES for f in ("ret", "pose_out", "pose_incre", "theta", "omega_hat", "omega_hat_sq2") + up.CLOUDS)
    assert [int(fx[f"{c}_ret"]) for c in up.CASES] == [1, 1, 0, 1]
    assert synth.pose_error(fx["w_plus_pose_out"], s["pose_out"]) == (0.0, 0.0) and up.same_bits(fx["w_plus_pose_incre"], s["pose_incre"])   # ref_scene2's registration
    # w = -1: the negated quaternion all the way, the same pose, the same state -- Eigen's AngleAxis turns the axis, not the angle
    assert up.same_bits(fx["w_minus_pose_incre"][:4], -fx["w_plus_pose_incre"][:4]) and up.same_bits(fx["w_minus_pose_incre"][4:], fx["w_plus_pose_incre"][4:])
    assert up.same_bits(fx["w_minus_pose_out"][:4], -fx["w_plus_pose_out"][:4]) and up.same_bits(fx["w_minus_pose_out"][4:], fx["w_plus_pose_out"][4:])
    assert fx["w_minus_pose_incre"][3] < 0 and float(fx["w_plus_theta"]) > 1e-3
    for f in ("theta", "omega_hat", "omega_hat_sq2") + up.CLOUDS:
        assert up.same_bits(fx[f"w_minus_{f}"], fx[f"w_plus_{f}"]), f
    # rejected: the pose restored, the increment and its state kept (PCR:561-573)
    assert up.same_bits(fx["rejected_pose_out"], s["pose_init"]) and up.same_bits(fx["rejected_pose_incre"], fx["w_plus_pose_incre"])
    assert all(up.same_bits(fx[f"rejected_{f}"], fx[f"w_plus_{f}"]) for f in ("theta", "omega_hat", "omega_hat_sq2"))
    # gated: nothing touched, a fresh object's zero state (PCR:199)
    assert up.same_bits(fx["gated_pose_out"], s["pose_init"]) and up.same_bits(fx["gated_pose_incre"], up.IDENT)
    assert float(fx["gated_theta"]) == 0.0 and not fx["gated_omega_hat"].any() and not fx["gated_omega_hat_sq2"].any()
    for name in up.CLOUDS:
        assert fx[f"w_plus_{name}"].shape == (len(s[name]), 3) and fx[f"w_plus_{name}"].dtype == np.float32
    sh = ur.blur_ratio(s["shifted"][:, 3], 1, s["t_min"], s["t_max"])
    assert (sh < 0).sum() > 900 and (sh == 1).sum() > 900 and np.isnan(s["shifted"][:, 3]).sum() > 20 and (~np.isfinite(s["full"][:, :3]).all(axis=1)).sum() > 0
    # the deskew is not a no-op on this scene: the plain transform with pose_curr is elsewhere
    far = np.abs(fx["w_plus_surface"] - orc.cloud_transform(fx["w_plus_pose_out"], s["surface"])[:, :3]).max()
    assert far > 1e-2, far


# ------------------------------------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("case", up.CASES)
def test_oracle_registration_reproduces_the_state(fx, trees, case):
    s = up.scene()
    ret, pc, pi, rep, st = orc.reg_solve_state(trees[0], trees[1], s["corners"], s["surface"], up.case_params(case), s["pose_init"], s["pose_init"],
                                               up.start_increment(case))
    _, want_pc, want_pi, theta, hat, hat_sq = state_of(fx, case)
    assert ret == int(fx[f"{case}_ret"]) and rep.gated == (case == "gated")
    gaps = dict(pose=np.abs(pc - want_pc).max(), increment=np.abs(pi - want_pi).max(), theta=abs(st["theta"] - theta),
                omega_hat=np.abs(st["omega_hat"] - hat).max(), omega_hat_sq2=np.abs(st["omega_hat_sq2"] - hat_sq).max())
    print(f"{case}: oracle against the fixture", {k: float(v) for k, v in gaps.items()})
    assert gaps["pose"] < 1e-9 and gaps["increment"] < 1e-9 and gaps["theta"] < 1e-9   # elementwise: the sign of the quaternion as well
    # the axis is vec / |vec|, |vec| ~ theta / 2: the increment's 1e-9 over the fixture's smallest non-zero theta / 2 (6.6e-3)
    assert gaps["omega_hat"] < 1e-9 / 6e-3 and gaps["omega_hat_sq2"] < 2e-9 / 6e-3


@pytest.mark.parametrize("case", up.CASES)
def test_host_build_and_oracle_make_the_state_of_the_increment_in_bits(fx, host, case):
    _, _, pi, theta, hat, hat_sq = state_of(fx, case)
    if case == "gated":   # no solve ran: the state is not the identity increment's (axis x), it is a fresh object's
        assert theta == 0.0 and not hat.any()
        return
    for got in (up.host_interp(host, pi[:4]), orc.compute_interp(pi[:4])):
        assert got[0] == theta and up.same_bits(got[1], hat) and up.same_bits(got[2], hat_sq)
    # the numpy restatement: other arctan2 / norm implementations, the tolerance tests/test_undistort_host.py holds the host build to
    r_theta, r_hat = ur.interp(pi[:4])
    eps = 2.0 ** -52
    assert abs(r_theta - theta) <= 4 * eps * theta and np.abs(r_hat - hat).max() <= 4 * eps and np.abs(r_hat @ r_hat - hat_sq).max() <= 8 * eps


@pytest.mark.parametrize("case", up.CASES)
def test_clouds_of_the_state_on_the_cpu(fx, host, case):
    s = up.scene()
    pl, pc, pi, theta, hat, hat_sq = state_of(fx, case)
    for name in up.CLOUDS:
        cloud, want = s[name], fx[f"{case}_{name}"]
        args = (theta, hat, hat_sq, 1, s["t_min"], s["t_max"])
        for who, got in (("oracle", orc.cloud_associate(cloud, pl, pc, pi, *args)), ("host build", up.host_undistort(host, cloud, pl, pc, pi[4:], *args))):
            assert up.same_bits(got[:, 3], cloud[:, 3]), (who, name)                     # intensity copied, PCR:659
            assert up.same_bits(np.ascontiguousarray(got[:, :3]), want), (who, name)
        up.check_rule(ur.undistort(cloud, pl, pc, pi, theta, hat, 1, s["t_min"], s["t_max"]).astype(np.float32), want, f"{case} {name}: numpy restatement")
        end = end_of_scan(cloud)
        assert up.same_bits(np.ascontiguousarray(orc.cloud_transform(pc, cloud)[end, :3]), np.ascontiguousarray(want[end]))


@pytest.mark.parametrize("case", ["w_plus", "w_minus"])
def test_host_model_of_the_device_registration_from_either_sign(fx, case):
    """tests/hostcheck: the registrar's loop over the device headers (LM controller, interp_rodrigues, point_to_map_undistort) under g++,
    started from the case's increment.  Its k-NN is the device's grid search, so the bound is the device's guard 1e-7, as in
    test_ref_golden.py's -m gpu tier."""
    from tests.hostcheck import hc
    s = up.scene()
    gc, gs = hc.Grid(s["corner_map"], 0.5), hc.Grid(s["surf_map"], 0.6)
    hp = hc.RegParams(1, s["icp_iters"], s["ceres_iters"], 2, 1, 1, 0, 2.0, 50.0, 0.1, 0.02, 0.8, 0.01, 0.01, 0.3, 20.0, 100.0, s["t_min"], s["t_max"])
    ret, pc, pi, rep = hc.reg_solve(gc, gs, s["corners"], s["surface"], hp, s["pose_init"], s["pose_init"], up.start_increment(case))
    gap = max(np.abs(pc - fx[f"{case}_pose_out"]).max(), np.abs(pi - fx[f"{case}_pose_incre"]).max())
    print(f"{case}: host model against the fixture {gap:.3g}")
    assert ret == 1 and gap < 1e-7


# ------------------------------------------------------------------------------------------------ GPU tier
@pytest.fixture(scope="module")
def rig(gpu_lib):
    from loam_livox_amd.api import Map_buffer, Point_cloud_registration
    s = up.scene()
    m = Map_buffer()
    m.setInputCloud(Map_buffer.CORNER, s["corner_map"])
    m.setInputCloud(Map_buffer.SURF, s["surf_map"])
    reg = Point_cloud_registration(max_features=len(s["full"]))
    yield dict(map=m, reg=reg)
    reg.close()
    m.close()


def register(rig, case):
    """the scene through ll_reg_solve with the case's parameters and start increment (m_para_buffer_incremental)"""
    s, reg = up.scene(), rig["reg"]
    o = up.case_params(case)
    p = reg.params
    p.if_motion_deblur, p.minimum_pt_time_stamp, p.maximum_pt_time_stamp = 1, s["t_min"], s["t_max"]
    p.icp_max_iterations, p.ceres_max_iterations, p.force_all_iterations = s["icp_iters"], s["ceres_iters"], 0
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = o.para_max_angular_rate, o.para_max_speed, o.max_final_cost
    p.current_frame_index, p.mapping_init_accumulate_frames = o.current_frame_index, o.mapping_init_accumulate_frames
    reg.m_pose_w_last = s["pose_init"].copy()
    reg.m_pose_w_curr = s["pose_init"].copy()
    reg.m_para_buffer_incremental = up.start_increment(case)
    ret = reg.find_out_incremental_transfrom(rig["map"], s["corners"], s["surface"])
    return ret, reg.m_pose_w_curr.copy(), reg.m_para_buffer_incremental.copy(), reg.interpolation(1)


def state_gaps(fx, case, pc, pi, it):
    pl, want_pc, want_pi, theta, hat, hat_sq = state_of(fx, case)
    return dict(pose_curr=np.abs(pc - want_pc).max(), pose_incre=np.abs(pi - want_pi).max(), record_incre=np.abs(it["pose_incre"][0] - want_pi).max(),
                pose_last=np.abs(it["pose_last"][0] - pl).max(), theta=abs(it["theta"][0] - theta), omega_hat=np.abs(it["omega_hat"][0] - hat).max(),
                omega_hat_sq2=np.abs(it["omega_hat"][0] @ it["omega_hat"][0] - hat_sq).max())


@pytest.mark.gpu
@pytest.mark.parametrize("case", up.CASES)
def test_hip_registration_leaves_the_reference_state(fx, rig, case):
    """All four cases, the exits included: a rejected slot keeps its last increment and state with pose_curr = pose_last, a gated slot's
    record is the identity increment with a zero state -- what the reference object holds (the fixture), so nothing to document apart."""
    ret, pc, pi, it = register(rig, case)
    gaps = state_gaps(fx, case, pc, pi, it)
    print(f"{case}: device against the fixture", {k: float(v) for k, v in gaps.items()})
    assert ret == int(fx[f"{case}_ret"]) and bool(rig["reg"].report.gated) == (case == "gated")
    assert all(v <= STATE_TOL for v in gaps.values()), gaps   # elementwise: a quaternion of the other sign fails


@pytest.mark.gpu
def test_hip_negative_w_returns_the_negated_increment_and_the_same_pose(rig):
    plus = register(rig, "w_plus")
    minus = register(rig, "w_minus")
    assert plus[0] == minus[0] == 1 and minus[2][3] < 0 < plus[2][3]
    gap_inc = max(np.abs(minus[2][:4] + plus[2][:4]).max(), np.abs(minus[2][4:] - plus[2][4:]).max())
    dt, dr = synth.pose_error(minus[1], plus[1])
    gap_state = max(abs(minus[3]["theta"][0] - plus[3]["theta"][0]), np.abs(minus[3]["omega_hat"][0] - plus[3]["omega_hat"][0]).max())
    print(f"w = -1 against w = +1 on the device: increment {gap_inc:.3g}, pose {dt:.3g} m {dr:.3g} rad, state {gap_state:.3g}")
    assert gap_inc <= STATE_TOL and dt <= STATE_TOL and dr <= STATE_TOL and gap_state <= STATE_TOL
    assert np.abs(minus[1][:4] + plus[1][:4]).max() <= STATE_TOL   # q_last * (-q_incre): the pose's quaternion negated, as the reference's


@pytest.mark.gpu
@pytest.mark.parametrize("case", up.CASES)
def test_hip_clouds_against_the_reference(fx, rig, case):
    s, reg = up.scene(), rig["reg"]
    ret, pc, pi, it = register(rig, case)
    assert all(v <= STATE_TOL for v in state_gaps(fx, case, pc, pi, it).values())   # what the rule below rests on
    clouds = [(name, s[name], fx[f"{case}_{name}"]) for name in up.CLOUDS]
    clouds += [(f"surface[:{n}]", s["surface"][:n], fx[f"{case}_surface"][:n]) for n in (255, 256, 257)]   # around the kernel's 256-lane block
    unequal = total = 0
    for name, cloud, want in clouds:
        got = reg.pointcloudAssociateToMap(cloud, if_undistore=1)
        assert got.shape == cloud.shape and up.same_bits(got[:, 3], cloud[:, 3]), name   # intensity copied, PCR:659
        unequal += up.check_rule(got, want, f"{case} {name}: ll_cloud_undistort against the reference")
        total += want.size
        end = end_of_scan(cloud)   # s >= 1 and NaN stamps: the plain transform with the registration's pose_curr, in bits
        assert end.sum() > 900 or name != "shifted"
        assert up.same_bits(got[end], reg.pointcloudAssociateToMap(cloud, pc)[end]), name
    print(f"{case}: {unequal} of {total} coordinates unequal to the reference's")
    if case in ("w_plus", "w_minus"):
        assert np.abs(reg.pointcloudAssociateToMap(s["surface"], if_undistore=1)[:, :3] - reg.pointcloudAssociateToMap(s["surface"], pc)[:, :3]).max() > 1e-2
