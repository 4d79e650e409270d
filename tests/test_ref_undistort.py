"""The undistort branch (point_cloud_registration.hpp:607-661) against the REFERENCE'S OWN CLASS compiled here (oracle/_ref/libll_ref.so,
`make -C oracle ref`; taps ref_reg_get_state / _set_state / _compute_interp / _cloud_associate of oracle/ref_shim.cpp).

  * the host build of csrc/ll_reg_core.h (tests/undistort_host.cpp: interp_rodrigues, point_to_map_undistort -- the text the kernels run)
    and the oracle's exports (orc_compute_interp, orc_cloud_associate) equal the reference IN BITS: all three are g++ / gcc
    -ffp-contract=off builds of the same operations against the same libm;
  * the float64 numpy restatement tests/undistort_ref.py, the yardstick of tests/test_gpu_undistort.py, is held to the same reference
    outputs under its own rule (numpy's sin / cos: one fp32 ulp, 1 in 10 000 unequal);
  * a registration started from an increment with w < 0, and the state a rejected and a gated registration leave behind.

Angles below ~1e-154: Eigen falls back to stableNorm() where |vec| < epsilon; the stand-in Eigen's stableNorm is norm(), which
underflows to 0 there, so those inputs take the `n == 0` branch (theta 0, axis x) on all sides.  They pin the sides to each other and
to the stand-in, not to Eigen's scaled norm.

Skipped where the library is neither built nor buildable; tests/test_ref_undistort_golden.py then still holds the committed outputs."""
import numpy as np
import pytest

from loam_livox_amd import synth
from oracle import orc, ref
from tests import undistort_pin as up
from tests import undistort_ref as ur

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built and /root/reference absent")

MIN_TS, MAX_TS = 0.25, 0.35


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return up.build_host_lib(tmp_path_factory.mktemp("ref_undistort"))


@pytest.fixture(scope="module")
def R():
    return ref.RefRegistration()


@pytest.fixture(scope="module")
def trees():
    s = up.scene()
    return orc.KdTree(s["corner_map"]), orc.KdTree(s["surf_map"])


# ------------------------------------------------------------------------------------------------ interpolation state
def quaternions():
    """A few thousand q = (x, y, z, w): angles from 1e-300 to 2 pi, half of them with w < 0, a fifth not of unit length, and
    vec == 0 with w = +-1"""
    rng = np.random.default_rng(607)
    out = [np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.0, 0.0, 0.0, -1.0]), np.array([0.0, 0.0, 0.0, 0.0]), np.array([0.0, -0.0, 0.0, -0.5])]
    angles = np.r_[10.0 ** rng.uniform(-300, 0, 1500), rng.uniform(0, 2 * np.pi, 1500), 1e-300, 1e-160, 1e-154, 1e-16, np.pi, 2 * np.pi]
    for k, a in enumerate(angles):
        axis = rng.normal(size=3)
        if k % 7 == 0:
            axis[rng.integers(0, 3)] = 0.0    # an axis in a coordinate plane: signed zeros in the matrix
        axis /= np.linalg.norm(axis)
        q = np.r_[np.sin(a / 2) * axis, np.cos(a / 2)]   # angles past pi give w < 0 of themselves
        if k % 2:
            q = -q
        if k % 5 == 0:
            q = q * rng.uniform(0.3, 3.0)
        out.append(q)
    return out


def test_interpolation_state_in_bits(host, R):
    qs = quaternions()
    assert len(qs) > 3000 and sum(q[3] < 0 for q in qs) > 1000 and sum(abs(np.linalg.norm(q) - 1) > 0.05 for q in qs) > 500
    unequal = {"host build": 0, "oracle": 0}
    for q in qs:
        want = R.compute_interp(q)
        for name, got in (("host build", up.host_interp(host, q)), ("oracle", orc.compute_interp(q))):
            same = up.same_bits(np.float64(got[0]), np.float64(want[0])) and up.same_bits(got[1], want[1]) and up.same_bits(got[2], want[2])
            unequal[name] += not same
        assert want[0] >= 0.0   # Eigen's angle is never negative: w < 0 turns the axis
    print(f"interpolation state: {unequal} of {len(qs)} quaternions unequal in any bit")
    assert unequal == {"host build": 0, "oracle": 0}


def test_numpy_restatement_of_the_state(R):
    """tests/undistort_ref.py interp under the tolerance tests/test_undistort_host.py holds the host build to against it: numpy's
    arctan2 and norm are other implementations (4 fp64 ulps of the values' scale)"""
    eps = 2.0 ** -52
    for q in quaternions()[::3]:
        theta, hat, hat_sq = R.compute_interp(q)
        r_theta, r_hat = ur.interp(q)
        assert abs(theta - r_theta) <= 4 * eps * abs(theta), q
        assert np.abs(hat - r_hat).max() <= 4 * eps and np.abs(hat_sq - r_hat @ r_hat).max() <= 8 * eps, q


# ------------------------------------------------------------------------------------------------ deskew
def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def make_state(rng, angle, shift, negative_w, axis_in_plane=False):
    """pose_last far from the origin, an increment of `angle` rad / `shift` m (q or -q), pose_curr = pose_last o increment"""
    pose_last = np.r_[ur.quat_from_rotvec(rng.normal(size=3) * 0.7), rng.uniform(-30, 30, 3)]
    axis = rng.normal(size=3)
    if axis_in_plane:
        axis[1] = 0.0    # zeros, and their signs, in hat and hat_sq
    inc = np.r_[ur.quat_from_rotvec(axis / np.linalg.norm(axis) * angle), rng.normal(size=3) / np.sqrt(3) * shift]
    if negative_w:
        inc[:4] = -inc[:4]
    pose_curr = np.r_[q_mul(pose_last[:4], inc[:4]), ur.quat_to_mat(pose_last[:4]) @ inc[4:] + pose_last[4:]]
    return pose_last, pose_curr, inc


def make_points(rng, n):
    """stamps below the range (s < 0), inside it, on both ends, above it, and NaN / inf; a few non-finite coordinates"""
    xyzi = np.zeros((n, 4), np.float32)
    xyzi[:, :3] = rng.uniform(-50, 50, (n, 3))
    xyzi[:, 3] = rng.uniform(MIN_TS - 0.1, MAX_TS + 0.1, n)
    xyzi[0::50, 3] = MAX_TS
    xyzi[1::50, 3] = MIN_TS
    xyzi[2::50, 3] = np.nan
    xyzi[3::250, 3] = np.inf
    xyzi[4::250, 3] = -np.inf
    xyzi[7::100, 0] = np.nan
    xyzi[8::100, 1] = np.inf
    xyzi[9::100, 2] = -np.inf
    return xyzi


STATES = [(angle, shift, neg, False) for angle, shift in ((1e-6, 1e-4), (1e-3, 0.01), (0.02, 0.1), (0.3, 0.5), (1.5, 1.0), (3.0, 2.0)) for neg in (0, 1)]
STATES += [(0.1, 0.2, 0, True), (0.1, 0.2, 1, True)]
# (deblur, if_undistore, min_ts, max_ts): the undistort branch; min_ts == max_ts (0/0, x/0 -> s = 1); deblur off; the plain branch with deblur on
SWITCHES = [(1, 1, MIN_TS, MAX_TS), (1, 1, MAX_TS, MAX_TS), (0, 1, MIN_TS, MAX_TS), (1, 0, MIN_TS, MAX_TS)]


def finite_rows(a):
    return np.isfinite(a[:, :3]).all(axis=1)


def test_deskew_in_bits_and_the_numpy_restatement_under_its_rule(host, R):
    n = 25_000
    n_coord = {"host build": 0, "oracle": 0, "numpy restatement": 0}
    total = 0
    for k, (angle, shift, neg, in_plane) in enumerate(STATES):
        rng = np.random.default_rng(622 + k)
        pose_last, pose_curr, inc = make_state(rng, angle, shift, neg, in_plane)
        theta, hat, hat_sq = R.compute_interp(inc[:4])
        assert (inc[3] < 0) == bool(neg) and theta > 0
        xyzi = make_points(rng, n)
        s = ur.blur_ratio(xyzi[:, 3], 1, MIN_TS, MAX_TS)
        assert (s < 0).sum() > n // 5 and (s == 1).sum() > n // 5 and ((s > 0) & (s < 1)).sum() > n // 5 and (s == 0).sum() >= n // 50
        for deblur, if_undistore, lo, hi in SWITCHES:
            R.set_state(theta, hat, hat_sq, inc, pose_last, pose_curr, deblur, lo, hi)
            st = R.state()
            assert st["theta"] == theta and up.same_bits(st["omega_hat"], hat) and up.same_bits(st["pose_curr"], pose_curr)   # the taps round-trip
            want = R.cloud_associate(xyzi, if_undistore)
            assert up.same_bits(want[:, 3], xyzi[:, 3])                                   # intensity copied, PCR:659
            ok = finite_rows(xyzi)
            assert not np.isfinite(want[~ok, :3]).all(axis=1).any() and np.isfinite(want[ok, :3]).all()   # NaN in, NaN out; no rule of their own
            what = f"{angle} rad / {shift} m, w {'<' if neg else '>'} 0, deblur {deblur}, if_undistore {if_undistore}, range {lo}..{hi}"
            orc_out = orc.cloud_associate(xyzi, pose_last, pose_curr, inc, theta, hat, hat_sq, deblur, lo, hi, if_undistore)
            assert up.same_bits(orc_out[:, 3], xyzi[:, 3])
            n_o = int((up.bits(orc_out[:, :3]) != up.bits(want[:, :3])).sum())
            n_coord["oracle"] += n_o
            # the host build has no if_undistore argument: the plain branch of PCR:627 is its deblur = 0
            got = up.host_undistort(host, xyzi, pose_last, pose_curr, inc[4:], theta, hat, hat_sq, deblur and if_undistore, lo, hi)
            assert up.same_bits(got[:, 3], xyzi[:, 3])
            n_h = int((up.bits(got[:, :3]) != up.bits(want[:, :3])).sum())
            n_coord["host build"] += n_h
            assert n_o == 0 and n_h == 0, (what, n_o, n_h)
            if not (deblur and if_undistore and lo != hi):   # every point takes the pose_curr branch: the plain transform, in bits
                assert up.same_bits(want, R.cloud_transform(pose_curr, xyzi)), what
            restated = ur.undistort(xyzi[ok], pose_last, pose_curr, inc, *ur.interp(inc[:4]), deblur and if_undistore, lo, hi)
            n_coord["numpy restatement"] += ur.check_rule(want[ok, :3], restated, "numpy restatement against the reference, " + what)
            total += 3 * n
        # the undistort branch did something: below 0.02 rad / 0.1 m the plain transform is within a centimetre, above it is not
        R.set_state(theta, hat, hat_sq, inc, pose_last, pose_curr, 1, MIN_TS, MAX_TS)
        moved = np.abs(R.cloud_associate(xyzi[ok], 1)[:, :3] - R.cloud_transform(pose_curr, xyzi[ok])[:, :3]).max()
        assert moved > 1e-2 if angle >= 0.02 else moved > 0
    print(f"deskewed coordinates unequal to the reference's: {n_coord} of {total}")


def test_points_that_take_the_end_of_scan_pose(R):
    """s == 1 (the stamp on max_ts), s > 1 and a NaN stamp (PCR:134) equal pointcloudAssociateToMap( ., ., 0 ) in bits; s == 0 does not:
    it is pose_last through the identity matrix"""
    rng = np.random.default_rng(627)
    pose_last, pose_curr, inc = make_state(rng, 0.3, 0.5, 1)
    theta, hat, hat_sq = R.compute_interp(inc[:4])
    xyzi = make_points(rng, 4000)
    xyzi = xyzi[finite_rows(xyzi)]
    R.set_state(theta, hat, hat_sq, inc, pose_last, pose_curr, 1, MIN_TS, MAX_TS)
    s = ur.blur_ratio(xyzi[:, 3], 1, MIN_TS, MAX_TS)
    out, plain = R.cloud_associate(xyzi, 1), R.cloud_associate(xyzi, 0)
    end = s == 1
    assert np.isnan(xyzi[end, 3]).sum() > 50 and (xyzi[end, 3] > MAX_TS).sum() > 500 and (xyzi[end, 3] == np.float32(MAX_TS)).sum() > 50
    assert up.same_bits(out[end], plain[end]) and up.same_bits(plain, R.cloud_transform(pose_curr, xyzi))
    assert np.abs(out[~end, :3] - plain[~end, :3]).max() > 1e-2
    at_start = s == 0
    assert at_start.sum() > 50
    ur.check_rule(out[at_start, :3], ur.plain(pose_last, xyzi[at_start]), "s == 0 against the plain transform with pose_last")


# ------------------------------------------------------------------------------------------------ registrations
def run_reference(case):
    s = up.scene()
    RR = ref.RefRegistration()
    RR.set_params(up.case_params(case))
    RR.set_maps(s["corner_map"], s["surf_map"])
    ret, pc, pi, rep = RR.solve(s["corners"], s["surface"], s["pose_init"], s["pose_init"], up.start_increment(case))
    return RR, (ret, pc, pi, rep)


def run_oracle(case, trees):
    s = up.scene()
    ret, pc, pi, rep, st = orc.reg_solve_state(trees[0], trees[1], s["corners"], s["surface"], up.case_params(case), s["pose_init"], s["pose_init"],
                                               up.start_increment(case))
    return (ret, pc, pi, rep), st


def assert_same_registration(r, o, tol=1e-9):
    """tests/test_ref_pin.py's tolerances for a deblur registration"""
    (ret_r, pc_r, pi_r, rep_r), (ret_o, pc_o, pi_o, rep_o) = r, o
    assert ret_r == ret_o
    dt, dr = synth.pose_error(pc_r, pc_o)
    assert dt < tol and dr < tol, (dt, dr)
    assert np.allclose(pi_r, pi_o, rtol=0, atol=tol)
    if not rep_o.gated:
        assert rep_r["n_blocks_last"] == rep_o.n_blocks_last
        assert abs(rep_r["final_cost"] - rep_o.final_cost) <= 1e-9 * max(1.0, rep_o.final_cost)
        assert abs(rep_r["initial_cost"] - rep_o.initial_cost) <= 1e-9 * max(1.0, rep_o.initial_cost)
        assert abs(rep_r["inlier_threshold"] - rep_o.inlier_threshold) <= 1e-9
        assert abs(rep_r["angular_diff_deg"] - rep_o.angular_diff_deg) <= 1e-5
        assert abs(rep_r["t_diff"] - rep_o.t_diff) <= 1e-9


def assert_state(host, RR, oracle_state, tol=1e-9):
    """The reference object's state: the host build and the oracle's export make it from the object's increment in bits (zero before a
    first solve); the oracle's registration leaves the same state within the registration's tolerance."""
    st = RR.state()
    if not (st["omega_hat"].any() or st["theta"]):
        assert not st["omega_hat_sq2"].any() and not oracle_state["theta"] and not oracle_state["omega_hat"].any() and not oracle_state["omega_hat_sq2"].any()
        return st
    for got in (up.host_interp(host, st["pose_incre"][:4]), orc.compute_interp(st["pose_incre"][:4])):
        assert got[0] == st["theta"] and up.same_bits(got[1], st["omega_hat"]) and up.same_bits(got[2], st["omega_hat_sq2"])
    assert abs(oracle_state["theta"] - st["theta"]) < tol
    assert np.abs(oracle_state["omega_hat"] - st["omega_hat"]).max() < 1e-6   # the axis of an angle theta carries the increment's error / theta
    return st


def test_registration_from_an_increment_with_negative_w(host, trees):
    """(0,0,0,-1, 0,0,0) is the identity rotation.  The reference ends on the pose of the w = +1 run exactly, with the increment's
    quaternion negated; an oracle that negates |vec| before the atan2 (the order before this test) interpolates the inverse rotation in
    every search after the first iteration and ends 0.19 m / 0.036 rad away."""
    s = up.scene()
    Rp, plus = run_reference("w_plus")
    Rm, minus = run_reference("w_minus")
    assert plus[0] == 1 and synth.pose_error(plus[1], s["pose_out"]) == (0.0, 0.0) and plus[3]["n_blocks_last"] == s["n_blocks_last"]
    assert minus[0] == 1 and np.array_equal(minus[1][4:], plus[1][4:]) and synth.pose_error(minus[1], plus[1]) == (0.0, 0.0)
    assert np.array_equal(minus[2][:4], -plus[2][:4]) and np.array_equal(minus[2][4:], plus[2][4:]) and minus[2][3] < 0
    assert minus[3]["n_blocks_last"] == plus[3]["n_blocks_last"]
    sp, sm = Rp.state(), Rm.state()
    assert sm["theta"] == sp["theta"] > 1e-4 and up.same_bits(sm["omega_hat"], sp["omega_hat"]) and up.same_bits(sm["omega_hat_sq2"], sp["omega_hat_sq2"])
    for case, RR, r in (("w_plus", Rp, plus), ("w_minus", Rm, minus)):
        o, ost = run_oracle(case, trees)
        print(case, "oracle against the reference: pose", synth.pose_error(o[1], r[1]), "increment", np.abs(o[2] - r[2]).max(),
              "theta", abs(ost["theta"] - RR.state()["theta"]))
        assert_same_registration(r, o)
        assert_state(host, RR, ost)


def test_deskewed_clouds_of_the_registered_scene(host):
    """the scene's own clouds with the state its registration left, both signs of w: host build and oracle in bits"""
    s = up.scene()
    for case in ("w_plus", "w_minus"):
        RR, (ret, pc, pi, rep) = run_reference(case)
        st = RR.state()
        assert up.same_bits(st["pose_curr"], pc) and up.same_bits(st["pose_incre"], pi) and up.same_bits(st["pose_last"], s["pose_init"])
        for name in up.CLOUDS:
            want = RR.cloud_associate(s[name], 1)
            args = (st["theta"], st["omega_hat"], st["omega_hat_sq2"], 1, s["t_min"], s["t_max"])
            assert up.same_bits(orc.cloud_associate(s[name], st["pose_last"], pc, pi, *args), want), (case, name)
            assert up.same_bits(up.host_undistort(host, s[name], st["pose_last"], pc, pi[4:], *args), want), (case, name)
            up.check_rule(ur.undistort(s[name], st["pose_last"], pc, pi, *ur.interp(pi[:4]), 1, s["t_min"], s["t_max"]).astype(np.float32), want,
                          f"{case} {name}: numpy restatement")


def test_state_after_a_rejected_registration(host, trees):
    """PCR:561-573 restores the pose and nothing else: the increment of the last iteration and its state stay in the object"""
    s = up.scene()
    RR, r = run_reference("rejected")
    _, accepted = run_reference("w_plus")
    o, ost = run_oracle("rejected", trees)
    assert r[0] == 0 and up.same_bits(r[1], s["pose_init"]) and up.same_bits(r[2], accepted[2])   # the same solve, then the cost gate
    assert_same_registration(r, o)
    st = assert_state(host, RR, ost)
    assert st["theta"] > 1e-4 and up.same_bits(st["pose_curr"], st["pose_last"]) and up.same_bits(st["pose_last"], s["pose_init"])
    # what a deskew of this object gives: interpolated from pose_last with the kept increment; s == 1 at pose_curr = pose_last
    want = RR.cloud_associate(s["shifted"], 1)
    args = (st["theta"], st["omega_hat"], st["omega_hat_sq2"], 1, s["t_min"], s["t_max"])
    assert up.same_bits(orc.cloud_associate(s["shifted"], st["pose_last"], st["pose_curr"], st["pose_incre"], *args), want)
    assert up.same_bits(up.host_undistort(host, s["shifted"], st["pose_last"], st["pose_curr"], st["pose_incre"][4:], *args), want)


@pytest.mark.parametrize("exit_", ["frame_index", "small_map"])
def test_state_after_the_exits_that_return_before_a_solve(host, trees, exit_):
    """PCR:199: current_frame_index not past mapping_init_accumulate_frames, or a surface map of no more than 50 points: 1, the poses
    as the node set them (LM:1290-1294), the increment as given, the state of a fresh object (zero, as the shim defines it)"""
    s = up.scene()
    prm = up.case_params("gated" if exit_ == "frame_index" else "w_plus")
    surf_map = s["surf_map"] if exit_ == "frame_index" else s["surf_map"][:50]
    RR = ref.RefRegistration()
    RR.set_params(prm)
    RR.set_maps(s["corner_map"], surf_map)
    r = RR.solve(s["corners"], s["surface"], s["pose_init"], s["pose_init"], up.IDENT)
    tree_s = trees[1] if exit_ == "frame_index" else orc.KdTree(surf_map)
    ret, pc, pi, rep, ost = orc.reg_solve_state(trees[0], tree_s, s["corners"], s["surface"], prm, s["pose_init"], s["pose_init"], up.IDENT)
    assert r[0] == 1 and ret == 1 and rep.gated == 1
    assert up.same_bits(r[1], s["pose_init"]) and up.same_bits(pc, s["pose_init"]) and up.same_bits(r[2], up.IDENT) and up.same_bits(pi, up.IDENT)
    st = assert_state(host, RR, ost)
    assert st["theta"] == 0.0 and not st["omega_hat"].any()
    # the deskew of such an object: the identity matrix and a zero shift from pose_last, exact -- the plain transform in bits
    want = RR.cloud_associate(s["shifted"], 1)
    z = np.zeros((3, 3))
    assert up.same_bits(want, RR.cloud_transform(s["pose_init"], s["shifted"]))
    assert up.same_bits(up.host_undistort(host, s["shifted"], st["pose_last"], st["pose_curr"], np.zeros(3), 0.0, z, z, 1, s["t_min"], s["t_max"]), want)
    assert up.same_bits(orc.cloud_associate(s["shifted"], st["pose_last"], st["pose_curr"], up.IDENT, 0.0, z, z, 1, s["t_min"], s["t_max"]), want)
