"""CPU tier of the registration information (ll_reg_information; tests/test_gpu_reg_information.py is the GPU tier).

tests/reg_info_host.cpp compiles loam_livox_amd/csrc/ll_reg_info_core.h -- the text reg_information_kernel runs -- with g++ -ffp-contract=off
and walks the kernel's 256 thread loops and its reduction order serially.  The yardstick is the oracle (tests/reg_info_inputs.py): blocks made
by orc.make_block_line / make_block_plane from the same neighbour points, summed by orc.blocks_eval at the same evaluation point."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from loam_livox_amd import api, capi, mapping, synth
from tests import reg_info_inputs as ri

ROOT = ri.ROOT
HEADER = os.path.join(ROOT, "include", "loam_livox_hip.h")
NEW_SYMBOLS = ("ll_reg_set_information", "ll_reg_information", "ll_reg_information_time")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("reg_info")
    return ri.build_driver(str(d / "reg_info_host")), str(d)


def check_against_oracle(exe, tmp, case):
    rec = ri.run_info(exe, tmp, case)
    ref = ri.oracle_record(case["blocks"], case["pose_last"], case["x"], deblur=case["deblur"], huber_a=case["huber_a"])
    assert rec["status"] == 0 and (rec["n_line"], rec["n_plane"]) == (case["n_line"], case["n_plane"])
    assert ref["n"] == case["n_line"] + case["n_plane"]
    worst = ri.worst_ratio(rec, ref)
    print(f"n_line {rec['n_line']} n_plane {rec['n_plane']} deblur {case['deblur']}: worst |v - v_orc| / bound = {worst:.3g}")
    assert worst <= 1.0
    assert np.array_equal(rec["H"], rec["H"].T)
    return rec, ref


# candidate counts at every thread-count and wavefront boundary of the kernel (64-lane wavefronts, 256 threads), and beyond one round
COUNTS = (1, 63, 64, 65, 255, 256, 257, 2049)


@pytest.mark.parametrize("deblur", [0, 1])
@pytest.mark.parametrize("n", COUNTS)
def test_record_equals_the_oracles_sum(driver, n, deblur):
    exe, tmp = driver
    check_against_oracle(exe, tmp, ri.make_case(100 + n, n // 3, n - n // 3, deblur=deblur))


@pytest.mark.parametrize("deblur", [0, 1])
@pytest.mark.parametrize("n", (65, 257))
def test_lines_only_and_planes_only(driver, n, deblur):
    exe, tmp = driver
    check_against_oracle(exe, tmp, ri.make_case(200 + n, n, 0, deblur=deblur))
    check_against_oracle(exe, tmp, ri.make_case(300 + n, 0, n, deblur=deblur))


def test_empty_scan_gated_aborted_and_iterationless_scans_have_zero_records(driver):
    exe, tmp = driver
    for case, kw, status in ((ri.make_case(1, 0, 0), {}, 1), (ri.make_case(2, 5, 9), dict(gated=1), 1), (ri.make_case(2, 5, 9), dict(icp_iters=0), 1),
                             (ri.make_case(2, 5, 9), dict(aborted=1), 2), (ri.make_case(2, 5, 9), dict(aborted=1, gated=1), 2)):
        rec = ri.run_info(exe, tmp, case, **kw)
        assert rec["status"] == status and rec["n_line"] == 0 and rec["n_plane"] == 0
        assert not rec["H"].any() and not rec["g"].any() and rec["cost"] == 0.0


@pytest.mark.parametrize("deblur", [0, 1])
def test_non_active_candidates_do_not_enter(driver, deblur):
    """non-finite features, candidates without five neighbours, a degenerate triple and a degenerate line are mixed in between the blocks
    (their neighbour positions point outside the map: never dereferenced), and the slots beyond the scan carry active flags"""
    exe, tmp = driver
    case = ri.make_case(7, 40, 90, deblur=deblur, inactive=True)
    assert case["n_corner"] > case["n_line"] + 10 and case["n_surf"] > case["n_plane"] + 30
    rec, _ = check_against_oracle(exe, tmp, case)
    plain = ri.make_case(7, 40, 90, deblur=deblur, inactive=False)
    assert (rec["n_line"], rec["n_plane"]) == (plain["n_line"], plain["n_plane"]) == (40, 90)


def test_a_wall_leaves_three_directions_exactly_unconstrained(driver):
    """every map point has z == 0 exactly, plane blocks only: rotation about z and translation along x and y are products with an exact
    zero in every term; the other three directions are constrained"""
    exe, tmp = driver
    case = ri.make_case(11, 0, 300, wall=True)
    assert not case["map_s"][:, 2].any()
    rec = ri.run_info(exe, tmp, case)
    H = rec["H"]
    free, held = [2, 3, 4], [0, 1, 5]
    # (the oracle sums in the map frame, where these zeros are roundings of size 1e-17: it is the yardstick of the constrained block)
    ref = ri.oracle_record(case["blocks"], case["pose_last"], case["x"])
    assert (rec["n_line"], rec["n_plane"], rec["status"]) == (0, 300, 0) and ri.worst_ratio(rec, ref, rows=held) <= 1.0
    assert np.abs(ref["H"][free, :]).max() <= 1e-12 * np.abs(ref["H"]).max()
    assert np.all(H[free, :] == 0.0) and np.all(H[:, free] == 0.0) and np.all(rec["g"][free] == 0.0)
    assert np.all(np.linalg.eigvalsh(H[np.ix_(held, held)]) > 0.0)
    w, v = np.linalg.eigh(H)
    assert np.abs(w[:3]).max() <= 2.0 ** -52 * w[-1] and np.all(w[3:] > 0.0)


# ------------------------------------------------------------------------------------------------ the pose's own frame
def _q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def _log_so3(R):
    """rotation vector of a rotation matrix close to the identity"""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v)
    return v if s < 1e-300 else v * (np.arcsin(min(1.0, s)) / s)


def _pose_step(pose_last, inc, d):
    """xi = [dt_map; theta_map]: how the composed pose pose_last o inc moves when the solver steps by d = [d_rot; d_t]"""
    def compose(x):
        return synth.quat_to_mat(pose_last[:4]) @ synth.quat_to_mat(x[:4]), synth.quat_to_mat(pose_last[:4]) @ x[4:] + pose_last[4:]
    nd = np.linalg.norm(d[:3])
    dq = np.r_[np.sin(nd) * d[:3] / nd, np.cos(nd)] if nd > 0 else np.array([0, 0, 0, 1.0])  # EigenQuaternionParameterization::Plus
    R0, t0 = compose(inc)
    R1, t1 = compose(np.r_[_q_mul(dq, inc[:4]), inc[4:] + d[3:]])
    return np.r_[t1 - t0, _log_so3(R1 @ R0.T)]


def test_information_in_pose_frame_against_central_differences(driver):
    """T = d xi / d d by central differences of the pose composition at two step sizes; T^T H_pose T must give H back, up to the
    differences' own error.  Along one axis of the tangent the composition is EXACTLY linear -- R_last Exp(2 h e) R_inc (R_last R_inc)^T =
    Exp(2 h R_last e), and the translation is linear in d_t -- so a central difference has no truncation error here; what it has is
    rounding: the two composed poses carry ~16 ulp of the pose's largest coordinate each, divided by 2 h.  An entry of T is therefore
    off by at most dT = 16 eps (|t|_max + 1) / (2 h), and an entry of T^T H_pose T by 2 * 36 * dT * |T|_max * |H_pose|_max <= 144 dT |H|_max
    (|T| <= 2, |H_pose| <= |H|).  Both step sizes are held to that; a wrong factor, sign or block order is off by O(1) at either."""
    exe, tmp = driver
    rng = np.random.default_rng(3)
    pose_last = np.r_[synth.quat_from_axis_angle(rng.normal(size=3), 1.1), rng.uniform(-20, 20, 3)]
    inc = np.r_[synth.quat_from_axis_angle(rng.normal(size=3), 0.05), rng.uniform(-0.2, 0.2, 3)]
    J = rng.normal(size=(40, 6))
    H = J.T @ J
    Hp = api.information_in_pose_frame(H, pose_last)
    assert np.allclose(Hp, Hp.T, rtol=0, atol=1e-12 * np.abs(Hp).max())
    errs = []
    for h in (1e-2, 1e-3):
        T = np.zeros((6, 6))
        for j in range(6):
            e = np.zeros(6)
            e[j] = h
            T[:, j] = (_pose_step(pose_last, inc, e) - _pose_step(pose_last, inc, -e)) / (2 * h)
        back = T.T @ Hp @ T
        errs.append(np.abs(back - H).max() / np.abs(H).max())
        dT = 16 * 2.0 ** -52 * (np.abs(pose_last[4:]).max() + 1.0) / (2 * h)
        assert errs[-1] <= 144 * dT
        assert np.allclose(T[:3, 3:], synth.quat_to_mat(pose_last[:4]), atol=dT) and np.allclose(T[3:, :3], 2 * synth.quat_to_mat(pose_last[:4]), atol=dT)
        assert np.abs(T[:3, :3]).max() <= dT and np.abs(T[3:, 3:]).max() <= dT
    print("information_in_pose_frame: relative error of T^T H_pose T against H at h = 1e-2, 1e-3:", errs)
    # the adapter's function is the same arithmetic
    Ha = ri.run_pose_frame(exe, tmp, [H], [pose_last])[0]
    assert np.allclose(Ha, Hp, rtol=0, atol=64 * 2.0 ** -52 * np.abs(Hp).max())
    # identity pose: translation block <- H_tt, rotation block <- H_rr / 4
    H0 = api.information_in_pose_frame(H, [0, 0, 0, 1, 0, 0, 0])
    assert np.array_equal(H0[:3, :3], H[3:, 3:]) and np.array_equal(H0[3:, 3:], 0.25 * H[:3, :3]) and np.array_equal(H0[:3, 3:], 0.5 * H[3:, :3])


# ------------------------------------------------------------------------------------------------ the adapter's Jacobi
def eigen_matrices(driver):
    exe, tmp = driver
    rng = np.random.default_rng(5)
    mats = [ri.run_info(exe, tmp, ri.make_case(40 + k, 30, 70, deblur=k % 2))["H"] for k in range(3)]
    mats.append(ri.run_info(exe, tmp, ri.make_case(11, 0, 300, wall=True))["H"])      # three exact zeros
    Q = np.linalg.qr(rng.normal(size=(6, 6)))[0]
    mats.append(Q @ np.diag([2.0, 2.0, 2.0, 5.0, 5.0, 7.0]) @ Q.T)                   # repeated
    mats.append(Q @ np.diag([0.0, 0.0, 1.0, 1.0, 1e6, 1e6]) @ Q.T)                   # repeated and zero, six decades
    mats += [np.zeros((6, 6)), np.eye(6), np.diag([6.0, 5, 4, 3, 2, 1])]
    mats.append(Q @ np.diag([1e-9, 1e-3, 1.0, 1e3, 1e6, 1e9]) @ Q.T)
    return [0.5 * (m + m.T) for m in mats]


def test_adapter_jacobi_against_numpy_eigh(driver):
    """eigenvalues within 64 2^-52 |H|_2 (the backward error of a Jacobi sweep times Weyl's bound); vectors by their residual and
    orthonormality under the same bound, never entry by entry"""
    exe, tmp = driver
    mats = eigen_matrices(driver)
    w, V, sweeps = ri.run_eigen(exe, tmp, mats)
    for H, wk, Vk, sw in zip(mats, w, V, sweeps):
        norm = np.linalg.norm(H, 2)
        tol = 64 * 2.0 ** -52 * norm
        ref = np.linalg.eigh(H)[0]
        assert np.all(np.diff(wk) >= 0) and sw < 20
        assert np.abs(wk - ref).max() <= tol
        assert np.abs(H @ Vk - Vk * wk).max() <= tol if norm > 0 else not np.abs(H @ Vk).any()
        assert np.abs(Vk.T @ Vk - np.eye(6)).max() <= 64 * 2.0 ** -52


# ------------------------------------------------------------------------------------------------ the driver once more, sanitised
def test_driver_under_address_and_undefined_behaviour_sanitizers(driver, tmp_path):
    """a stand-alone program, never code loaded into Python"""
    _, tmp = driver
    exe = ri.build_driver(str(tmp_path / "reg_info_host_san"), extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for case in (ri.make_case(7, 40, 90, deblur=1, inactive=True), ri.make_case(8, 0, 0), ri.make_case(9, 100, 157)):
        plain, san = ri.run_info(driver[0], tmp, case), ri.run_info(exe, str(tmp_path), case)
        assert np.array_equal(plain["H"], san["H"]) and np.array_equal(plain["g"], san["g"]) and plain["cost"] == san["cost"]
    ri.run_eigen(exe, str(tmp_path), eigen_matrices(driver))


# ------------------------------------------------------------------------------------------------ symbols and refusals
def test_new_symbols_are_declared_exported_and_bound():
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in capi.SYMBOLS and capi.SYMBOLS[name][0] is C.c_int32
    assert "ll_reg_information_record;" in text
    assert C.sizeof(capi.RegInformation) == 43 * 8 + 16
    L = capi.load()   # (binds every symbol of capi.SYMBOLS, or raises)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(NEW_SYMBOLS) <= exported and all(hasattr(L, n) for n in NEW_SYMBOLS)


def test_null_handle_refusals_carry_their_text_without_a_device():
    L = capi.load()
    rec = capi.RegInformation()
    ms = C.c_float(0)
    for call, fn in ((lambda: L.ll_reg_set_information(None, 1), "ll_reg_set_information"),
                     (lambda: L.ll_reg_information(None, 1, C.byref(rec)), "ll_reg_information"),
                     (lambda: L.ll_reg_information_time(None, C.byref(ms)), "ll_reg_information_time")):
        rc = call()
        msg = L.ll_last_error().decode()
        assert rc != 0 and fn in msg and "null handle" in msg, (rc, msg)


# ------------------------------------------------------------------------------------------------ the loops over stub handles
class Stub:
    """a handle that records every method call in `log` and answers with what `answers` holds for it"""

    def __init__(self, log, name, answers=None):
        self._log, self._name, self._answers = log, name, answers or {}
        self.params = types.SimpleNamespace()
        self.debug_flags = 0

    def __getattr__(self, method):
        if method.startswith("__"):
            raise AttributeError(method)

        def call(*a, **k):
            self._log.append((self._name, method))
            ans = self._answers.get(method)
            return ans(*a, **k) if callable(ans) else ans
        return call


def stub_world(monkeypatch, S, aborted_first=False):
    log = []
    state = dict(collects=0)

    def report(aborted):
        r = capi.RegReport()
        r.accepted, r.aborted = 1, int(aborted)
        return r

    def collect(n):
        state["collects"] += 1
        ab = aborted_first and state["collects"] == 1
        pc = np.tile(np.array([0, 0, 0, 1, 0.1 * state["collects"], 0, 0], np.float64), (n, 1))
        return np.ones(n, np.int32), pc, pc.copy(), [report(ab and s == 0) for s in range(n)]

    def information(n):
        return [dict(H=np.eye(6) * (10 * state["collects"] + s + 1), g=np.zeros(6), cost=0.0, n_line=1, n_plane=2, status=0,
                     eigenvalues=np.full(6, 10.0 * state["collects"] + s + 1), eigenvectors=np.eye(6)) for s in range(n)]

    reg = dict(collect=collect, information=information)
    hist = dict(add_voxel=True, refresh=(1, 2))
    for cls, answers in (("Livox_laser", {}), ("Point_cloud_registration", reg), ("Map_buffer", {}), ("VoxelGrid", {}), ("History_buffer", hist)):
        monkeypatch.setattr(mapping, cls, lambda *a, _c=cls, _an=answers, **k: Stub(log, _c, _an))
    return log


def reg_calls(log):
    return [m for c, m in log if c == "Point_cloud_registration" and m in ("set_information", "information", "collect")]


@pytest.mark.parametrize("information", [False, True])
def test_laser_mapping_over_stub_handles(monkeypatch, information):
    log = stub_world(monkeypatch, 1)
    lm = mapping.Laser_mapping(scan_points=1000, information=information)
    assert reg_calls(log) == (["set_information"] if information else [])
    scan = np.zeros((10, 4), np.float32)
    for _ in range(3):
        assert lm.process_new_scan(scan) == 1
    if not information:
        assert reg_calls(log) == ["collect"] * 3 and lm.last_information is None
        with pytest.raises(RuntimeError):
            lm.degenerate_directions(1.0)
        return
    assert reg_calls(log) == ["set_information"] + ["collect", "information"] * 3
    info = lm.last_information
    assert info["H"][0, 0] == 31.0 and info["H_pose"].shape == (6, 6) and info["n_plane"] == 2
    assert np.array_equal(info["H_pose"], api.information_in_pose_frame(info["H"], [0, 0, 0, 1, 0.2, 0, 0]))   # the pose before the frame
    assert lm.degenerate_directions(31.5).shape == (6, 6) and lm.degenerate_directions(31.0).shape == (0, 6)


def test_laser_mapping_repeat_of_an_aborted_registration_replaces_the_record(monkeypatch):
    log = stub_world(monkeypatch, 1, aborted_first=True)
    lm = mapping.Laser_mapping(scan_points=1000, information=True)
    assert lm.process_new_scan(np.zeros((10, 4), np.float32)) == 1 and lm.aborted_solves == 1
    assert reg_calls(log) == ["set_information", "collect", "information", "collect", "information"]
    assert lm.last_information["H"][0, 0] == 21.0   # the second collect's


@pytest.mark.parametrize("information", [False, True])
def test_laser_mapping_batch_over_stub_handles(monkeypatch, information):
    S = 3
    log = stub_world(monkeypatch, S, aborted_first=True)
    kw = dict(information=True) if information else {}
    lb = mapping.Laser_mapping_batch(S, refresh_threads=1, scan_points=1000, **kw)
    assert reg_calls(log) == (["set_information"] if information else [])
    scans = [np.zeros((10, 4), np.float32)] * S
    assert lb.process_new_scans(scans).tolist() == [1, 1, 1]       # slot 0 aborted and repeated
    assert lb.process_new_scans([scans[0], None, scans[2]]).tolist() == [1, -1, 1]
    if not information:
        assert reg_calls(log) == ["collect"] * 3 and lb.last_information == [None] * S
        return
    assert reg_calls(log) == ["set_information"] + ["collect", "information"] * 3
    first = [lb.last_information[s]["H"][0, 0] for s in range(S)]
    assert first == [31.0, 12.0, 33.0]    # slot 0: the repeat's (collect 2) then step 2 (collect 3); slot 1 idle in step 2: step 1's record
    assert all("H_pose" in lb.last_information[s] for s in range(S))
    assert lb.degenerate_directions(1, 100.0).shape == (6, 6)
    with pytest.raises(TypeError):
        mapping.Laser_mapping_batch(S, informations=True)
