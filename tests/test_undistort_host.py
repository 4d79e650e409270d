"""CPU tier of the deskewed clouds (ll_cloud_undistort*, ll_history_set_undistort; tests/test_gpu_undistort.py is the GPU tier).

tests/undistort_host.cpp compiles loam_livox_amd/csrc/ll_reg_core.h point_to_map_undistort / interp_rodrigues -- the text the kernels run --
with g++ -ffp-contract=off.  The yardstick is the float64 numpy restatement of point_cloud_registration.hpp:622-661 and :607-620 in
tests/undistort_ref.py, under the rule its docstring derives: every coordinate within one fp32 ulp, at most 1 in 10 000 unequal."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from loam_livox_amd import api, capi, mapping
from tests import api_standin
from tests import undistort_ref as ur
from tests.undistort_pin import build_host_lib, host_interp, host_plain, host_undistort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "loam_livox_hip.h")
NEW_SYMBOLS = {"ll_reg_interpolation": 6, "ll_cloud_undistort": 5, "ll_cloud_undistort_fe_device": 8, "ll_history_set_undistort": 3}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build_host_lib(tmp_path_factory.mktemp("undistort"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def make_state(rng, angle, shift):
    """pose_last far from the origin, an increment of `angle` rad / `shift` m, pose_curr = pose_last o increment"""
    pose_last = np.r_[ur.quat_from_rotvec(rng.normal(size=3) * 0.7), rng.uniform(-30, 30, 3)]
    axis = rng.normal(size=3)
    inc = np.r_[ur.quat_from_rotvec(axis / np.linalg.norm(axis) * angle), rng.normal(size=3) / np.sqrt(3) * shift]
    pose_curr = np.r_[q_mul(pose_last[:4], inc[:4]), ur.quat_to_mat(pose_last[:4]) @ inc[4:] + pose_last[4:]]
    return pose_last, pose_curr, inc


MIN_TS, MAX_TS = 0.25, 0.35


def make_points(rng, n):
    """stamps across the range, below it (s < 0: not clamped), above it (s > 1 -> 1), and exactly on both ends"""
    xyzi = np.zeros((n, 4), np.float32)
    xyzi[:, :3] = rng.uniform(-50, 50, (n, 3))
    xyzi[:, 3] = rng.uniform(MIN_TS - 0.05, MAX_TS + 0.05, n)
    xyzi[: n // 50, 3] = MAX_TS
    xyzi[n // 50: n // 25, 3] = MIN_TS
    return xyzi


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("angle,shift", [(0.3, 0.5), (0.02, 0.1), (1e-6, 1e-4)])
def test_undistort_against_the_numpy_restatement(lib, angle, shift):
    rng = np.random.default_rng(int(angle * 1e6) + 1)
    pose_last, pose_curr, inc = make_state(rng, angle, shift)
    theta, hat, hat_sq = host_interp(lib, inc[:4])
    xyzi = make_points(rng, 5000)
    s = ur.blur_ratio(xyzi[:, 3], 1, MIN_TS, MAX_TS)
    assert (s < 0).sum() > 100 and (s == 1).sum() > 500 and ((s > 0) & (s < 1)).sum() > 2000
    got = host_undistort(lib, xyzi, pose_last, pose_curr, inc[4:], theta, hat, hat_sq, 1, MIN_TS, MAX_TS)
    r_theta, r_hat = ur.interp(inc[:4])
    want = ur.undistort(xyzi, pose_last, pose_curr, inc, r_theta, r_hat, 1, MIN_TS, MAX_TS)
    assert np.array_equal(got[:, 3], xyzi[:, 3])   # intensity copied, PCR:659
    ur.check_rule(got[:, :3], want, f"host build, increment {angle} rad / {shift} m")
    # the deskew is not a no-op at these increments: the plain transform is somewhere else
    if angle >= 0.02:
        assert np.abs(got[:, :3] - host_plain(lib, pose_curr, xyzi)[:, :3]).max() > 1e-2


# ------------------------------------------------------------------------------------------------ 2
def test_end_of_scan_branch_is_point_to_map_with_pose_curr_bit_for_bit(lib):
    rng = np.random.default_rng(2)
    pose_last, pose_curr, inc = make_state(rng, 0.3, 0.5)
    theta, hat, hat_sq = host_interp(lib, inc[:4])
    xyzi = make_points(rng, 2000)
    plain = host_plain(lib, pose_curr, xyzi)
    at_end = xyzi.copy()
    at_end[:, 3] = MAX_TS                      # s == 1
    for pts, deblur, lo, hi in ((at_end, 1, MIN_TS, MAX_TS), (xyzi, 0, MIN_TS, MAX_TS), (xyzi, 1, MAX_TS, MAX_TS)):  # s == 1; deblur off; min == max (0/0, x/0 -> 1)
        got = host_undistort(lib, pts, pose_last, pose_curr, inc[4:], theta, hat, hat_sq, deblur, lo, hi)
        assert got[:, :3].tobytes() == plain[:, :3].tobytes()
    above = xyzi.copy()
    above[:, 3] = MAX_TS + rng.uniform(1e-6, 1.0, len(xyzi)).astype(np.float32)   # s > 1 -> 1 (PCR:137)
    assert host_undistort(lib, above, pose_last, pose_curr, inc[4:], theta, hat, hat_sq, 1, MIN_TS, MAX_TS)[:, :3].tobytes() == plain[:, :3].tobytes()


def test_non_finite_points_behave_as_in_the_plain_transform(lib):
    rng = np.random.default_rng(3)
    pose_last, pose_curr, inc = make_state(rng, 0.1, 0.2)
    theta, hat, hat_sq = host_interp(lib, inc[:4])
    xyzi = make_points(rng, 64)
    xyzi[::4, 0] = np.nan
    xyzi[1::8, 3] = np.nan    # a non-finite stamp counts as s = 1 (PCR:137)
    xyzi[2::8, 1] = np.inf
    got = host_undistort(lib, xyzi, pose_last, pose_curr, inc[4:], theta, hat, hat_sq, 1, MIN_TS, MAX_TS)
    bad = ~np.isfinite(xyzi[:, :3]).all(axis=1)
    assert not np.isfinite(got[bad, :3]).all(axis=1).any() and np.isfinite(got[~bad, :3]).all()
    nan_w = np.isnan(xyzi[:, 3]) & ~bad
    assert nan_w.any() and got[nan_w, :3].tobytes() == host_plain(lib, pose_curr, xyzi)[nan_w, :3].tobytes()


# ------------------------------------------------------------------------------------------------ 3
def test_zero_state_is_point_to_map_with_pose_last_bit_for_bit(lib):
    """a gated slot's record: identity increment, theta 0, zero matrices -- I p + 0 is exact"""
    rng = np.random.default_rng(4)
    pose_last, pose_curr, _ = make_state(rng, 0.3, 0.5)
    xyzi = make_points(rng, 2000)
    z9 = np.zeros(9)
    got = host_undistort(lib, xyzi, pose_last, pose_last, np.zeros(3), 0.0, z9, z9, 1, MIN_TS, MAX_TS)
    assert got.tobytes() == host_plain(lib, pose_last, xyzi).tobytes()


# ------------------------------------------------------------------------------------------------ 4
def test_interp_twin_against_the_restatement(lib):
    """PCR:607-620 for quaternions with w < 0, a zero vector part and tiny angles.  Tolerance: theta is one atan2 and one product
    (each within an ulp in either implementation), the axis two divisions and a square root: 4 fp64 ulps of the values' scale."""
    rng = np.random.default_rng(5)
    cases = [np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.0, 0.0, 0.0, -1.0])]
    for angle in (1e-300, 1e-160, 1e-12, 1e-8, 1e-3, 0.3, 3.0):
        axis = rng.normal(size=3)
        q = np.r_[np.sin(angle / 2) * axis / np.linalg.norm(axis), np.cos(angle / 2)]
        cases += [q, -q, np.r_[q[:3], -q[3]]]
    eps = 2.0 ** -52
    for q in cases:
        theta, hat, hat_sq = host_interp(lib, q)
        r_theta, r_hat = ur.interp(q)
        assert abs(theta - r_theta) <= 4 * eps * abs(r_theta), q
        assert np.abs(hat - r_hat).max() <= 4 * eps and np.abs(hat_sq - r_hat @ r_hat).max() <= 8 * eps, q
        assert np.array_equal(hat, -hat.T)
    th, hat, hat_sq = host_interp(lib, cases[0])
    assert th == 0.0 and hat[2, 1] == 1.0 and hat[1, 2] == -1.0   # Eigen's axis for the identity: (1, 0, 0)
    assert host_interp(lib, cases[1])[0] == 0.0
    # w < 0: the angle stays positive and the axis turns (n = -n after the angle) -- q and -q are one rotation and give one state,
    # and Rodrigues' matrix of it is the quaternion's
    for q in (c for c in cases[2:] if c[3] < 0):
        theta, hat, hat_sq = host_interp(lib, q)
        t2, h2, _ = host_interp(lib, -q)
        assert theta >= 0.0 and (theta > 0.0 or np.abs(q[:3]).max() < 1e-150) and theta == t2 and np.array_equal(hat, h2)
        R = np.eye(3) + np.sin(theta) * hat + (1 - np.cos(theta)) * hat_sq
        assert np.abs(R - ur.quat_to_mat(q)).max() <= 1e-14


# ------------------------------------------------------------------------------------------------ symbols and marshalling
def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for name, n_args in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(capi.SYMBOLS[name][1]), name
        assert capi.SYMBOLS[name][0] is C.c_int32 and name in exported and hasattr(L, name)
    assert capi.SYMBOLS["ll_cloud_undistort_fe_device"][1][6] is C.c_int64


def test_null_handle_refusals_carry_their_text_without_a_device():
    L = capi.load()
    n = C.c_int64(0)
    buf = np.zeros(8, np.float32)
    acc = np.ones(1, np.int32)
    for call, fn in ((lambda: L.ll_reg_interpolation(None, 1, None, None, None, None), "ll_reg_interpolation"),
                     (lambda: L.ll_cloud_undistort(None, 0, _p(buf), _p(buf), 1), "ll_cloud_undistort"),
                     (lambda: L.ll_cloud_undistort_fe_device(None, None, 1, 0, _p(acc), _p(buf), 2, C.byref(n)), "ll_cloud_undistort_fe_device"),
                     (lambda: L.ll_history_set_undistort(None, None, 0), "ll_history_set_undistort")):
        rc = call()
        msg = L.ll_last_error().decode()
        assert rc != 0 and fn in msg and "null" in msg, (rc, msg)


def test_api_methods_over_the_recording_stand_in(monkeypatch):
    lib = api_standin.Recording_library()
    monkeypatch.setattr(capi, "_lib", lib)
    reg = api.Point_cloud_registration(max_scans=3, max_features=100)
    hist = api.History_buffer(5, 100)
    cloud = np.arange(12, dtype=np.float32).reshape(3, 4)
    before = len(lib.calls)
    reg.pointcloudAssociateToMap(cloud, np.array([0, 0, 0, 1, 0, 0, 0.0]))
    assert [c[0] for c in lib.calls[before:]] == ["ll_cloud_transform"]          # the default is today's path
    out = reg.pointcloudAssociateToMap(cloud, if_undistore=1, slot=2)
    name, args = lib.calls[-1]
    assert name == "ll_cloud_undistort" and args[1] == 2 and args[4] == 3 and args[2] == api_standin.plain(cloud) and out.shape == (3, 4)
    it = reg.interpolation(3)
    name, args = lib.calls[-1]
    assert name == "ll_reg_interpolation" and args[1] == 3 and [a["shape"] for a in args[2:]] == [[3], [3, 3, 3], [3, 7], [3, 7]]
    assert sorted(it) == ["omega_hat", "pose_incre", "pose_last", "theta"]
    hist.set_undistort(reg, slot=1)
    name, args = lib.calls[-1]
    assert name == "ll_history_set_undistort" and args[0] == api_standin.plain(hist.h) and args[1] == api_standin.plain(reg.h) and args[2] == 1

    class Out:   # what the method needs of a torch tensor
        shape = (10, 4)

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 0x5000

    lib.answer("ll_cloud_undistort_fe_device", 0, {7: 9})
    fe = api.Livox_laser(max_points=100, max_scans=3)
    assert reg.cloud_undistort_fe_device(fe, 3, 2, np.array([1, 0, 1]), Out(), 4) == 9
    name, args = lib.calls[-1]
    assert name == "ll_cloud_undistort_fe_device" and args[2:4] == [3, 2] and args[4]["dtype"] == "int32" and args[5] == {"pointer": 0x5000} and args[6] == 10
    lib.fail.add("ll_history_set_undistort")
    with pytest.raises(capi.LoamLivoxError):
        hist.set_undistort(reg)


# ------------------------------------------------------------------------------------------------ the mapping loop over stub handles
class Stub:
    def __init__(self, log, name, answers=None):
        self._log, self._name, self._answers = log, name, answers or {}
        self.params = types.SimpleNamespace(time_internal_pts=1e-5, max_points=1000)
        self.debug_flags = 0

    def __getattr__(self, method):
        if method.startswith("__"):
            raise AttributeError(method)

        def call(*a, **k):
            self._log.append((self._name, method, a, k))
            ans = self._answers.get(method)
            return ans(*a, **k) if callable(ans) else ans
        return call


def stub_world(monkeypatch):
    log = []

    def collect(n):
        r = capi.RegReport()
        r.accepted = 1
        pc = np.tile(np.array([0, 0, 0, 1, 0.1, 0, 0], np.float64), (n, 1))
        return np.ones(n, np.int32), pc, pc.copy(), [r]

    fe = dict(full_selection=lambda *a, **k: np.array([0, 3, 7], np.int32))
    hist = dict(add_voxel=True, add=True, refresh=(1, 2))
    reg = dict(collect=collect, find_out_incremental_transfrom=1)
    for cls, answers in (("Livox_laser", fe), ("Spinning_laser", {}), ("Point_cloud_registration", reg), ("Map_buffer", {}), ("VoxelGrid", {}), ("History_buffer", hist)):
        monkeypatch.setattr(mapping, cls, lambda *a, _c=cls, _an=answers, **k: Stub(log, _c, _an))
    return log


def names(log):
    return [(c, m) for c, m, _, _ in log]


def test_laser_mapping_flags_off_make_todays_calls_and_on_add_theirs(monkeypatch):
    scan = np.zeros((10, 4), np.float32)
    runs = {}
    for flags in ((0, 0), (1, 0), (0, 1), (1, 1)):
        log = stub_world(monkeypatch)
        lm = mapping.Laser_mapping(scan_points=1000, if_motion_deblur=flags[0], if_undistort=flags[1])
        plain = mapping.Laser_mapping(scan_points=1000) if flags == (0, 0) else None
        del log[:]
        for k in range(2):
            assert lm.process_new_scan(scan, time_stamp=0.5 + 0.1 * k) == 1
        runs[flags] = (names(log), lm)
        if plain is not None:
            del log[:]
            for k in range(2):
                plain.process_new_scan(scan, time_stamp=0.5 + 0.1 * k)
            assert names(log) == runs[flags][0]                      # the default constructor and flags 0 / 0: the same calls
            assert not hasattr(lm.reg.params, "if_motion_deblur")    # ... and nothing set on the registrar
    base = runs[(0, 0)][0]
    assert ("History_buffer", "set_undistort") not in base and ("Livox_laser", "full_selection") not in base
    assert [c for c in runs[(0, 1)][0] if c != ("History_buffer", "set_undistort")] == base
    assert runs[(0, 1)][0].count(("History_buffer", "set_undistort")) == 2
    i = runs[(0, 1)][0].index(("History_buffer", "set_undistort"))
    assert runs[(0, 1)][0][i - 1] == ("History_buffer", "set_gate_pose") and runs[(0, 1)][0][i + 1] == ("History_buffer", "add_voxel")
    assert [c for c in runs[(1, 0)][0] if c != ("Livox_laser", "full_selection")] == base
    lm = runs[(1, 1)][1]
    assert lm.reg.params.if_motion_deblur == 1
    # the frame's range: from the previous frame's last stamp to this frame's (laser_mapping.hpp:1336-1347), stamp = the extractor's
    last = [np.float32(np.float64(t) + np.float64(np.float32(7) * np.float32(1e-5))) for t in (0.5, 0.6)]
    assert lm.reg.params.minimum_pt_time_stamp == float(last[0]) and lm.reg.params.maximum_pt_time_stamp == float(last[1])


def test_process_clouds_with_undistort_sets_the_history_and_the_full_cloud(monkeypatch):
    log = stub_world(monkeypatch)
    lm = mapping.Laser_mapping(scan_points=1000, input_downsample_mode=0, if_motion_deblur=1, if_undistort=1)
    del log[:]
    full = np.zeros((5, 4), np.float32)
    full[:, 3] = [0.1, 0.4, 0.2, 0.3, 0.0]
    assert lm.process_clouds(full, full[:3], full[:2]) == 1
    seq = names(log)
    i = seq.index(("History_buffer", "set_undistort"))
    assert seq[i - 1] == ("History_buffer", "set_gate_pose") and seq[i + 1] == ("History_buffer", "add")
    assert lm.reg.params.maximum_pt_time_stamp == float(np.float32(0.4)) and lm.reg.params.minimum_pt_time_stamp == 0.0


def test_spinning_lidars_refuse_both_flags(monkeypatch):
    stub_world(monkeypatch)
    for kw in (dict(if_motion_deblur=1), dict(if_undistort=1)):
        with pytest.raises(ValueError, match="time stamp"):
            mapping.Laser_mapping(scan_points=1000, lidar_type="velodyne", **kw)
    mapping.Laser_mapping(scan_points=1000, lidar_type="velodyne")
