"""What the tests that hold the undistort branch (point_cloud_registration.hpp:607-661) to the reference's compiled class share:
tests/test_ref_undistort.py (the live reference, CPU), tests/golden/gen_ref_undistort.py (the fixture's generator) and
tests/test_ref_undistort_golden.py (the committed fixture: CPU tier and -m gpu).

The scene is the committed tests/golden/ref_scene2.npz -- a moving scan, motion deblur on, 5 ICP iterations -- registered four times:
from the identity increment, from (0,0,0,-1, 0,0,0) (the same rotation, w < 0), with a cost limit that rejects it (PCR:561-573), and with
a frame index at which the gate returns before the first solve (PCR:199)."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np

from loam_livox_amd import synth
from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "golden", "ref_scene2.npz")
FIXTURE = os.path.join(HERE, "golden", "ref_undistort.npz")
CASES = ("w_plus", "w_minus", "rejected", "gated")
CLOUDS = ("corners", "surface", "full", "shifted")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
REJECT_COST = 1e-9    # max_final_cost of the rejected case: below any final cost of a real scan
GATED_FRAME = 10      # current_frame_index of the gated case (mapping_init_accumulate_frames is 50)
_scene = None


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def check_rule(got, want, what):
    """tests/undistort_ref.py check_rule (one fp32 ulp, 1 coordinate in 10 000 unequal) on the rows that are finite in `want`; a point
    with a non-finite coordinate has no rule of its own (NaN in, NaN out): it must be non-finite in `got` as well.  xyzi or xyz rows."""
    from tests import undistort_ref as ur
    got, want = np.asarray(got)[:, :3], np.asarray(want)[:, :3]
    ok = np.isfinite(want).all(axis=1)
    assert got.shape == want.shape and not np.isfinite(got[~ok]).all(axis=1).any(), what
    return ur.check_rule(got[ok], want[ok], what)


def scene():
    """The inputs: dict(corners, surface, full, pose_init, t_min, t_max, corner_map, surf_map, pose_out, pose_incre, n_blocks_last);
    the synthetic map is re-created from its seed and checked against the scene's checksums."""
    global _scene
    if _scene is None:
        g = np.load(SCENE)
        assert int(g["deblur"]) == 1
        _, corner, surf = synth.make_maps(int(g["map_points"]), seed=int(g["map_seed"]))
        assert zlib.crc32(np.ascontiguousarray(corner).tobytes()) == int(g["corner_crc"]), "synthetic corner map changed"
        assert zlib.crc32(np.ascontiguousarray(surf).tobytes()) == int(g["surf_crc"]), "synthetic surface map changed"
        _scene = dict(corners=g["all_corners"], surface=g["all_surface"], full=g["all_full"], pose_init=g["pose_init"], t_min=float(g["t_min"]),
                      t_max=float(g["t_max"]), icp_iters=int(g["icp_iters"]), ceres_iters=int(g["ceres_iters"]), corner_map=corner, surf_map=surf,
                      pose_out=g["pose_out"], pose_incre=g["pose_incre"], n_blocks_last=int(g["n_blocks_last"]))
        _scene["shifted"] = shifted_stamps(_scene["surface"], _scene["t_min"], _scene["t_max"])
    return _scene


def shifted_stamps(surface, t_min, t_max):
    """The surface cloud with its stamps moved by one range-width: the first third down (s in [-1, 0): extrapolated, PCR:633 only
    prints), the second third up (s > 1 -> 1, PCR:134), the rest in place, and every 97th stamp NaN (-> 1)."""
    c = np.array(surface, np.float32, copy=True)
    n, width = len(c), np.float32(t_max) - np.float32(t_min)
    c[: n // 3, 3] -= width
    c[n // 3: 2 * (n // 3), 3] += width
    c[5::97, 3] = np.nan
    return c


def case_params(case):
    """orc.RegParams of a case: those tests/golden/gen_ref_golden.py registered the scene with, and the case's one change"""
    s = scene()
    prm = orc.RegParams.defaults(icp_iters=s["icp_iters"], ceres_iters=s["ceres_iters"], deblur=1)
    prm.minimum_pt_time_stamp, prm.maximum_pt_time_stamp = s["t_min"], s["t_max"]
    if case == "rejected":
        prm.max_final_cost = REJECT_COST
    if case == "gated":
        prm.current_frame_index = GATED_FRAME
    return prm


def start_increment(case):
    inc = IDENT.copy()
    if case == "w_minus":
        inc[3] = -1.0
    return inc


# ------------------------------------------------------------------------------------------------ the host build of ll_reg_core.h
def build_host_lib(directory):
    """tests/undistort_host.cpp (point_to_map_undistort, interp_rodrigues, point_to_map of csrc/ll_reg_core.h) under g++ -ffp-contract=off"""
    so = os.path.join(str(directory), "libundistort_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "undistort_host.cpp")])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.uh_undistort.argtypes = [vp, vp, vp, C.c_double, vp, vp, C.c_int, C.c_float, C.c_float, vp, C.c_int, vp]
    L.uh_point_to_map.argtypes = [vp, vp, C.c_int, vp]
    L.uh_interp.argtypes = [vp, vp, vp, vp]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_interp(L, q):
    q = np.ascontiguousarray(q, np.float64)
    th, hat, hat_sq = np.zeros(1), np.zeros(9), np.zeros(9)
    L.uh_interp(_p(q), _p(th), _p(hat), _p(hat_sq))
    return float(th[0]), hat.reshape(3, 3), hat_sq.reshape(3, 3)


def host_undistort(L, xyzi, pose_last, pose_curr, inc_t, theta, hat, hat_sq, deblur, min_ts, max_ts):
    xyzi = np.ascontiguousarray(xyzi, np.float32)
    a = [np.ascontiguousarray(v, np.float64) for v in (pose_last, pose_curr, inc_t, hat, hat_sq)]
    out = np.zeros_like(xyzi)
    L.uh_undistort(_p(a[0]), _p(a[1]), _p(a[2]), float(theta), _p(a[3]), _p(a[4]), int(deblur), float(min_ts), float(max_ts), _p(xyzi), len(xyzi), _p(out))
    return out


def host_plain(L, pose, xyzi):
    xyzi = np.ascontiguousarray(xyzi, np.float32)
    pose = np.ascontiguousarray(pose, np.float64)
    out = np.zeros_like(xyzi)
    L.uh_point_to_map(_p(pose), _p(xyzi), len(xyzi), _p(out))
    return out
