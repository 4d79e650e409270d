"""include/loam_livox_adapter.hpp, the Spinning_laser overloads of Point_cloud_registration and History_buffer: a small C++ program
(tests/cpp/spin_reg_demo.cpp) registers one spinning-lidar scan and pushes it into a history device to device and through the host
clouds.  CPU tier: it compiles and links against the C-ABI library.  GPU tier: the two routes give the same bits, the pose is the
oracle's, and m_if_motion_deblur is refused."""
import os
import subprocess

import numpy as np
import pytest

from loam_livox_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "spin_reg_demo.cpp")


def build_demo(out_dir):
    from loam_livox_amd import build
    lib = build.build()
    exe = os.path.join(str(out_dir), "spin_reg_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_spin_reg_demo_compiles_and_links(tmp_path):
    assert os.path.exists(build_demo(tmp_path))


def read_route(data, o):
    ret = int(np.frombuffer(data, np.int32, 1, o)[0])
    pose = np.frombuffer(data, np.float64, 7, o + 4).copy()
    o += 4 + 56
    clouds = []
    for _ in range(2):
        n = int(np.frombuffer(data, np.int32, 1, o)[0])
        clouds.append(np.frombuffer(data, np.float32, 4 * n, o + 4).reshape(n, 4).copy())
        o += 4 + 16 * n
    return (ret, pose, clouds), o


@pytest.mark.gpu
@pytest.mark.parametrize("scan_line", [16, 64])
def test_spin_reg_demo_routes_agree_and_match_the_oracle(tmp_path, small_world, scan_line):
    from oracle import orc
    from tests import spin_ref
    exe = build_demo(tmp_path)
    sc = synth.make_spin_scan(small_world["world"], 3, scan_line=scan_line, n_azimuth=900)
    init = synth.pose_compose(sc.pose_true, np.r_[synth.quat_from_axis_angle(np.array([0.3, -0.2, 1.0]), 0.008), 0.03, -0.02, 0.01])
    paths = {k: str(tmp_path / (k + ".bin")) for k in ("corner", "surf", "scan", "pose", "out")}
    np.ascontiguousarray(small_world["corner"][:, :3], np.float32).tofile(paths["corner"])
    np.ascontiguousarray(small_world["surf"][:, :3], np.float32).tofile(paths["surf"])
    sc.xyzi.astype(np.float32).tofile(paths["scan"])
    np.ascontiguousarray(init, np.float64).tofile(paths["pose"])
    subprocess.check_call([exe, paths["corner"], paths["surf"], paths["scan"], str(scan_line), paths["pose"], paths["out"]], timeout=180)
    data = open(paths["out"], "rb").read()
    dev, o = read_route(data, 0)
    host, o = read_route(data, o)
    refused = int(np.frombuffer(data, np.int32, 1, o)[0])
    assert dev[0] == host[0] == 1 and dev[1].tobytes() == host[1].tobytes()
    for kind in (0, 1):
        assert len(dev[2][kind]) > 0 and dev[2][kind].tobytes() == host[2][kind].tobytes(), kind
    assert refused == 1
    c = spin_ref.clouds(spin_ref.extract(sc.xyzi, scan_line=scan_line))
    prm = orc.RegParams.defaults(icp_iters=10, ceres_iters=20, force_all=0)
    ret, pc, _, _ = orc.reg_solve(small_world["tree_c"], small_world["tree_s"], c[spin_ref.TOPICS[2]], c[spin_ref.TOPICS[4]], prm, init, init)
    dt, dr = synth.pose_error(dev[1], pc)
    assert ret == 1 and dt < 1e-7 and dr < 1e-7
