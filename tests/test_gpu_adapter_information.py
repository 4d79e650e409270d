"""-m gpu: the registration information through include/loam_livox_adapter.hpp (tests/cpp/adapter_information.cpp): a
Point_cloud_registration with m_if_compute_information = 1 gives the record the Python mirror gives for the same scan, bit for bit, its
Jacobi agrees with numpy.linalg.eigh, its H_pose with api.information_in_pose_frame; an object with the member at 0 computes nothing."""
import os
import subprocess

import numpy as np
import pytest

from loam_livox_amd import api
from loam_livox_amd.api import Map_buffer, Point_cloud_registration
from tests.conftest import oracle_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "adapter_information.cpp")


@pytest.mark.gpu
def test_adapter_record_equals_the_python_mirrors(tmp_path, gpu_lib, small_world, scans):
    from loam_livox_amd import build
    lib = build.build()
    exe = str(tmp_path / "adapter_information")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    sc = scans[0]
    _, _, _, _, fc, fs = oracle_features(sc)
    fc, fs = fc[:200], fs[::4][:3000]
    xyzi = lambda a: np.ascontiguousarray(np.c_[a[:, :3], np.zeros(len(a))] if a.shape[1] == 3 else a, np.float32)
    paths = [str(tmp_path / n) for n in ("mc.f32", "ms.f32", "sc.f32", "ss.f32", "pose.f64", "out.bin")]
    for p, a in zip(paths, (xyzi(small_world["corner"]), xyzi(small_world["surf"]), xyzi(fc), xyzi(fs))):
        a.tofile(p)
    np.asarray(sc.pose_init, np.float64).tofile(paths[4])
    done = subprocess.run([exe] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert done.returncode == 0, done.stderr.decode(errors="replace")
    raw = open(paths[5], "rb").read()
    head, d = np.frombuffer(raw[:20], np.int32), np.frombuffer(raw[20:], np.float64)
    H, g, cost, w, V, Hp = d[:36].reshape(6, 6), d[36:42], d[42], d[43:49], d[49:85].reshape(6, 6), d[85:121].reshape(6, 6)
    assert head[4] == 1   # the object with the member at 0 had no record, and the same pose

    m = Map_buffer()
    m.setInputCloud(Map_buffer.CORNER, small_world["corner"])
    m.setInputCloud(Map_buffer.SURF, small_world["surf"])
    reg = Point_cloud_registration(max_scans=1, max_features=100000)
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations = 4, 20
    p.para_max_angular_rate, p.para_max_speed = 20.0, 0.3
    p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
    reg.set_information(True)
    reg.m_pose_w_last, reg.m_pose_w_curr = sc.pose_init.copy(), sc.pose_init.copy()
    ret = reg.find_out_incremental_transfrom(m, fc, fs)
    rec = reg.information(1)[0]
    reg.close(); m.close()
    assert head[0] == ret and (head[1], head[2], head[3]) == (rec["n_line"], rec["n_plane"], rec["status"]) and rec["status"] == 0 and rec["n_plane"] > 1000
    assert np.array_equal(H.view(np.uint64), rec["H"].view(np.uint64)) and np.array_equal(g.view(np.uint64), rec["g"].view(np.uint64)) and cost == rec["cost"]
    tol = 64 * 2.0 ** -52 * np.linalg.norm(H, 2)
    assert np.abs(w - rec["eigenvalues"]).max() <= tol and np.abs(H @ V - V * w).max() <= tol and np.abs(V.T @ V - np.eye(6)).max() <= 64 * 2.0 ** -52
    ref = api.information_in_pose_frame(H, sc.pose_init)
    assert np.abs(Hp - ref).max() <= 64 * 2.0 ** -52 * np.abs(ref).max()
