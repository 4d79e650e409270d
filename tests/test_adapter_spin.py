"""include/loam_livox_adapter.hpp Spinning_laser: a small C++ program (tests/cpp/spin_demo.cpp) on the reference's point-cloud
shape.  CPU tier: it compiles and links against the C-ABI library.  GPU tier: its five clouds equal the host restatement's."""
import os
import subprocess

import numpy as np
import pytest

from loam_livox_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "spin_demo.cpp")


def build_demo(out_dir):
    from loam_livox_amd import build
    lib = build.build()
    exe = os.path.join(str(out_dir), "spin_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_spin_demo_compiles_and_links(tmp_path):
    assert os.path.exists(build_demo(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("scan_line", [16, 64])
def test_spin_demo_matches_restatement(tmp_path, scan_line):
    from tests import spin_ref
    exe = build_demo(tmp_path)
    sc = synth.make_spin_scan(synth.make_world(4, 4), 21, scan_line=scan_line, n_azimuth=900)
    scan, out = tmp_path / "scan.bin", tmp_path / "out.bin"
    sc.xyzi.astype(np.float32).tofile(scan)
    subprocess.check_call([exe, str(scan), str(scan_line), str(out)], timeout=120)
    data = out.read_bytes()
    ref = spin_ref.clouds(spin_ref.extract(sc.xyzi, scan_line=scan_line))
    o = 0
    for topic in spin_ref.TOPICS:
        n = int(np.frombuffer(data, np.int32, 1, o)[0])
        o += 4
        c = np.frombuffer(data, np.float32, 4 * n, o).reshape(n, 4)
        o += 16 * n
        assert c.shape == ref[topic].shape, topic
        assert np.array_equal(c[:, :3], ref[topic][:, :3]), topic
        tol = np.maximum(2.0 ** -22, 2 * np.spacing(np.abs(ref[topic][:, 3])))
        assert np.all(np.abs(c[:, 3].astype(np.float64) - ref[topic][:, 3]) <= (tol if topic == spin_ref.TOPICS[0] else 1e-4)), topic
