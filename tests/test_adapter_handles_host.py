"""CPU tier of include/loam_livox_adapter.hpp, ownership (tests/test_gpu_adapter_lifetime.py is the GPU tier): tests/cpp/adapter_lifetime_host.cpp
runs every handle-owning class of the adapter against the recording stand-in of tests/cpp/adapter_standin.cpp -- construct, use, move,
move-assign, destroy, every handle destroyed exactly once, the pool's registrars back where they came from, the copy rules of VoxelGrid and
Point_cloud_registration, map_cloud on a negative count -- as a plain program and as one built with the address and undefined-behaviour
sanitizers.  The header also compiles warning-free without Eigen and against the Eigen stand-in of oracle/ref_stubs.  No device, no library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "adapter_lifetime_host.cpp")
BASE = ["g++", "-std=c++14", "-Wall", "-Werror", "-DLOAM_LIVOX_ADAPTER_NO_EIGEN", "-I", os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("adapter_lifetime_host")
    plain, san = str(d / "adapter_lifetime_host"), str(d / "adapter_lifetime_host_san")
    subprocess.check_call(BASE + ["-O1", "-o", plain, SRC])
    subprocess.check_call(BASE + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san, SRC])
    return dict(plain=plain, san=san)


def test_every_owner_moves_and_destroys_its_handle_once(exes):
    p = subprocess.run([exes["plain"]], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok: "), p.stderr[-4000:]


def test_the_driver_runs_clean_under_the_sanitizers(exes):
    p = subprocess.run([exes["san"]], capture_output=True, text=True)
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


USES_THE_POSE_HELPERS = r'''
#include "loam_livox_adapter.hpp"
namespace ll = loam_livox_hip;
int main()
{
    ll::Point_cloud_registration reg;
    double p[7], q[7] = {0, 0, 0, 1, 1, 2, 3};
    ll::to_pose7(reg.m_q_w_curr, reg.m_t_w_curr, p);         // the pose types
    ll::to_pose7(reg.m_q_w_incre, reg.m_t_w_incre, p);       // the views of m_para_buffer_incremental
    ll::from_pose7(q, reg.m_q_w_incre, reg.m_t_w_incre);
    ll::from_pose7(q, reg.m_q_w_last, reg.m_t_w_last);
    ll::Point_cloud_registration copy(reg);
    copy = reg;
    return copy.m_para_buffer_incremental[6] == 3.0 ? 0 : 1;
}
'''


@pytest.mark.parametrize("eigen", ["none", "ref_stubs"])
def test_header_compiles_without_eigen_and_with_the_stand_in(tmp_path, eigen):
    src = tmp_path / "pose_helpers.cpp"
    src.write_text(USES_THE_POSE_HELPERS)
    flags = ["-DLOAM_LIVOX_ADAPTER_NO_EIGEN"] if eigen == "none" else ["-I", os.path.join(ROOT, "oracle", "ref_stubs")]
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")] + flags + [str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    if eigen == "ref_stubs":   # ... and that build does take the Eigen path
        r = subprocess.run(["g++", "-std=c++14", "-E", "-dM", "-I", os.path.join(ROOT, "include")] + flags + [str(src)], capture_output=True, text=True)
        assert "#define LOAM_LIVOX_ADAPTER_EIGEN 1" in r.stdout
