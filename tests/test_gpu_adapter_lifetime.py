"""GPU tier of the ownership rule of include/loam_livox_adapter.hpp (tests/test_adapter_handles_host.py is the CPU tier; the device twin of
tests/test_gpu_api_lifetime.py): tests/cpp/adapter_lifetime.cpp, one process on inputs of 64 points -- a Points_cloud_map appended to,
moved and read through its new owner; a VoxelGrid filtered, copied, both filtered again; a Spinning_laser that outgrows its first capacity
between two extractions; a Mapping_refine entered through add_logged and one entered through refine_pointcloud."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "adapter_lifetime.cpp")


@pytest.mark.gpu
def test_owners_on_the_device(tmp_path, gpu_lib):
    from loam_livox_amd import build
    lib = build.build()
    exe = str(tmp_path / "adapter_lifetime")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert done.returncode == 0 and done.stdout.decode().strip() == "ok", done.stderr.decode(errors="replace")
