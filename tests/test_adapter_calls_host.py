"""CPU tier of include/loam_livox_adapter.hpp, calls: tests/cpp/adapter_calls_host.cpp runs every method that goes through one of the
header's shared helpers (the cloud readers, extract_cells, add_logged, the map refinement, the spinning extractions, the scene alignment,
the pose graph, the three registration routes, pointcloudAssociateToMap) against the recording stand-in, on clouds of 0, 1 and 5 points.
The C calls it makes -- names, scalars, handles, arrays -- and what the methods return are compared with tests/adapter_calls.txt, recorded
with the header of the commit before the helpers existed (the file's first line is the command).  No device, no library.

Left out of the comparison, and why: the header now reads every cloud back one way -- ask the size, and fill only when there is a point.
Before, three of the seven readers made their fill call for an empty cloud too (extract_specify_points with a null buffer, merge_last and
the fetch of refine_pointcloud / refine_mapping with a one-point stand-in buffer); the library answers such a call with 0 and touches
nothing.  In the cases of EMPTY_READS exactly that call is gone, and the test says so line by line; every other line of every case is
the recording's."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "adapter_calls_host.cpp")
RECORDING = os.path.join(ROOT, "tests", "adapter_calls.txt")

# case -> the fill calls for an empty cloud that the recording has and the header no longer makes
EMPTY_READS = {
    "Points_cloud_map::extract_specify_points, 0 line and 0 plane points": ["ll_cellmap_feature_clouds(cellmap#0, null, 0, null, 0, null)"] * 2,
    "Points_cloud_map::extract_specify_points, 5 line and 0 plane points": ["ll_cellmap_feature_clouds(cellmap#0, null, 0, null, 0, null)"],
    "Mapping_refine::refine_pointcloud, an output of 0 points": ["ll_map_refine_fetch(map_refine#1, out, 0)"],
    "Mapping_refine::refine_mapping, outputs of 0 points": ["ll_map_refine_fetch(map_refine#1, out, 0)"],
    "Mapping_refine::merge_last, 0 points": ["ll_map_refine_fetch_merged(map_refine#1, out, 0)"],
}


def cases(lines):
    """the log cut at its '== title' lines: [(title, lines)], what precedes the first title under ''"""
    out = [("", [])]
    for l in lines:
        if l.startswith("== "):
            out.append((l[3:], []))
        else:
            out[-1][1].append(l)
    return out


@pytest.fixture(scope="module")
def logs(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adapter_calls_host") / "adapter_calls_host")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-DLOAM_LIVOX_ADAPTER_NO_EIGEN", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    recorded = open(RECORDING).read().split("\n")
    assert recorded[0].startswith("# ")
    return cases(p.stdout.split("\n")), cases(recorded[1:])


def test_calls_and_results_equal_the_recording(logs):
    got, want = logs
    assert [t for t, _ in got] == [t for t, _ in want]
    differing = [t for (t, g), (_, w) in zip(got, want) if g != w]
    assert sorted(differing) == sorted(EMPTY_READS), differing
    for (t, g), (_, w) in zip(got, want):
        if t in EMPTY_READS:
            # the recording's lines minus exactly those fill calls: each is the last call before the method returns (the size call stays)
            gone = [k for k, l in enumerate(w[:-1]) if l in EMPTY_READS[t] and w[k + 1].startswith("->")]
            assert [w[k] for k in gone] == EMPTY_READS[t], t
            assert g == [l for k, l in enumerate(w) if k not in gone], t


def test_the_cases_cover_the_helpers(logs):
    got, _ = logs
    titles = [t for t, _ in got]
    log = "\n".join(l for _, ls in got for l in ls)
    for reader in ("History_buffer::map_cloud", "History_batch::map_cloud", "History_batch::read_group", "Points_cloud_map::extract_specify_points",
                   "Points_cloud_map::find_cells_in_radius_filtered", "Mapping_refine::merge_last", "Mapping_refine::refine_pointcloud"):
        assert sum(t.startswith(reader) for t in titles) >= 3, reader                                   # empty, one point, five points
    for name in ("Points_cloud_map::extract_cells", "History_batch::extract_cells", "Mapping_refine::add_logged", "Mapping_refine::refine_mapping",
                 "Spinning_laser::extract,", "Spinning_laser::extract_device", "Scene_alignment::find_tranfrom_of_two_mappings", "pose_graph_optimization",
                 "find_out_incremental_transfrom with map clouds", "find_out_incremental_transfrom against map()", "find_out_incremental_transfrom( spin )",
                 "pointcloudAssociateToMap"):
        assert any(t.startswith(name) for t in titles), name
    assert log.count("ll_runtime_hint_hw_queues(16)") == 1                       # once per process, before the first create
    assert len(re.findall(r"ll_spin_create\(", log)) == 5 and "ll_spin_create(16, 0.100000001, 0.800000012, 0, 5, 1, 8192)" in log   # grown past the capacity
    unchanged = dict(got)["find_out_incremental_transfrom with map clouds, scans of 1 and 4 points, the map unchanged"]
    assert not any(l.startswith("ll_map_upload_gen") for l in unchanged) and sum(l.startswith("ll_map_generation") for l in unchanged) == 2
    assert "ll_map_upload_gen(map#0, 0, xyz[15]:3279dff3f1ac209a, 8, 5, 0)" in log   # 8 floats per point go as they lie: stride 8, no staging copy
