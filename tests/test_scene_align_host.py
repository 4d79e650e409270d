"""CPU tier of the device scene alignment (tests/test_gpu_scene_align.py is the GPU tier): the selection chain of
ll_cellmap_select_kernels.hip -- flag, scan, gather -- compiled for the CPU from the kernel unit itself (tests/cellmap_feature_clouds_host.cpp
on tests/cellmap_batch_shim) gives, bit for bit, the line cloud, the plane cloud and the counts that oracle.orc_scene_alignment.keyframe_clouds
takes out of an oracle CellMap built from the same points; and the new entry points are declared, exported and bound and refuse null
handles and bad parameters without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from loam_livox_amd import capi
from tests.test_cellmap_extract_host import BOX, dump_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE, LINE, PLANE = 0, 1, 2
# cells of exactly one point, of 65 (one more than a wavefront), 257 (one more than a block) and 1000 points, as tests/test_cellmap_extract_host.py
SIZES = [1, 1, 1, 65, 257, 1000, 23]
N_CELLS = 300
BLOCK = 256   # threads per block of the gather


def geometry(kinds=(SPHERE, LINE, PLANE), seed=7, remainder=0):
    """(points [n, 3] float32 in a shuffled insertion order, the cell of every point [n, 3], the kind each cell was shaped as, by cell):
    300 cells around the origin -- thin rods (lines), flat patches (planes), blobs (spheres) of the kinds allowed, well inside their
    cells -- with a total point count that leaves `remainder` modulo the block size.  The cells with the smallest and the largest key
    are a rod and a patch (when allowed): the first and the last cell of the table are selected."""
    rng = np.random.default_rng(seed)
    ks = set()
    while len(ks) < N_CELLS:
        # (close to the origin: the float second moments of a cell lose about 1e-5 m^2 out there, the thin directions below keep 1e-4)
        ks.add(tuple(int(v) for v in rng.integers(-4, 5, 3)))
    ks = np.array(sorted(ks), np.int64)
    middle = np.array(SIZES + list(rng.integers(1, 25, N_CELLS - 2 - len(SIZES))), np.int64)[rng.permutation(N_CELLS - 2)]
    sizes = np.r_[17, middle, 31]
    pad = int(np.flatnonzero(sizes == 23)[0])
    sizes[pad] += (remainder - int(sizes.sum())) % BLOCK          # (a cell of 23 .. 278 points makes the total come out)
    kind = np.array(kinds)[rng.integers(0, len(kinds), N_CELLS)]
    kind[np.flatnonzero(sizes == 1000)[0]] = PLANE if PLANE in kinds else kinds[0]
    kind[np.flatnonzero(sizes == 257)[0]] = LINE if LINE in kinds else kinds[0]
    kind[np.flatnonzero(sizes == 65)[0]] = kinds[0]
    kind[0] = LINE if LINE in kinds else kinds[0]
    kind[-1] = PLANE if PLANE in kinds else kinds[0]
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    pts = []
    for k, n, what in zip(ks, sizes, kind):
        centre = k.astype(np.float64) * float(BOX) + float(BOX) * 0.5
        # (rods and patches sit on harmonics of evenly spaced angles, which are uncorrelated for five points or more: the sample
        #  covariance is diagonal up to rounding, whatever the size of the cell, and no random draw tilts a label)
        ang = 2 * np.pi * (np.arange(n) / max(n, 1)) + rng.uniform(0, 2 * np.pi)
        if what == LINE:      # a rod: long in one direction, a thin circle across it
            p = np.stack([0.3 * np.cos(2 * ang), 0.03 * np.cos(ang), 0.03 * np.sin(ang)], axis=1)
        elif what == PLANE:   # a patch: a wide ring, thin in the third direction
            p = np.stack([0.3 * np.cos(ang), 0.3 * np.sin(ang), 0.03 * np.cos(2 * ang)], axis=1)
        else:                 # a blob: the six axis directions in turn at nearly one radius, no direction stands out
            p = axes[np.arange(n) % 6] * rng.uniform(0.24, 0.26, (n, 1))
        p = p[:, rng.permutation(3)] * float(BOX)
        pts.append(centre + p)
    pts = np.concatenate(pts).astype(np.float32)
    cell = np.repeat(ks, sizes, axis=0)
    order = rng.permutation(len(pts))
    return pts[order], cell[order], kind


MAPS = {"all kinds, a multiple of the block": dict(remainder=0), "all kinds, one more than a multiple": dict(remainder=1),
        "no line cell": dict(kinds=(SPHERE, PLANE), remainder=77), "no plane cell": dict(kinds=(SPHERE, LINE), remainder=78),
        "only sphere cells": dict(kinds=(SPHERE,), remainder=79)}


def oracle_map(pts):
    from oracle.orc_cellmap import CellMap
    km = CellMap(1.0)
    km.append(np.c_[pts, np.zeros(len(pts), np.float32)].astype(np.float32))
    return km


@pytest.fixture(scope="module")
def references():
    """per map: the geometry, the oracle's cell map and its keyframe_clouds -- computed once, shared, not changed"""
    from oracle.orc_scene_alignment import keyframe_clouds
    out = {}
    for name, kw in MAPS.items():
        pts, cell, kind = geometry(**kw)
        km = oracle_map(pts)
        k, ok = km.cell_index(pts)
        assert ok.all() and np.array_equal(k, cell), name          # every point lies in the cell it was made for
        out[name] = dict(pts=pts, cell=cell, kind=kind, km=km, labels=km.features(), clouds=keyframe_clouds(km))
    return out


def test_the_geometry_has_the_shapes_the_cases_need(references):
    for name, r in references.items():
        f, src = r["labels"], dump_form(r["pts"], r["cell"])
        lens = np.diff(src["cstart"])
        assert len(lens) == N_CELLS and 4000 <= len(r["pts"]) <= 6000, name
        for n in (1, 65, 257, 1000):
            assert (lens == n).any(), name
        assert len(r["pts"]) % BLOCK == MAPS[name].get("remainder", 0), name
        assert f["margin"][lens >= 5].min() > 1e-3, name               # no cell sits on a decision boundary: the labels are not in doubt
        shaped = np.where(lens >= 5, r["kind"], SPHERE)                # (a cell of fewer than five points is a sphere whatever its shape)
        assert np.array_equal(f["type"], shaped), name                 # rods are lines, patches planes, blobs spheres
        want = set(MAPS[name].get("kinds", (SPHERE, LINE, PLANE)))
        assert set(np.unique(f["type"])) == want | {SPHERE}, name
    both = references["all kinds, a multiple of the block"]["labels"]["type"]
    assert both[0] == LINE and both[-1] == PLANE                       # the first and the last cell are selected
    assert all((both == t).sum() >= 1 for t in (SPHERE, LINE, PLANE))
    line, plane, _ = references["all kinds, a multiple of the block"]["clouds"]
    assert len(line) > 257 and len(plane) > 1000
    assert len(references["no line cell"]["clouds"][0]) == 0 and len(references["no line cell"]["clouds"][1]) > 0
    assert len(references["no plane cell"]["clouds"][1]) == 0 and len(references["no plane cell"]["clouds"][0]) > 0
    assert len(references["only sphere cells"]["clouds"][0]) == len(references["only sphere cells"]["clouds"][1]) == 0


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cellmap_feature_clouds") / "cellmap_feature_clouds_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-x", "c++", "-I", os.path.join(ROOT, "tests", "cellmap_batch_shim"),
                           "-I", os.path.join(ROOT, "loam_livox_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cellmap_feature_clouds_host.cpp")])
    return exe


def run_host(exe, tmp, src, resolution=1.0):
    buf = np.array([len(src["pts"]), len(src["ckey"])], np.int32).tobytes() + np.float32(resolution).tobytes()
    buf += src["pts"].tobytes() + src["ckey"].tobytes() + src["cstart"].tobytes()
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    open(pin, "wb").write(buf)
    subprocess.check_call([exe, pin, pout])
    raw = open(pout, "rb").read()
    n_line, n_plane = (int(v) for v in np.frombuffer(raw, np.int32, 2))
    nc = len(src["ckey"])
    labels = np.frombuffer(raw, np.int32, nc, 8)
    pos = 8 + 4 * nc
    line = np.frombuffer(raw, np.float32, 4 * n_line, pos).reshape(-1, 4)
    plane = np.frombuffer(raw, np.float32, 4 * n_plane, pos + 16 * n_line).reshape(-1, 4)
    assert pos + 16 * (n_line + n_plane) == len(raw)
    return n_line, n_plane, labels, line, plane


@pytest.mark.parametrize("name", list(MAPS))
def test_chain_on_the_host_equals_the_oracle(host_exe, tmp_path, references, name):
    r = references[name]
    n_line, n_plane, labels, line, plane = run_host(host_exe, str(tmp_path), dump_form(r["pts"], r["cell"]))
    want_line, want_plane, _ = r["clouds"]
    assert np.array_equal(labels, r["labels"]["type"])
    assert (n_line, n_plane) == (len(want_line), len(want_plane))
    assert np.array_equal(line.view(np.uint32), want_line.view(np.uint32))
    assert np.array_equal(plane.view(np.uint32), want_plane.view(np.uint32))
    assert not line[:, 3].any() and not plane[:, 3].any()


def test_an_empty_map(host_exe, tmp_path):
    src = dict(pts=np.zeros((0, 4), np.float32), ckey=np.zeros(0, np.uint64), cstart=np.zeros(1, np.int32))
    n_line, n_plane, labels, line, plane = run_host(host_exe, str(tmp_path), src)
    assert (n_line, n_plane, len(labels), len(line), len(plane)) == (0, 0, 0, 0, 0)


def test_the_intensity_a_map_stores_does_not_come_out(host_exe, tmp_path, references):
    """every point is x, y, z, 0.0f whatever lies in the fourth component of the store"""
    r = references["all kinds, one more than a multiple"]
    src = dump_form(r["pts"], r["cell"])
    src["pts"] = src["pts"].copy()
    src["pts"][:, 3] = 5.0
    _, _, _, line, plane = run_host(host_exe, str(tmp_path), src)
    assert np.array_equal(line.view(np.uint32), r["clouds"][0].view(np.uint32)) and np.array_equal(plane.view(np.uint32), r["clouds"][1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ entry points without a device
NEW = {"ll_cellmap_feature_clouds": 8, "ll_scene_align_default_params": 1, "ll_scene_align_create": 3, "ll_scene_align_destroy": 1,
       "ll_scene_align_run": 8, "ll_scene_align_work": 2}


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "loam_livox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = capi.load()
    for name, n_args in NEW.items():
        decl = re.search(r"\b(int|void)\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl and name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert len(decl.group(2).split(",")) == len(fn.argtypes) == n_args, name
        assert fn.restype is (C.c_int32 if decl.group(1) == "int" else None), name
    from loam_livox_amd.api import Cell_map, Scene_aligner
    from loam_livox_amd.keyframes import Keyframe_assembly
    from loam_livox_amd.scene_alignment import Scene_alignment
    import inspect
    assert callable(Cell_map.feature_clouds) and callable(Scene_aligner.run)
    assert inspect.signature(Scene_alignment.__init__).parameters["on_device"].default is False
    assert inspect.signature(Keyframe_assembly.__init__).parameters["device_alignment"].default is False


def test_default_params_are_the_reference_defaults():
    p = capi.scene_align_default_params()
    f32 = lambda v: C.c_float(v).value
    assert (p.line_res, p.plane_res, p.maximum_icp_iteration, p.accepted_threshold) == (f32(0.4), f32(0.4), 10, f32(0.2))   # SA:27-28, 35-36
    assert (p.maximum_residual_block, p.registrar_init, p.subsample_seed) == (5000, 1, 1)                                   # SA:34


def test_null_handles_and_bad_parameters_are_refused_without_a_device():
    L = capi.load()
    n, thr, nr = C.c_int64(-7), C.c_double(0), C.c_int32(0)
    p = capi.scene_align_default_params()
    pose, rep, work = np.zeros(7), (capi.RegReport * 3)(), np.zeros(4, np.int64)
    assert L.ll_cellmap_feature_clouds(None, None, 0, C.byref(n), None, 0, C.byref(n), None) < 0
    assert b"ll_cellmap_feature_clouds: null" in L.ll_last_error() and n.value == -7
    h = C.c_void_p()
    assert L.ll_scene_align_create(0, 1024, None) < 0 and b"ll_scene_align_create: null" in L.ll_last_error()
    assert L.ll_scene_align_create(0, 0, C.byref(h)) < 0 and b"initial_points out of range" in L.ll_last_error() and not h.value
    assert L.ll_scene_align_run(None, None, None, C.byref(p), capi.ptr(pose), C.byref(thr), rep, C.byref(nr)) < 0
    assert b"ll_scene_align_run: null" in L.ll_last_error()
    assert L.ll_scene_align_work(None, capi.ptr(work)) < 0 and b"ll_scene_align_work: null" in L.ll_last_error()
    L.ll_scene_align_destroy(None)
    L.ll_scene_align_default_params(None)


def test_keyframe_assembly_hands_the_switch_on():
    """device_alignment reaches the assembly through the loop_closure settings of the mapping loops, which pass them on as they are"""
    from loam_livox_amd import keyframes

    class Full:
        def close(self):
            pass
    ka = keyframes.Keyframe_assembly(full_cell_map=Full(), **dict(device_alignment=True))
    assert ka.device_alignment and ka._scene_alignment is None
    ka.close()
    assert not keyframes.Keyframe_assembly(full_cell_map=Full()).device_alignment
