"""CPU tier of the cell maps of the batched match buffer (tests/test_gpu_cellmap_batch.py is the GPU tier): the entry points are
declared, exported and bound; null arguments are refused without a device; Laser_mapping_batch(cell_maps=True) enables the maps
once and keeps adding for exactly the accepted slots (against stubbed device handles); and the deferred store -- log, epochs,
materialisation -- built on the host from the kernels' own decision functions (tests/cellmap_batch_host.cpp includes
ll_cellmap_batch_core.h) equals the oracle's cell map after every append, and so do the launch chains of
ll_cellmap_batch_kernels.hip themselves, compiled for the CPU against a stand-in for the HIP headers (tests/cellmap_batch_shim)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from loam_livox_amd import capi, mapping
from oracle.orc_cellmap import CellMap
from tests.test_multimap_host import _Stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ll_history_batch_enable_cell_maps", "ll_history_batch_sync_cell_maps", "ll_history_batch_cell_map_stats", "ll_history_batch_cell_map_dump",
       "ll_history_batch_cell_map_device_view", "ll_history_batch_cell_map_work")


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "loam_livox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = capi.load()
    for name in NEW:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl, name
        assert name in capi.SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is C.c_int32
        assert len(decl.group(1).split(",")) == len(fn.argtypes), name  # the argument lists have the same length
    from loam_livox_amd.api import Cell_map, Cell_map_slot, History_buffer_batch
    for m in ("enable_cell_maps", "sync_cell_maps", "cell_map"):
        assert callable(getattr(History_buffer_batch, m))
    for m in ("stats", "dump", "device_view"):  # the names of api.Cell_map
        assert callable(getattr(Cell_map_slot, m)) and callable(getattr(Cell_map, m))
    adapter = open(os.path.join(ROOT, "include", "loam_livox_adapter.hpp")).read()
    body = adapter[adapter.index("class History_batch"):adapter.index("class Points_cloud_map")]
    for name in NEW[:-1]:
        assert name in body, name
    for m in ("sync", "cell_map"):
        assert callable(getattr(mapping.Laser_mapping_batch, m))


def test_null_arguments_are_refused_without_a_device():
    L = capi.load()
    n, i = C.c_int64(0), C.c_int32(0)
    p, q = C.c_void_p(), C.c_void_p()
    out = (C.c_int64 * 4)()
    assert L.ll_history_batch_enable_cell_maps(None, 1000, 1.0, 3) < 0 and b"ll_history_batch_enable_cell_maps: null" in L.ll_last_error()
    assert L.ll_history_batch_sync_cell_maps(None) < 0 and b"ll_history_batch_sync_cell_maps: null" in L.ll_last_error()
    assert L.ll_history_batch_cell_map_stats(None, 0, 0, C.byref(n), C.byref(n), C.byref(i)) < 0 and b"ll_history_batch_cell_map_stats: null" in L.ll_last_error()
    assert L.ll_history_batch_cell_map_dump(None, 0, 0, None, 0, None, None, None, 0) < 0 and b"ll_history_batch_cell_map_dump: null" in L.ll_last_error()
    assert L.ll_history_batch_cell_map_device_view(None, 0, 0, C.byref(p), C.byref(q), C.byref(n), None) < 0
    assert b"ll_history_batch_cell_map_device_view: null" in L.ll_last_error()
    assert L.ll_history_batch_cell_map_work(None, out) < 0 and b"ll_history_batch_cell_map_work: null" in L.ll_last_error()


# ---- the loop's bookkeeping, device handles stubbed ---------------------------------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    st = _Stubs()
    outer = st

    class HistBatch:
        def __init__(self, n_sequences, *a, **kw):
            self.S = n_sequences
            self.frames = [0] * n_sequences

        def enable_cell_maps(self, initial_points_per_map, cell_resolution, threshold_cell_revisit):
            outer.log.append(("enable_cell_maps", initial_points_per_map, cell_resolution, threshold_cell_revisit))

        def sync_cell_maps(self):
            outer.log.append(("sync_cell_maps",))

        def cell_map(self, s, kind):
            outer.log.append(("cell_map", s, kind))
            return (s, kind)

        def add_voxel(self, vc, vs, poses, gate=None, active=None, t=0.0, a=0.0):
            on = [bool(x) for x in active]
            outer.log.append(("add_voxel", tuple(on)))
            for s in range(self.S):
                self.frames[s] += on[s]
            return np.array(on)

        def refresh(self, maps, active=None):
            return np.array(self.frames), np.array(self.frames)

        def size(self, s):
            return min(self.frames[s], 5)

        def close(self):
            pass

    def no_single_handles(*a, **kw):
        raise AssertionError("the batched mode must not create per-sequence History_buffer handles")

    classes = dict(st.classes, History_buffer=no_single_handles, History_buffer_batch=HistBatch)
    for k, v in classes.items():
        monkeypatch.setattr(mapping, k, v)
    return st


def test_loop_enables_the_maps_once_and_adds_for_the_accepted_slots(stubbed):
    st = stubbed
    st.reject.add((1, 4))  # sequence 1 is rejected at its frame 4
    lb = mapping.Laser_mapping_batch(3, batched_history=True, cell_maps=True, scan_points=100, init_accumulate_frames=2, cell_map_max_points=4096,
                                     cell_resolution=0.8, threshold_cell_revisit=7)
    assert [e for e in st.log if e[0] == "enable_cell_maps"] == [("enable_cell_maps", 4096, 0.8, 7)]
    scan = np.zeros((100, 4), np.float32)
    for step in range(6):
        st.log.clear()
        out = lb.process_new_scans([scan, scan if step >= 1 else None, scan])
        adds = [e for e in st.log if e[0] == "add_voxel"]
        assert len(adds) == 1 and adds[0][1] == tuple(bool(out[s] == 1) for s in range(3))
        assert not [e for e in st.log if e[0] in ("enable_cell_maps", "sync_cell_maps")]  # enabled once, never put in order by the loop itself
    assert out.tolist() == [1, 0, 1]
    st.log.clear()
    lb.sync()
    assert lb.cell_map(2, 1) == (2, 1)
    assert st.log == [("sync_cell_maps",), ("cell_map", 2, 1)]
    lb.close()
    # a first allocation below one scan is raised to it; without the keyword the store starts at 2^18 points per map
    st.log.clear()
    mapping.Laser_mapping_batch(2, batched_history=True, cell_maps=True, scan_points=100, cell_map_max_points=10).close()
    mapping.Laser_mapping_batch(2, batched_history=True, cell_maps=True, scan_points=100).close()
    assert [e[1] for e in st.log if e[0] == "enable_cell_maps"] == [100, 1 << 18]


def test_cell_maps_need_the_batched_history_and_keep_cell_maps_stays_refused(stubbed):
    with pytest.raises(ValueError, match="batched_history"):
        mapping.Laser_mapping_batch(2, cell_maps=True, scan_points=100)
    with pytest.raises(ValueError, match="batched_history"):
        mapping.Laser_mapping_batch(2, batched_history=False, cell_maps=True, scan_points=100)
    for kw in (dict(keep_cell_maps=True), dict(keep_cell_maps=True, cell_maps=True), dict(matching_mode=1, cell_maps=True)):
        with pytest.raises(ValueError):
            mapping.Laser_mapping_batch(2, batched_history=True, scan_points=100, **kw)
    with pytest.raises(TypeError):
        mapping.Laser_mapping(scan_points=100, cell_maps=True)  # not an argument of Laser_mapping
    lb = mapping.Laser_mapping_batch(2, batched_history=True, scan_points=100)
    assert lb.cell_maps is False and not [e for e in stubbed.log if e[0] == "enable_cell_maps"]
    lb.sync()  # nothing to wait for
    with pytest.raises(ValueError):
        lb.cell_map(0, 0)
    lb.close()


# ---- the deferred store on the host ---------------------------------------------------------------------------------------------------------
THR, RES, N_STEPS = 3, 1.0, 12


def clouds():
    """A, B = A + (0, 50, 0): 300 valid points each; C: A moved by a third of a cell, two of its points not storable"""
    rng = np.random.default_rng(11)
    A = rng.uniform(-4.0, 4.0, (300, 3)).astype(np.float32)
    B = (A + np.array([0, 50, 0], np.float32)).astype(np.float32)
    Cc = (A + np.float32(0.17)).astype(np.float32)
    Cc[7] = [np.nan, 0, 0]
    Cc[100] = [0, 3e6, 0]  # beyond 2^20 cells
    return dict(A=A, B=B, C=Cc, E=np.zeros((0, 3), np.float32))


# per map: a cloud per step, "-" = the map sits the step out, "E" = an empty cloud
SCHEDULE = ["ABBBACABEACB",   # a revisit after three appends elsewhere (steps 0 - 4), an empty cloud
            "A---ABB-BAAC",   # skips three steps, then the same cells again: its own counter has not moved, no reset
            "CEAA-BCCCA-B"]   # an empty cloud on a map that holds one cloud


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cellmap_batch") / "cellmap_batch_host")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cellmap_batch_host.cpp")])
    return exe


def run_host(exe, tmp, reads):
    cl = clouds()
    buf = np.array([3, N_STEPS, THR], np.int32).tobytes() + np.float32(RES).tobytes()
    for t in range(N_STEPS):
        buf += np.int32(reads[t]).tobytes()
        for m in range(3):
            c = SCHEDULE[m][t]
            buf += np.int32(-1).tobytes() if c == "-" else np.int32(len(cl[c])).tobytes() + cl[c].tobytes()
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    open(pin, "wb").write(buf)
    subprocess.check_call([exe, pin, pout])
    raw = np.fromfile(pout, np.int32)
    pos, out = 0, {}
    for t in range(N_STEPS):
        if not reads[t]:
            continue
        for m in range(3):
            frame, nc, npts = raw[pos:pos + 3]
            pos += 3
            ijk = raw[pos:pos + 3 * nc].reshape(nc, 3)
            pos += 3 * nc
            start = raw[pos:pos + nc + 1]
            pos += nc + 1
            last = raw[pos:pos + nc]
            pos += nc
            pts = raw[pos:pos + 3 * npts].reshape(npts, 3)  # (bits)
            pos += 3 * npts
            out[(t, m)] = (int(frame), ijk, start, last, pts)
    assert pos + 1 == len(raw) and raw[pos] == sum(bool(r) for r in reads)  # one materialisation per read step
    return out


def oracle_states():
    cl = clouds()
    maps = [CellMap(RES, THR) for _ in range(3)]
    states, counts = {}, {}
    for t in range(N_STEPS):
        for m in range(3):
            c = SCHEDULE[m][t]
            if c != "-":
                maps[m].append(cl[c])
            keys = sorted(maps[m].cells)
            pts = [maps[m].cell_points(k) for k in keys]
            start = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
            states[(t, m)] = (maps[m].frame, np.array(keys, np.int32).reshape(-1, 3), start, np.array([maps[m].cells[k]["last"] for k in keys], np.int32),
                              (np.concatenate(pts) if pts else np.zeros((0, 3), np.float32)).astype(np.float32).view(np.int32))
            counts[(t, m)] = maps[m].n_points()
    return states, counts


def assert_same(got, want, tag):
    assert got[0] == want[0], (tag, "frame counter", got[0], want[0])
    assert np.array_equal(got[1], want[1]), (tag, "cell indices")
    assert np.array_equal(got[2], want[2]), (tag, "cell_start")
    assert np.array_equal(got[3], want[3]), (tag, "last-update stamps")
    assert got[4].shape == want[4].shape and np.array_equal(got[4], want[4]), (tag, "points in order")


def test_deferred_store_on_the_host_equals_the_oracle_after_every_append(host_exe, tmp_path):
    want, counts = oracle_states()
    # what the schedules are there for, on the oracle: A B B B A drops the 300 old points of A; A, three idle steps, A does not
    assert [counts[(t, 0)] for t in range(5)] == [300, 600, 900, 1200, 1200]
    assert [counts[(t, 1)] for t in range(5)] == [300, 300, 300, 300, 600]
    assert counts[(0, 2)] == counts[(1, 2)] == 298 and want[(1, 2)][0] == want[(0, 2)][0] + 1  # two points dropped; the empty cloud moves the counter
    got = run_host(host_exe, str(tmp_path), [1] * N_STEPS)
    for t in range(N_STEPS):
        for m in range(3):
            assert_same(got[(t, m)], want[(t, m)], (t, m, "read after every append"))
    # the same appends behind a log that is put in order three times only
    reads = [int(t in (3, 7, 11)) for t in range(N_STEPS)]
    late = run_host(host_exe, str(tmp_path), reads)
    assert sorted({t for t, _ in late}) == [3, 7, 11]
    for key, g in late.items():
        assert_same(g, want[key], key + ("three reads",))


# ---- the kernels' own source on the host ----------------------------------------------------------------------------------------------------
def test_launch_chains_of_the_kernel_unit_on_the_host_equal_the_oracle(tmp_path):
    """cb_append / cb_materialise as compiled from ll_cellmap_batch_kernels.hip: every kernel runs once per thread, one after the other"""
    exe = str(tmp_path / "cellmap_batch_kernels_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-x", "c++", "-I", os.path.join(ROOT, "tests", "cellmap_batch_shim"),
                           "-I", os.path.join(ROOT, "loam_livox_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cellmap_batch_kernels_host.cpp")])
    want, _ = oracle_states()
    got = run_host(exe, str(tmp_path), [1] * N_STEPS)
    for key, g in got.items():
        assert_same(g, want[key], key + ("kernel source, read after every append",))
    late = run_host(exe, str(tmp_path), [int(t in (3, 7, 11)) for t in range(N_STEPS)])
    assert sorted({t for t, _ in late}) == [3, 7, 11]
    for key, g in late.items():
        assert_same(g, want[key], key + ("kernel source, three reads",))
