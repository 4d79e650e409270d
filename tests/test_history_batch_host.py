"""CPU tier of the batched match buffer (tests/test_gpu_history_batch.py is the GPU tier): the entry points are declared, exported and
bound; null arguments are refused without a device; Laser_mapping_batch(batched_history=True) keeps every sequence's books right
(against stubbed device handles); the grid geometry both grid builds share equals a plain restatement; the adapter demo compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from loam_livox_amd import capi, mapping
from tests.placement import plain_geometry  # (the numpy restatement of map_grid_geometry)
from tests.test_multimap_host import _Stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ll_history_batch_create": "int", "ll_history_batch_destroy": "void", "ll_history_batch_add_voxel": "int", "ll_history_batch_add_fe": "int",
       "ll_history_batch_refresh": "int", "ll_history_batch_size": "int32_t", "ll_history_batch_map_cloud": "int64_t", "ll_map_grid_geometry": "int"}


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "loam_livox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = capi.load()
    for name, ret in NEW.items():
        decl = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl, name
        assert name in capi.SYMBOLS
        fn = getattr(L, name)
        assert len(decl.group(1).split(",")) == len(fn.argtypes), name  # the argument lists have the same length
    assert L.ll_history_batch_create.restype is C.c_int32 and L.ll_history_batch_map_cloud.restype is C.c_int64
    from loam_livox_amd.api import History_buffer_batch
    for m in ("add_voxel", "add_fe", "refresh", "size", "map_cloud", "close"):
        assert callable(getattr(History_buffer_batch, m))
    adapter = open(os.path.join(ROOT, "include", "loam_livox_adapter.hpp")).read()
    assert "class History_batch" in adapter


def test_null_arguments_are_refused_without_a_device():
    L = capi.load()
    h = C.c_void_p()
    assert L.ll_history_batch_create(0, 2, 5, 100, 0.1, 0.4, None) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_create(0, 0, 5, 100, 0.1, 0.4, C.byref(h)) < 0 and b"n_sequences" in L.ll_last_error()
    assert L.ll_history_batch_create(0, 1 << 11, 1 << 10, 1 << 10, 0.1, 0.4, C.byref(h)) < 0 and b"2^31" in L.ll_last_error()
    assert L.ll_history_batch_add_voxel(None, None, None, None, None, None, 0.0, 0.0, None) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_add_fe(None, None, None, None, None, 0.0, 0.0, None) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_refresh(None, None, None, None, None) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_size(None, 0) == -1
    assert L.ll_history_batch_map_cloud(None, 0, 0, None, 0) < 0
    L.ll_history_batch_destroy(None)
    assert L.ll_map_grid_geometry(None, 0.5, None, None, None) < 0


# ---- the loop's bookkeeping, device handles stubbed ---------------------------------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    st = _Stubs()
    outer = st

    class HistBatch:
        def __init__(self, n_sequences, *a, **kw):
            self.S = n_sequences
            self.frames = [0] * n_sequences

        def _add(self, name, poses, gate, active, t, a):
            on = [bool(x) for x in active]
            assert gate is not None
            outer.log.append((name, tuple(on), [float(p[4]) for p in poses], [float(g[4]) for g in gate]))
            for s in range(self.S):
                self.frames[s] += on[s]
            return np.array(on)

        def add_voxel(self, vc, vs, poses, gate=None, active=None, t=0.0, a=0.0):
            return self._add("add_voxel", poses, gate, active, t, a)

        def add_fe(self, fe, poses, gate=None, active=None, t=0.0, a=0.0):
            return self._add("add_fe", poses, gate, active, t, a)

        def refresh(self, maps, active=None):
            on = [bool(x) for x in active]
            assert [m is not None for m in maps] == on
            outer.log.append(("refresh", tuple(on)))
            return np.array([10 * f for f in self.frames]), np.array([100 * f for f in self.frames])

        def size(self, s):
            return min(self.frames[s], 5)

        def map_cloud(self, s, kind):
            return np.zeros((self.frames[s], 4), np.float32)

        def close(self):
            outer.log.append(("close_batch",))

    def no_single_handles(*a, **kw):
        raise AssertionError("the batched mode must not create per-sequence History_buffer handles")

    classes = dict(st.classes, History_buffer=no_single_handles, History_buffer_batch=HistBatch)
    for k, v in classes.items():
        monkeypatch.setattr(mapping, k, v)
    return st


def test_batched_loop_bookkeeping(stubbed):
    st = stubbed
    st.reject.add((1, 4))      # sequence 1 is rejected at its frame 4
    st.abort_once.add((2, 3))  # sequence 2's frame 3 is abandoned by the grouped solver once, then registers
    lb = mapping.Laser_mapping_batch(3, batched_history=True, scan_points=100, init_accumulate_frames=2)
    assert lb._pool is None  # no thread pool
    scan = np.zeros((100, 4), np.float32)
    results = []
    for step in range(6):
        scans = [scan, scan if step >= 1 else None, scan]  # sequence 1 starts a step late
        poses_before = lb.poses.copy()
        st.log.clear()
        out = lb.process_new_scans(scans)
        results.append(out.tolist())
        enq = [e for e in st.log if e[0] == "enqueue"]
        adds = [e for e in st.log if e[0] in ("add_voxel", "add_fe")]
        refs = [e for e in st.log if e[0] == "refresh"]
        accepted = tuple(bool(out[s] == 1) for s in range(3))
        # one add and one refresh per step, over exactly the accepted slots: a rejected slot and an idle slot are inactive
        assert len(adds) == 1 and len(refs) == 1 and adds[0][0] == "add_voxel"
        assert adds[0][1] == accepted and refs[0][1] == accepted
        for s in range(3):
            if accepted[s]:
                assert adds[0][3][s] == poses_before[s, 4]  # the gate pose is the pose BEFORE the registration
                assert adds[0][2][s] == lb.poses[s, 4]      # the clouds move with the registered pose
        if step == 3:  # the repeat of an abandoned solve: its slot alone, groups off, flags put back -- and one add for all three slots
            assert len(enq) == 2 and enq[1][1] == (False, False, True) and enq[1][3] == 32 and lb.reg.debug_flags == 0
            assert accepted == (True, True, True)
        else:
            assert len(enq) == 1
    assert results == [[1, -1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 0, 1]]
    assert lb.frame_index.tolist() == [6, 5, 6]
    assert lb.aborted_solves == 1
    assert lb.poses[:, 4].tolist() == [3.0, 1.0, 3.0]
    assert lb.map_sizes[0] == (60, 600) and lb.map_sizes[1] == (40, 400)
    # histories[s] is a view of slot s
    assert [len(h) for h in lb.histories] == [5, 4, 5] and lb.histories[1].map_cloud(0).shape == (4, 4)
    st.log.clear()
    assert lb.process_new_scans([None, None, None]).tolist() == [-1, -1, -1] and lb.frame_index.tolist() == [6, 5, 6]
    assert not [e for e in st.log if e[0] in ("add_voxel", "add_fe", "refresh")]
    assert lb.stage_s[3] == 6 and lb.stage_s[4] > 0 and lb.stage_s[1] > 0 and lb.stage_s[2] > 0
    lb.close()
    assert ("close_batch",) in st.log


def test_batched_loop_without_input_downsampling_adds_the_extractor_features(stubbed):
    lb = mapping.Laser_mapping_batch(2, batched_history=True, scan_points=100, init_accumulate_frames=0, input_downsample_mode=0)
    scan = np.zeros((100, 4), np.float32)
    lb.process_new_scans([scan, None])
    adds = [e for e in stubbed.log if e[0] in ("add_voxel", "add_fe")]
    assert len(adds) == 1 and adds[0][0] == "add_fe" and adds[0][1] == (True, False)
    lb.close()


def test_default_mode_is_unchanged(monkeypatch):
    st = _Stubs()
    for k, v in st.classes.items():
        monkeypatch.setattr(mapping, k, v)

    def no_batch(*a, **kw):
        raise AssertionError("the default mode must not create a History_buffer_batch")

    monkeypatch.setattr(mapping, "History_buffer_batch", no_batch)
    lb = mapping.Laser_mapping_batch(2, scan_points=100)
    assert lb.batched_history is False and lb.history_batch is None and len(lb.histories) == 2 and lb._pool is not None
    lb.close()
    for kw in (dict(lidar_type="velodyne"), dict(matching_mode=1), dict(loop_closure_if_enable=1), dict(keep_cell_maps=True)):
        with pytest.raises(ValueError):
            mapping.Laser_mapping_batch(2, batched_history=True, **kw)


# ---- the grid geometry --------------------------------------------------------------------------------------------------------------------
def test_grid_geometry_equals_a_plain_restatement():
    from loam_livox_amd.api import map_grid_geometry
    rng = np.random.default_rng(5)
    boxes = []
    for _ in range(200):
        lo = rng.uniform(-80, 80, 3).astype(np.float32)
        boxes.append((np.r_[lo, lo + rng.uniform(0, 60, 3).astype(np.float32)], float(rng.choice([0.4, 0.45, 0.6, 1.2, 1.45]))))
    boxes.append((np.array([1.5, -2.0, 0.25, 1.5, -2.0, 0.25], np.float32), 0.45))        # a single point
    boxes.append((np.array([np.inf] * 3 + [-np.inf] * 3, np.float32), 0.45))              # no finite point
    boxes.append((np.array([np.nan] * 6, np.float32), 0.4))                               # (as the batched build decodes an empty box)
    boxes.append((np.array([-400, -400, -50, 400, 400, 50], np.float32), 0.4))            # 2000 x 2000 x 250 cells: one growth step
    boxes.append((np.array([-3000, -3000, -300, 3000, 3000, 300], np.float32), 0.4))      # several
    grown = 0
    for mm, cell in boxes:
        dims, h, slack = map_grid_geometry(mm, cell)
        wd, wh, ws = plain_geometry(mm, cell)
        assert dims == wd, (mm, cell)
        assert np.float32(h).tobytes() == wh.tobytes() and np.float32(slack).tobytes() == ws.tobytes(), (mm, cell, h, wh, slack, ws)
        assert dims[0] * dims[1] * dims[2] <= 1 << 27
        grown += np.float32(h) != np.float32(cell)
    assert grown == 2
    assert map_grid_geometry(boxes[-3][0], 0.4)[0] == (1, 1, 1) and map_grid_geometry(boxes[-4][0], 0.45)[0] == (1, 1, 1)


# ---- the adapter --------------------------------------------------------------------------------------------------------------------------
def test_history_batch_demo_compiles_and_links(tmp_path):
    from loam_livox_amd import build
    lib = build.build()
    exe = os.path.join(str(tmp_path), "history_batch_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "history_batch_demo.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
