"""CPU tier of motion deblur with a map per slot (ll_reg_set_time_ranges, ll_fe_selection_last, ll_history_batch_set_undistort;
tests/test_gpu_deblur_maps.py and tests/test_gpu_deblur_batch_loop.py are the GPU tier): the symbols, their argument lists and their
refusals without a device, the Python mirror over the recording stand-in, and Laser_mapping_batch over stub handles -- flags 0 / 0
make the default constructor's calls, the flags put set_time_ranges in front of every enqueue (the repeat of an aborted solve
included) with the ranges of laser_mapping.hpp:1336-1347 per sequence, and set_undistort in front of the add."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from loam_livox_amd import api, capi, mapping
from tests import api_standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "loam_livox_hip.h")
NEW_SYMBOLS = {"ll_reg_set_time_ranges": 4, "ll_fe_selection_last": 4, "ll_history_batch_set_undistort": 2}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for name, n_args in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(capi.SYMBOLS[name][1]), name
        assert capi.SYMBOLS[name][0] is C.c_int32 and name in exported and hasattr(L, name)
    # the adapter names the two it calls as weak references, like the information pair and the undistort calls
    adapter = open(os.path.join(ROOT, "include", "loam_livox_adapter.hpp")).read()
    for name in ("ll_reg_set_time_ranges", "ll_history_batch_set_undistort"):
        assert re.search(r"\bint\s+%s\s*\([^;]*\)\s*__attribute__\(\(weak\)\);" % name, adapter), name
        assert "!&%s" % name in adapter, name


def test_null_arguments_are_refused_with_their_text_without_a_device():
    L = capi.load()
    f = np.zeros(2, np.float32)
    i = np.zeros(2, np.int32)
    for call, fn in ((lambda: L.ll_reg_set_time_ranges(None, _p(f), _p(f), 2), "ll_reg_set_time_ranges"),
                     (lambda: L.ll_fe_selection_last(None, 2, 2, _p(i)), "ll_fe_selection_last"),
                     (lambda: L.ll_history_batch_set_undistort(None, None), "ll_history_batch_set_undistort")):
        rc = call()
        msg = L.ll_last_error().decode()
        assert rc != 0 and fn in msg and "null" in msg, (rc, msg)


def test_api_methods_over_the_recording_stand_in(monkeypatch):
    lib = api_standin.Recording_library()
    monkeypatch.setattr(capi, "_lib", lib)
    reg = api.Point_cloud_registration(max_scans=3, max_features=100)
    fe = api.Livox_laser(max_points=100, max_scans=3)
    hb = api.History_buffer_batch(3, 5, 100)
    lo, hi = [0.5, 1.25, 2.0], np.array([0.75, 1.5, 2.25])
    reg.set_time_ranges(lo, hi)
    name, args = lib.calls[-1]
    assert name == "ll_reg_set_time_ranges" and args[0] == api_standin.plain(reg.h) and args[3] == 3
    assert args[1] == api_standin.plain(np.array(lo, np.float32)) and args[2] == api_standin.plain(hi.astype(np.float32))
    with pytest.raises(ValueError):
        reg.set_time_ranges(lo, hi[:2])
    last = fe.selection_last(3, 2)
    name, args = lib.calls[-1]
    assert name == "ll_fe_selection_last" and args[:3] == [api_standin.plain(fe.h), 3, 2] and args[3]["dtype"] == "int32" and args[3]["shape"] == [3]
    assert last.shape == (3,) and last.dtype == np.int32
    hb.set_undistort(reg)
    name, args = lib.calls[-1]
    assert name == "ll_history_batch_set_undistort" and args == [api_standin.plain(hb.h), api_standin.plain(reg.h)]
    for name, call in (("ll_reg_set_time_ranges", lambda: reg.set_time_ranges(lo, hi)), ("ll_fe_selection_last", lambda: fe.selection_last(3)),
                       ("ll_history_batch_set_undistort", lambda: hb.set_undistort(reg))):
        lib.fail.add(name)
        with pytest.raises(capi.LoamLivoxError):
            call()


# ------------------------------------------------------------------------------------------------ the lock-step loop over stub handles
class Stub:
    def __init__(self, log, name, answers=None):
        self._log, self._name, self._answers = log, name, answers or {}
        self.params = types.SimpleNamespace(time_internal_pts=1e-5, max_points=1000)
        self.debug_flags = 0

    def __getattr__(self, method):
        if method.startswith("__"):
            raise AttributeError(method)

        def call(*a, **k):
            self._log.append((self._name, method, a, k))
            ans = self._answers.get(method)
            return ans(*a, **k) if callable(ans) else ans
        return call


S = 3
LAST = np.array([7, 11, 5], np.int32)   # selection_last's answer: the last full position of every slot


def stub_world(monkeypatch, abort_first=False):
    log = []
    state = {"collects": 0}

    def collect(n):
        state["collects"] += 1
        reps = [capi.RegReport() for _ in range(n)]
        for r in reps:
            r.accepted = 1
        if abort_first and state["collects"] == 1:
            reps[1].aborted = 1
        pc = np.tile(np.array([0, 0, 0, 1, 0.1, 0, 0], np.float64), (n, 1))
        return np.ones(n, np.int32), pc, pc.copy(), reps

    def set_debug_flags(flags, _st=state):
        _st["flags"] = flags

    fe = dict(selection_last=lambda n, kind=2: LAST[:n].copy())
    hist = dict(add_voxel=True, refresh=(1, 2))
    hb = dict(add_voxel=np.ones(S, bool), refresh=(np.ones(S, np.int64), np.ones(S, np.int64)))
    reg = dict(collect=collect)
    for cls, answers in (("Livox_laser", fe), ("Point_cloud_registration", reg), ("Map_buffer", {}), ("VoxelGrid", {}), ("History_buffer", hist),
                         ("History_buffer_batch", hb)):
        monkeypatch.setattr(mapping, cls, lambda *a, _c=cls, _an=answers, **k: Stub(log, _c, _an))
    return log


def names(log):
    return [(c, m) for c, m, _, _ in log]


def run_steps(lb, log, stamps_of):
    del log[:]
    scan = np.zeros((10, 4), np.float32)
    for k, scans in enumerate(([scan] * S, [scan, None, scan])):   # the second step: sequence 1 idle
        out = lb.process_new_scans(scans, stamps_of(k))
        assert out.tolist() == [1 if x is not None else -1 for x in scans]
    return list(log)


def stamps_of(k):
    return [0.5 + 0.1 * k, 1.5 + 0.1 * k, 2.5 + 0.1 * k]


def stamp(t, idx):
    return float(np.float32(np.float64(t) + np.float64(np.float32(idx) * np.float32(1e-5))))


@pytest.mark.parametrize("batched_history", [False, True])
def test_flags_off_make_the_default_constructors_calls(monkeypatch, batched_history):
    log = stub_world(monkeypatch)
    kw = dict(scan_points=1000, batched_history=batched_history, refresh_threads=1)
    base = names(run_steps(mapping.Laser_mapping_batch(S, **kw), log, stamps_of))
    lb = mapping.Laser_mapping_batch(S, if_motion_deblur=0, if_undistort=0, **kw)
    assert names(run_steps(lb, log, stamps_of)) == base
    assert isinstance(lb.reg.params, types.SimpleNamespace) and "if_motion_deblur" not in vars(lb.reg.params)   # ... and nothing set on the registrar
    for c in (("Livox_laser", "selection_last"), ("Point_cloud_registration", "set_time_ranges"), ("History_buffer", "set_undistort"),
              ("History_buffer_batch", "set_undistort")):
        assert c not in base


@pytest.mark.parametrize("batched_history", [False, True])
def test_flags_on_put_the_ranges_before_every_enqueue_and_the_records_before_the_add(monkeypatch, batched_history):
    log = stub_world(monkeypatch)
    kw = dict(scan_points=1000, batched_history=batched_history, refresh_threads=1)
    base = names(run_steps(mapping.Laser_mapping_batch(S, **kw), log, stamps_of))
    lb = mapping.Laser_mapping_batch(S, if_motion_deblur=1, if_undistort=1, **kw)
    calls = run_steps(lb, log, stamps_of)
    seq = names(calls)
    assert lb.reg.params.if_motion_deblur == 1
    hist = "History_buffer_batch" if batched_history else "History_buffer"
    extra = {("Livox_laser", "selection_last"), ("Point_cloud_registration", "set_time_ranges"), (hist, "set_undistort")}
    assert [c for c in seq if c not in extra] == base                # nothing else moved
    # one selection_last per step, behind the selection; one set_time_ranges directly in front of every enqueue
    assert seq.count(("Livox_laser", "selection_last")) == 2
    for i, c in enumerate(seq):
        if c == ("Livox_laser", "selection_last"):
            assert seq[i - 1] == ("Livox_laser", "select_batch")
        if c[0] == "Point_cloud_registration" and c[1].startswith("enqueue"):
            assert seq[i - 1] == ("Point_cloud_registration", "set_time_ranges")
    ranges = [a for c, m, a, _ in calls if m == "set_time_ranges"]
    assert len(ranges) == 2 == sum(1 for c in seq if c[1].startswith("enqueue"))
    # step 0: every sequence from 0 to its frame's last stamp; step 1: from there to the next one -- the idle sequence keeps its stamp
    first = [stamp(stamps_of(0)[s], LAST[s]) for s in range(S)]
    second = [stamp(stamps_of(1)[s], LAST[s]) for s in range(S)]
    assert list(ranges[0][0]) == [0.0] * S and list(ranges[0][1]) == first
    assert list(ranges[1][0]) == first and list(ranges[1][1]) == [second[0], first[1], second[2]]
    assert lb.m_last_time_stamp.tolist() == [second[0], first[1], second[2]]
    # the records: in front of the add
    if batched_history:
        assert seq.count((hist, "set_undistort")) == 2
        for i, c in enumerate(seq):
            if c == (hist, "set_undistort"):
                assert seq[i + 1] == (hist, "add_voxel") and calls[i][2][0] is lb.reg
    else:
        und = [(i, a) for i, (c, m, a, _) in enumerate(calls) if (c, m) == (hist, "set_undistort")]
        assert [a[1] for _, a in und] == [0, 1, 2, 0, 2] and all(a[0] is lb.reg for _, a in und)   # sequence s's record, slot s
        adds = [i for i, c in enumerate(seq) if c == (hist, "add_voxel")]
        assert len(adds) == 5 and max(i for i, _ in und[:3]) < adds[0] and max(i for i, _ in und[3:]) < adds[3]   # all on the calling thread, before the adds start


def test_the_repeat_of_an_aborted_solve_gets_its_ranges_too(monkeypatch):
    log = stub_world(monkeypatch, abort_first=True)
    lb = mapping.Laser_mapping_batch(S, if_motion_deblur=1, if_undistort=1, scan_points=1000, batched_history=True)
    del log[:]
    scan = np.zeros((10, 4), np.float32)
    lb.process_new_scans([scan] * S, stamps_of(0))
    seq = names(log)
    enq = [i for i, c in enumerate(seq) if c[1].startswith("enqueue")]
    assert len(enq) == 2 and lb.aborted_solves == 1
    assert all(seq[i - 1] == ("Point_cloud_registration", "set_time_ranges") for i in enq)
    ranges = [a for c, m, a, _ in log if m == "set_time_ranges"]
    assert list(ranges[0][0]) == list(ranges[1][0]) and list(ranges[0][1]) == list(ranges[1][1])   # the step's ranges, not the next step's
    assert seq.count(("Livox_laser", "selection_last")) == 1
    # with deblur the repeat takes every active slot: it overwrites the deskew records of the slots it would leave idle
    maps = [a[0] for c, m, a, _ in log if m.startswith("enqueue")]
    assert all(x is not None for x in maps[1]) and len(maps[1]) == S


def test_undistort_with_full_maps_is_refused(monkeypatch):
    stub_world(monkeypatch)
    with pytest.raises(ValueError, match="full_maps"):
        mapping.Laser_mapping_batch(S, scan_points=1000, batched_history=True, full_maps=True, if_undistort=1)
    with pytest.raises(ValueError, match="full_maps"):
        mapping.Laser_mapping_batch(S, scan_points=1000, batched_history=True, full_maps=True, key_frames=True, if_motion_deblur=1, if_undistort=1)
    mapping.Laser_mapping_batch(S, scan_points=1000, batched_history=True, full_maps=True, if_motion_deblur=1)   # deblur alone is allowed
